"""Row statistics handed from a producer GEMM to the LayerNorm-folded GEMM that reads its output (csrc/linear.hip:
tile_epilogue's stat_out, the STATIN kernels; tramba_linear_rowstat_cl / tramba_linear2_rowstat_cl ->
tramba_linear_ln_rowstat_cl; modules.ROW_STATS).

  A. the slab a producer leaves, per row and 64-column tile (sum, sum of squares) of the ROUNDED output, against fp64 sums of
     that output, on every form that carries the epilogue, under every fill of the uninitialised allocations;
  B. the consumer with supplied statistics on every form, under the criteria of test_layernorm_folded_into_the_gemm;
  C. producer -> consumer through the modules: a VSSBlock pair and a FreqBlockv6 against the CPU oracle, switch on and off.

Bound of A (the project's E32 rule): the error of a partial is measured relative to the largest sum of MAGNITUDES of a case
(sum |y| for S1, sum y^2 for S2: the quantity every summation-error bound is stated in, and one that does not vanish when a
row's values cancel); E32 is that measure for a numpy float32 evaluation of the same 64-term sums, left to right, and no less
than 2^-24, half an ulp of the largest sum; the slab is held to 8 x E32.  The kernel adds a lane's 8 columns left to right and
the 8 lanes of a row pairwise, so its error is of E32's size; summing the unrounded fp32 values instead of the 16-bit ones
would be off by ~2^-9 per term, three orders above the bound."""
import numpy as np
import pytest
import torch

import buffer_cases as bc
import synth
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
IDS = {BF16: "bf16", F16: "f16"}


def hip():
    from tramba_amd import hip as h
    return h


class _tuned:
    """tune_set(TUNE_GEMM_TILE, value) for the body, 0 again after it"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        hip().tune_set(hip().TUNE_GEMM_TILE, self.value)

    def __exit__(self, *exc):
        hip().tune_set(hip().TUNE_GEMM_TILE, 0)


def _rnd(seed, *shape, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# ============================================================================= A. the producer's slab
PRODUCER_M = (1, 64, 65, 130)
PRODUCER_N = (64, 128, 192, 200, 100)     # 200: a ragged last tile of 8 columns; 100: N % 8 != 0, the epilogue's scalar branch
# TUNE_GEMM_TILE values that reach a form with the new epilogue (gemm_plan): plain entry 0 = the rule (PC3 here), 7 = DMA4,
# 13 / 14 = DMA2 / DMA3, 16 / 17 = PC3 / PC4, 18 = the rule without PC (DMA3); two-source entry 0 = linear_pc_kernel<A_TWO>,
# 18 = linear_lean_kernel
PLAIN_FORMS = (0, 7, 13, 14, 16, 17, 18)
TWO_SRC_FORMS = (0, 18)
VARIANTS = ("plain", "bias_res", "bias_gelu")


def _tile_sums(y, n):
    """(M, nct, 64) float64 view of y's valid columns, zero-padded to whole 64-column tiles"""
    m = y.shape[0]
    nct = (n + 63) // 64
    pad = np.zeros((m, nct * 64), dtype=np.float64)
    pad[:, :n] = y.double().cpu().numpy()
    return pad.reshape(m, nct, 64)


def _slab_errors(y, slab, n):
    """(measure of the slab, E32) for S1 and S2, see the module docstring"""
    t = _tile_sums(y, n)
    t32 = t.astype(np.float32)                       # exact: the values are 16-bit
    out = []
    for got, terms64, terms32 in ((slab[..., 0], t, t32), (slab[..., 1], t * t, t32 * t32)):
        ref = terms64.sum(-1)
        scale = float(np.abs(terms64).sum(-1).max())
        host32 = np.add.accumulate(terms32, axis=-1, dtype=np.float32)[..., -1].astype(np.float64)
        e32 = max(float(np.abs(host32 - ref).max()) / scale, 2.0 ** -24)
        out.append((float(np.abs(got.double().cpu().numpy() - ref).max()) / scale, e32))
    return out


def _producer_run(entry, form, dtype):
    H = hip()
    res = []
    with _tuned(form):
        for m in PRODUCER_M:
            for n in PRODUCER_N:
                k = 128
                x, w = _rnd(m + n, m, k, dtype=dtype), _rnd(m + n + 1, n, k, dtype=dtype, scale=k ** -0.5)
                bias, r = _rnd(m + n + 2, n), _rnd(m + n + 3, m, n, dtype=dtype)
                for var in VARIANTS:
                    b_, r_ = (None if var == "plain" else bias), (r if var == "bias_res" else None)
                    act = H.ACT_GELU if var == "bias_gelu" else H.ACT_NONE
                    if entry == "plain":
                        y = H.linear_cl(x, w, b_, r_, act, rowstat=True)
                    else:
                        y = H.linear2_cl(x[:, :64].contiguous(), x[:, 64:].contiguous(), w, b_, r_, act, rowstat=True)
                    tag = getattr(y, "_tramba_rowstat", None)
                    assert tag is not None, (entry, form, m, n, var)      # every forced form here can emit
                    assert tuple(tag[0].shape) == (m, (n + 63) // 64, 2) and tag[1] == y._version
                    res += [y, tag[0]]
    return res


@pytest.mark.parametrize("dtype", [BF16, F16], ids=IDS.values())
@pytest.mark.parametrize("entry,form", [("plain", f) for f in PLAIN_FORMS] + [("two_src", f) for f in TWO_SRC_FORMS])
def test_slab_against_fp64_sums_of_the_rounded_output(entry, form, dtype):
    """M in {1, 64, 65, 130} x N in {64, 128, 192, 200, 100}, with and without bias / residual / GELU: every partial within
    8 x E32 of the fp64 sum of the output as stored; y itself bit-identical to the call without the slab; and y and the slab
    finite and bit-identical under NaN, zero and noise fills of every uninitialised allocation (rows at or above M and the
    allocator's slack reach nothing)."""
    H = hip()
    base = bc.check_independent(lambda: _producer_run(entry, form, dtype), what=f"row-stat slab {entry} form {form} {dtype}")
    it = iter(base)
    worst = [0.0, 0.0]
    with _tuned(form):
        for m in PRODUCER_M:
            for n in PRODUCER_N:
                k = 128
                x, w = _rnd(m + n, m, k, dtype=dtype), _rnd(m + n + 1, n, k, dtype=dtype, scale=k ** -0.5)
                bias, r = _rnd(m + n + 2, n), _rnd(m + n + 3, m, n, dtype=dtype)
                for var in VARIANTS:
                    y, slab = next(it), next(it)
                    b_, r_ = (None if var == "plain" else bias), (r if var == "bias_res" else None)
                    act = H.ACT_GELU if var == "bias_gelu" else H.ACT_NONE
                    if entry == "plain":
                        y0 = H.linear_cl(x, w, b_, r_, act)
                    else:
                        y0 = H.linear2_cl(x[:, :64].contiguous(), x[:, 64:].contiguous(), w, b_, r_, act)
                    assert torch.equal(y0.cpu(), y), (m, n, var)
                    for q, (err, e32) in enumerate(_slab_errors(y, slab, n)):
                        worst[q] = max(worst[q], err / e32)
                        assert err <= 8.0 * e32, (entry, form, m, n, var, "S1S2"[2 * q:2 * q + 2], err, e32)
    print(f"slab {entry} form {form} {IDS[dtype]}: worst error / E32: S1 {worst[0]:.2f}, S2 {worst[1]:.2f}")


def test_forms_that_cannot_emit_return_no_statistics():
    """the weight-stationary form, an fp32 output and a K that is no multiple of 64 (linear_tiled_kernel) leave the call as it
    was: same bits, no slab on the tensor"""
    H = hip()
    x, w = _rnd(1, 100, 128, dtype=BF16), _rnd(2, 128, 128, dtype=BF16, scale=128 ** -0.5)
    with _tuned(19):
        y, y0 = H.linear_cl(x, w, rowstat=True), H.linear_cl(x, w)
    assert not hasattr(y, "_tramba_rowstat") and torch.equal(y, y0)
    y, y0 = H.linear_cl(x, w, out_dtype=torch.float32, rowstat=True), H.linear_cl(x, w, out_dtype=torch.float32)
    assert not hasattr(y, "_tramba_rowstat") and torch.equal(y, y0)
    x, w = _rnd(3, 100, 72, dtype=BF16), _rnd(4, 128, 72, dtype=BF16, scale=72 ** -0.5)
    y, y0 = H.linear_cl(x, w, rowstat=True), H.linear_cl(x, w)
    assert not hasattr(y, "_tramba_rowstat") and torch.equal(y, y0)
    xf = x.float()
    assert not hasattr(H.linear_cl(xf, w.float(), rowstat=True), "_tramba_rowstat")


# ============================================================================= B. the consumer with supplied statistics
CONSUMER_FORMS = (0, 13, 14, 16, 17, 18)      # the rule, DMA2, DMA3, PC3, PC4, the rule without PC


@pytest.mark.parametrize("dtype", [BF16, F16], ids=IDS.values())
@pytest.mark.parametrize("k", [64, 128, 192, 512])
def test_consumer_with_supplied_statistics(k, dtype):
    """the construction and the criteria of test_layernorm_folded_into_the_gemm (rows with a +6.0 mean included) with the row
    partials supplied: 64-term fp32 sums of the rounded input, made on the host.  Every form: within 2e-2 / 3e-3 of the
    scale of the fp64 result, no worse than 2 x the two-launch path + 1e-3 of the scale, and the same against the
    self-derived statistics of the same form."""
    H = hip()
    import tramba_amd as ta
    from tramba_amd.modules import _fold_layernorm
    for m in PRODUCER_M:
        for n in (8, 72, 136):
            act, res = (2 if n != 8 else 0), n == 136
            g = torch.Generator().manual_seed(m + n + k)
            x = torch.randn(m, k, generator=g) * 1.3 + 0.2
            x[::7] += 6.0
            x = x.to(DEV, dtype)
            lin, norm = ta.Linear2d(k, n, bias=True).to(DEV), ta.LayerNorm2d(k).to(DEV)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(n, k, generator=g) * k ** -0.5)
                lin.bias.copy_(0.1 * torch.randn(n, generator=g))
                norm.weight.copy_(1 + 0.2 * torch.randn(k, generator=g))
                norm.bias.copy_(0.1 * torch.randn(k, generator=g))
            r = torch.randn(m, n, generator=g).to(DEV, dtype) if res else None
            wf, cs, tb = _fold_layernorm(lin, norm, dtype)
            xd = x.double().cpu()
            want = torch.nn.functional.layer_norm(xd, (k,), norm.weight.double().cpu(), norm.bias.double().cpu(), norm.eps) \
                @ lin.weight.double().cpu().t() + lin.bias.double().cpu()
            if act == 2:
                want = torch.nn.functional.gelu(want)
            if res:
                want = want + r.double().cpu()
            two = H.linear_cl(H.layernorm_cl(x, norm.weight.detach(), norm.bias.detach(), norm.eps),
                              lin.weight.detach().to(dtype), lin.bias.detach(), r, act).double().cpu()
            x64 = x.float().cpu().view(m, k // 64, 64)
            slab = torch.stack((x64.sum(-1), (x64 * x64).sum(-1)), -1).contiguous().to(DEV)
            scale = float(want.abs().max())
            tol = (2e-2 if dtype == BF16 else 3e-3) * scale
            e_two = float((two - want).abs().max())
            for form in CONSUMER_FORMS:
                with _tuned(form):
                    got = H.linear_ln_cl(x, wf, cs, tb, norm.eps, r, act, rowstat=slab).double().cpu()
                    own = H.linear_ln_cl(x, wf, cs, tb, norm.eps, r, act).double().cpu()
                e, e_own = float((got - want).abs().max()), float((own - want).abs().max())
                assert e <= tol, (m, n, k, form, e, e_two, scale)
                assert e <= 2.0 * e_two + 1e-3 * scale, (m, n, k, form, e, e_two)
                assert e <= 2.0 * e_own + 1e-3 * scale, (m, n, k, form, e, e_own)


def test_a_slab_of_the_wrong_shape_is_refused():
    H = hip()
    x, w = _rnd(5, 65, 128, dtype=BF16), _rnd(6, 72, 128, dtype=BF16, scale=128 ** -0.5)
    cs, tb = w.float().sum(1).contiguous(), _rnd(7, 72)
    for shape in ((65, 1, 2), (64, 2, 2), (65, 2)):
        with pytest.raises(H.TrambaHipError, match="rowstat"):
            H.linear_ln_cl(x, w, cs, tb, 1e-5, rowstat=torch.zeros(shape, device=DEV))


# ============================================================================= C. producer -> consumer through the modules
def _load(module):
    sd = module.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    new.update({k: v for k, v in sd.items() if k not in new})
    module.load_state_dict(new, strict=True)
    return module


def _chain(kind):
    import tramba_amd as ta
    if kind == "freq":
        return [_load(ta.FreqBlockv6(dim=64, input_resolution=(24, 24)))], (1, 64, 24, 24), om.freq_block
    side = 24 if kind == "vss24" else 12
    return ([_load(ta.VSSBlock(hidden_dim=64, drop_path=0.0, channel_first=True)) for _ in range(2)], (1, 64, side, side),
            om.vss_block)


@pytest.fixture(scope="module", params=["vss24", "vss12", "freq"])
def chain(request):
    """the blocks (fp32, on the host), their input and the CPU oracle's fp32 output, computed once"""
    blocks, shape, oracle = _chain(request.param)
    x = synth.synth_input("lnstats_" + request.param, shape)
    want = x
    with torch.no_grad():
        for b in blocks:
            want = oracle(om.SD({k: v.detach().cpu() for k, v in b.state_dict().items()}), want)
    return request.param, blocks, x, want


def _err_stats(got, want):
    """test_gpu_model._err_stats: max-abs and RMS error relative to the RMS of the reference map"""
    d = got.double() - want.double()
    ref = float(want.double().square().mean().sqrt())
    return float(d.abs().max()) / ref, float(d.square().mean().sqrt()) / ref


@pytest.mark.parametrize("dtype", [BF16, F16], ids=IDS.values())
def test_chain_against_the_oracle_with_the_switch_on_and_off(chain, dtype):
    """16-bit inference through the modules: within the tolerance of test_block_inference_low_precision_against_reference_golden
    of the oracle with modules.ROW_STATS on and off, bitwise equal run to run with it on, and the supplied statistics are in
    fact used where a producer precedes the LayerNorm (VSSBlock pair: norm2 -> fc1 of both blocks and norm -> in_proj of the
    second; FreqBlockv6: none yet -- its attention output is added by the framework)."""
    import copy
    import tramba_amd as ta
    from tramba_amd import modules as M
    H = hip()
    kind, blocks, x, want = chain
    blocks = [copy.deepcopy(b).to(DEV).eval() for b in blocks]
    for b in blocks:
        for mod in b.modules():            # the prepare_inference policy on a bare block (test_gpu_model.py)
            if isinstance(mod, ta.Linear2d):
                mod.weight.data = mod.weight.data.to(dtype)
            elif isinstance(mod, ta.SS2D):
                mod.x_proj_weight.data = mod.x_proj_weight.data.to(dtype)
    supplied = []
    orig = H.linear_ln_cl

    def spy(*a, **kw):
        supplied.append((kw.get("rowstat") if "rowstat" in kw else (a[8] if len(a) > 8 else None)) is not None)
        return orig(*a, **kw)

    def run():
        y = M.to_cl(x.to(DEV, dtype))          # the blocks of a stage hand the channels-last map on as it is (models.py)
        with torch.no_grad():
            for b in blocks:
                y = b._forward_cl(y)
        return M.from_cl(y).float().cpu()
    outs = {}
    H.linear_ln_cl = spy
    try:
        for on in (True, False):
            M.ROW_STATS = on
            del supplied[:]
            outs[on] = run()
            if on and kind != "freq":
                assert supplied == [False, True, True, True], (kind, supplied)
            else:
                assert supplied and not any(supplied), (kind, on, supplied)
        M.ROW_STATS = True
        again = run()
    finally:
        H.linear_ln_cl = orig
        M.ROW_STATS = True
    assert torch.equal(again, outs[True])
    tmax, trms = (0.08, 0.012) if dtype == BF16 else (0.01, 0.0015)
    for on in (True, False):
        emax, erms = _err_stats(outs[on], want)
        print(f"{kind} {IDS[dtype]} ROW_STATS={on}: max {emax:.4f} rms {erms:.5f} of the oracle map's RMS")
        assert emax <= tmax and erms <= trms, (kind, on, emax, erms)


def test_a_slab_that_does_not_fit_the_consumer_is_not_read():
    """Linear2d._forward_norm_cl falls back to deriving its own statistics, bit for bit, when the tensor carries a slab whose
    partial count is not K / 64, or one made before the tensor was written to again"""
    import tramba_amd as ta
    H = hip()
    m, k, n = 130, 128, 72
    lin, norm = ta.Linear2d(k, n, bias=True).to(DEV).to(BF16), ta.LayerNorm2d(k).to(DEV)
    w0 = _rnd(8, k, k, dtype=BF16, scale=k ** -0.5)
    with torch.no_grad():
        x = H.linear_cl(_rnd(9, m, k, dtype=BF16), w0, None, _rnd(10, m, k, dtype=BF16), rowstat=True)
        slab, version = x._tramba_rowstat
        assert H.rowstat_for(x, k) is slab and tuple(slab.shape) == (m, 2, 2)
        plain = x.clone()                                                     # (a new tensor object: no slab)
        assert H.rowstat_for(plain, k) is None
        want = lin._forward_norm_cl(plain, norm)
        with_stats = lin._forward_norm_cl(x, norm)
        assert float((with_stats.float() - want.float()).abs().max()) <= 2e-2 * float(want.float().abs().max())
        # a slab with one partial per row (as for K = 64) on a K = 128 input; poisoned, so that reading it would show
        x._tramba_rowstat = (torch.full((m, 1, 2), float("nan"), device=DEV), x._version)
        assert H.rowstat_for(x, k) is None and torch.equal(lin._forward_norm_cl(x, norm), want)
        # the right shape, but x was written to after the producer
        x._tramba_rowstat = (torch.full((m, 2, 2), float("nan"), device=DEV), version)
        x.add_(0)
        assert H.rowstat_for(x, k) is None and torch.equal(lin._forward_norm_cl(x, norm), want)
