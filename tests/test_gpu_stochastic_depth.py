"""GPU tests of stochastic depth on the training path: the residual-stream kernels with a per-sample mask
(tramba_add_layernorm_cl, tramba_layernorm_bwd_res_cl and its dxm output), the autograd glue around them
(_AddLayerNormCL, _AddMaskedF32, _AddMasked, the deferred add between blocks), whole blocks in train() mode against the
oracle, and the captured training step's fresh draw per replay.

RNG streams are never compared with the reference: every test either injects the masks (_InjectedPool) or
reads back the masks the device drew and hands those same masks to the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from oracle import model as om
from oracle import ops as oo

pytestmark = pytest.mark.gpu
DEV = "cuda"

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# per-sample mask values: distinct (an off-by-one sample index cannot hide behind a {0, 1/keep} pattern), one of them 0
MASK_VALUES = [2.0, 0.0, 1.25, 0.5]


def hip():
    from tramba_amd import hip as h
    return h


def _masks(b):
    return torch.tensor((MASK_VALUES * b)[:b] if b > 1 else [0.5], dtype=F32)


def _sample_rows(b, rows):
    """the sample of every row of a (b * rows_per_sample, C) map"""
    return torch.arange(b).repeat_interleave(rows // b)


def _ulp(ref, dtype):
    """one unit in the last place of `dtype` at the fp64 values `ref` (subnormals: the fixed spacing below tiny)"""
    fi = torch.finfo(dtype)
    return fi.eps * torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(fi.tiny))))


def _act(act):
    h = hip()
    return {h.ACT_NONE: lambda t: t, h.ACT_GELU: F.gelu, h.ACT_SILU: F.silu}[act]


# ------------------------------------------------------------------------------------------------ kernels
# tramba_add_layernorm_cl: rows form when C % VM == 0, C / VM <= 64 and w / b 16-byte aligned (VM = 4 fp32, 8 16-bit),
# the wave form otherwise
ADD_LN_CASES = ([(F32, c) for c in (4, 12, 128, 256)] + [(F32, c) for c in (7, 260, 512, 1024, 2048)]
                + [(t, c) for t in (BF16, F16) for c in (8, 24, 200, 512)]
                + [(t, c) for t in (BF16, F16) for c in (6, 7, 20, 520, 1024, 2048)])


def _check_add_ln(dtype, c, w, b, g):
    h = hip()
    tol = 1e-5 if dtype == F32 else 2e-2
    for bsz, hh, ww in ((1, 7, 9), (3, 12, 12), (4, 7, 9)):      # 63 rows per sample: boundaries inside waves / workgroups
        x = (torch.randn(bsz, hh, ww, c, generator=g) * 1.5 + 0.3).to(dtype)
        y = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
        m = _masks(bsz)
        for with_y, with_m, act in ((False, False, h.ACT_NONE), (True, False, h.ACT_NONE), (True, True, h.ACT_NONE),
                                    (True, True, h.ACT_GELU), (True, True, h.ACT_SILU), (False, False, h.ACT_GELU)):
            dual = act != h.ACT_NONE
            xs, n, na = h.add_layernorm_cl(x.to(DEV), y.to(DEV) if with_y else None, m.to(DEV) if with_m else None,
                                           w.to(DEV), b.to(DEV), 1e-5, act, dual=dual)
            what = (dtype, c, bsz, with_y, with_m, act)
            if with_y:
                ref = x.double() + y.double() * (m.double().view(-1, 1, 1, 1) if with_m else 1.0)
                got = xs.cpu()
                assert got.dtype == dtype
                err = (got.double() - ref).abs()
                assert bool((err <= _ulp(ref, dtype)).all()), (what, float(err.max()))
                if with_m:
                    drop = (m == 0).nonzero().flatten()
                    assert len(drop) == 0 or torch.equal(got[drop], x[drop]), what
                base = got
            else:
                assert xs is None
                base = x
            want = F.layer_norm(base.double(), (c,), w.double(), b.double(), 1e-5)
            got_n = n.cpu()
            np.testing.assert_allclose(got_n.double().numpy(), want.numpy(), rtol=tol, atol=tol, err_msg=str(what))
            if dual:
                want_a = _act(act)(got_n.double())                 # the activation of n AS STORED
                np.testing.assert_allclose(na.cpu().double().numpy(), want_a.numpy(), rtol=tol, atol=tol, err_msg=str(what))
            else:
                assert na is None


@pytest.mark.parametrize("dtype,c", ADD_LN_CASES)
def test_add_layernorm_masked_against_fp64(dtype, c):
    """x' = x + y * mask[sample] within one ulp of the fp64 sum, dropped samples bit-equal to x, n = LayerNorm(x' as stored)
    and act(n as stored), every dispatch form, four distinct per-sample mask values"""
    g = torch.Generator().manual_seed(c * 7 + {F32: 0, BF16: 1, F16: 2}[dtype])
    w, b = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    _check_add_ln(dtype, c, w, b, g)


@pytest.mark.parametrize("dtype,c", [(F32, 128), (BF16, 200)])
def test_add_layernorm_unaligned_params_take_the_wave_form(dtype, c):
    """a rows-form C with w / b views 4 bytes past a 16-byte boundary: the dispatcher must fall back to the wave form"""
    g = torch.Generator().manual_seed(c)
    wb = torch.randn(2, c + 1, generator=g)
    wfull, bfull = (1 + 0.1 * wb[0]).to(DEV), (0.1 * wb[1]).to(DEV)
    w, b = wfull[1:], bfull[1:]
    assert w.data_ptr() % 16 != 0 and b.data_ptr() % 16 != 0
    h = hip()
    x = torch.randn(4, 7, 9, c, generator=g).to(dtype)
    y = torch.randn(4, 7, 9, c, generator=g).to(dtype)
    m = _masks(4)
    xs, n, _ = h.add_layernorm_cl(x.to(DEV), y.to(DEV), m.to(DEV), w, b, 1e-5, h.ACT_NONE)
    ref = x.double() + y.double() * m.double().view(-1, 1, 1, 1)
    assert bool(((xs.cpu().double() - ref).abs() <= _ulp(ref, dtype)).all())
    want = F.layer_norm(xs.cpu().double(), (c,), w.cpu().double(), b.cpu().double(), 1e-5)
    tol = 1e-5 if dtype == F32 else 2e-2
    np.testing.assert_allclose(n.cpu().double().numpy(), want.numpy(), rtol=tol, atol=tol)


# tramba_layernorm_bwd_res_cl: rows form (C % VM == 0, C <= 64 VM), wide form (16-bit, C % 8 == 0, 512 < C <= 2048),
# generic form (everything else).  `big`: 3 x 83 x 89 = 22161 rows, 5 rows per wave (above the floors of 4 / 2), which do not
# divide the row count
LN_BWD_CASES = ([(F32, c, False) for c in (4, 256)] + [(F32, 64, True)]                                  # rows
                + [(t, c, False) for t in (BF16, F16) for c in (8, 512)] + [(BF16, 200, True)]           # rows
                + [(t, c, False) for t in (BF16, F16) for c in (520, 1024, 1536, 2048)]                  # wide
                + [(F32, c, False) for c in (260, 512, 1024, 2048)]                                      # generic
                + [(t, c, False) for t in (F32, BF16, F16) for c in (6, 7)] + [(t, 20, False) for t in (BF16, F16)]
                + [(F16, 7, True)])


def _ln_ref(x, dy, w, b, gres):
    """fp64 autograd of LayerNorm plus the skip connection's gradient"""
    c = x.shape[-1]
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.layer_norm(xr, (c,), wr, br, 1e-5).backward(dy.double())
    dx = xr.grad if gres is None else xr.grad + gres.double()
    return dx, wr.grad, br.grad


@pytest.mark.parametrize("dtype,c,big", LN_BWD_CASES)
def test_layernorm_bwd_res_masked_against_fp64(dtype, c, big):
    """dx (+ gres) against fp64 autograd; dxm == (dx * mask[sample]) rounded once, bit for bit, and exactly 0 for a
    dropped sample; dw / db against fp64, and bit-equal when the slab sums are deferred"""
    h = hip()
    g = torch.Generator().manual_seed(c * 3 + int(big) + {F32: 0, BF16: 10, F16: 20}[dtype])
    bsz, hh, ww = (3, 83, 89) if big else (3, 7, 9)
    rows = bsz * hh * ww
    x = (torch.randn(bsz, hh, ww, c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
    gres = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    m = _masks(bsz)
    sample = _sample_rows(bsz, rows).view(bsz, hh, ww, 1)
    tol = 2e-5 if dtype == F32 else 3e-2
    ptol = 1e-4 if dtype == F32 else 3e-2
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    refs = {}
    for with_g in (False, True):
        refs[with_g] = _ln_ref(x, dy, w, b, gres if with_g else None)
        for with_m in (False, True):
            dx, dxm, dw, db = h.layernorm_bwd_res_cl(xd, dyd, wd, 1e-5, gres=gres.to(DEV) if with_g else None,
                                                     mask=m.to(DEV) if with_m else None, want_masked=with_m)
            what = (dtype, c, rows, with_g, with_m)
            dx_ref, dw_ref, db_ref = refs[with_g]
            dx = dx.cpu()
            np.testing.assert_allclose(dx.double().numpy(), dx_ref.numpy(), rtol=tol, atol=tol, err_msg=str(what))
            np.testing.assert_allclose(dw.cpu().double().numpy(), dw_ref.numpy(), rtol=ptol,
                                       atol=ptol * float(dw_ref.abs().max()), err_msg=str(what))
            np.testing.assert_allclose(db.cpu().double().numpy(), db_ref.numpy(), rtol=ptol,
                                       atol=ptol * float(db_ref.abs().max()), err_msg=str(what))
            if with_m:
                want = (dx.float() * m[sample]).to(dtype)
                got = dxm.cpu()
                assert torch.equal(got, want), (what, int((got != want).sum()))
                assert bool((got[m == 0] == 0).all()), what
            else:
                assert dxm is None
    # deferred slab sums: recorded inside the context, run at its exit -- the same sums in the same order
    _, _, dw0, db0 = h.layernorm_bwd_res_cl(xd, dyd, wd, 1e-5, gres=gres.to(DEV), mask=m.to(DEV), want_masked=True)
    with h.deferred_sums():
        _, _, dw1, db1 = h.layernorm_bwd_res_cl(xd, dyd, wd, 1e-5, gres=gres.to(DEV), mask=m.to(DEV), want_masked=True,
                                                defer=True)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


@pytest.mark.parametrize("dtype,c,p", [(F32, 16, 2), (F32, 64, 4), (BF16, 24, 2), (BF16, 520, 2), (F16, 1024, 2),
                                       (F32, 512, 2), (F32, 7, 2), (BF16, 6, 4), (F16, 20, 2)])
def test_shuffle_norm_bwd_against_fp64(dtype, c, p):
    """the same dispatcher with P > 1 (dy indexed by the shuffled row): rows, wide and generic forms, odd H and W"""
    h = hip()
    g = torch.Generator().manual_seed(c * p)
    bsz, hh, ww = 2, 5, 3
    x = (torch.randn(bsz, hh, ww, p * p * c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(bsz, hh * p, ww * p, c, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = oo.layernorm2d(oo.pixel_shuffle_groups(xr, p), wr, br)
    yr.backward(dy.double().permute(0, 3, 1, 2))
    dx, dw, db = h.shuffle_norm_bwd_cl(x.to(DEV), dy.to(DEV), w.to(DEV), p)
    tol = 2e-5 if dtype == F32 else 3e-2
    ptol = 1e-4 if dtype == F32 else 3e-2
    np.testing.assert_allclose(dx.cpu().double().numpy(), xr.grad.permute(0, 2, 3, 1).numpy(), rtol=tol, atol=tol)
    np.testing.assert_allclose(dw.cpu().double().numpy(), wr.grad.numpy(), rtol=ptol, atol=ptol * float(wr.grad.abs().max()))
    np.testing.assert_allclose(db.cpu().double().numpy(), br.grad.numpy(), rtol=ptol, atol=ptol * float(br.grad.abs().max()))


# ------------------------------------------------------------------------------------------------ autograd Functions
AUTOGRAD_CASES = {
    # name: (y given, mask given, act, y requires grad, xs used, n used)
    "no_y_passthrough": (False, False, "none", False, True, True),
    "y_no_mask": (True, False, "none", True, True, True),
    "y_mask_gelu_dual": (True, True, "gelu", True, True, True),
    "y_detached": (True, True, "none", False, True, True),
    "only_xs_used": (True, True, "none", True, True, False),
    "only_n_used": (True, True, "none", True, False, True),
}


def _add_ln_function(dtype, case, deferred):
    from tramba_amd import modules as M
    h = hip()
    with_y, with_m, act, y_grad, use_xs, use_n = AUTOGRAD_CASES[case]
    act = {"none": h.ACT_NONE, "gelu": h.ACT_GELU}[act]
    g = torch.Generator().manual_seed(len(case))
    bsz, hh, ww, c = 4, 7, 9, 24
    x = (torch.randn(bsz, hh, ww, c, generator=g) * 1.5 + 0.3).to(dtype)
    y = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    r1 = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
    r2 = torch.randn(bsz, hh, ww, c, generator=g).to(dtype)
    m = _masks(bsz)
    xg = x.to(DEV).requires_grad_(True)
    yg = y.to(DEV).requires_grad_(y_grad) if with_y else None
    wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    xs, n, na = M._AddLayerNormCL.apply(xg, yg, m.to(DEV) if with_m else None, wg, bg, 1e-5, act, True)
    loss = 0
    if use_xs:
        loss = loss + (xs.float() * r1.to(DEV).float()).sum()
    if use_n:
        loss = loss + (n.float() * r2.to(DEV).float()).sum()
    if deferred:
        with h.deferred_sums():
            loss.backward()
    else:
        loss.backward()
    got = {"x": xg.grad, "w": wg.grad, "b": bg.grad, "y": yg.grad if with_y else None, "na": na, "n": n}
    # fp64 reference
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    xsr = xr + yr * (m.double().view(-1, 1, 1, 1) if with_m else 1.0) if with_y else xr
    nr = F.layer_norm(xsr, (c,), wr, br, 1e-5)
    lr = 0
    if use_xs:
        lr = lr + (xsr * r1.double()).sum()
    if use_n:
        lr = lr + (nr * r2.double()).sum()
    lr.backward()
    want = {"x": xr.grad, "w": wr.grad if use_n else None, "b": br.grad if use_n else None,
            "y": yr.grad if (with_y and y_grad) else None}
    return got, want, act


@pytest.mark.parametrize("case", list(AUTOGRAD_CASES))
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_add_layernorm_function_against_fp64_autograd(dtype, case):
    """_AddLayerNormCL: the gradients of x, y, w and b of <x', r1> + <n, r2> against fp64 autograd, in every branch of its
    backward, with fp32 w / b, outside and inside deferred_sums() (bit-equal)"""
    tol = 1e-4 if dtype == F32 else 3e-2
    got0, want, act = _add_ln_function(dtype, case, deferred=False)
    got1, _, _ = _add_ln_function(dtype, case, deferred=True)
    for k in ("x", "y", "w", "b"):
        if want[k] is None:
            assert got0[k] is None or not bool(got0[k].any()), (case, k)
            continue
        a = got0[k].cpu().double()
        np.testing.assert_allclose(a.numpy(), want[k].numpy(), rtol=tol, atol=tol * float(want[k].abs().max()),
                                   err_msg=f"{case} {k}")
        assert torch.equal(got0[k], got1[k]), (case, k)
    if act != hip().ACT_NONE:
        np.testing.assert_allclose(got0["na"].detach().cpu().double().numpy(),
                                   F.gelu(got0["n"].detach().cpu().double()).numpy(), rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_add_masked_functions_against_fp64(dtype):
    """the stage-end add (_AddMaskedF32, (B) fp32 mask) and the non-fused path's add (_AddMasked, mask broadcast in the
    activation dtype): x + y * m[sample], gx = g, gy = g * m[sample]"""
    from tramba_amd import modules as M
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 5, 6, 16, generator=g).to(dtype)
    y = torch.randn(4, 5, 6, 16, generator=g).to(dtype)
    gy = torch.randn(4, 5, 6, 16, generator=g).to(dtype)
    m = _masks(4)
    tol = 1e-6 if dtype == F32 else 1e-2
    for fn, mask in ((M._AddMaskedF32, m.to(DEV)), (M._AddMasked, m.to(DEV, dtype).view(-1, 1, 1, 1))):
        xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
        out = fn.apply(xg, yg, mask)
        out.backward(gy.to(DEV))
        md = m.double().view(-1, 1, 1, 1)
        pairs = ((out.detach(), x.double() + y.double() * md), (xg.grad, gy.double()), (yg.grad, gy.double() * md))
        for got, want in pairs:
            np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=tol, atol=tol, err_msg=fn.__name__)
        assert bool((yg.grad[m.to(DEV) == 0] == 0).all()) and torch.equal(out[1].cpu(), x[1]), fn.__name__


# ------------------------------------------------------------------------------------------------ blocks, masks injected
class _InjectedPool:
    """Stands in for modules._MaskPool: the k-th use of a DropPath in a forward gets rows[(name, k)] ((B) fp32), in the
    activation dtype or as the fp32 row the fused residual kernels read -- exactly what the real table hands out."""

    def __init__(self, rows, names):
        self.rows, self.names, self.count, self.taken = rows, names, {}, []

    def begin_step(self):
        pass

    def forget_draw(self):
        pass

    def take(self, mod, keep, batch, dtype, device, want_f32=False):
        name = self.names[id(mod)]
        k = self.count.get(name, 0)
        self.count[name] = k + 1
        row = self.rows[(name, k)]
        assert row.shape == (batch,)
        self.taken.append((name, k))
        return row.to(device=device, dtype=F32 if want_f32 else dtype)


def _install(model, rows):
    """hand every DropPath under `model` (and the model itself, for the models' begin_step) one injected pool"""
    import tramba_amd as ta
    names = {id(m): n for n, m in model.named_modules() if isinstance(m, ta.DropPath)}
    pool = _InjectedPool(rows, names)
    for m in model.modules():
        if isinstance(m, ta.DropPath):
            m.__dict__["_pool"] = pool
    model.__dict__["_tramba_mask_pool"] = pool
    return pool


def _block_cases():
    import tramba_amd as ta
    from tramba_amd import modules as M

    class MyScan(ta.CrossScan):                     # a user's scan plugin (raster, with its backward): no built-in
        _tramba_family = None                       # family, so the SS2D leaves the fused path

    class MyMerge(ta.CrossMerge):
        _tramba_family = None

    def plugin_block():
        blk = ta.VSSBlock(hidden_dim=16, drop_path=0.3, channel_first=True)
        blk.op = ta.SS2D(d_model=16, d_state=1, channel_first=True, scan=MyScan, merge=MyMerge)
        return blk

    def two_blocks():
        return torch.nn.Sequential(ta.VSSBlock(hidden_dim=16, drop_path=0.2, channel_first=True),
                                   ta.VSSBlock(hidden_dim=16, drop_path=0.5, channel_first=True))

    def run_two(mod, x):
        return M.from_cl(M._run_blocks(list(mod), M.to_cl(x)))

    def oracle_two(sd, x, masks):
        s = om.SD(sd)
        mm = (None, None) if masks is None else masks
        x = om.vss_block(s.sub("0"), x, None if masks is None else (mm[("0.drop_path", 0)], mm[("0.drop_path", 1)]))
        return om.vss_block(s.sub("1"), x, None if masks is None else (mm[("1.drop_path", 0)], mm[("1.drop_path", 1)]))

    def one(fn):
        return lambda sd, x, masks: fn(om.SD(sd), x, None if masks is None else (masks[("drop_path", 0)],
                                                                                  masks[("drop_path", 1)]))

    keep7 = 1 / 0.7
    return {
        # name: (constructor, input shape, run, oracle, {(DropPath name, use): (B) mask}, SS2D expected on the fused path)
        "vss16_distinct": (lambda: ta.VSSBlock(hidden_dim=16, drop_path=0.3, channel_first=True), (4, 16, 12, 12),
                           None, one(om.vss_block),
                           {("drop_path", 0): [2.0, 0.0, 1.25, 0.5], ("drop_path", 1): [0.5, 1.25, 0.0, 2.0]}, True),
        "helix16": (lambda: ta.MultiScaleDecoderBlock(hidden_dim=16, drop_path=0.3, channel_first=True), (4, 16, 12, 12),
                    None, one(om.multiscale_decoder_block),
                    {("drop_path", 0): [keep7, 0.0, keep7, keep7], ("drop_path", 1): [0.0, keep7, keep7, 0.0]}, True),
        "vss1024": (lambda: ta.VSSBlock(hidden_dim=1024, drop_path=0.5, channel_first=True), (2, 1024, 12, 12),
                    None, one(om.vss_block), {("drop_path", 0): [2.0, 0.0], ("drop_path", 1): [0.0, 2.0]}, True),
        "two_vss16": (two_blocks, (3, 16, 12, 12), run_two, oracle_two,
                      {("0.drop_path", 0): [1.25, 0.0, 1.25], ("0.drop_path", 1): [0.0, 1.25, 1.25],
                       ("1.drop_path", 0): [2.0, 2.0, 0.0], ("1.drop_path", 1): [0.0, 2.0, 2.0]}, True),
        "vss16_plugin": (plugin_block, (4, 16, 12, 12), None, one(om.vss_block),
                         {("drop_path", 0): [0.5, 2.0, 0.0, 1.25], ("drop_path", 1): [1.25, 0.0, 2.0, 0.5]}, False),
    }


BLOCK_CASES = ["vss16_distinct", "helix16", "vss1024", "two_vss16", "vss16_plugin"]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", BLOCK_CASES)
def test_block_train_mode_with_injected_masks_against_oracle(case, dtype):
    """blocks in train() mode with drop_path > 0 and prescribed per-sample masks: the output, the input gradient and every
    parameter gradient against autograd through the fp64 oracle given the same masks (bounds of
    test_block_parameter_gradients_elementwise_against_oracle_autograd); the oracle's gradients without masks must miss the
    bound by 10x on some branch parameter, so that the case can tell a right mask from a wrong one"""
    from test_gpu_grad import _oracle_grads, _rel_l2
    from test_gpu_model import _load_synth
    ctor, shape, run, oracle, rows, fused = _block_cases()[case]
    m = _load_synth(ctor()).train()
    rows = {k: torch.tensor(v, dtype=F32) for k, v in rows.items()}
    pool = _install(m, rows)
    x = synth.synth_input("sd_" + case, shape)
    xin = x.to(DEV).to(dtype).requires_grad_()
    x = xin.detach().float().cpu()
    y = run(m, xin) if run is not None else m(xin)
    assert sorted(pool.taken) == sorted(rows), pool.taken              # every injected row was read, each once
    ops = [mod for mod in m.modules() if type(mod).__name__ == "SS2D"]
    assert all(o._train_path_ok(xin) == fused for o in ops)
    gy = synth.synth_input("sd_gy_" + case, tuple(y.shape))
    params = list(m.named_parameters())
    grads = torch.autograd.grad(y, [xin] + [p for _, p in params], gy.to(DEV).to(y.dtype))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    masks64 = {k: v.double() for k, v in rows.items()}
    gx_ref, gp_ref, y_ref = _oracle_grads(lambda s, xx: oracle(s, xx, masks64), sd, x, gy=gy)
    _, gp_none, _ = _oracle_grads(lambda s, xx: oracle(s, xx, None), sd, x, gy=gy)

    def err(g, ref):
        if dtype == F32:
            return float((g.double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        return _rel_l2(g, ref)

    bound = 2e-3 if dtype == F32 else 6e-2
    out = [("output", y.detach(), y_ref.detach()), ("input", grads[0], gx_ref)]
    out += [(n, g, gp_ref[n]) for (n, _), g in zip(params, grads[1:])]
    bad = {}
    for name, g, ref in out:
        assert g.shape == ref.shape, name
        e = err(g, ref)
        if e > bound:
            bad[name] = e
    assert not bad, bad
    branch = [n for n, _ in params if ".op." in "." + n or ".mlp." in "." + n]
    assert branch
    blind = {n: err(gp_none[n], gp_ref[n]) for n in branch if float(gp_ref[n].abs().max()) > 0}
    assert blind and max(blind.values()) >= 10 * bound, sorted(blind.items(), key=lambda t: -t[1])[:4]


# ------------------------------------------------------------------------------------------------ the captured step
# max |replay - eager| / max |eager| over every parameter gradient: measured 0 on an MI355X (the replay and the eager step
# are bit-identical); the same comparison with the other replay's masks measured 32
REPLAY_BOUND = 0.0


def _eager_grads(state, table_rows, x, y):
    """gradients of one eager training step of Tramba-V loaded from `state`, stochastic depth fed `table_rows`"""
    import tramba_amd as ta
    from tramba_amd import train
    m = ta.bulid_model(use_pretrain=False, img_size=384).to(DEV).train()
    m.load_state_dict(state)
    m.compute_dtype = BF16
    pool = _install(m, table_rows)
    opt = train.get_opt(1e-4, m)
    train.train_step(m, opt, x, y)
    assert sorted(pool.taken) == sorted(table_rows)
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _grad_gap(got, want):
    assert got.keys() == want.keys()
    return max(float((got[n].double() - want[n].double()).abs().max()) / max(float(want[n].double().abs().max()), 1e-30)
               for n in want if float(want[n].abs().max()) > 0)


def test_graphed_train_step_draws_fresh_masks_per_replay():
    """GraphedTrainStep on Tramba-V 384 (bf16, the model's own drop-path rates): the stochastic-depth table is drawn INSIDE
    the capture -- two replays read different tables -- and each replay's gradients equal those of an eager step from the
    same weights fed that replay's masks, while the other replay's masks miss by 100x the bound (so that a frozen or
    misrouted mask cannot pass)"""
    import tramba_amd as ta
    from tramba_amd import modules as M, train
    torch.manual_seed(3)
    m = ta.bulid_model(use_pretrain=False, img_size=384).to(DEV).train()
    m.compute_dtype = BF16
    opt = train.get_opt(1e-4, m, capturable=True)
    step = ta.GraphedTrainStep(m, opt)
    x = torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = (torch.rand(2, 1, 384, 384, generator=torch.Generator().manual_seed(1)) > 0.7).float().to(DEV)
    names = {id(mod): n for n, mod in m.named_modules() if isinstance(mod, ta.DropPath)}
    snaps, tables, grads = [], [], []
    for _ in range(2):
        snaps.append({k: v.detach().clone() for k, v in m.state_dict().items()})
        step(x, y)
        torch.cuda.synchronize()
        (key,) = step._graphs
        buf32 = step._graphs[key][4][2]
        rows = {}
        for (mid, k), (row, ref) in M.model_mask_pool(m).slots.items():
            if ref() is not None and mid in names:
                rows[(names[mid], k)] = buf32[row].detach().cpu().clone()
        tables.append(rows)
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    for t in tables:
        v = torch.stack(list(t.values()))
        assert bool((v == 0).any()) and bool((v != 0).any())
    assert tables[0].keys() == tables[1].keys() and len(tables[0]) >= 40
    assert any(not torch.equal(tables[0][k], tables[1][k]) for k in tables[0]), "the replays reuse one mask table"
    gaps = [_grad_gap(grads[i], _eager_grads(snaps[i], tables[i], x, y)) for i in range(2)]
    control = _grad_gap(grads[0], _eager_grads(snaps[0], tables[1], x, y))
    assert max(gaps) <= REPLAY_BOUND, gaps
    # bit equality leaves no bound to multiply: a wrong table must move some gradient by >= 10 % of its largest entry
    assert control >= 0.1, control
