"""selective_scan_fwd / _bwd for d_state 3, 5..16 (the state-looped kernel pair) and SS2D / VSSBlock at d_state 16, against the
fp64 oracle.  tests/test_scan_dstate_host.py anchors that oracle at N = 16 and shows, without a GPU, that the tolerances used
here leave room for fp32 arithmetic on these very inputs (forward: <= 0.05 of rtol = atol = 2e-4; gradients: <= 1e-5 where the
bound is 3e-4).

Tests 1 and 2 decay by about 0.74 per position, so the state dies inside a chunk and a lost chunk carry would go unseen; tests
3 and 4 use the regimes of tests/golden/scan_memory_cases.py, where it outlives all four chunks, under that module's rule: an
fp32 output within 8 x E32 of the fp64 reference on the max- and the RMS-relative measure, a 16-bit output with every element
within u |want| + (that bound) max |want|.  `init16` is the regime SS2D(d_state=16) is born in (A[d, n] = -(n + 1), dt 1e-3 ..
1e-1): there dA gets 2.5 x 8 x E32, the allowance DESIGN section 4 "known property (1)" grants gA for the same reason -- near a
decay of 1 the error of the hardware exp2 enters it twice, through the state and through the adjoint."""
import numpy as np
import pytest
import torch

import scan_dstate_cases as sdc
import scan_memory_cases as smc
from oracle import model as om

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:]


def hip():
    from tramba_amd import hip as h
    return h


def _args(g):
    return g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["delta_bias"]


@pytest.mark.parametrize("dtype", sdc.FWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sdc.SHAPES, ids=IDS)
def test_forward_fast_decay(shape, dtype):
    """tolerances of test_selective_scan_fwd: rtol = atol = 2e-4 for the fp32 output, 2e-2 for the same-dtype 16-bit output"""
    nb, k, dper, n, l = shape
    a, want, want2 = sdc.fwd_case(shape, dtype)
    g = {k_: v.to(DEV) for k_, v in a.items()}
    out, ckpt = hip().selective_scan_fwd(*_args(g), True, True)
    assert out.dtype == F32 and out.shape == (nb, k * dper, l)
    got = out.cpu().double()
    print(shape, dtype, "share of the tolerance used:", float(((got - want).abs() / (2e-4 + 2e-4 * want.abs())).max()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-4)
    assert ckpt.shape == (nb, k * dper, hip().selective_scan_nchunk(l, dtype), n) and ckpt.dtype == F32
    assert bool(torch.isfinite(ckpt).all())
    # no softplus / no D / no bias / same-dtype output
    out2, _ = hip().selective_scan_fwd(g["u"], g["delta"].abs(), g["A"], g["B"], g["C"], None, None, False, False, False)
    assert out2.dtype == dtype
    tol = 2e-4 if dtype == F32 else 2e-2
    np.testing.assert_allclose(out2.cpu().double().numpy(), want2.numpy(), rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", sdc.BWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sdc.SHAPES, ids=IDS)
def test_backward_fast_decay(shape, dtype):
    """measure and tolerance of test_selective_scan_bwd: max |err| / max(1, max |want|) < 3e-4, 1.5e-2 for 16-bit du / ddelta"""
    a, dout, want = sdc.bwd_case(shape, dtype)
    g = {k_: v.to(DEV) for k_, v in a.items()}
    _, ckpt = hip().selective_scan_fwd(*_args(g), True, True)
    got = hip().selective_scan_bwd(*_args(g), dout.to(DEV), ckpt, True)
    errs = {name: sdc.grad_error(x.cpu(), w) for name, x, w in zip(sdc.GRADS, got, want)}
    print(shape, dtype, {k_: f"{v:.2e}" for k_, v in errs.items()})
    for name, err in errs.items():
        tol = 3e-4 if (dtype == F32 or name not in ("du", "ddelta")) else 1.5e-2
        assert err < tol, (name, err)


def _hold(recs):
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    for r in recs:
        assert r["ok"], r


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("n", [3, 8, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_state_outlives_the_chunks(regime, n, dtype):
    """rows 2 x 4 x 8, L = 1561 (fp32, scalar accesses) / 1600 (bf16, 16-byte accesses): four 512-position chunks, the last
    ragged; every output and gradient within 8 x E32 (E32 5.8e-7 .. 1.7e-6)"""
    _hold(smc.boundary_records(hip(), torch.device(DEV), regime, n, dtype))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
def test_init16_regime(dtype):
    """the constructor's own A and dt at d_state 16: 8 x E32, 2.5 x 8 x E32 for dA (module docstring)"""
    H = hip()
    o, ref, e = sdc.init16_e32(dtype)
    g = [t.to(DEV) for t in (o.u, o.delta, o.A, o.B, o.C, o.D, o.delta_bias)]
    assert H.selective_scan_nchunk(o.l, dtype) == 4
    out, ckpt = H.selective_scan_fwd(*g, True, True)
    grads = H.selective_scan_bwd(*g, o.dout.to(DEV), ckpt, True)
    torch.cuda.synchronize()
    H.device_error()
    label = f"init16 {str(dtype)[6:]} L={o.l}"
    recs = [smc.record(label, "out", out, ref["out"], e["out"])]
    for name, got in zip(smc.BOUNDARY_OUTPUTS[1:], grads):
        assert bool(torch.isfinite(got.float()).all()), name
        out_dtype = dtype if name in ("du", "ddelta") else F32
        rec = smc.record(label, "gA" if name == "dA" else name, got, ref[name], e[name], out_dtype)   # "gA": the 2.5 x rule
        rec["output"] = name
        recs.append(rec)
    _hold(recs)


def test_forward_is_the_same_run_to_run():
    a, _, _ = sdc.fwd_case((1, 4, 4, 16, 1153), BF16)
    g = {k_: v.to(DEV) for k_, v in a.items()}
    first, ck1 = hip().selective_scan_fwd(*_args(g), True, True)
    again, ck2 = hip().selective_scan_fwd(*_args(g), True, True)
    assert torch.equal(first, again) and torch.equal(ck1, ck2)


# ----------------------------------------------------------------------------- modules
def _ss2d(case):
    import tramba_amd as ta
    from tramba_amd import ops
    torch.manual_seed(11)
    if case == "default":      # the constructor's own d_state: raster, K = 4
        m, shape, family, k = ta.SS2D(d_model=16, channel_first=True), (2, 16, 12, 12), "raster", 4
    else:                      # helix, K = 8; L = 576 is two chunks
        m = ta.SS2D(d_model=16, d_state=16, channel_first=True, scan=ops.CrossScan_Line, merge=ops.CrossMerge_Line, k_group=8)
        shape, family, k = (1, 16, 24, 24), "helix", 8
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    x = torch.randn(*shape, generator=g)
    return m, x, family, k


@pytest.mark.parametrize("case", ["default", "helix"])
def test_ss2d_at_the_default_dstate(case):
    """forward rtol 1e-3 / atol 1e-4 and gradients to a relative L2 of 1e-3 (the project's block-level fp32 figures, DESIGN
    section 4 "Numerics") against the oracle and autograd through it; bf16 forward within 4e-2 of the map's largest magnitude"""
    m, x, family, k = _ss2d(case)
    assert m.d_state == 16
    sd = {k_: v.detach().clone() for k_, v in m.state_dict().items()}
    assert sd["A_logs"].shape == (k * 32, 16) and sd["x_proj_weight"].shape == (k, 1 + 32, 32)
    # oracle, with autograd through it
    leaves = {k_: v.clone().requires_grad_() for k_, v in sd.items()}
    xo = x.clone().requires_grad_()
    want = om.ss2d(om.SD(leaves), xo, family)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(13))
    (want * gy).sum().backward()
    # library
    m.to(DEV)
    xg = x.to(DEV).requires_grad_()
    got = m(xg)
    assert got.dtype == F32 and got.shape == want.shape
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-3, atol=1e-4)
    (got * gy.to(DEV)).sum().backward()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    errs = {"x": rel(xg.grad.cpu(), xo.grad)}
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        errs[name] = rel(p.grad.cpu(), leaves[name].grad)
    print(case, {k_: f"{v:.2e}" for k_, v in errs.items()})
    for name, err in errs.items():
        assert err <= 1e-3, (name, err)
    # bf16, inference: the oracle on the same rounded weights and input
    m16 = m.to(BF16).eval()
    sd16 = {k_: v.detach().cpu().float() for k_, v in m16.state_dict().items()}
    x16 = x.to(BF16)
    with torch.no_grad():
        got16 = m16(x16.to(DEV)).float().cpu()
        want16 = om.ss2d(om.SD(sd16), x16.float(), family)
    assert bool(torch.isfinite(got16).all())
    err16 = float((got16 - want16).abs().max()) / float(want16.abs().max())
    print(case, f"bf16 forward: {err16:.2e} of the largest magnitude")
    assert err16 <= 4e-2


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
def test_vss_block_at_dstate_16_runs(dtype):
    import tramba_amd as ta
    torch.manual_seed(21)
    m = ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0).to(DEV, dtype)
    x = torch.randn(2, 16, 12, 12, device=DEV, dtype=dtype, requires_grad=True)
    y = m(x)
    assert y.shape == x.shape
    y.float().square().mean().backward()
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad.float()).all())
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad.float()).all()), name


def test_multiscale_decoder_block_at_dstate_16_runs():
    import tramba_amd as ta
    torch.manual_seed(22)
    m = ta.MultiScaleDecoderBlock(hidden_dim=16, drop_path=0.0, channel_first=True, ssm_d_state=16).to(DEV)
    x = torch.randn(1, 16, 12, 12, device=DEV, requires_grad=True)
    y = m(x)
    y.square().mean().backward()
    assert y.shape == x.shape and bool(torch.isfinite(x.grad).all())
    assert m.op.A_logs.grad.shape == (8 * 32, 16) and bool(torch.isfinite(m.op.A_logs.grad).all())
