"""CPU side of the d_state 1..16 selective scan: the ABI's range and its error text, no CPU fallback, the oracle anchored at
N = 16 where tests/test_gpu_scan_dstate.py leans on it, and the tolerances of that file shown fit for its inputs (what a plain
fp32 evaluation of the same formulas loses on them) without a GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scan_dstate_cases as sdc
import scan_memory_cases as smc
from oracle import selective_scan as oss

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:]


def test_max_dstate_is_exported():
    from tramba_amd import hip
    assert hip.lib().tramba_selective_scan_max_dstate() == 16
    assert hip.selective_scan_max_dstate() == 16


@pytest.mark.parametrize("n", [0, 17])
def test_dstate_out_of_range_is_an_error_that_names_the_limit(n):
    """dummy non-null addresses: the range check comes before any launch"""
    from tramba_amd import hip
    lib = hip.lib()
    p = ctypes.c_void_p(64)
    nb, kd, k, l = 1, 4, 2, 16
    rc = lib.tramba_selective_scan_fwd(p, p, p, p, p, p, p, p, p, nb, kd, k, n, l, hip.dt(torch.zeros(1)), hip.dt(torch.zeros(1)),
                                       1, None)
    msg = lib.tramba_last_error().decode()
    assert rc < 0 and "d_state" in msg and "16" in msg, (rc, msg)
    rc = lib.tramba_selective_scan_bwd(*([p] * 16), nb, kd, k, n, l, hip.dt(torch.zeros(1)), 1, 1, None)
    msg = lib.tramba_last_error().decode()
    assert rc < 0 and "d_state" in msg and "16" in msg, (rc, msg)


def test_no_cpu_fallback_at_dstate_16():
    from tramba_amd import hip
    a = sdc.scan_inputs(1, 2, 2, 16, 33, F32)
    with pytest.raises(hip.TrambaHipError):
        hip.selective_scan_fwd(a["u"], a["delta"], a["A"], a["B"], a["C"], a["D"], a["delta_bias"], True, True)


def test_private_copy_rule():
    """N <= 4: today's rule; N > 4: the workspace never exceeds what N = 4 takes at the same shape (ncopy * N <= 64)"""
    from tramba_amd import hip
    for kd, k in ((32, 4), (1024, 4), (4096, 4), (64, 8), (6, 2)):
        base = max(1, min(16, (kd // k) // 8))
        for n in (1, 2, 3, 4):
            assert hip.scan_bc_copies(kd, k, n) == base
        for n in range(5, 17):
            c = hip.scan_bc_copies(kd, k, n)
            assert 1 <= c <= base and c * n <= max(64, n) and (c == base or (c + 1) * n > 64)


# ----------------------------------------------------------------------------- the oracle at N = 16
def test_oracle_equals_the_numpy_form_at_16_states():
    a = sdc.scan_inputs(1, 2, 2, 16, 33, F32, seed=5)
    args = (a["u"], a["delta"], a["A"], a["B"], a["C"], a["D"], a["delta_bias"], True)
    got, want = oss.selective_scan_fwd(*args), oss.selective_scan_numpy(*args)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_oracle_closed_form_at_16_states():
    """A = 0, B = C = 1, no softplus: every state is cumsum(delta u), so y = 16 cumsum(delta u) + D u"""
    g = torch.Generator().manual_seed(2)
    nb, k, dper, n, l = 1, 2, 2, 16, 33
    u, delta = torch.randn(nb, k * dper, l, generator=g).double(), torch.rand(nb, k * dper, l, generator=g).double()
    D = torch.randn(k * dper, generator=g).double()
    one = torch.ones(nb, k, n, l, dtype=torch.float64)
    got = oss.selective_scan_fwd(u, delta, torch.zeros(k * dper, n), one, one, D, None, False)
    want = 16 * torch.cumsum(delta * u, -1) + D[None, :, None] * u
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _torch_scan(u, delta, A, B, C, D, bias):
    """the recurrence in fp64 torch, differentiable: u, delta (nb, KD, L), A (KD, N), B, C (nb, K, N, L)"""
    nb, kd, l = u.shape
    rep = kd // B.shape[1]
    Bx, Cx = B.repeat_interleave(rep, 1), C.repeat_interleave(rep, 1)     # (nb, KD, N, L)
    dt = F.softplus(delta + bias[None, :, None])
    h = torch.zeros(nb, kd, A.shape[1], dtype=u.dtype)
    ys = []
    for p in range(l):
        h = torch.exp(dt[:, :, p, None] * A) * h + dt[:, :, p, None] * Bx[..., p] * u[:, :, p, None]
        ys.append((Cx[..., p] * h).sum(-1))
    return torch.stack(ys, -1) + D[None, :, None] * u


def test_oracle_backward_equals_autograd_at_16_states():
    a = sdc.scan_inputs(2, 2, 3, 16, 29, F32, seed=7)
    names = ("u", "delta", "A", "B", "C", "D", "delta_bias")
    leaves = [a[k_].double().requires_grad_() for k_ in names]
    dout = torch.randn(2, 6, 29, generator=torch.Generator().manual_seed(8)).double()
    (_torch_scan(*leaves) * dout).sum().backward()
    got = oss.selective_scan_bwd(*(a[k_].double() for k_ in names), dout, True)
    for name, g, leaf in zip(sdc.GRADS, got, leaves):
        assert float((g - leaf.grad).abs().max()) <= 1e-10 * max(1.0, float(leaf.grad.abs().max())), name


# ----------------------------------------------------------------------------- the GPU tolerances are fit for the inputs
@pytest.mark.parametrize("dtype", sdc.FWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sdc.SHAPES, ids=IDS)
def test_forward_tolerance_has_room(shape, dtype):
    """the oracle's fp32-arithmetic forward uses at most 0.05 of rtol = atol = 2e-4 on every element, both calls of the GPU
    test (measured: at most 0.013)"""
    a, want, want2 = sdc.fwd_case(shape, dtype)
    f = lambda t: t.float()
    got = oss.selective_scan_fwd_f32(f(a["u"]), f(a["delta"]), a["A"], f(a["B"]), f(a["C"]), a["D"], a["delta_bias"], True)
    got2 = oss.selective_scan_fwd_f32(f(a["u"]), f(a["delta"]).abs(), a["A"], f(a["B"]), f(a["C"]), None, None, False)
    for g, w in ((got, want), (got2, want2)):
        used = float(((g.double() - w).abs() / (2e-4 + 2e-4 * w.abs())).max())
        print(shape, dtype, f"share of the forward tolerance used by fp32 arithmetic: {used:.4f}")
        assert used <= 0.05


@pytest.mark.parametrize("dtype", sdc.BWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sdc.SHAPES, ids=IDS)
def test_backward_tolerance_has_room(shape, dtype):
    """the fp32 tile-wise evaluation of scan_memory_cases is within 1e-5 of every gradient, on the measure of the GPU test whose
    bound is 3e-4 (measured: at most 4e-7)"""
    a, dout, want = sdc.bwd_case(shape, dtype)
    o = sdc.as_boundary(shape, dtype, a, dout)
    ev = smc._bpack(o, smc._tiled(smc._bterms(o, F32), True))
    for name, w in zip(sdc.GRADS, want):
        err = sdc.grad_error(ev[name], w)
        print(shape, dtype, name, f"fp32 tile-wise evaluation: {err:.2e}")
        assert err <= 1e-5, (name, err)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
def test_init16_case_builds_and_has_a_bound(dtype):
    o, ref, e = sdc.init16_e32(dtype)
    assert o.A.shape == (32, 16) and float(o.A[5, 15]) == -16.0 and o.delta_bias.shape == (32,)
    dt = F.softplus(o.delta_bias.double())
    assert 1e-3 * (1 - 1e-6) <= float(dt.min()) and float(dt.max()) <= 1e-1 * (1 + 1e-6)
    assert set(e) == set(smc.BOUNDARY_OUTPUTS)
    for name, (e_max, e_rms) in e.items():
        print(name, f"E32 max {e_max:.2e} rms {e_rms:.2e}")
        assert np.isfinite(e_max) and np.isfinite(e_rms) and e_max > 0 and e_rms > 0, name
        assert bool(torch.isfinite(ref[name]).all())
