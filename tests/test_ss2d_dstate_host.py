"""The host side of the fused channels-last SS2D scan at d_state N = 2..16 (hip.ss2d_scan_n_cl): the C ABI, the x_dbl group
layout, the segment plan and the argument checks, all without a device -- and, on the CPU, the room that the tolerances of
tests/test_gpu_ss2d_dstate.py leave for fp32 arithmetic on the very inputs that file runs."""
import ctypes
import os
import re

import pytest
import torch

import scan_memory_cases as smc
import ss2d_dstate_cases as sdc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tramba_ss2d_group_stride_n", "tramba_ss2d_scan_n_workspace", "tramba_ss2d_scan_n_plan", "tramba_ss2d_scan_n_cl")


def hip():
    from tramba_amd import hip as h
    return h


def plan(b, l, d, k, n):
    return hip().ss2d_scan_n_plan(b, l, d, k, n)


def test_header_and_export():
    header = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    lib = hip().lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    assert "tramba_ss2d_group_stride(int r);" in header            # the N = 1 entry stays
    assert lib.tramba_abi_version() == 7                            # additions only


def test_group_stride():
    lib, H = hip().lib(), hip()
    for r in range(1, 65):
        assert lib.tramba_ss2d_group_stride_n(r, 1) == lib.tramba_ss2d_group_stride(r) == H.ss2d_group_stride(r)
        r8 = (r + 7) & ~7
        for n in range(1, 17):
            rg = lib.tramba_ss2d_group_stride_n(r, n)
            assert rg % 4 == 0 and r8 + 2 * n <= rg < r8 + 2 * n + 4, (r, n, rg)
            assert H.ss2d_group_stride(r, n) == rg == sdc.group_stride(r, n)


def _pad_n1_before(x_proj_weight):
    """pad_x_proj_weight as it stood before it took a state count"""
    k, r2, d = x_proj_weight.shape
    rg = hip().ss2d_group_stride(r2 - 2)
    w = x_proj_weight.new_zeros((k, rg, d))
    w[:, :r2 - 2] = x_proj_weight[:, :r2 - 2]
    w[:, rg - 4:rg - 2] = x_proj_weight[:, r2 - 2:]
    return w.reshape(k * rg, d)


def test_pad_x_proj_weight():
    H = hip()
    g = torch.Generator().manual_seed(3)
    k, d = 3, 24
    for r in (1, 2, 8, 9, 40, 64):
        w = torch.randn(k, r + 2, d, generator=g)
        assert torch.equal(H.pad_x_proj_weight(w), _pad_n1_before(w))
        assert torch.equal(H.pad_x_proj_weight(w, 1), _pad_n1_before(w))
    x = torch.randn(7, d, generator=g, dtype=torch.float64)
    for n in (2, 3, 16):
        for r in (1, 8, 9, 40):
            w = torch.randn(k, r + 2 * n, d, generator=g, dtype=torch.float64)
            p = H.pad_x_proj_weight(w, n)
            rg, r8 = H.ss2d_group_stride(r, n), (r + 7) & ~7
            assert p.shape == (k * rg, d) and torch.equal(p, sdc.pad_weight(w, n))
            out = (x @ p.t()).view(7, k, rg)
            used = torch.zeros(rg, dtype=torch.bool)
            used[:r] = True
            used[r8:r8 + 2 * n] = True
            assert bool((p.view(k, rg, d)[:, ~used] == 0).all())          # every padding row is zero
            for j in range(k):
                dts, bs, cs = torch.split(x @ w[j].t(), [r, n, n], dim=1)
                assert torch.equal(out[:, j, :r], dts)
                assert torch.equal(out[:, j, r8:r8 + n], bs) and torch.equal(out[:, j, r8 + n:r8 + 2 * n], cs)
    with pytest.raises(H.TrambaHipError):
        H.pad_x_proj_weight(torch.zeros(2, 4, 8), 2)                      # R + 2N = 4 leaves no rank


def test_plan_query():
    lib = hip().lib()
    for name, (b, h, d, r, fam, n) in sdc.CORE_CASES.items():
        l, k = h * h, sdc.k_of(fam)
        nt, nseg = plan(b, l, d, k, n)
        assert (nt, nseg) == plan(b, l, d, k, n)                          # deterministic
        assert nt >= 1 and nseg >= 1 and nseg * nt * 32 >= l and (nseg - 1) * nt * 32 < l, (name, nt, nseg)
        ws = lib.tramba_ss2d_scan_n_workspace(b, l, d, k, n)
        if nseg > 1:
            assert ws >= b * k * nseg * n * d * 8, name
        else:
            assert ws > 0
    b, h, d, r, fam, n = sdc.SINGLE_PASS
    assert plan(b, h * h, d, sdc.k_of(fam), n)[1] == 1
    b, h, d, r, fam, n = sdc.MULTI_SEG
    assert 1 < plan(b, h * h, d, sdc.k_of(fam), n)[1]
    b, h, d, r, fam, n = sdc.MANY_SEG
    assert h == 48 and plan(b, h * h, d, sdc.k_of(fam), n)[1] > 8
    # the memory cases of the GPU file: more than 8 segments too, for both state counts
    fam, h, d, r = sdc.MEMORY_SHAPE
    for n in (3, 16):
        assert plan(1, h * h, d, sdc.k_of(fam), n)[1] > 8
    # a chip-filling batch keeps whole sequences in few segments, a small one cuts them up
    assert plan(64, 96 * 96, 256, 8, 16)[1] < plan(1, 96 * 96, 256, 8, 16)[1]


def test_argument_checks_need_no_device():
    lib = hip().lib()
    nt, nseg = ctypes.c_int(-5), ctypes.c_int(-5)
    for n in (0, 1, 17):
        rc = lib.tramba_ss2d_scan_n_cl(None, None, None, None, None, None, None, None, None, 0, 1, 64, 32, 4, 2, n, 0, 0, None)
        assert rc == -1, (n, rc)                                          # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert "ss2d_scan_n_cl" in msg and (("tramba_ss2d_scan_cl" in msg) == (n == 1)), (n, msg)
        rc = lib.tramba_ss2d_scan_n_plan(1, 64, 32, 4, n, ctypes.addressof(nt), ctypes.addressof(nseg))
        assert rc == -1 and (nt.value, nseg.value) == (-5, -5), n
        assert ("tramba_ss2d_scan_cl" in lib.tramba_last_error().decode()) == (n == 1)
        assert lib.tramba_ss2d_scan_n_workspace(1, 64, 32, 4, n) == 0
    rc = lib.tramba_ss2d_scan_n_cl(None, None, None, None, None, None, None, None, None, 0, 1, 64, 32, 4, 2, 16, 0, 0, None)
    assert rc == -1 and "null" in lib.tramba_last_error().decode()        # a valid N gets as far as the tensors


# ----------------------------------------------------------------------------- tolerance headroom, on the CPU
CORE_DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]
IDS = lambda v: v if isinstance(v, str) else "-".join(str(t)[6:] for t in v)


@pytest.mark.parametrize("dtypes", CORE_DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(sdc.CORE_CASES), ids=IDS)
def test_core_tolerances_leave_a_factor_2_for_fp32_arithmetic(name, dtypes):
    """the kernel's documented fp32 form (bf16 hi + lo dt_proj operands, exp2 / log2), evaluated on the CPU position by position
    and tile-wise by the planned segments, uses at most half of rtol = atol = 2e-4 (fp32) / 4e-2 (16-bit) on every GPU case"""
    dtype, ys_dtype = dtypes
    c = sdc.core_case(sdc.CORE_CASES[name], dtype)
    nt, _ = plan(c.b, c.l, c.d, c.k, c.n)
    # the restatement itself, in fp64, is the oracle (gather, layout offsets, state sum)
    if dtype == F32:
        ref = sdc.reference(sdc.core_as_scan_case(c))
        assert smc.rel_errors(ref, c.ys_want)[0] < 1e-5          # x_dbl went through an fp32 GEMM here
    shares = [sdc.tolerance_share(sdc.core_emulated(c, ys_dtype, seg), c.want, sdc.CORE_TOL[dtype]) for seg in (None, nt)]
    print(name, IDS(dtypes), "share of the tolerance used by fp32 arithmetic: %.3f (sequential) %.3f (by segments)" % tuple(shares))
    assert max(shares) <= 0.5, shares


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda t: str(t)[6:])
@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_memory_rule_leaves_room(regime, n, dtype):
    """E32 of the long-memory cases: each of the two fp32 evaluations sits, by construction, a factor FACTOR = 8 inside the
    bound; what is checked here is that E32 is an fp32-sized number -- no larger than 2^-16, the documented relative accuracy
    of the coarsest step of the arithmetic, the hi + lo bf16 dt_proj without its lo * lo product -- i.e. that 8 x E32 is a
    bound with teeth, and that the two evaluations agree to within half of it"""
    fam, h, d, r = sdc.MEMORY_SHAPE
    nt, nseg = plan(1, h * h, d, sdc.k_of(fam), n)
    c, ref, e = sdc.memory_e32(regime, n, dtype, nt)
    seq, til = sdc.emulate(c), sdc.emulate(c, nt)
    between = smc.rel_errors(til, seq.double())
    print(regime, n, str(dtype)[6:], f"nseg={nseg} E32 max {e[0]:.3e} rms {e[1]:.3e}; tile-wise against sequential {between[0]:.3e}")
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1.0
    assert 0.0 < e[0] <= 2.0 ** -16 and e[1] <= e[0]
    assert between[0] <= 0.5 * smc.bound(e[0]) and between[1] <= 0.5 * smc.bound(e[1])
