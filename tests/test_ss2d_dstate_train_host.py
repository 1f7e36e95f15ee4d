"""The host side of the fused channels-last SS2D training path at d_state N = 2..16: the C ABI of the scan backward and its
glue, the backward's own segment plan and workspace formula, the argument checks, the padded x_proj layout, the opt-in switch
and the allocation census, all without a device -- and, on the CPU, the fixture's fp64 adjoint against autograd through the
oracle, and the room that the tolerances of tests/test_gpu_ss2d_dstate_train.py leave for fp32 arithmetic on the very inputs
that file runs."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import buffer_cases as bc
import scan_memory_cases as smc
import ss2d_dstate_cases as sdc
import ss2d_dstate_train_cases as tc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tramba_ss2d_scan_n_bwd_cl", "tramba_ss2d_scan_n_bwd_workspace", "tramba_ss2d_scan_n_bwd_plan",
       "tramba_ss2d_bwd_prep_n_cl", "tramba_ss2d_bwd_assemble_n_cl")
IDS = lambda v: v if isinstance(v, str) else "-".join(str(t)[6:] for t in (v if isinstance(v, tuple) else (v,)))


def hip():
    from tramba_amd import hip as h
    return h


def plan(b, l, d, k, n):
    return hip().ss2d_scan_n_bwd_plan(b, l, d, k, n)


def test_header_export_and_binding():
    header = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    H = hip()
    lib = H.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name) and name in H.SIGNATURES, name
    assert "vmamba.py:230-262" in header and "selective_scan_cuda_oflex.bwd" in header
    for old in ("tramba_ss2d_bwd_prep_cl(", "tramba_ss2d_bwd_assemble_cl(", "tramba_ss2d_scan_bwd_cl("):
        assert old in header                                           # the N = 1 entries stay
    assert lib.tramba_abi_version() == 7                               # additions only


def _documented_plan(b, l, d, k, n):
    """~4096 waves, no fewer than 4 tiles per segment, at most 160 / N, one segment up to 6 tiles"""
    ntiles = (l + 31) // 32
    want = max(4096 // (b * k * ((d + 31) // 32)), 1)
    nt = max((ntiles + want - 1) // want, 4)
    if ntiles <= 6:
        nt = ntiles
    nt = min(nt, 160 // n)
    return nt, (ntiles + nt - 1) // nt


def test_plan_and_workspace_formula():
    lib = hip().lib()
    shapes = [(b, h * h, d, sdc.k_of(fam), n) for b, h, d, r, fam, n in sdc.CORE_CASES.values()]
    shapes += [(4, 96 * 96, 256, 8, n) for n in (2, 3, 16)] + [(1, 96 * 96, 256, 8, 16), (4, 48 * 48, 512, 8, 16), (64, 9216, 256, 8, 16)]
    for b, l, d, k, n in shapes:
        nt, nseg = plan(b, l, d, k, n)
        assert (nt, nseg) == _documented_plan(b, l, d, k, n), (b, l, d, k, n)
        assert nt >= 1 and nt * n <= 160 and nseg * nt * 32 >= l and (nseg - 1) * nt * 32 < l
        for dtype in (0, 1, 2):
            ws = lib.tramba_ss2d_scan_n_bwd_workspace(b, l, d, k, n, dtype)
            assert ws == (16 if nseg == 1 else b * k * nseg * n * d * 12), (b, l, d, k, n)
    # r does not enter the workspace: the documented formula for r in {1, 8, 40, 64} is the same number
    for n in (2, 3, 16):
        nt, nseg = plan(2, 2304, 40, 8, n)
        assert lib.tramba_ss2d_scan_n_bwd_workspace(2, 2304, 40, 8, n, 1) == 2 * 8 * nseg * n * 40 * 12
    assert plan(1, 144, 32, 4, 2) == (5, 1) and plan(1, 576, 64, 8, 16)[1] > 2
    assert plan(64, 96 * 96, 256, 8, 16)[1] <= plan(1, 96 * 96, 256, 8, 16)[1]


def test_argument_checks_need_no_device():
    lib = hip().lib()
    nt, nseg = ctypes.c_int(-5), ctypes.c_int(-5)
    nul = [None] * 14
    one = ctypes.c_void_p(16)
    ptrs = [one] * 14

    def call(args, ws_bytes, b, l, d, k, r, n, dtype=0, gdtype=0):
        return lib.tramba_ss2d_scan_n_bwd_cl(*args, ws_bytes, b, l, d, k, r, n, dtype, gdtype, None)

    for n in (0, 1, 17):
        assert call(nul, 0, 1, 64, 32, 4, 2, n) == -1
        msg = lib.tramba_last_error().decode()
        assert "ss2d_scan_n_bwd_cl" in msg and (("tramba_ss2d_scan_bwd_cl" in msg) == (n == 1)), (n, msg)
        rc = lib.tramba_ss2d_scan_n_bwd_plan(1, 64, 32, 4, n, ctypes.addressof(nt), ctypes.addressof(nseg))
        assert rc == -1 and (nt.value, nseg.value) == (-5, -5), n
        assert lib.tramba_ss2d_scan_n_bwd_workspace(1, 64, 32, 4, n, 0) == 0
        assert lib.tramba_ss2d_bwd_prep_n_cl(*[one] * 6, 1, 64, 4, 2, 0 if n == 1 else n, 1, 0, None) == -1
        assert lib.tramba_ss2d_bwd_assemble_n_cl(*[one] * 4, 1, 64, 4, 2, 0 if n == 1 else n, 0, None) == -1
    assert lib.tramba_ss2d_scan_n_bwd_workspace(1, 64, 32, 4, 2, 7) == 0                    # no such dtype
    assert call(nul, 0, 1, 64, 32, 4, 2, 16) == -1 and "null" in lib.tramba_last_error().decode()
    assert call(ptrs, 0, 1, 64, 32, 4, 65, 16) == -1 and "dt_rank 65" in lib.tramba_last_error().decode()
    # several segments: a workspace one byte short, and a misaligned one
    b, l, d, k, n = 1, 576, 64, 8, 16
    need = lib.tramba_ss2d_scan_n_bwd_workspace(b, l, d, k, n, 0)
    assert plan(b, l, d, k, n)[1] > 1 and need > 16
    assert call(ptrs, need - 1, b, l, d, k, 4, n) == -1
    assert "workspace of %d bytes" % need in lib.tramba_last_error().decode()
    odd = [one] * 13 + [ctypes.c_void_p(24)]
    assert call(odd, need, b, l, d, k, 4, n) == -1 and "16-byte aligned" in lib.tramba_last_error().decode()
    assert call(ptrs, need, b, l, d, k, 4, n, 1, 2) == -1 and "gym" in lib.tramba_last_error().decode()


def _xproj_padded_before(w, dtype):
    """modules._xproj_padded as it stood before it took a state count (no shadow is current on the host)"""
    k, r2, d = w.shape
    r = r2 - 2
    rg = hip().ss2d_group_stride(r)
    wl = w.detach().to(dtype)
    parts = [wl[:, :r]]
    if rg - 4 - r:
        parts.append(torch.zeros((k, rg - 4 - r, d), dtype=dtype))
    parts += [wl[:, r:], torch.zeros((k, 2, d), dtype=dtype)]
    return torch.cat(parts, dim=1).view(k * rg, d)


def test_xproj_padded():
    from tramba_amd import modules as M
    H = hip()
    g = torch.Generator().manual_seed(5)
    k, d = 3, 24
    for r in (1, 2, 8, 9, 40, 64):
        w = torch.randn(k, r + 2, d, generator=g)
        for dtype in (F32, BF16):
            want = _xproj_padded_before(w, dtype)
            for got in (M._xproj_padded(w, dtype), M._xproj_padded(w, dtype, 1)):
                assert got[1] is None and got[0].dtype == dtype and torch.equal(got[0], want)
    for n in (2, 3, 16):
        for r in (1, 8, 9, 40):
            w = torch.randn(k, r + 2 * n, d, generator=g)
            p, t = M._xproj_padded(w, F32, n)
            rg, r8 = H.ss2d_group_stride(r, n), (r + 7) & ~7
            assert t is None and p.shape == (k * rg, d) and torch.equal(p, sdc.pad_weight(w, n))
            used = torch.zeros(rg, dtype=torch.bool)
            used[:r] = True
            used[r8:r8 + 2 * n] = True
            p3 = p.view(k, rg, d)
            assert bool((p3[:, ~used] == 0).all())
            assert torch.equal(p3[:, :r], w[:, :r]) and torch.equal(p3[:, r8:r8 + 2 * n], w[:, r:])


def test_the_switch():
    import tramba_amd as ta
    assert ta.get_fused_dstate_training() is False                      # off by default
    assert ta.set_fused_dstate_training(True) is False and ta.get_fused_dstate_training() is True
    assert ta.set_fused_dstate_training(False) is True
    with ta.fused_dstate_training(True):
        assert ta.get_fused_dstate_training() is True
        with ta.fused_dstate_training(False):
            assert ta.get_fused_dstate_training() is False
        assert ta.get_fused_dstate_training() is True
    assert ta.get_fused_dstate_training() is False
    with pytest.raises(RuntimeError):
        with ta.fused_dstate_training(True):
            raise RuntimeError("inside")
    assert ta.get_fused_dstate_training() is False                      # restored on an exception
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError):
            ta.set_fused_dstate_training(bad)
    assert ta.get_fused_dstate_training() is False
    m = ta.SS2D(d_model=16, channel_first=True)
    x = torch.zeros(1, 12, 12, 16)
    with ta.fused_dstate_training(True):
        assert not m._train_fused_n_ok(x)                                # a host tensor never takes it
    assert m.d_state == 16 and not m._train_fused_ok(x)


def test_no_new_uninitialised_allocation_site():
    """the census of tramba_amd/*.py against the parent commit's: same number of sites per file and per allocator, and the
    lines of hip.py's scan wrappers are the pre-existing ones (shapes may now depend on N, the call sites do not multiply)"""
    now = {}
    for f, line, name in bc.CENSUS.torch:
        now[(f, name)] = now.get((f, name), 0) + 1
    try:
        files = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", "HEAD~", "tramba_amd/"], capture_output=True,
                               text=True, check=True).stdout.split()
    except (OSError, subprocess.CalledProcessError):
        files = []
    if files:      # a checkout with history: the parent's census, file by file
        before = {}
        for path in files:
            if path.endswith(".py"):
                src = subprocess.run(["git", "-C", ROOT, "show", "HEAD~:" + path], capture_output=True, text=True, check=True).stdout
                for f, line, name, kind in bc.census_of_source(src, os.path.basename(path)):
                    if kind == "torch":
                        before[(f, name)] = before.get((f, name), 0) + 1
        grown = {k_: (before.get(k_, 0), v) for k_, v in now.items() if v > before.get(k_, 0)}
        assert not grown, grown
    # with or without history: every census line inside the functions this change touched is a pre-existing fragment
    known = ("gu = torch.empty((b, k, l, d), dtype=x.dtype, device=x.device)", "graw = torch.empty_like(gu)",
             "gB = torch.empty((b, k, ", "gC = torch.empty_like(gB)", "gpar = torch.empty((", "ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)",
             "ranks = torch.empty((b, k, l, ", "gseq = torch.empty((b, k, l, rg), dtype=torch.float32, device=xdbl.device)",
             "out = torch.empty((b, l, k * rg), dtype=dtype, device=gseq.device)")
    text = open(os.path.join(ROOT, "tramba_amd", "hip.py")).read().splitlines()
    start = next(i for i, s in enumerate(text) if s.startswith("def ss2d_scan_n_bwd_plan("))
    stop = next(i for i, s in enumerate(text) if s.startswith("def ss2d_merge_grad_cl("))
    sites = [s for (f, line), s in bc.SITE_LINES.items() if f == "hip.py" and start < line <= stop]
    assert len(sites) == 9 and all(any(s.startswith(frag) for frag in known) for s in sites), sites
    src = open(os.path.join(ROOT, "tramba_amd", "modules.py")).read()
    body = src[src.index("def _xproj_padded("):src.index("class SS2D(nn.Module)")]
    for name in bc.TORCH_ALLOCATORS:
        assert "." + name + "(" not in body, name


# ----------------------------------------------------------------------------- the fixture against the oracle
@pytest.mark.parametrize("name", ["single_launch", "segments_k8", "d40_window", "ragged_r1", "rank40"])
def test_the_fp64_adjoint_is_the_oracles(name):
    """the kernel-level fp64 reference (documented adjoint, position by position), carried to the leaves by the linear maps
    around the kernel, equals autograd through oracle.ops.ss2d_core + cross_merge (x_dbl went through an fp32 GEMM and the
    oracle rounds A to fp32: 1e-5)"""
    o = tc.oracle_grads(name, F32)
    comp = tc.compose(o.scan, o.case.wx, tc.reference(o.scan, o.gym))
    for k_, g in o.grads.items():
        assert comp[k_].shape == g.shape and smc.rel_errors(comp[k_], g)[0] < 1e-5, k_


# ----------------------------------------------------------------------------- tolerance headroom, on the CPU
KERNEL_DTYPES = [(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]


@pytest.mark.parametrize("dtypes", KERNEL_DTYPES, ids=IDS)
@pytest.mark.parametrize("name", tc.KERNEL_CASES, ids=IDS)
def test_kernel_tolerances_leave_a_factor_2_for_fp32_arithmetic(name, dtypes):
    """the backward's documented fp32 form evaluated on the CPU on the exact GPU inputs, position by position and tile-wise by
    the planned segments, uses at most half of each bound (3e-4 gu / 5e-4 others in fp32, 3e-2 / 5e-2 in 16 bit)"""
    dtype, gdtype = dtypes
    b, h, d, r, fam, n = tc.CORE_CASES[name]
    nt, _ = plan(b, h * h, d, sdc.k_of(fam), n)
    c, gym, ref, e32 = tc.core_e32(name, dtype, gdtype, nt)
    shares = {out: e32[out] / tc.base_tol(out, dtype) for out in tc.OUTPUTS}
    print(name, IDS(dtypes), {k_: f"{v:.3f}" for k_, v in shares.items()})
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in ref.values())
    assert max(shares.values()) <= 0.5, shares
    for out in tc.OUTPUTS:
        assert tc.bound(out, dtype, e32[out], stored16=out in ("gu", "graw")) == tc.base_tol(out, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_memory_rule_has_teeth(regime, n, dtype):
    """E32 of the long-memory cases is an fp32-sized number for fp32 activations (<= 2^-14 on every gradient: the forward's
    2^-16 through one more recurrence) and a bf16-sized one for bf16 (<= 2^-6), so 8 x E32 is a bound with teeth"""
    fam, h, d, r = sdc.MEMORY_SHAPE
    nt, nseg = plan(1, h * h, d, sdc.k_of(fam), n)
    assert nseg > 8
    c, gym, ref, e32 = tc.memory_e32(regime, n, dtype, nt)
    print(regime, n, IDS(dtype), f"nseg={nseg}", {k_: f"{v:.2e}" for k_, v in e32.items()})
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert 0.0 < max(e32.values()) <= (2.0 ** -14 if dtype == F32 else 2.0 ** -6), e32
