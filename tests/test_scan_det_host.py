"""CPU side of the deterministic (atomic-free) selective-scan backward: the two new ABI entries and their argument checks, the
workspace formula and its bound, no CPU fallback, the switch in tramba_amd.ops, and the tolerance of tests/test_gpu_scan_det.py
shown fit for the order in which that form adds dB / dC (rows of a slab ascending, then slabs ascending) without a GPU."""
import ctypes

import pytest
import torch

import scan_dstate_cases as sdc
import scan_memory_cases as smc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:]

# (nb, k, dper, n, l) of the compile-time-N kernels and the slab logic, the list of tests/test_gpu_scan_det.py
NEW_SHAPES = [
    (2, 2, 3, 1, 37),       # rows of a wave would straddle a group and a batch
    (1, 2, 40, 1, 1153),    # five slabs of eight rows, three ragged chunks
    (2, 3, 7, 4, 200),      # dper not a multiple of any slab, K = 3
    (1, 2, 5, 2, 1000),
    (2, 1, 8, 4, 2304),     # 16-byte path
    (1, 2, 18, 16, 520),    # state-looped, slabs with a remainder
    # beyond the issue's six: several slabs AND batch > 1 at once (slab, group and batch all enter the partial's address)
    (2, 2, 11, 1, 300),
    (2, 3, 9, 5, 264),      # state-looped, 16-byte path
]


def _slab_rows(l):
    """rows of a group one workgroup covers: eight waves of 64 / LPR rows, LPR = 16, 32 or 64 lanes per row by the length"""
    need = (l + 7) // 8
    return 8 * (64 // (16 if need <= 16 else 32 if need <= 32 else 64))


def _work(nb, kd, k, n, l, dtype=F32):
    from tramba_amd import hip
    return hip.lib().tramba_selective_scan_bwd_det_work(nb, kd, k, n, l, hip._DT[dtype])


def test_symbols_are_exported_and_bound():
    import tramba_amd as ta
    from tramba_amd import hip, ops
    lib = hip.lib()
    for name in ("tramba_selective_scan_bwd_det_work", "tramba_selective_scan_bwd_det"):
        assert name in hip.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    assert lib.tramba_abi_version() == 7
    assert ta.set_deterministic_scan is ops.set_deterministic_scan and ta.deterministic_scan is ops.deterministic_scan
    assert callable(hip.selective_scan_bwd_det_work)


@pytest.mark.parametrize("bad", [(0, 8, 2, 1, 64), (1, 0, 2, 1, 64), (1, 8, 0, 1, 64), (1, 8, 2, 1, 0), (1, 9, 2, 1, 64),
                                 (1, 8, 2, 0, 64), (1, 8, 2, 17, 64), (-1, 8, 2, 1, 64)], ids=IDS)
def test_sizing_rejects_bad_arguments(bad):
    from tramba_amd import hip
    assert _work(*bad) < 0
    assert hip.lib().tramba_last_error() != b""
    with pytest.raises(hip.TrambaHipError):
        hip.selective_scan_bwd_det_work(*bad, F32)


def test_sizing_rejects_a_bad_dtype():
    from tramba_amd import hip
    assert hip.lib().tramba_selective_scan_bwd_det_work(1, 8, 2, 1, 64, 7) < 0


@pytest.mark.parametrize("kd,k,n,l", [(16, 2, 1, 1024), (8, 2, 1, 1024), (10, 2, 1, 1024), (20, 2, 1, 1024), (6, 2, 4, 1024), (9216, 4, 16, 1024), (9216, 4, 1, 1024),
                                      (80, 2, 1, 1153), (21, 3, 4, 200), (36, 2, 16, 520), (6, 2, 1, 37), (34, 2, 3, 100),
                                      (18, 2, 16, 257), (2, 2, 5, 8), (128, 2, 2, 64), (70, 2, 2, 64), (64, 2, 2, 200)])
def test_workspace_formula_and_bound(kd, k, n, l):
    """bytes = 4 (2 ceil(dper / S) B K N L + B KD (N + 2)); per tensor never more than ceil(dper / 4) copies of (B, K, N, L):
    the table has dper a multiple of the slab, not a multiple of it, and smaller than it, at all three slab sizes"""
    nb = 3
    dper = kd // k
    s = _slab_rows(l)
    got = _work(nb, kd, k, n, l)
    bknl = nb * k * n * l
    small = 4 * nb * kd * (n + 2)
    assert got == 4 * 2 * -(-dper // s) * bknl + small
    assert got - small <= 2 * -(-dper // 4) * bknl * 4
    for dtype in (BF16, F16):
        assert _work(nb, kd, k, n, l, dtype) == got     # fp32 partials whatever the i/o dtype


def test_workspace_is_linear_in_batch_states_and_length():
    kd, k = 40, 2
    base = _work(1, kd, k, 1, 1024)
    for nb in (2, 3, 7):
        assert _work(nb, kd, k, 1, 1024) == nb * base
    # in N: the B K N L partials and the dA rows grow with N, the dD / d delta_bias rows do not
    w = [_work(2, kd, k, n, 1024) for n in range(1, 17)]
    steps = {b - a for a, b in zip(w, w[1:])}
    assert len(steps) == 1 and steps.pop() > 0
    # in L, within one slab size (the slab size follows the lanes per row, i.e. the length)
    for lens in ((520, 1040, 2080, 1153), (136, 200, 256), (8, 37, 128)):
        assert len({_slab_rows(l) for l in lens}) == 1
        w = {l: _work(2, kd, k, 4, l) for l in lens}
        fixed = 4 * 2 * kd * (4 + 2)
        per_l = {(w[l] - fixed) / l for l in lens}
        assert len(per_l) == 1, per_l


def _launch(n=1, work_bytes=1 << 30, null=None, nb=1, kd=4, k=2, l=16):
    """the launch entry on dummy non-null addresses: every check below comes before any launch"""
    from tramba_amd import hip
    lib = hip.lib()
    p = ctypes.c_void_p(64)
    ptrs = [p] * 17
    if null is not None:
        ptrs[null] = None
    rc = lib.tramba_selective_scan_bwd_det(*ptrs, work_bytes, nb, kd, k, n, l, hip.dt(torch.zeros(1)), 1, None)
    return rc, lib.tramba_last_error().decode()


@pytest.mark.parametrize("null", [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 16])
def test_launch_entry_refuses_null_tensors(null):
    """u, delta, A, B, C, dout, ckpt, du, ddelta, dA, dB, dC and the workspace (D, delta_bias, dD, d delta_bias may be absent)"""
    rc, msg = _launch(null=null)
    assert rc < 0 and "null" in msg, (rc, msg)


@pytest.mark.parametrize("n", [0, 17, -3])
def test_launch_entry_names_dstate_and_the_limit(n):
    rc, msg = _launch(n=n)
    assert rc < 0 and "d_state" in msg and "16" in msg, (rc, msg)


def test_launch_entry_refuses_a_short_workspace():
    need = _work(1, 4, 2, 1, 16)
    assert need > 0
    for short in (0, need - 1):
        rc, msg = _launch(work_bytes=short)
        assert rc < 0 and "workspace" in msg and str(need) in msg, (rc, msg)
    rc, msg = _launch(kd=5)
    assert rc < 0 and "multiple" in msg, (rc, msg)


def test_no_cpu_fallback():
    from tramba_amd import hip
    a = sdc.scan_inputs(1, 2, 2, 16, 33, F32)
    ckpt = torch.zeros(1, 4, 1, 16)
    with pytest.raises(hip.TrambaHipError):
        hip.selective_scan_bwd(a["u"], a["delta"], a["A"], a["B"], a["C"], a["D"], a["delta_bias"], torch.zeros(1, 4, 33), ckpt,
                               True, deterministic=True)


# ----------------------------------------------------------------------------- the switch
def test_switch_defaults_round_trips_and_restores():
    from tramba_amd import ops
    assert ops.get_deterministic_scan() is False and ops._scan_is_deterministic() is False
    try:
        assert ops.set_deterministic_scan(True) is False
        assert ops.get_deterministic_scan() is True and ops._scan_is_deterministic() is True
        assert ops.set_deterministic_scan("torch") is True
        assert ops.set_deterministic_scan(False) == "torch"
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError):
                ops.set_deterministic_scan(bad)
        assert ops.get_deterministic_scan() is False
        with ops.deterministic_scan(True):
            assert ops._scan_is_deterministic() is True
            with ops.deterministic_scan(False):
                assert ops._scan_is_deterministic() is False
            assert ops._scan_is_deterministic() is True
        assert ops.get_deterministic_scan() is False
        with pytest.raises(KeyError):
            with ops.deterministic_scan(True):
                raise KeyError("inside")
        assert ops.get_deterministic_scan() is False
    finally:
        ops.set_deterministic_scan(False)


def test_torch_mode_follows_the_framework_flag():
    from tramba_amd import ops
    before = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        with ops.deterministic_scan("torch"):
            torch.use_deterministic_algorithms(False)
            assert ops._scan_is_deterministic() is False
            torch.use_deterministic_algorithms(True)
            assert ops._scan_is_deterministic() is True
            torch.use_deterministic_algorithms(False)
            assert ops._scan_is_deterministic() is False
        torch.use_deterministic_algorithms(True)
        assert ops._scan_is_deterministic() is False       # mode False does not look at the flag
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


# ----------------------------------------------------------------------------- the GPU tolerance is fit for the sum order
def _slabwise(e, o, s):
    """(L, nb KD, N) per-row fp32 contributions -> (nb, K, N, L): rows of a slab of s added in ascending order with one fp32
    accumulator (rows past the group's end add 0), then the slabs in ascending order"""
    v = e.reshape(o.l, o.nb, o.k, o.dper, o.n)
    slabs = []
    for r0 in range(0, o.dper, s):
        acc = v[:, :, :, r0]
        for r in range(r0 + 1, min(r0 + s, o.dper)):
            acc = acc + v[:, :, :, r]
        slabs.append(acc)
    tot = slabs[0]
    for part in slabs[1:]:
        tot = tot + part
    return tot.permute(1, 2, 3, 0)


@pytest.mark.parametrize("dtype", sdc.BWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", NEW_SHAPES, ids=IDS)
def test_backward_tolerance_has_room_for_the_slab_order(shape, dtype):
    """as test_backward_tolerance_has_room of tests/test_scan_dstate_host.py, on the shapes this form adds and with dB / dC
    summed as the deterministic kernels sum them, at their three slab sizes (8, 16, 32 rows) and at 4 rows: at most 1e-5 on the measure whose bound is 3e-4,
    i.e. a thirtieth of it"""
    a, dout, want = sdc.bwd_case(shape, dtype)
    o = sdc.as_boundary(shape, dtype, a, dout)
    r = smc._tiled(smc._bterms(o, F32), True)
    assert r["eb"].dtype == F32
    ev = smc._bpack(o, r)
    for name, w in zip(sdc.GRADS, want):
        if name in ("dB", "dC"):
            continue
        err = sdc.grad_error(ev[name], w)
        print(shape, dtype, name, f"fp32 tile-wise evaluation: {err:.2e} = {err / 3e-4:.4f} of the bound")
        assert err <= 1e-5, (name, err)
    for s in (4, 8, 16, 32):
        for name, key, w in (("dB", "eb", want[3]), ("dC", "ec", want[4])):
            err = sdc.grad_error(_slabwise(r[key], o, s), w)
            print(shape, dtype, name, f"slab {s}: {err:.2e} = {err / 3e-4:.4f} of the bound")
            assert err <= 1e-5, (name, s, err)
