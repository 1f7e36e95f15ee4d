"""The deterministic (atomic-free) backward of the reference-layout selective scan, hip.selective_scan_bwd(...,
deterministic=True), and the switch tramba_amd.ops.deterministic_scan that routes SelectiveScanOflex and the modules above it
there.  Parity is measured as tests/test_gpu_scan_dstate.py measures the atomic form (same shapes, same fp64 references, same
bounds) plus eight shapes for the compile-time-N kernels and the slab logic; tests/test_scan_det_host.py shows without a GPU that
those bounds leave room for the order in which this form adds dB / dC.  What the atomic form cannot offer is tested bit for
bit: run to run, across a workspace that moved, across streams, whatever the workspace held, and under graph replay."""
import types

import pytest
import torch

import buffer_cases as bc
import scan_dstate_cases as sdc
import scan_memory_cases as smc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:]

# (nb, k, dper, n, l): the list of tests/test_scan_det_host.py
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
BITWISE_SHAPES = [(1, 2, 40, 1, 1153), (2, 3, 7, 4, 200), (1, 4, 4, 16, 1153)]


def hip():
    from tramba_amd import hip as h
    return h


def _args(g):
    return g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["delta_bias"]


def _device_case(shape, dtype):
    a, dout, want = sdc.bwd_case(shape, dtype)
    g = {k_: v.to(DEV) for k_, v in a.items()}
    return g, dout.to(DEV), want


def _det(g, dout, ckpt=None):
    if ckpt is None:
        _, ckpt = hip().selective_scan_fwd(*_args(g), True, True)
    return hip().selective_scan_bwd(*_args(g), dout, ckpt, True, deterministic=True)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- parity
@pytest.mark.parametrize("dtype", sdc.BWD_DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sdc.SHAPES + NEW_SHAPES, ids=IDS)
def test_backward_fast_decay(shape, dtype):
    """measure and tolerance of test_backward_fast_decay of tests/test_gpu_scan_dstate.py: max |err| / max(1, max |want|) < 3e-4,
    1.5e-2 for 16-bit du / ddelta; same dtypes and shapes of the outputs as the atomic form"""
    nb, k, dper, n, l = shape
    g, dout, want = _device_case(shape, dtype)
    got = _det(g, dout)
    kd = k * dper
    shapes = ((nb, kd, l), (nb, kd, l), (kd, n), (nb, k, n, l), (nb, k, n, l), (kd,), (kd,))
    for name, x, s in zip(sdc.GRADS, got, shapes):
        assert x.shape == s and x.is_contiguous() and x.dtype == (dtype if name in ("du", "ddelta") else F32), name
    errs = {name: sdc.grad_error(x.cpu(), w) for name, x, w in zip(sdc.GRADS, got, want)}
    print(shape, dtype, {k_: f"{v:.2e}" for k_, v in errs.items()})
    for name, err in errs.items():
        tol = 3e-4 if (dtype == F32 or name not in ("du", "ddelta")) else 1.5e-2
        assert err < tol, (name, err)


@pytest.mark.parametrize("shape", [(2, 3, 7, 4, 200), (1, 2, 18, 16, 520)], ids=IDS)
def test_backward_without_skip_bias_and_softplus(shape):
    """D = None, delta_bias = None, no softplus, on |delta|: dD and d delta_bias are None, the other five as above"""
    from oracle import selective_scan as oss
    a, dout, _ = sdc.bwd_case(shape, F32)
    delta = a["delta"].abs()
    want = oss.selective_scan_bwd(a["u"], delta, a["A"], a["B"], a["C"], None, None, dout, False)
    H = hip()
    args = [t.to(DEV) for t in (a["u"], delta, a["A"], a["B"], a["C"])] + [None, None]
    _, ckpt = H.selective_scan_fwd(*args, False, True)
    got = H.selective_scan_bwd(*args, dout.to(DEV), ckpt, False, deterministic=True)
    assert got[5] is None and got[6] is None
    for name, x, w in list(zip(sdc.GRADS, got, want))[:5]:
        err = sdc.grad_error(x.cpu(), w)
        print(shape, name, f"{err:.2e}")
        assert err < 3e-4, (name, err)


# ----------------------------------------------------------------------------- long memory
def _det_shim():
    """the library as scan_memory_cases.boundary_records takes it, its backward the deterministic one"""
    H = hip()
    return types.SimpleNamespace(
        selective_scan_nchunk=H.selective_scan_nchunk, selective_scan_fwd=H.selective_scan_fwd, device_error=H.device_error,
        selective_scan_bwd=lambda *a, **kw: H.selective_scan_bwd(*a, deterministic=True, **kw))


def _hold(recs):
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    for r in recs:
        assert r["ok"], r


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("n", [1, 4, 8, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_state_outlives_the_chunks(regime, n, dtype):
    """rows 2 x 4 x 8, four 512-position chunks with the last ragged, the state alive across all of them: every output and
    gradient within 8 x E32 of the fp64 oracle (the rule of tests/golden/scan_memory_cases.py)"""
    _hold(smc.boundary_records(_det_shim(), torch.device(DEV), regime, n, dtype))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
def test_init16_regime(dtype):
    """test_init16_regime of tests/test_gpu_scan_dstate.py on the deterministic backward: 8 x E32, 2.5 x 8 x E32 for dA"""
    H = hip()
    o, ref, e = sdc.init16_e32(dtype)
    g = [t.to(DEV) for t in (o.u, o.delta, o.A, o.B, o.C, o.D, o.delta_bias)]
    out, ckpt = H.selective_scan_fwd(*g, True, True)
    grads = H.selective_scan_bwd(*g, o.dout.to(DEV), ckpt, True, deterministic=True)
    torch.cuda.synchronize()
    H.device_error()
    label = f"init16 {str(dtype)[6:]} L={o.l} deterministic"
    recs = []
    for name, got in zip(smc.BOUNDARY_OUTPUTS[1:], grads):
        assert bool(torch.isfinite(got.float()).all()), name
        out_dtype = dtype if name in ("du", "ddelta") else F32
        rec = smc.record(label, "gA" if name == "dA" else name, got, ref[name], e[name], out_dtype)   # "gA": the 2.5 x rule
        rec["output"] = name
        recs.append(rec)
    _hold(recs)


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("shape", BITWISE_SHAPES, ids=IDS)
def test_bitwise_run_to_run(shape, dtype):
    """five consecutive calls; again after the shared workspace has been grown (and so moved) by an unrelated request of
    another size; again on a side stream (its own workspace) while the first stream runs the same op"""
    H = hip()
    g, dout, _ = _device_case(shape, dtype)
    _, ckpt = H.selective_scan_fwd(*_args(g), True, True)
    first = _det(g, dout, ckpt)
    for i in range(4):
        assert _same(first, _det(g, dout, ckpt)), i
    dev = g["u"].device
    before = H._scan_workspace(dev, 1)
    grown = H._scan_workspace(dev, before.numel() + (3 << 20) + 8)
    assert grown.data_ptr() != before.data_ptr() and grown.numel() != before.numel()
    assert _same(first, _det(g, dout, ckpt))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _det(g, dout, ckpt)
    on_main = _det(g, dout, ckpt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(first, on_side) and _same(first, on_main)
    H.device_error()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("shape", [(1, 2, 40, 1, 1153), (2, 3, 7, 4, 200), (1, 2, 18, 16, 520), (2, 2, 6, 12, 72)], ids=IDS)
def test_results_do_not_depend_on_what_the_workspace_held(shape, dtype):
    """a fresh workspace full of NaN bit patterns (both poisons fill a payload buffer with 0xFF bytes; the float outputs get
    NaN or noise), against a run on the allocator's own memory: finite and bit-identical"""
    H = hip()
    g, dout, _ = _device_case(shape, dtype)
    _, ckpt = H.selective_scan_fwd(*_args(g), True, True)
    plain = _det(g, dout, ckpt)
    assert all(bool(torch.isfinite(t.float()).all()) for t in plain)
    key = (str(g["u"].device), H._stream())
    for fill in ("nan", "noise"):
        with bc.poisoned_allocations(fill):
            if key in H._scan_ws:          # retire the stream's workspace, so that this call allocates (and poisons) a new one
                H._scan_ws_retired.append(H._scan_ws.pop(key))
            got = _det(g, dout, ckpt)
            torch.cuda.synchronize()
        ws = H._scan_ws[key]
        need = H.selective_scan_bwd_det_work(shape[0], shape[1] * shape[2], shape[1], shape[3], shape[4], dtype)
        assert ws.numel() > need + 64 and bool((ws[-64:] == 0xFF).all())     # the poison was there: the unused tail keeps it
        assert all(bool(torch.isfinite(t.float()).all()) for t in got), fill
        assert _same(plain, got), fill


def test_graph_replay_equals_eager():
    """forward + deterministic backward (three slabs per group, so both launches) captured after a warm-up on the capture
    stream: three replays, each bit for bit the eager result"""
    H = hip()
    g, dout, _ = _device_case((1, 2, 18, 16, 520), BF16)

    def step():
        out, ckpt = H.selective_scan_fwd(*_args(g), True, True)
        return (out,) + tuple(H.selective_scan_bwd(*_args(g), dout, ckpt, True, deterministic=True))

    eager = step()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                             # warm-up: the side stream's workspace exists before the capture
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            got = step()
    torch.cuda.current_stream().wait_stream(s)
    for i in range(3):
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, got), i
    H.device_error()


# ----------------------------------------------------------------------------- autograd and modules
def _oflex_grads():
    from tramba_amd import ops
    a, dout, _ = sdc.bwd_case((1, 4, 4, 16, 1153), F32)
    leaves = [a[k_].to(DEV).requires_grad_() for k_ in ("u", "delta", "A", "B", "C", "D", "delta_bias")]
    out = ops.SelectiveScanOflex.apply(*leaves, True)
    out.backward(dout.to(DEV))
    return [t.grad for t in leaves]


def test_autograd_function_is_bitwise_reproducible():
    from tramba_amd import ops
    with ops.deterministic_scan(True):
        first, again = _oflex_grads(), _oflex_grads()
    assert all(x is not None for x in first) and _same(first, again)
    atomic = _oflex_grads()
    for name, x, y in zip(sdc.GRADS, first, atomic):
        rel = float((x.double() - y.double()).norm() / y.double().norm())
        assert rel <= 1e-5, (name, rel)


def _module(kind):
    import tramba_amd as ta
    torch.manual_seed(31)
    if kind == "ss2d":
        m = ta.SS2D(d_model=16, channel_first=True)            # the constructor's own d_state, 16
        assert m.d_state == 16
    else:
        m = ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0)
    gen = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=gen))
    x = torch.randn(2, 16, 12, 12, generator=gen)
    gy = torch.randn(2, 16, 12, 12, generator=gen)
    return m.to(DEV), x.to(DEV), gy.to(DEV)


def _module_grads(m, x, gy, scan_grads):
    """one forward + backward -> {name: gradient}; the scan's own seven gradients are appended to scan_grads"""
    from tramba_amd import ops
    ext = ops.selective_scan_cuda_oflex
    orig = ext.bwd

    def bwd(*a, **kw):
        res = orig(*a, **kw)
        scan_grads.append(res)
        return res

    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_()
    ext.bwd = bwd
    try:
        (m(xi) * gy).sum().backward()
    finally:
        del ext.bwd                         # the staticmethod of the class is back
    grads = {"x": xi.grad.clone()}
    grads.update({name: p.grad.clone() for name, p in m.named_parameters()})
    return grads


@pytest.mark.parametrize("kind", ["ss2d", "vssblock"])
def test_modules_are_bitwise_reproducible_and_match_the_atomic_mode(kind):
    """SS2D(d_model=16) at its default d_state and VSSBlock(ssm_d_state=16), input (2, 16, 12, 12), fp32: under
    deterministic_scan(True) two backward passes give the same bits for the scan's seven gradients, the input and every
    parameter; the gradients match the default (atomic) mode to a relative L2 of 1e-5"""
    from tramba_amd import ops
    m, x, gy = _module(kind)
    scans = [], [], []
    with ops.deterministic_scan(True):
        first = _module_grads(m, x, gy, scans[0])
        again = _module_grads(m, x, gy, scans[1])
    atomic = _module_grads(m, x, gy, scans[2])
    assert len(scans[0]) == len(scans[1]) == len(scans[2]) >= 1
    for a, b in zip(scans[0], scans[1]):
        assert _same(a, b)
    assert set(first) == set(again) == set(atomic)
    for name in first:
        assert first[name] is not None and torch.equal(first[name], again[name]), name
    for name in first:
        rel = float((first[name].double() - atomic[name].double()).norm() / atomic[name].double().norm())
        print(kind, name, f"deterministic vs atomic: {rel:.2e}")
        assert rel <= 1e-5, (name, rel)


def test_the_switch_is_honoured(monkeypatch):
    """mode False: hip.selective_scan_bwd is called for the atomic entry; True: for the new one; "torch": by the framework's
    flag at backward time"""
    from tramba_amd import ops
    H = hip()
    calls = []
    entries = []
    orig = H.selective_scan_bwd
    lib = H.lib()

    def counted(*a, **kw):
        calls.append(bool(kw.get("deterministic", False)))
        return orig(*a, **kw)

    class CountingLib:
        def __getattr__(self, name):
            if name in ("tramba_selective_scan_bwd", "tramba_selective_scan_bwd_det"):
                entries.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(H, "selective_scan_bwd", counted)
    monkeypatch.setattr(H, "lib", lambda: CountingLib())
    _oflex_grads()
    assert calls == [False] and entries == ["tramba_selective_scan_bwd"]
    with ops.deterministic_scan(True):
        _oflex_grads()
    assert calls == [False, True] and entries == ["tramba_selective_scan_bwd", "tramba_selective_scan_bwd_det"]
    _oflex_grads()
    assert calls == [False, True, False] and entries[-1] == "tramba_selective_scan_bwd"
    before = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        with ops.deterministic_scan("torch"):
            torch.use_deterministic_algorithms(True, warn_only=True)
            _oflex_grads()
            torch.use_deterministic_algorithms(False)
            _oflex_grads()
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)
    assert calls[3:] == [True, False] and entries[-2:] == ["tramba_selective_scan_bwd_det", "tramba_selective_scan_bwd"]
