"""GPU tests of the step-control kernels (tramba_grad_accumulate, tramba_grad_norm, tramba_adam_step_ctl) and of the
controlled optimisation step built on them: eager, as hipGraphs, and under a data-parallel reducer."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

from oracle import ops as oo
from test_gpu_sched_ema import _Flat, edge_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the shapes of tests/test_gpu_step_ends.py's Adam tests: 1 .. 100003 elements, ragged tails
ADAM_SHAPES = [(1,), (3,), (4,), (5,), (8191,), (8192,), (8193,), (3, 7, 11), (100003,), (64, 1, 7, 7), (1024, 512), (2, 16389)]


def _rel_l2(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-30))


def _numel(ts):
    return (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])


def _odd_views(tensors, start=1):
    """copies of the tensors as views at odd offsets of one flat buffer (the unaligned path)"""
    flat = torch.zeros(start + sum(t.numel() + 1 for t in tensors), device=DEV)
    views, off = [], start
    for t in tensors:
        v = flat[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        views.append(v)
        off += t.numel() + 1
    assert any(v.data_ptr() % 16 for v in views)
    return views


# ------------------------------------------------------------------------------------------------- tramba_grad_accumulate
@pytest.mark.parametrize("layout", ["aligned", "odd_gradients", "odd_both"])
def test_grad_accumulate_adds_in_micro_batch_order(layout):
    from tramba_amd import hip
    g = torch.Generator().manual_seed(5)
    micro = [[(torch.randn(s, generator=g) * 10.0 ** (i % 5 - 2)).to(DEV) for i, s in enumerate(ADAM_SHAPES)] for _ in range(4)]
    if layout != "aligned":
        micro = [_odd_views(gs, start=1 + k) for k, gs in enumerate(micro)]
    acc = [torch.full(s, float("nan"), device=DEV) for s in ADAM_SHAPES]     # a first micro-batch that ADDS cannot pass
    if layout == "odd_both":
        acc = _odd_views(acc, start=3)
    rec, f = hip.step_ctl_record(DEV)
    n = len(acc)
    for k, gs in enumerate(micro):
        assert int(f["micro"]) == k
        hip.grad_accumulate_raw(hip.pointer_array(acc), hip.pointer_array(gs), _numel(acc), n, rec)
    assert int(f["micro"]) == 4
    for a, g0, g1, g2, g3 in zip(acc, *micro):
        assert torch.equal(a, ((g0 + g1) + g2) + g3), tuple(a.shape)
    # a null gradient stands for zeros: stored on a first micro-batch, nothing to add later
    f["micro"].zero_()
    grads = (ctypes.c_void_p * n)(*[None if i % 2 else t.data_ptr() for i, t in enumerate(micro[0])])
    hip.grad_accumulate_raw(hip.pointer_array(acc), grads, _numel(acc), n, rec)
    hip.grad_accumulate_raw(hip.pointer_array(acc), hip.pointer_array(micro[1]), _numel(acc), n, rec)
    grads = (ctypes.c_void_p * n)(*[None if i % 3 == 0 else t.data_ptr() for i, t in enumerate(micro[2])])
    hip.grad_accumulate_raw(hip.pointer_array(acc), grads, _numel(acc), n, rec)
    for i, a in enumerate(acc):
        want = (torch.zeros_like(a) if i % 2 else micro[0][i]) + micro[1][i]
        want = want if i % 3 == 0 else want + micro[2][i]
        assert torch.equal(a, want), i


def test_grad_accumulate_many_tensors_span_several_launches():
    """more tensors than one launch carries (128): every one is visited exactly once"""
    from tramba_amd import hip
    g = torch.Generator().manual_seed(6)
    shapes = [(1 + (37 * i) % 300,) for i in range(700)]
    a = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    b = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    acc = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    rec, f = hip.step_ctl_record(DEV)
    for gs in (a, b):
        hip.grad_accumulate_raw(hip.pointer_array(acc), hip.pointer_array(gs), _numel(acc), len(acc), rec)
    assert all(torch.equal(c, x + y) for c, x, y in zip(acc, a, b))


@pytest.mark.parametrize("count", [128, 129])                  # kAccTensors = 128 in csrc/loss_optim.hip
def test_grad_accumulate_fills_its_table_and_one_slot_more(count):
    """128 tensors fill the one launch's table to its last slot; 129 make two launches of 65 and 64"""
    from tramba_amd import hip
    g = torch.Generator().manual_seed(16)
    sizes = edge_sizes(count)
    a = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    b = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    acc = [torch.full((n,), float("nan"), device=DEV) for n in sizes]      # a tensor that no workgroup visits keeps its NaNs
    rec, f = hip.step_ctl_record(DEV)
    for gs in (a, b):
        hip.grad_accumulate_raw(hip.pointer_array(acc), hip.pointer_array(gs), _numel(acc), count, rec)
    assert int(f["micro"]) == 2
    wrong = [i for i, (c, x, y) in enumerate(zip(acc, a, b)) if not torch.equal(c, x + y)]
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------- tramba_grad_norm
def _norm(tensors, mean_scale=1.0, max_norm=0.0, skip_nonfinite=True, rec=None):
    from tramba_amd import hip
    if rec is None:
        rec = hip.step_ctl_record(DEV)
    numel = _numel(tensors)
    ws = torch.empty((hip.grad_norm_workspace(numel, len(tensors)) + 7) // 8, dtype=torch.float64, device=DEV)
    hip.grad_norm_raw(hip.pointer_array(tensors), numel, len(tensors), mean_scale, max_norm, skip_nonfinite, rec[0], ws)
    torch.cuda.synchronize()
    return rec


BOUND = 2.0 ** -22     # <= 2^27 exact products added in fp64: 2^-26 relative; the root halves it; the cast to fp32: 2^-24


@pytest.mark.parametrize("scale", [1e-6, 1.0, 1e6])
@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_grad_norm_against_numpy_fp64(scale, layout):
    g = torch.Generator().manual_seed(9)
    host = [torch.randn(s, generator=g) * scale * 10.0 ** (i % 3 - 1) for i, s in enumerate(ADAM_SHAPES)]
    ts = [t.to(DEV) for t in host]
    if layout == "odd":
        ts = _odd_views(ts)
    want = float(np.sqrt(sum(float((t.numpy().astype(np.float64) ** 2).sum()) for t in host)))
    for mean_scale, max_norm in ((1.0, 0.0), (0.25, 0.5 * 0.25 * want), (0.25, 4.0 * want), (0.125, 1e-3 * want)):
        rec, f = _norm(ts, mean_scale, max_norm)
        norm, sc = float(f["norm"]), float(f["scale"])
        print(f"scale {scale:g} {layout}: norm {norm!r} want {want * mean_scale!r} rel {abs(norm / (want * mean_scale) - 1):.3e}")
        assert abs(norm - want * mean_scale) <= BOUND * want * mean_scale
        want_scale = mean_scale * min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else mean_scale
        assert abs(sc - want_scale) <= BOUND * want_scale, (sc, want_scale)
        assert int(f["skip"]) == 0 and int(f["micro"]) == 0 and int(f["skipped_steps"]) == 0
        again = _norm(ts, mean_scale, max_norm)
        assert torch.equal(again[0], rec)                                   # two runs: identical bits


def test_grad_norm_many_tensors_span_several_launches():
    """more tensors than one launch carries (160): the partials of every launch land in their own slots"""
    g = torch.Generator().manual_seed(13)
    shapes = [(1 + (41 * i) % 9000,) for i in range(700)]
    host = [torch.randn(s, generator=g) * 10.0 ** (i % 4 - 2) for i, s in enumerate(shapes)]
    want = float(np.sqrt(sum(float((t.numpy().astype(np.float64) ** 2).sum()) for t in host)))
    ts = [t.to(DEV) for t in host]
    rec, f = _norm(ts, 0.5, 0.0)
    assert abs(float(f["norm"]) - 0.5 * want) <= BOUND * 0.5 * want and int(f["skip"]) == 0
    assert torch.equal(_norm(ts, 0.5, 0.0)[0], rec)
    ts[650][-1] = float("nan")                                   # a small tensor of a late launch
    assert int(_norm(ts, 0.5, 0.0)[1]["skip"]) == 1


@pytest.mark.parametrize("count", [160, 161])                  # kNormTensors = 160 in csrc/loss_optim.hip
def test_grad_norm_fills_its_table_and_one_slot_more(count):
    """160 tensors fill the one launch's table to its last slot; 161 make two launches of 81 and 80"""
    g = torch.Generator().manual_seed(17)
    host = [torch.randn(n, generator=g) * 10.0 ** (i % 4 - 2) for i, n in enumerate(edge_sizes(count))]
    want = float(np.sqrt(sum(float((t.numpy().astype(np.float64) ** 2).sum()) for t in host)))
    ts = [t.to(DEV) for t in host]
    rec, f = _norm(ts, 0.5, 0.0)
    print(f"{count} tensors: norm {float(f['norm'])!r} want {0.5 * want!r} rel {abs(float(f['norm']) / (0.5 * want) - 1):.3e}")
    assert abs(float(f["norm"]) - 0.5 * want) <= BOUND * 0.5 * want and int(f["skip"]) == 0
    assert torch.equal(_norm(ts, 0.5, 0.0)[0], rec)                        # two runs: identical bits
    # the sum would not miss a single element at 0.01: a NaN in the last element of each tensor in turn, the last tensor's
    # among them, must raise the flag
    for i in range(count):
        was = ts[i][-1].clone()
        ts[i][-1] = float("nan")
        assert int(_norm(ts, 0.5, 0.0)[1]["skip"]) == 1, i
        ts[i][-1] = was
    assert torch.equal(_norm(ts, 0.5, 0.0)[0], rec)


def test_grad_norm_survives_a_square_that_overflows_fp32():
    g = torch.Generator().manual_seed(10)
    host = [torch.randn(s, generator=g) for s in ADAM_SHAPES[4:9]]
    host[2][17] = 3e19
    want = float(np.sqrt(sum(float((t.numpy().astype(np.float64) ** 2).sum()) for t in host)))
    rec, f = _norm([t.to(DEV) for t in host], 1.0, 1.0)
    assert np.isfinite(float(f["norm"])) and abs(float(f["norm"]) - want) <= BOUND * want
    assert int(f["skip"]) == 0 and int(f["skipped_steps"]) == 0


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")])
def test_grad_norm_finds_every_non_finite_element(value):
    from tramba_amd import hip
    g = torch.Generator().manual_seed(12)
    shapes = [(100003,), (5,), (8193,), (2, 16389)]
    rec = hip.step_ctl_record(DEV)
    planted = 0
    for which in (0, len(shapes) - 1):
        n = int(np.prod(shapes[which]))
        for pos in (0, n // 2, n - 1):
            ts = [torch.randn(s, generator=g).to(DEV) for s in shapes]
            ts[which].view(-1)[pos] = value
            rec[1]["micro"].fill_(3)
            _norm(ts, 0.5, 1.0, True, rec)
            planted += 1
            assert int(rec[1]["skip"]) == 1 and int(rec[1]["skipped_steps"]) == planted, (which, pos)
            assert int(rec[1]["micro"]) == 0
            # the caller did not ask for skipping: the flag stays down, nothing is counted
            loose = _norm(ts, 0.5, 1.0, False)
            assert int(loose[1]["skip"]) == 0 and int(loose[1]["skipped_steps"]) == 0
    clean = _norm([torch.randn(s, generator=g).to(DEV) for s in shapes], 0.5, 1.0, True, rec)
    assert int(clean[1]["skip"]) == 0 and int(clean[1]["skipped_steps"]) == planted


# ------------------------------------------------------------------------------------------------- tramba_adam_step_ctl
def _adam_run(wd, grads_per_step, init, gscale=None, skip=None, views=False):
    from tramba_amd import train
    params = [torch.nn.Parameter(p.to(DEV)) for p in init]
    opt = train.Adam(params, 1e-2, weight_decay=wd)
    for grads in grads_per_step:
        gs = [gr.to(DEV) for gr in grads]
        if views:
            gs = _odd_views(gs)
        for p, gr in zip(params, gs):
            p.grad = gr
        opt.step(gscale=gscale, skip=skip)
    torch.cuda.synchronize()
    state = [opt.state[p] for p in params]
    return ([p.detach() for p in params], [s["exp_avg"] for s in state], [s["exp_avg_sq"] for s in state],
            [s["step"] for s in state])


def _same(a, b):
    return all(torch.equal(x, y) for xs, ys in zip(a, b) for x, y in zip(xs, ys))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_ctl(wd):
    from tramba_amd import hip
    g = torch.Generator().manual_seed(7)
    init = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    steps = [[torch.randn(s, generator=g) * (10.0 ** (i % 3 - 2)) for i, s in enumerate(ADAM_SHAPES)] for _ in range(4)]
    plain = _adam_run(wd, steps, init)
    one, zero = torch.ones((), device=DEV), torch.zeros((), dtype=torch.int32, device=DEV)
    # (a) both pointers null is the plain entry; called here through the ctl entry itself
    params = [torch.nn.Parameter(p.to(DEV)) for p in init]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    ts = [torch.zeros((), device=DEV) for _ in params]
    for grads in steps:
        gs = [gr.to(DEV) for gr in grads]
        rc = hip.lib().tramba_adam_step_ctl(hip.pointer_array(params), hip.pointer_array(gs), hip.pointer_array(ms),
                                            hip.pointer_array(vs), hip.pointer_array(ts), _numel(params), len(params), 1e-2, 0.9,
                                            0.999, 1e-8, wd, None, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    assert _same(([p.detach() for p in params], ms, vs, ts), plain)
    # (b) gscale = 1, skip = 0
    assert _same(_adam_run(wd, steps, init, gscale=one, skip=zero), plain)
    assert _same(_adam_run(wd, steps, init, gscale=one, skip=zero, views=True), plain)
    # (c) a scale: the plain entry on gradients multiplied in fp32 beforehand, and the fp64 oracle on the exact products
    for s in (0.25, 0.3):
        sc = torch.full((), s, device=DEV)
        got = _adam_run(wd, steps, init, gscale=sc)
        pre = [[(gr.to(DEV) * sc).cpu() for gr in grads] for grads in steps]
        assert _same(got, _adam_run(wd, pre, init)), s
        assert _same(_adam_run(wd, steps, init, gscale=sc, skip=zero, views=True), got), s
        want_p, want_m, want_v = oo.adam_steps(init, [[gr.double() * float(sc) for gr in grads] for grads in steps], 1e-2,
                                               (0.9, 0.999), 1e-8, wd)
        for i in range(len(init)):
            assert _rel_l2(got[0][i], want_p[i]) < 1e-6, (s, ADAM_SHAPES[i])
            assert _rel_l2(got[1][i], want_m[i]) < 1e-6 and _rel_l2(got[2][i], want_v[i]) < 1e-6
    # (d) skip = 1: every tensor and every step counter keeps its bits
    two = _adam_run(wd, steps[:2], init)
    flag = torch.ones((), dtype=torch.int32, device=DEV)
    params = [torch.nn.Parameter(p.clone()) for p in two[0]]
    from tramba_amd import train
    opt = train.Adam(params, 1e-2, weight_decay=wd)
    for p, m, v, t in zip(params, two[1], two[2], two[3]):
        opt.state[p] = {"step": t.clone(), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        p.grad = torch.full_like(p, float("nan"))
    opt.step(gscale=torch.full((), 0.5, device=DEV), skip=flag)
    torch.cuda.synchronize()
    st = [opt.state[p] for p in params]
    assert _same(([p.detach() for p in params], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st],
                  [s["step"] for s in st]), two)


@pytest.mark.parametrize("count", [72, 73])                    # kAdamTensors = 72 in csrc/loss_optim.hip
def test_adam_step_ctl_fills_its_table_and_one_slot_more(count):
    """72 tensors fill the one launch's table to its last slot; 73 make two launches of 37 and 36.  Every tensor against the
    fp64 oracle at test_adam_step_ctl's tolerance, guard elements on either side of each."""
    from tramba_amd import hip
    g = torch.Generator().manual_seed(18)
    sizes = edge_sizes(count)
    init = [torch.randn(n, generator=g) for n in sizes]
    steps = [[torch.randn(n, generator=g) * (10.0 ** (i % 3 - 2)) for i, n in enumerate(sizes)] for _ in range(2)]
    start = iter(init)
    p = _Flat(sizes, 4, lambda n: next(start))
    gr, m, v = (_Flat(sizes, 4, torch.zeros) for _ in range(3))
    ts = torch.zeros(count, device=DEV)
    sc, zero = torch.full((), 0.3, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV)
    for grads in steps:
        for view, x in zip(gr.views, grads):
            view.copy_(x)
        rc = hip.lib().tramba_adam_step_ctl(hip.pointer_array(p.views), hip.pointer_array(gr.views), hip.pointer_array(m.views),
                                            hip.pointer_array(v.views), hip.pointer_array([ts[i] for i in range(count)]),
                                            (ctypes.c_int64 * count)(*sizes), count, 1e-2, 0.9, 0.999, 1e-8, 0.01,
                                            sc.data_ptr(), zero.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    want_p, want_m, want_v = oo.adam_steps(init, [[x.double() * float(sc) for x in grads] for grads in steps], 1e-2, (0.9, 0.999),
                                           1e-8, 0.01)
    for i in range(count):
        errs = _rel_l2(p.views[i], want_p[i]), _rel_l2(m.views[i], want_m[i]), _rel_l2(v.views[i], want_v[i])
        assert max(errs) < 1e-6, (i, sizes[i], errs)
    assert bool((ts == 2.0).all())
    assert all(t.guards_intact() for t in (p, gr, m, v))
    for view, x in zip(gr.views, steps[-1]):                               # the gradients are read, never written
        assert torch.equal(view.cpu(), x)


def test_adam_step_ctl_replay_follows_the_record():
    """(e) captured once, replayed with the record changed between replays"""
    from tramba_amd import hip, train
    g = torch.Generator().manual_seed(8)
    shapes = [(1001,), (33, 5), (8193,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [torch.randn(s, generator=g) for s in shapes]
    rec, f = hip.step_ctl_record(DEV)
    params = [torch.nn.Parameter(p.to(DEV)) for p in init]
    opt = train.Adam(params, 1e-2, capturable=True)
    for p, gr in zip(params, grads):
        p.grad = gr.to(DEV)
    f["scale"].fill_(1.0)
    opt.step(gscale=f["scale"], skip=f["skip"])             # eager: creates the state (step 1, scale 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(gscale=f["scale"], skip=f["skip"])
    f["scale"].fill_(0.5)
    graph.replay()                                          # step 2 at scale 0.5
    f["skip"].fill_(1)
    graph.replay()                                          # skipped
    f["skip"].fill_(0)
    f["scale"].fill_(2.0)
    graph.replay()                                          # step 3 at scale 2
    torch.cuda.synchronize()
    scaled = [[gr * s for gr in grads] for s in (1.0, 0.5, 2.0)]
    want = _adam_run(0.0, scaled, init)
    got = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params],
           [opt.state[p]["step"] for p in params])
    assert _same(got, want)
    assert all(float(t) == 3.0 for t in got[3])


# ------------------------------------------------------------------------------------------------- the controlled step
def _tramba_v(seed, capturable=False, lr=1e-4):
    import tramba_amd as ta
    from tramba_amd import train
    torch.manual_seed(seed)
    m = ta.bulid_model(use_pretrain=False, img_size=384).to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, ta.DropPath):
            mod.drop_prob = 0.0
    m.compute_dtype = torch.bfloat16
    return m, train.get_opt(lr, m, capturable=capturable)


def _batch(n):
    x = torch.randn(n, 3, 384, 384, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = (torch.rand(n, 1, 384, 384, generator=torch.Generator().manual_seed(1)) > 0.7).float().to(DEV)
    return x, y


def test_tramba_v_accumulated_step_against_standing_gradients_and_the_whole_batch():
    """Tramba-V 384x384 bf16, 8 images as 4 micro-batches of 2.  The accumulators equal, bit for bit and on EVERY
    parameter (no exception: the training path sums without atomics), four backward passes into standing gradients;
    and the step agrees with one plain step on the 8 images as a batch agrees with its halves
    (test_tramba_v_train_step_at_the_baseline_batch: its probes, its tolerances)."""
    from tramba_amd import train
    m, opt = _tramba_v(0)
    x, y = _batch(8)
    names = dict((p, n) for n, p in m.named_parameters())
    probes = [p for n, p in m.named_parameters() if p.numel() >= 65536][::12] + [p for n, p in m.named_parameters() if "A_logs" in n][:3]
    for p in m.parameters():
        p.grad = None
    l8 = train.tramba_loss(m(x), y)
    l8.backward()
    l8, g8 = float(l8.detach()), [p.grad.detach().double().clone() for p in probes]
    for p in m.parameters():
        p.grad = None
    for xs, ys in zip(x.chunk(4), y.chunk(4)):
        train.tramba_loss(m(xs), ys).backward()             # as it was done before: the engine adds into .grad
    standing = {p: p.grad.detach().clone() for p in m.parameters() if p.grad is not None}
    control = train.StepControl(accumulate=4)
    loss = float(train.train_step(m, opt, x, y, control=control))
    torch.cuda.synchronize()
    differ = [names[p] for p, g in standing.items() if p.grad is None or not torch.equal(p.grad, g)]
    assert not differ and len(standing) == sum(p.grad is not None for p in m.parameters()), (len(differ), differ[:8])
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in standing.values()))) / 4
    print(f"loss: 8 images {l8!r}, 4 x 2 images {loss!r}; norm of the mean gradient {float(control.grad_norm)!r} ({total!r})")
    assert abs(float(control.grad_norm) - total) <= 1e-5 * total
    assert abs(loss - l8) <= 2e-3 * abs(l8), (loss, l8)
    for p, g in zip(probes, g8):
        got = p.grad.detach().double() * 0.25
        cos = float((g * got).sum() / (g.norm() * got.norm() + 1e-30))
        assert cos > 0.995 and 0.97 < float(got.norm() / g.norm()) < 1.03, (names[p], cos, float(got.norm() / g.norm()))
    assert int(control.skipped_steps) == 0


def _kernel_counts(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    counts = {}
    for ev in prof.key_averages():
        counts[ev.key] = counts.get(ev.key, 0) + ev.count
    pick = lambda word: sum(c for k, c in counts.items() if word in k)   # noqa: E731
    return {"adam": pick("adam_kernel"), "shadow": pick("shadow_cast"), "accumulate": pick("grad_accumulate_kernel"),
            "norm": pick("grad_norm_finish_kernel")}


def test_graphed_controlled_step_follows_the_eager_one():
    import tramba_amd as ta
    from tramba_amd import train
    x, y = _batch(8)
    m, opt = _tramba_v(11)
    # the norm of the first step's mean gradient, without stepping: the clip norm is chosen below it
    for xs, ys in zip(x.chunk(4), y.chunk(4)):
        train.tramba_loss(m(xs), ys).backward()
    norm0 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None))) / 4
    for p in m.parameters():
        p.grad = None
    clip = 0.5 * norm0
    make = lambda: train.StepControl(accumulate=4, clip_norm=clip, skip_nonfinite=True)   # noqa: E731
    control = make()
    eager = [float(train.train_step(m, opt, x, y, control=control))]
    eager_norm = float(control.grad_norm)
    assert eager_norm > clip and eager_norm == pytest.approx(norm0, rel=1e-4)          # clipping is active
    assert float(control._fields["scale"]) == pytest.approx(0.25 * clip / eager_norm, rel=1e-5)
    eager += [float(train.train_step(m, opt, x, y, control=control)) for _ in range(5)]
    # launches per optimizer step: Adam and the shadow refresh once, not once per micro-batch
    plain = _kernel_counts(lambda: train.train_step(m, opt, x[:2], y[:2]))
    ctl = _kernel_counts(lambda: train.train_step(m, opt, x, y, control=control))
    print("kernel launches, plain step:", plain, "controlled step of 4 micro-batches:", ctl)
    assert plain["adam"] > 0 and plain["shadow"] > 0 and plain["accumulate"] == 0
    assert ctl["adam"] == plain["adam"] and ctl["shadow"] == plain["shadow"] and ctl["norm"] == 1
    assert ctl["accumulate"] > 0 and ctl["accumulate"] % 4 == 0
    del m, opt

    m, opt = _tramba_v(11, capturable=True)
    control = make()
    step = ta.GraphedTrainStep(m, opt, control=control)
    probe = next(p for n, p in m.named_parameters() if n.endswith("weight") and p.ndim == 2)
    start = probe.detach().clone()
    got = [float(step(x, y))]
    assert float(control.grad_norm) == pytest.approx(eager_norm, rel=1e-5)
    assert int(control.skipped_steps) == 0 and not torch.equal(start, probe)
    assert all(float(st["step"]) == 1.0 for st in opt.state.values())                 # the warm-up steps were undone
    got += [float(step(x, y)) for _ in range(5)]
    print("eager", eager, "graphed", got)
    assert got[0] == pytest.approx(eager[0], rel=1e-5)
    assert np.allclose(got, eager, rtol=3e-2), (got, eager)
    # one replay on a batch with a NaN pixel (in the third micro-batch): nothing moves, the step is counted
    entry = next(iter(step._graphs.values()))
    assert len(step._graphs) == 1 and entry["mid"] is not None and len(entry["update"]) == 1
    state = lambda: [p.detach().clone() for p in m.parameters()] + [v.clone() for st in opt.state.values() for v in st.values()]   # noqa: E731
    before = state()
    bad = x.clone()
    bad[5, 1, 100, 100] = float("nan")
    step(bad, y)
    after = state()
    assert int(control.skipped_steps) == 1
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    loss = float(step(x, y))                                                         # the next clean replay steps again
    assert np.isfinite(loss) and int(control.skipped_steps) == 1
    assert not all(torch.equal(a, b) for a, b in zip(after, state()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    # a short last group (2 micro-batches): an update graph of its own, the full one stays
    mid, full = entry["mid"], next(iter(entry["update"].values()))
    short = float(step(list(x.chunk(4))[:2], list(y.chunk(4))[:2]))
    assert np.isfinite(short) and len(step._graphs) == 1 and len(entry["update"]) == 2
    assert entry["mid"] is mid and next(iter(entry["update"].values())) is full
    assert float(control._fields["scale"]) <= 0.5 and np.isfinite(float(step(x, y)))


def test_a_step_that_died_between_micro_batches_does_not_leak_into_the_next():
    """the record's counter is left standing by a step that raised after its first micro-batch: the next step still stores"""
    from tramba_amd import train
    x, y = _dp_data(4)
    x, y = x.to(DEV), y.to(DEV)
    class Fragile(_TinyDP):
        fail_at, calls = -1, 0

        def forward(self, z):
            self.calls += 1
            if self.calls == self.fail_at:
                raise RuntimeError("the loader handed over a broken batch")
            return super().forward(z)

    runs = []
    for broken in (False, True):
        model = Fragile().to(DEV).train()
        opt = train.get_opt(1e-3, model)
        control = train.StepControl(accumulate=2)
        train.train_step(model, opt, x, y, control=control)
        if broken:
            model.fail_at = model.calls + 2
            with pytest.raises(RuntimeError, match="broken batch"):
                train.train_step(model, opt, x, y, control=control)          # the second forward raises
            assert int(control._fields["micro"]) == 1
        train.train_step(model, opt, x, y, control=control)
        runs.append(([p.detach().clone() for p in model.parameters()], float(control.grad_norm)))
    assert runs[0][1] == pytest.approx(runs[1][1], rel=1e-5)
    for a, b in zip(*[r[0] for r in runs]):
        assert _rel_l2(a, b) < 1e-5


def test_graphed_control_refuses_what_cannot_be_captured():
    """fp64 device parameters take torch's functions, whose skip decision is a host read: a clear refusal, no capture error"""
    import tramba_amd as ta
    from tramba_amd import train

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = torch.nn.Conv2d(3, 1, 3, padding=1)

        def forward(self, z):
            return [self.encoder(z)]

    model = Toy().double().to(DEV).train()
    opt = train.get_opt(1e-3, model, capturable=True)
    assert type(opt) is torch.optim.Adam
    step = ta.GraphedTrainStep(model, opt, control=train.StepControl(accumulate=2, skip_nonfinite=True))
    x = torch.randn(4, 3, 16, 16, dtype=torch.float64, device=DEV)
    y = (torch.rand(4, 1, 16, 16, device=DEV) > 0.5).double()
    with pytest.raises(RuntimeError, match="can be captured"):
        step(x, y)


# ------------------------------------------------------------------------------------------------- data parallel
class _TinyDP(torch.nn.Module):
    """a VSSBlock behind the interface train.train_step expects (a list of logit maps; the name holds "encoder")"""

    def __init__(self):
        super().__init__()
        import tramba_amd as ta
        torch.manual_seed(11)
        self.encoder = ta.VSSBlock(hidden_dim=64, drop_path=0.0, channel_first=True)
        self.compute_dtype = None

    def forward(self, z):
        return [self.encoder(z).mean(dim=1, keepdim=True)]


class _TinySpare(_TinyDP):
    """plus a per-channel gain that only the forwards listed in `on` use (`calls` counts them)"""

    def __init__(self):
        super().__init__()
        self.spare = torch.nn.Parameter(torch.full((64,), 0.5))
        self.on, self.calls = (), 0

    def forward(self, z):
        out = self.encoder(z)
        if self.calls in self.on:
            out = out * (1.0 + self.spare.view(1, -1, 1, 1))
        self.calls += 1
        return [out.mean(dim=1, keepdim=True)]


def test_a_parameter_used_late_or_not_at_all_on_the_device():
    """The device form of the store-on-first rule: a parameter first used in a step's SECOND micro-batch must not add onto
    an older step's sums, and one that a step does not use at all must not count in that step's norm (which is taken over
    the flat accumulator buffer) nor be stepped."""
    import copy
    from tramba_amd import train
    model = _TinySpare().to(DEV).train()
    opt = train.get_opt(1e-3, model)
    assert isinstance(opt, train.Adam)
    control = train.StepControl(accumulate=2)
    x, y = _dp_data(4)
    x, y = x.to(DEV), y.to(DEV)
    for on in ((0, 1), (1,), (), (0,)):
        ref = copy.deepcopy(model)
        ref.on, ref.calls = on, 0
        for xs, ys in zip(x.chunk(2), y.chunk(2)):
            train.tramba_loss(ref(xs), ys).backward()
        want = {n: p.grad for n, p in ref.named_parameters()}
        spare_before = model.spare.detach().clone()
        model.on, model.calls = on, 0
        train.train_step(model, opt, x, y, control=control)
        for n, p in model.named_parameters():
            if want[n] is None:
                assert p.grad is None, (on, n)
            else:
                assert _rel_l2(p.grad, want[n]) < 1e-5, (on, n, _rel_l2(p.grad, want[n]))
        norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in want.values() if g is not None))) / 2
        assert float(control.grad_norm) == pytest.approx(norm, rel=1e-5), on
        if not on:
            assert float(control._acc[model.spare].abs().max()) == 0.0
            assert torch.equal(model.spare.detach(), spare_before)
        else:
            assert not torch.equal(model.spare.detach(), spare_before)


def _dp_data(n):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, 64, 24, 24, generator=g), (torch.rand(n, 1, 24, 24, generator=g) > 0.5).float()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_gpu_worker(rank, world, port, out_dir, steps):
    import torch.distributed as dist
    from tramba_amd import parallel, train
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)                       # both ranks share the one card of the test box
        model = _TinyDP().to("cuda").train()
        parallel.broadcast_parameters(model, src=0)
        red = parallel.GradBucketReducer(model, bucket_mb=0.05)
        opt = train.get_opt(1e-2, model)
        control = train.StepControl(accumulate=2, clip_norm=1e3, skip_nonfinite=True)
        x, y = _dp_data(8)
        xs = [x[2 * j:2 * j + 2].to("cuda") for j in range(rank, 4, world)]
        ys = [y[2 * j:2 * j + 2].to("cuda") for j in range(rank, 4, world)]
        for _ in range(steps):
            train.train_step(model, opt, xs, ys, reducer=red, control=control)
        torch.cuda.synchronize()
        torch.save({"sd": {k: v.cpu() for k, v in model.state_dict().items()}, "nbuckets": len(red.buckets),
                    "norm": float(control.grad_norm), "skipped": int(control.skipped_steps)},
                   os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_dp2_times_accumulate2_on_the_device_matches_one_process_accumulate4(tmp_path):
    """two ranks on one card x accumulate=2 (gloo carrying the accumulated buckets, once per optimizer step) against one
    process x accumulate=4, the device kernels in both"""
    import torch.multiprocessing as mp
    from tramba_amd import train
    steps, world = 3, 2
    mp.spawn(_dp_gpu_worker, args=(world, _free_port(), str(tmp_path), steps), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert r0["nbuckets"] > 1 and r0["skipped"] == 0
    model = _TinyDP().to(DEV).train()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(accumulate=4, clip_norm=1e3, skip_nonfinite=True)
    x, y = _dp_data(8)
    x, y = x.to(DEV), y.to(DEV)
    for _ in range(steps):
        train.train_step(model, opt, x, y, control=control)
    moved, ref0 = 0.0, _TinyDP().state_dict()
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(r0["sd"][k].numpy(), v.cpu().numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k
        moved = max(moved, float((v.cpu() - ref0[k]).abs().max()))
    assert moved > 1e-3
    assert r0["norm"] == r1["norm"] and r0["norm"] == pytest.approx(float(control.grad_norm), rel=2e-3)


def _rccl_one_rank_worker(rank, port):
    import faulthandler
    import torch.distributed as dist
    import tramba_amd as ta
    from tramba_amd import parallel, train
    faulthandler.enable(file=sys.stderr, all_threads=True)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        x, y = _dp_data(8)
        x, y = x.to(DEV), y.to(DEV)
        ref = _TinyDP().to(DEV).train()
        opt = train.get_opt(1e-3, ref)
        control = train.StepControl(accumulate=4, clip_norm=1e3)
        want = [float(train.train_step(ref, opt, x, y, control=control)) for _ in range(3)]
        for graphed in (False, True):
            model = _TinyDP().to(DEV).train()
            red = parallel.GradBucketReducer(model, bucket_mb=0.05)
            assert red.world == 1 and red._native_avg and len(red.buckets) > 1
            red.world = 2                      # force the collective path (a one-rank group averages over one rank)
            opt = train.get_opt(1e-3, model, capturable=graphed)
            control = train.StepControl(accumulate=4, clip_norm=1e3)
            if graphed:
                step = ta.GraphedTrainStep(model, opt, reducer=red, control=control)
                got = [float(step(x, y)) for _ in range(3)]
            else:
                got = [float(train.train_step(model, opt, x, y, reducer=red, control=control)) for _ in range(3)]
            torch.cuda.synchronize()
            assert np.allclose(got, want, rtol=2e-3), (graphed, got, want)
            for (k, a), b in zip(model.state_dict().items(), ref.state_dict().values()):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
            red.remove_hooks()
    finally:
        dist.destroy_process_group()


def test_controlled_step_on_a_one_rank_rccl_group():
    """the accumulated buckets through RCCL's ncclAvg (one rank), eagerly and captured into the update graph; in a fresh
    child process: an abort inside the runtime fails this test only"""
    import torch.multiprocessing as mp
    mp.spawn(_rccl_one_rank_worker, args=(_free_port(),), nprocs=1, join=True)
