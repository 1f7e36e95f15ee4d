"""GPU tests of dynamic loss scaling: the two library entries (tramba_grad_norm_scaled, tramba_loss_scale_update), and the
controlled step with a scale -- fp16 compute with and without one, fp32 compute bit for bit, overflow and recovery, the
captured step against the eager one, two data-parallel ranks."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1,), (3,), (5,), (8191,), (8192,), (8193,), (3, 7, 11), (100003,), (64, 1, 7, 7), (2, 16389)]
BOUND = 2.0 ** -22     # the bound of tests/test_gpu_step_control.py: fp64 sums of exact products, the root, one cast to fp32


def _numel(ts):
    return (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])


def _odd_views(tensors, start=1):
    flat = torch.zeros(start + sum(t.numel() + 1 for t in tensors), device=DEV)
    views, off = [], start
    for t in tensors:
        v = flat[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        views.append(v)
        off += t.numel() + 1
    return views


def _norm(tensors, mean_scale, max_norm, ls="plain", skip_nonfinite=True):
    """ls "plain": tramba_grad_norm; None: tramba_grad_norm_scaled with a null scaler; else a loss-scale record"""
    from tramba_amd import hip
    rec, f = hip.step_ctl_record(DEV)
    numel = _numel(tensors)
    ws = torch.empty((hip.grad_norm_workspace(numel, len(tensors)) + 7) // 8, dtype=torch.float64, device=DEV)
    if isinstance(ls, str):
        hip.grad_norm_raw(hip.pointer_array(tensors), numel, len(tensors), mean_scale, max_norm, skip_nonfinite, rec, ws)
    else:
        hip.grad_norm_scaled_raw(hip.pointer_array(tensors), numel, len(tensors), mean_scale, max_norm, skip_nonfinite, rec, ls, ws)
    torch.cuda.synchronize()
    return rec, f


# ------------------------------------------------------------------------------------------------- 3. tramba_grad_norm_scaled
@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_grad_norm_scaled(layout):
    from tramba_amd import hip
    g = torch.Generator().manual_seed(9)
    host = [torch.randn(s, generator=g) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SHAPES)]
    want = float(np.sqrt(sum(float((t.numpy().astype(np.float64) ** 2).sum()) for t in host)))
    place = (lambda ts: _odd_views(ts)) if layout == "odd" else (lambda ts: ts)
    ts = place([t.to(DEV) for t in host])
    for mean_scale, max_norm in ((1.0, 0.0), (0.25, 0.5 * 0.25 * want), (0.25, 4.0 * want), (0.125, 1e-3 * want)):
        plain, f = _norm(ts, mean_scale, max_norm)
        assert abs(float(f["norm"]) - want * mean_scale) <= BOUND * want * mean_scale
        assert torch.equal(_norm(ts, mean_scale, max_norm, None)[0], plain)           # the null scaler: bit for bit
        for k in (4, 16):
            ls, lf = hip.loss_scale_record(DEV, 2.0 ** k)
            scaled = place([(t * 2.0 ** k).to(DEV) for t in host])                    # exact: far from fp32's ends
            rec, fs = _norm(scaled, mean_scale, max_norm, ls)
            # the unscaled call's record, bit for bit: norm, skip, micro and skipped_steps as they are, and the scale
            # -- which by its definition carries the factor 2^-k for the optimizer -- once that exact factor is taken out
            same = rec.clone()
            same.view(torch.float32)[1] *= 2.0 ** k
            assert torch.equal(same, plain), (k, mean_scale, max_norm, float(fs["norm"]), float(f["norm"]), float(fs["scale"]))
            assert abs(float(fs["norm"]) - want * mean_scale) <= BOUND * want * mean_scale
            want_scale = mean_scale * min(1.0, max_norm / (float(fs["norm"]) + 1e-6)) if max_norm > 0 else mean_scale
            assert abs(float(fs["scale"]) * 2.0 ** k - want_scale) <= BOUND * want_scale   # the un-scaling rides in the scale
            assert torch.equal(_norm(scaled, mean_scale, max_norm, ls)[0], rec)        # a second run: identical bits
            assert float(lf["scale"]) == 2.0 ** k and float(lf["inv_scale"]) == 2.0 ** -k and int(lf["backoffs"]) == 0


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_grad_norm_scaled_finds_the_first_and_the_last_element(value):
    from tramba_amd import hip
    g = torch.Generator().manual_seed(12)
    ls, _ = hip.loss_scale_record(DEV, 2.0 ** 16)
    for which, pos in ((0, 0), (len(SHAPES) - 1, -1)):
        ts = [torch.randn(s, generator=g).to(DEV) for s in SHAPES]
        assert int(_norm(ts, 0.5, 1.0, ls)[1]["skip"]) == 0
        ts[which].view(-1)[pos] = value
        rec, f = _norm(ts, 0.5, 1.0, ls)
        assert int(f["skip"]) == 1 and int(f["skipped_steps"]) == 1, (which, pos)
        assert int(_norm(ts, 0.5, 1.0, ls, skip_nonfinite=False)[1]["skip"]) == 0


# ------------------------------------------------------------------------------------------------- 4. tramba_loss_scale_update
def _rule(scale, good, backoffs, skipped, growth, backoff, interval, lo, hi):
    if skipped:
        return max(lo, scale * backoff), 0, backoffs + 1
    good += 1
    if good == interval:
        return min(hi, scale * growth), 0, backoffs
    return scale, good, backoffs


FLAGS = [0] * 7 + [1] * 5 + [0, 1, 0, 0, 0]
HYPER = (2.0, 0.5, 2, 1.0, 16.0)          # growth, backoff, growth_interval, min_scale, max_scale


def _read(lf):
    return float(lf["scale"]), int(lf["good_steps"]), int(lf["backoffs"]), float(lf["inv_scale"])


def test_loss_scale_update_follows_the_rule_eagerly_and_replayed():
    from tramba_amd import hip
    want, state = [], (4.0, 0, 0)
    for flag in FLAGS:
        state = _rule(*state, flag, *HYPER)
        want.append(state + (1.0 / state[0],))
    scales = [w[0] for w in want]
    assert scales.count(16.0) >= 2 and scales.count(1.0) >= 2                   # both clamps bite
    ctl, f = hip.step_ctl_record(DEV)
    ls, lf = hip.loss_scale_record(DEV, 4.0)
    got = []
    for flag in FLAGS:
        f["skip"].fill_(flag)
        hip.loss_scale_update_raw(ls, ctl, *HYPER)
        got.append(_read(lf))
    assert got == want
    assert int(f["skipped_steps"]) == 0 and int(ls.view(torch.int32)[3]) == 0    # nothing else is written
    # other hyper-parameters: growth 4 and backoff 1/4 between 2^-3 and 2^20
    ls, lf = hip.loss_scale_record(DEV, 2.0 ** 18)
    other, state, got, want = (4.0, 0.25, 1, 0.125, 2.0 ** 20), (2.0 ** 18, 0, 0), [], []
    for flag in [0, 0] + [1] * 13 + [0]:
        f["skip"].fill_(flag)
        hip.loss_scale_update_raw(ls, ctl, *other)
        got.append(_read(lf))
        state = _rule(*state, flag, *other)
        want.append(state + (1.0 / state[0],))
    assert got == want and want[1][0] == 2.0 ** 20 and want[-2][0] == 0.125
    # captured once, replayed with the flag changed between replays: the record decides, not the values at capture
    ls, lf = hip.loss_scale_record(DEV, 4.0)
    f["skip"].fill_(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.loss_scale_update_raw(ls, ctl, *HYPER)
    torch.cuda.synchronize()
    assert _read(lf) == (4.0, 0, 0, 0.25)                                       # a capture executes nothing
    got, want, state = [], [], (4.0, 0, 0)
    for flag in FLAGS:
        f["skip"].fill_(flag)
        graph.replay()
        got.append(_read(lf))
        state = _rule(*state, flag, *HYPER)
        want.append(state + (1.0 / state[0],))
    assert got == want


# ------------------------------------------------------------------------------------------------- the controlled step
class _Tiny(torch.nn.Module):
    """one decoder block + a per-channel head behind the interface train.train_step expects (a list of logit maps; the
    names hold "encoder"): 16-bit activations when compute_dtype is set, fp32 master weights"""

    def __init__(self, compute_dtype=None, drop_path=0.0):
        super().__init__()
        import tramba_amd as ta
        torch.manual_seed(11)
        self.encoder = ta.MultiScaleDecoderBlock(hidden_dim=32, drop_path=drop_path, channel_first=True)
        self.encoder_head = torch.nn.Parameter(torch.randn(32) * 0.2)
        self.encoder_bias = torch.nn.Parameter(torch.zeros(1))
        self.compute_dtype = compute_dtype

    def forward(self, z):
        if self.training:           # as the library's models do: one stochastic-depth table per model and forward
            from tramba_amd.modules import model_mask_pool
            model_mask_pool(self).begin_step()
        h = self.encoder(z if self.compute_dtype is None else z.to(self.compute_dtype))
        w = self.encoder_head.to(h.dtype).view(1, -1, 1, 1)
        return [(h * w).sum(dim=1, keepdim=True) + self.encoder_bias.to(h.dtype).view(1, 1, 1, 1)]


def _tiny_data(n=2):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, 32, 24, 24, generator=g).to(DEV), (torch.rand(n, 1, 24, 24, generator=g) > 0.5).float().to(DEV)


def _rel_l2(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-300))


def _full_state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for st in opt.state.values():
        out += [st[k].clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out


# ---- 5. the reason for the feature
WEIGHT = 2.0 ** -12          # on the loss: with the mean over 2 x 24 x 24 pixels the gradient per logit stays below 2^-22


def parity_errors():
    """relative L2 error of every parameter gradient of _Tiny at 2 x 32 x 24 x 24 against the fp32 library run, for
    fp16 without a scaler, fp16 with LossScale(init=2^16) and bf16; and the largest fp32 loss gradient per logit"""
    from tramba_amd import train
    x, y = _tiny_data()
    loss_fn = train.SodLoss(loss_weights=(WEIGHT,))
    ref = _Tiny().to(DEV).train()
    out = ref(x)[0]
    out.retain_grad()
    loss_fn([out], y).backward()
    per_logit = float(out.grad.abs().max())
    want = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    errs = {}
    for tag, dtype, scaler in (("fp16", torch.float16, None), ("fp16_scaled", torch.float16, train.LossScale(init=2.0 ** 16)),
                               ("bf16", torch.bfloat16, None)):
        m = _Tiny(dtype).to(DEV).train()
        control = train.StepControl(skip_nonfinite=True) if scaler is None else train.StepControl(loss_scale=scaler)
        train.train_step(m, train.get_opt(1e-6, m), x, y, control=control, loss=loss_fn)
        assert int(control.skipped_steps) == 0
        inv = 1.0 if scaler is None else 2.0 ** -16
        if scaler is not None:
            assert float(control.loss_scale) == 2.0 ** 16
        errs[tag] = {n: _rel_l2(p.grad * inv, want[n]) for n, p in m.named_parameters()}
    return per_logit, errs


def test_fp16_needs_the_scale_and_with_it_beats_bf16():
    """Without a scaler the fp16 backward starts from loss gradients below fp16's normal range and some parameter gradient
    is mostly wrong (> 0.5 relative L2: the underflow, which pins this test's construction); with LossScale(init=2^16)
    every parameter's gradient, un-scaled, is no further from the fp32 run than the bf16 run's and inside the bf16 block
    bound of tests/test_gpu_grad.py (6e-2).  TRAMBA_WRITE_PROFILES=1 writes the errors to profiles/loss_scale_parity.json.

    Measured (MI355X, profiles/loss_scale_parity.json): fp16 + 2^16 at 1.5e-4 .. 2.5e-3 against bf16's 2.1e-3 .. 1.1e-2.
    This test is what found that the scan backward must not store the raw time step's gradient in fp16: while it did,
    encoder.op.dt_projs_weight came out at 1.3e-1 (most of that tensor was subnormal even under the scale); the fp16 scan
    backward now runs its fp32 form (modules._SS2DInnerCL.backward) and that parameter is at 1.5e-3."""
    per_logit, errs = parity_errors()
    for tag, e in errs.items():
        print(tag, {n: f"{v:.3e}" for n, v in e.items()})
    print("largest fp32 loss gradient per logit", per_logit)
    if os.environ.get("TRAMBA_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "loss_scale_parity.json"), "w") as f:
            json.dump({"module": "MultiScaleDecoderBlock(32) + per-channel head, 2 x 32 x 24 x 24, loss weight 2^-12",
                       "reference": "the same module in fp32 on the library", "max_loss_gradient_per_logit": per_logit,
                       "relative_l2_error": errs}, f, indent=1)
    assert 0 < per_logit <= 2.0 ** -22
    assert max(errs["fp16"].values()) > 0.5, errs["fp16"]
    bad = {n: (e, errs["bf16"][n]) for n, e in errs["fp16_scaled"].items() if e > errs["bf16"][n] or e > 6e-2}
    assert not bad, bad


# ---- 6. fp32 compute: the scale changes no bit
def test_fp32_compute_with_a_scale_is_the_unscaled_run_bit_for_bit():
    from tramba_amd import train
    x, y = _tiny_data(4)
    runs = []
    for scaler in (None, train.LossScale(init=2.0 ** 8)):
        m = _Tiny(None, drop_path=0.2).to(DEV).train()
        opt = train.get_opt(1e-3, m)
        control = (train.StepControl(accumulate=2, skip_nonfinite=True) if scaler is None
                   else train.StepControl(accumulate=2, loss_scale=scaler))
        torch.manual_seed(3)                                    # the stochastic-depth draws of both runs
        smallest = float("inf")
        for step in range(3):
            train.train_step(m, opt, torch.roll(x, step, 0), y, control=control)
            gs = torch.cat([p.grad.abs().flatten() for p in m.parameters() if p.grad is not None])
            smallest = min(smallest, float(gs[gs > 0].min()))
        assert int(control.skipped_steps) == 0
        runs.append((_full_state(m, opt), smallest, float(control.grad_norm)))
    assert runs[0][1] >= 2.0 ** -100, runs[0][1]                # the precondition: nothing near fp32's lower end
    assert len(runs[0][0]) == len(runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][2] == runs[1][2]                             # the norm stays the unscaled one
    fresh = [p.detach() for p in _Tiny().to(DEV).parameters()]
    assert not all(torch.equal(a, b) for a, b in zip(fresh, runs[0][0]))


# ---- 7. overflow and recovery
def test_overflow_is_skipped_and_the_scale_recovers():
    from tramba_amd import train
    x, y = _tiny_data()
    m = _Tiny(torch.float16).to(DEV).train()
    opt = train.get_opt(1e-3, m)
    control = train.StepControl(loss_scale=train.LossScale(init=2.0 ** 30, growth_interval=2))
    scale, skips, before = 2.0 ** 30, 0, None
    for _ in range(40):
        train.train_step(m, opt, x, y, control=control)
        if int(control._fields["skip"]) == 0:
            break
        skips += 1
        scale /= 2
        now = _full_state(m, opt)
        if before is not None:                                  # (the first step creates the optimizer state: as zeros)
            assert all(torch.equal(a, b) for a, b in zip(before, now)), skips
        else:
            fresh = _Tiny().to(DEV)
            assert all(torch.equal(a, b) for a, b in zip(fresh.parameters(), m.parameters()))
            assert all(float(st["step"]) == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
        before = now
        assert int(control.skipped_steps) == skips and int(control.scale_backoffs) == skips
        assert float(control.loss_scale) == scale
    print(f"{skips} steps skipped, first step taken at scale 2^{int(np.log2(scale))}")
    assert skips >= 1 and int(control._fields["skip"]) == 0     # the first steps are skipped, then one is not
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert not all(torch.equal(a, b) for a, b in zip(before, _full_state(m, opt)))
    assert all(float(st["step"]) == 1 for st in opt.state.values())
    assert float(control.loss_scale) == scale and int(control.skipped_steps) == skips
    train.train_step(m, opt, x, y, control=control)             # the second step that is not skipped: the scale doubles
    assert int(control.skipped_steps) == skips and int(control.scale_backoffs) == skips
    assert float(control.loss_scale) == 2 * scale
    assert all(float(st["step"]) == 2 for st in opt.state.values())


# ---- 8. graphed against eager
def test_graphed_step_with_a_scale_follows_the_eager_one():
    import tramba_amd as ta
    from tramba_amd import train
    x, y = _tiny_data(4)
    make = lambda: train.StepControl(accumulate=2, clip_norm=1.0,   # noqa: E731
                                     loss_scale=train.LossScale(init=2.0 ** 30, growth_interval=2))
    runs = []
    for graphed in (False, True):
        m = _Tiny(torch.float16).to(DEV).train()
        opt = train.get_opt(1e-3, m, capturable=graphed)
        control = make()
        step = ta.GraphedTrainStep(m, opt, control=control) if graphed else (lambda a, b: train.train_step(m, opt, a, b, control=control))
        seq = []
        for k in range(16):
            loss = float(step(x, y))
            seq.append((float(control.loss_scale), int(control.skipped_steps), float(control.grad_norm), loss))
            if graphed and k == 0:      # the two warm-up steps were undone: the scaler record shows exactly one step
                assert int(control.scale_backoffs) + int(control._ls["good_steps"]) == 1
                assert all(float(st["step"]) == (0.0 if seq[0][1] else 1.0) for st in opt.state.values())
        runs.append(seq)
    eager, got = runs
    print("eager", eager, "graphed", got)
    assert [s[:2] for s in got] == [s[:2] for s in eager]
    assert np.array_equal(np.array([s[2] for s in got]), np.array([s[2] for s in eager]), equal_nan=True)
    assert eager[0][1] == 1 and eager[7][1] == 8 and eager[-1][1] < 16   # the first eight are skipped (measured: twelve), the last are steps
    assert got[0][3] == pytest.approx(eager[0][3], rel=1e-5)
    assert np.allclose([s[3] for s in got], [s[3] for s in eager], rtol=3e-2)


# ---- 9. two data-parallel ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir, steps):
    import torch.distributed as dist
    from tramba_amd import parallel, train
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)                       # both ranks share the one card of the test box
        model = _Tiny().to("cuda").train()
        parallel.broadcast_parameters(model, src=0)
        red = parallel.GradBucketReducer(model, bucket_mb=0.05)
        opt = train.get_opt(1e-2, model)
        control = train.StepControl(accumulate=2, clip_norm=1e3, loss_scale=train.LossScale(init=2.0 ** 16, growth_interval=1))
        x, y = _tiny_data(8)
        xs, ys = [x[2 * j:2 * j + 2] for j in range(rank, 4, world)], [y[2 * j:2 * j + 2] for j in range(rank, 4, world)]
        for _ in range(steps):
            train.train_step(model, opt, xs, ys, reducer=red, control=control)
        torch.cuda.synchronize()
        torch.save({"sd": {k: v.cpu() for k, v in model.state_dict().items()}, "control": control.state_dict(),
                    "norm": float(control.grad_norm)}, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_move_their_scale_together(tmp_path):
    """two gloo ranks on one card x accumulate=2 with a scaler, two steps: the norm runs after the all-reduce, so both
    ranks take the same decision -- the same scale and the same parameters; and those of one process x accumulate=4"""
    import torch.multiprocessing as mp
    from tramba_amd import train
    steps, world = 2, 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), steps), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert r0["control"] == r1["control"] == {"skipped_steps": 0, "scale": 2.0 ** 18, "good_steps": 0, "backoffs": 0}
    assert r0["norm"] == r1["norm"]
    model = _Tiny().to(DEV).train()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(accumulate=4, clip_norm=1e3, loss_scale=train.LossScale(init=2.0 ** 16, growth_interval=1))
    x, y = _tiny_data(8)
    for _ in range(steps):
        train.train_step(model, opt, x, y, control=control)
    fresh = _Tiny().state_dict()
    moved = 0.0
    for k, v in model.state_dict().items():
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k
        np.testing.assert_allclose(r0["sd"][k].numpy(), v.cpu().numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
        moved = max(moved, float((v.cpu() - fresh[k]).abs().max()))
    assert moved > 1e-3 and r0["norm"] == pytest.approx(float(control.grad_norm), rel=2e-3)
