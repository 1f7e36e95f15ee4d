"""Gradient accumulation, norm clipping and the skip of a non-finite step (train.StepControl): the semantics, on host
tensors through torch's own functions, against plain-torch restatements written here; and the argument checks of the new
library entries (no launch is issued for a rejected call, so no device is needed)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _Wrap(nn.Module):
    """the model contract of the path: a list of logits, 'encoder' in some names"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(7)
        self.encoder = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GELU(), nn.Conv2d(8, 8, 3, padding=1), nn.GELU(),
                                     nn.Conv2d(8, 1, 1))
        self.decoder = nn.Conv2d(1, 1, 1)

    def forward(self, x):
        y = self.encoder(x)
        return [nn.functional.avg_pool2d(y, 2), self.decoder(y)]


class _WrapSpare(_Wrap):
    """plus a head only some micro-batches use (`use_spare`, switched by the test), and one nobody uses"""

    def __init__(self):
        super().__init__()
        self.spare = nn.Conv2d(1, 1, 1)
        self.never = nn.Conv2d(1, 1, 1)
        self.calls = 0
        self.spare_on = ()

    def forward(self, x):
        outs = super().forward(x)
        if self.calls in self.spare_on:
            outs[1] = outs[1] + 0.5 * self.spare(outs[1])
        self.calls += 1
        return outs


def _data(n, dtype=torch.float32):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, 3, 16, 16, generator=g)
    m = (torch.rand(n, 1, 16, 16, generator=g) > 0.7).float()
    return x.to(dtype), m.to(dtype)


def _plain_accumulated_step(model, opt, xs, ys, clip):
    """the restatement: standing gradients, g /= count, clip_grad_norm_, torch's Adam"""
    from tramba_amd import train
    opt.zero_grad(set_to_none=True)
    for x, y in zip(xs, ys):
        train.tramba_loss(model(x), y).backward()
    params = [p for p in model.parameters() if p.grad is not None]
    with torch.no_grad():
        for p in params:
            p.grad /= len(xs)
    norm = torch.nn.utils.clip_grad_norm_(params, float("inf") if clip is None else clip)
    opt.step()
    return norm


def _moments(opt):
    return [(st["exp_avg"], st["exp_avg_sq"], st["step"]) for st in opt.state.values()]


def _observed_norm():
    model = _Wrap().double()
    x, m = _data(8, torch.float64)
    opt = torch.optim.Adam(model.parameters(), 1e-2)
    return float(_plain_accumulated_step(model, opt, x.chunk(4), m.chunk(4), None))


@pytest.mark.parametrize("clip_factor", [4.0, 0.25])
def test_accumulate_and_clip_follow_the_torch_restatement(clip_factor):
    """fp64 toy model, accumulate=4, three steps: parameters, both moments and the reported norm against standing
    gradients / 4 + clip_grad_norm_ + torch.optim.Adam.  A clip norm above the observed norm changes nothing."""
    from tramba_amd import train
    clip = _observed_norm() * clip_factor
    x, m = _data(8, torch.float64)
    got, want = _Wrap().double(), _Wrap().double()
    opt_g, opt_w = train.get_opt(1e-2, got), train.get_opt(1e-2, want)
    assert type(opt_g) is torch.optim.Adam
    control = train.StepControl(accumulate=4, clip_norm=clip)
    free = _Wrap().double()                         # the same run without a clip norm
    opt_f, control_f = train.get_opt(1e-2, free), train.StepControl(accumulate=4)
    for step in range(3):
        xs = torch.roll(x, step, 0)
        loss = train.train_step(got, opt_g, xs, m, control=control)
        train.train_step(free, opt_f, xs, m, control=control_f)
        norm = _plain_accumulated_step(want, opt_w, xs.chunk(4), m.chunk(4), clip)
        assert abs(float(control.grad_norm) - float(norm)) <= 1e-12 * float(norm)
        assert control.grad_norm.dim() == 0 and loss.dim() == 0 and not loss.requires_grad
        if clip_factor < 1:
            assert float(norm) > clip               # clipping is active
    for (k, a), b in zip(got.state_dict().items(), want.state_dict().values()):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0, err_msg=k)
    for sa, sb in zip(_moments(opt_g), _moments(opt_w)):
        for a, b in zip(sa, sb):
            np.testing.assert_allclose(torch.as_tensor(a).numpy(), torch.as_tensor(b).numpy(), rtol=1e-12, atol=0)
    same = all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), free.state_dict().values()))
    assert same == (clip_factor > 1)                # above the norm: exactly the unclipped run; below: another one
    assert int(control.skipped_steps) == 0


def test_first_loss_is_the_mean_of_the_micro_batch_losses():
    from tramba_amd import train
    model, x_m = _Wrap(), _data(8)
    x, m = x_m
    with torch.no_grad():
        want = sum(train.tramba_loss(model(a), b) for a, b in zip(x.chunk(4), m.chunk(4))) / 4
    got = train.train_step(model, train.get_opt(1e-2, model), list(x.chunk(4)), list(m.chunk(4)),
                           control=train.StepControl(accumulate=4))
    np.testing.assert_allclose(float(got), float(want), rtol=1e-6)


def test_a_non_finite_micro_batch_skips_the_step():
    """One micro-batch with a NaN pixel: nothing moves and the step is counted; the clean steps that follow equal a run
    that never saw the bad batch.  Without skip_nonfinite the same batch poisons the weights."""
    from tramba_amd import train
    x, m = _data(8, torch.float64)
    bad = x.clone()
    bad[5, 1, 3, 3] = float("nan")
    got, clean, loose = _Wrap().double(), _Wrap().double(), _Wrap().double()
    opt_g, opt_c, opt_l = (train.get_opt(1e-2, mm) for mm in (got, clean, loose))
    cg = train.StepControl(accumulate=4, skip_nonfinite=True)
    cc = train.StepControl(accumulate=4, skip_nonfinite=True)
    train.train_step(got, opt_g, x, m, control=cg)
    train.train_step(clean, opt_c, x, m, control=cc)
    before = {k: v.clone() for k, v in got.state_dict().items()}
    state = [[torch.as_tensor(t).clone() for t in st] for st in _moments(opt_g)]
    train.train_step(got, opt_g, bad, m, control=cg)
    assert int(cg.skipped_steps) == 1
    for k, v in got.state_dict().items():
        assert torch.equal(v, before[k]), k
    for st, old in zip(_moments(opt_g), state):
        for a, b in zip(st, old):
            assert torch.equal(torch.as_tensor(a), b)
    for _ in range(2):
        train.train_step(got, opt_g, x, m, control=cg)
        train.train_step(clean, opt_c, x, m, control=cc)
    for k, v in got.state_dict().items():
        assert torch.equal(v, clean.state_dict()[k]), k
    assert int(cg.skipped_steps) == 1 and int(cc.skipped_steps) == 0
    cl = train.StepControl(accumulate=4, skip_nonfinite=False)
    train.train_step(loose, opt_l, bad, m, control=cl)
    assert int(cl.skipped_steps) == 0
    assert not all(bool(torch.isfinite(v).all()) for v in loose.state_dict().values())   # the switch is real


def test_parameters_used_by_some_micro_batches_or_by_none():
    """`spare` is used by micro-batches 1 and 3 of 4: its gradient is the mean over all four with zeros for the others;
    `never` keeps grad None and is not stepped.  A second step whose FIRST micro-batch does not use `spare` must not see
    the first step's values in the accumulator."""
    from tramba_amd import train
    x, m = _data(8, torch.float64)
    got, want = _WrapSpare().double(), _WrapSpare().double()
    opt_g, opt_w = train.get_opt(1e-2, got), train.get_opt(1e-2, want)
    control = train.StepControl(accumulate=4)
    for step in range(2):
        got.calls = want.calls = 0
        got.spare_on = want.spare_on = (1, 3)
        train.train_step(got, opt_g, x, m, control=control)
        _plain_accumulated_step(want, opt_w, x.chunk(4), m.chunk(4), None)
        np.testing.assert_allclose(got.spare.weight.grad.numpy(), want.spare.weight.grad.numpy(), rtol=1e-12)
        assert float(got.spare.weight.grad.abs().sum()) > 0
        assert got.never.weight.grad is None and got.never.bias.grad is None
    fresh = _WrapSpare().double()
    assert torch.equal(got.never.weight, fresh.never.weight) and got.never.weight not in opt_g.state
    for (k, a), b in zip(got.state_dict().items(), want.state_dict().values()):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0, err_msg=k)


def test_fit_groups_batches_and_argument_errors(tmp_path):
    """7 batches, accumulate=3: three optimizer steps, the last over one batch; checkpoint files as today."""
    from tramba_amd import train
    model = _Wrap()
    opt = train.get_opt(1e-2, model)
    x, m = _data(14)
    control = train.StepControl(accumulate=3)
    hist = train.fit(model, opt, lambda epoch: [(x[2 * i:2 * i + 2], m[2 * i:2 * i + 2]) for i in range(7)], 5, 1e-2, [], [],
                     str(tmp_path), "toy", control=control, evaluate=lambda mod, e: 0.5 - 0.01 * e)
    steps = {float(st["step"]) for st in opt.state.values()}
    assert steps == {15.0}, steps                                  # 5 epochs x 3 steps
    assert len(hist) == 5 and all(np.isfinite(h["loss"]) for h in hist)
    assert os.path.exists(tmp_path / "toy" / "toy_resume.pth")
    assert len(list((tmp_path / "toy").glob("toy_MAE_*_5.pth"))) == 1
    # one epoch, by hand: the last group is a step over one batch (scale 1 / 1)
    a, b = _Wrap(), _Wrap()
    oa, ob = train.get_opt(1e-2, a), train.get_opt(1e-2, b)
    train.fit(a, oa, lambda epoch: [(x[2 * i:2 * i + 2], m[2 * i:2 * i + 2]) for i in range(7)], 1, 1e-2, [], [],
              str(tmp_path), "toy2", control=train.StepControl(accumulate=3))
    for lo, hi in ((0, 3), (3, 6), (6, 7)):
        _plain_accumulated_step(b, ob, [x[2 * i:2 * i + 2] for i in range(lo, hi)], [m[2 * i:2 * i + 2] for i in range(lo, hi)],
                                None)
    for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
        np.testing.assert_allclose(u.numpy(), v.numpy(), rtol=2e-5, atol=2e-6, err_msg=k)

    for kw in ({"accumulate": 0}, {"accumulate": -2}, {"accumulate": 1.5}, {"clip_norm": 0.0}, {"clip_norm": -1.0}):
        with pytest.raises(ValueError):
            train.StepControl(**kw)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(ValueError):
        train.train_step(model, opt, x[:7], m[:7], control=control)            # 7 images do not split into 3
    with pytest.raises(ValueError):
        train.train_step(model, opt, [x[:2]] * 4, [m[:2]] * 4, control=control)   # more micro-batches than accumulate
    with pytest.raises(ValueError):
        train.train_step(model, opt, [x[:2], x[:4]], [m[:2], m[:4]], control=control)
    with pytest.raises(ValueError):
        train.train_step(model, opt, [x[:2]], m[:2], control=control)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k                                    # ... before any work


def _dp_worker(rank, world, port, out_dir, steps):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tramba_amd import parallel, train
    calls = []
    real = dist.all_reduce

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    dist.all_reduce = counted
    model = _Wrap()
    if rank != 0:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)
    parallel.broadcast_parameters(model, src=0)
    opt = train.get_opt(1e-2, model)
    x, m = _data(8)
    # find_unused reads per-step flags: refused under a control object, before any work
    picky = parallel.GradBucketReducer(model, find_unused=True)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        train.train_step(model, opt, x[:4], m[:4], reducer=picky, control=train.StepControl(accumulate=2))
        refused = False
    except RuntimeError as e:
        refused = "find_unused" in str(e)
    refused = refused and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    picky.remove_hooks()
    red = parallel.GradBucketReducer(model, bucket_mb=0.0005)
    control = train.StepControl(accumulate=2, clip_norm=1e3)
    # micro-batch j of the single process is images [2j, 2j+1]: rank r takes micro-batches r and r + world
    xs, ms = [x[2 * j:2 * j + 2] for j in range(rank, 4, world)], [m[2 * j:2 * j + 2] for j in range(rank, 4, world)]
    losses = [float(train.train_step(model, opt, xs, ms, reducer=red, control=control)) for _ in range(steps)]
    torch.save({"sd": model.state_dict(), "losses": losses, "nbuckets": len(red.buckets), "all_reduces": len(calls), "find_unused_refused": refused,
                "norm": float(control.grad_norm), "bytes": red.bytes_per_step()}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_dp2_times_accumulate2_matches_one_process_accumulate4(tmp_path):
    """N micro-batches accumulated == N ranks averaged: two gloo ranks x accumulate=2 against one process x accumulate=4
    on the interleaved data, and exactly one all-reduce round per optimizer step."""
    from tramba_amd import train
    steps, world = 3, 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), steps), nprocs=world, join=True)
    r0, r1 = torch.load(os.path.join(tmp_path, "r0.pt")), torch.load(os.path.join(tmp_path, "r1.pt"))
    assert r0["nbuckets"] > 1 and r0["find_unused_refused"] and r1["find_unused_refused"]
    assert r0["all_reduces"] == steps * r0["nbuckets"] and r1["all_reduces"] == steps * r1["nbuckets"]
    model = _Wrap()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(accumulate=4, clip_norm=1e3)
    x, m = _data(8)
    for _ in range(steps):
        train.train_step(model, opt, x, m, control=control)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(r0["sd"][k].numpy(), v.numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k
    np.testing.assert_allclose(r0["norm"], float(control.grad_norm), rtol=2e-5)
    assert r0["norm"] == r1["norm"]                 # every rank sees the same norm, hence the same clip and skip decision
    assert r0["bytes"] == sum(p.numel() * 4 for p in model.parameters())


def test_reducer_refuses_low_precision_buckets_and_a_parameter_set_of_its_own_under_a_control():
    """(the find_unused refusal needs two ranks: test_dp2_times_accumulate2_matches_one_process_accumulate4)"""
    from tramba_amd import parallel, train
    model = _Wrap()
    x, m = _data(4)
    red = parallel.GradBucketReducer(model, bucket_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bucket_dtype"):
        train.train_step(model, train.get_opt(1e-2, model), x, m, reducer=red, control=train.StepControl(accumulate=2))
    red.remove_hooks()
    # the norm is taken over the reducer's whole buckets: a trainable parameter that no optimizer group owns is refused
    red = parallel.GradBucketReducer(model)
    opt = torch.optim.Adam(model.encoder.parameters(), 1e-2)
    with pytest.raises(ValueError, match="same set"):
        train.train_step(model, opt, x, m, reducer=red, control=train.StepControl(accumulate=2))
    red.remove_hooks()


def test_single_process_reducer_buckets_are_the_accumulators():
    from tramba_amd import parallel, train
    model, plain = _Wrap(), _Wrap()
    x, m = _data(8)
    red = parallel.GradBucketReducer(model, bucket_mb=0.0005)
    opt, opt_p = train.get_opt(1e-2, model), train.get_opt(1e-2, plain)
    control = train.StepControl(accumulate=4)
    for _ in range(2):
        train.train_step(model, opt, x, m, reducer=red, control=control)
        _plain_accumulated_step(plain, opt_p, x.chunk(4), m.chunk(4), None)
    flat_ptrs = {(f.data_ptr(), f.data_ptr() + f.numel() * 4) for f in red.flat}
    for p in model.parameters():
        assert any(lo <= p.grad.data_ptr() < hi for lo, hi in flat_ptrs)
    for (k, a), b in zip(model.state_dict().items(), plain.state_dict().values()):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
    red.remove_hooks()


# ----------------------------------------------------------------------------- the library entries: rejected arguments
def _arr(kind, values):
    return (kind * len(values))(*values)


def test_new_entries_are_declared_and_reject_bad_arguments_without_a_launch():
    from tramba_amd import hip
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_grad_accumulate", "tramba_grad_norm", "tramba_grad_norm_workspace", "tramba_adam_step_ctl"):
        assert name in hip.SIGNATURES and hasattr(lib, name)
    # plausible non-null addresses: a rejected call never touches them
    buf = (ctypes.c_char * 64)()
    addr = ctypes.addressof(buf)
    ptrs, nulls = _arr(ctypes.c_void_p, [addr]), _arr(ctypes.c_void_p, [None])
    one, neg = _arr(ctypes.c_int64, [1]), _arr(ctypes.c_int64, [-4])

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        assert word in lib.tramba_last_error().decode()

    rejected(lib.tramba_grad_accumulate(None, ptrs, one, 1, addr, None), "grad_accumulate")
    rejected(lib.tramba_grad_accumulate(ptrs, None, one, 1, addr, None), "grad_accumulate")
    rejected(lib.tramba_grad_accumulate(ptrs, ptrs, None, 1, addr, None), "grad_accumulate")
    rejected(lib.tramba_grad_accumulate(ptrs, ptrs, one, 1, None, None), "grad_accumulate")
    rejected(lib.tramba_grad_accumulate(ptrs, ptrs, one, 0, addr, None), "count")
    rejected(lib.tramba_grad_accumulate(ptrs, ptrs, one, -3, addr, None), "count")
    rejected(lib.tramba_grad_accumulate(nulls, ptrs, one, 1, addr, None), "tensor 0")
    rejected(lib.tramba_grad_accumulate(ptrs, ptrs, neg, 1, addr, None), "tensor 0")

    rejected(lib.tramba_grad_norm(None, one, 1, 1.0, 0.0, 0, addr, addr, 64, None), "grad_norm")
    rejected(lib.tramba_grad_norm(ptrs, None, 1, 1.0, 0.0, 0, addr, addr, 64, None), "grad_norm")
    rejected(lib.tramba_grad_norm(ptrs, one, 1, 1.0, 0.0, 0, None, addr, 64, None), "grad_norm")
    rejected(lib.tramba_grad_norm(ptrs, one, 1, 1.0, 0.0, 0, addr, None, 64, None), "grad_norm")
    rejected(lib.tramba_grad_norm(ptrs, one, 0, 1.0, 0.0, 0, addr, addr, 64, None), "count")
    rejected(lib.tramba_grad_norm(nulls, one, 1, 1.0, 0.0, 0, addr, addr, 64, None), "tensor 0")
    rejected(lib.tramba_grad_norm(ptrs, neg, 1, 1.0, 0.0, 0, addr, addr, 64, None), "tensor 0")
    rejected(lib.tramba_grad_norm(ptrs, one, 1, 0.0, 0.0, 0, addr, addr, 64, None), "mean_scale")
    rejected(lib.tramba_grad_norm(ptrs, one, 1, 1.0, 0.0, 0, addr, addr, 4, None), "workspace")
    assert lib.tramba_grad_norm_workspace(one, 1) == 12
    assert lib.tramba_grad_norm_workspace(_arr(ctypes.c_int64, [8192, 8193, 1]), 3) == 4 * 12
    assert lib.tramba_grad_norm_workspace(None, 1) == 0 and lib.tramba_grad_norm_workspace(neg, 1) == 0

    d = [1e-3, 0.9, 0.999, 1e-8, 0.0]
    rejected(lib.tramba_adam_step_ctl(None, ptrs, ptrs, ptrs, ptrs, one, 1, *d, None, None, None), "adam_step")
    rejected(lib.tramba_adam_step_ctl(ptrs, ptrs, ptrs, ptrs, ptrs, one, 0, *d, None, None, None), "adam_step")
    rejected(lib.tramba_adam_step_ctl(ptrs, nulls, ptrs, ptrs, ptrs, one, 1, *d, addr, addr, None), "tensor 0")
    rejected(lib.tramba_adam_step_ctl(ptrs, ptrs, ptrs, ptrs, ptrs, neg, 1, *d, addr, addr, None), "tensor 0")
    rejected(lib.tramba_adam_step_ctl(ptrs, ptrs, ptrs, ptrs, ptrs, one, 1, -1.0, 0.9, 0.999, 1e-8, 0.0, addr, addr, None),
             "hyper-parameters")


def test_record_layout_matches_the_header():
    """the 24-byte record of the header and the typed views hip.step_ctl_record hands out"""
    import re
    from tramba_amd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tramba_hip.h")).read()
    body = re.search(r"typedef struct tramba_step_ctl \{(.*?)\} tramba_step_ctl;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t|int64_t)\s+(\w+);", body, re.M)
    assert fields == [("float", "norm"), ("float", "scale"), ("int32_t", "skip"), ("int32_t", "micro"),
                      ("int64_t", "skipped_steps")]
    assert hip.STEP_CTL_BYTES == 4 + 4 + 4 + 4 + 8
