"""Dynamic loss scaling (train.LossScale, StepControl(loss_scale=...)): the semantics on host tensors through torch's own
functions, against restatements written here; the checkpoint keys; and the argument checks of the two library entries
(no launch is issued for a rejected call, so no device is needed)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Toy(nn.Module):
    """the model contract of the path: a list of logit maps, 'encoder' in some names"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(7)
        self.encoder = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GELU(), nn.Conv2d(8, 1, 1))
        self.decoder = nn.Conv2d(1, 1, 1)
        self.seen = []              # what `watch()` returned at every forward

    watch = None

    def forward(self, x):
        if self.watch is not None:
            self.seen.append(self.watch())
        y = self.encoder(x)
        return [nn.functional.avg_pool2d(y, 2), self.decoder(y)]


def _data(n=6):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, 3, 16, 16, generator=g, dtype=torch.float64)
    m = (torch.rand(n, 1, 16, 16, generator=g) > 0.7).double()
    return x, m


def _state(model, opt):
    out = [v.clone() for v in model.state_dict().values()]
    for st in opt.state.values():
        out += [torch.as_tensor(st[k]).clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out


def _rule(scale, good, skipped, growth, backoff, interval, lo, hi):
    """the issue's rule, restated: -> (scale, good_steps, backoffs added)"""
    if skipped:
        return max(lo, scale * backoff), 0, 1
    good += 1
    if good == interval:
        return min(hi, scale * growth), 0, 0
    return scale, good, 0


# ----------------------------------------------------------------------------- 1. symbols and refusals
def test_new_symbols_are_exported_bound_and_refuse_bad_arguments():
    from tramba_amd import hip
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_\w+)\s*\(", header))
    for name in ("tramba_grad_norm_scaled", "tramba_loss_scale_update"):
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    body = re.search(r"typedef struct tramba_loss_scale \{(.*?)\} tramba_loss_scale;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t|int64_t)\s+(\w+);", body, re.M)
    assert fields == [("float", "scale"), ("float", "inv_scale"), ("int32_t", "good_steps"), ("int32_t", "reserved"),
                      ("int64_t", "backoffs")]
    assert hip.LOSS_SCALE_BYTES == 4 + 4 + 4 + 4 + 8

    buf = (ctypes.c_char * 64)()            # a plausible non-null address: a rejected call never touches it
    addr = ctypes.addressof(buf)

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        assert word in lib.tramba_last_error().decode(), lib.tramba_last_error().decode()

    up = lib.tramba_loss_scale_update
    rejected(up(None, addr, 2.0, 0.5, 2000, 1.0, 65536.0, None), "null")
    rejected(up(addr, None, 2.0, 0.5, 2000, 1.0, 65536.0, None), "null")
    for growth in (3.0, 1.5, 1.0, 0.5, 0.0, -2.0, float("nan"), float("inf")):
        rejected(up(addr, addr, growth, 0.5, 2000, 1.0, 65536.0, None), "growth")
    for backoff in (0.3, 0.75, 1.0, 2.0, 0.0, -0.5, float("nan")):
        rejected(up(addr, addr, 2.0, backoff, 2000, 1.0, 65536.0, None), "backoff")
    for interval in (0, -1):
        rejected(up(addr, addr, 2.0, 0.5, interval, 1.0, 65536.0, None), "growth_interval")
    for lo in (3.0, 0.0, -1.0, 0.7, float("nan")):
        rejected(up(addr, addr, 2.0, 0.5, 2000, lo, 65536.0, None), "min_scale")
    for hi in (65535.0, 0.0, float("inf"), 3e38):
        rejected(up(addr, addr, 2.0, 0.5, 2000, 1.0, hi, None), "max_scale")
    rejected(up(addr, addr, 2.0, 0.5, 2000, 4.0, 2.0, None), "min_scale")

    ptrs, one = (ctypes.c_void_p * 1)(addr), (ctypes.c_int64 * 1)(1)
    ns = lib.tramba_grad_norm_scaled
    rejected(ns(None, one, 1, 1.0, 0.0, 0, addr, addr, addr, 64, None), "grad_norm")
    rejected(ns(ptrs, one, 1, 1.0, 0.0, 0, None, addr, addr, 64, None), "grad_norm")
    rejected(ns(ptrs, one, 1, 1.0, 0.0, 0, addr, addr, None, 64, None), "grad_norm")
    rejected(ns(ptrs, one, 0, 1.0, 0.0, 0, addr, addr, addr, 64, None), "count")
    rejected(ns(ptrs, one, 1, 0.0, 0.0, 0, addr, addr, addr, 64, None), "mean_scale")
    rejected(ns(ptrs, one, 1, 1.0, 0.0, 0, addr, addr, addr, 4, None), "workspace")


def test_host_arguments():
    from tramba_amd import train
    import tramba_amd as ta
    assert ta.LossScale is train.LossScale
    d = train.LossScale()
    assert (d.init, d.growth, d.backoff, d.growth_interval, d.min_scale, d.max_scale) == (65536.0, 2.0, 0.5, 2000, 1.0, 2.0 ** 24)
    for kw in ({"init": 3.0}, {"growth": 3.0}, {"growth": 1.0}, {"growth": 0.5}, {"backoff": 0.3}, {"backoff": 1.0}, {"backoff": 2.0},
               {"growth_interval": 0}, {"growth_interval": 2.5}, {"min_scale": 0.0}, {"min_scale": 3.0}, {"max_scale": 1e6},
               {"max_scale": float("inf")}, {"min_scale": 4.0, "max_scale": 2.0}):
        with pytest.raises(ValueError):
            train.LossScale(**kw)
    assert train.StepControl(loss_scale="dynamic").scaler.key() == d.key()
    assert train.StepControl(loss_scale="dynamic").skip_nonfinite is True            # implied
    assert train.StepControl(loss_scale=d, skip_nonfinite=True).skip_nonfinite is True
    assert train.StepControl().skip_nonfinite is False and train.StepControl().scaler is None
    with pytest.raises(ValueError, match="skip_nonfinite"):
        train.StepControl(loss_scale="dynamic", skip_nonfinite=False)
    with pytest.raises(ValueError):
        train.StepControl(loss_scale="static")
    with pytest.raises(TypeError):
        train.StepControl(loss_scale=65536.0)
    with pytest.raises(RuntimeError, match="no loss scale"):
        train.StepControl().loss_scale
    with pytest.raises(RuntimeError, match="no step"):
        train.StepControl(loss_scale="dynamic").scale_backoffs


# ----------------------------------------------------------------------------- 2. the fp64 host path
@pytest.mark.parametrize("k", [-8, 0, 8, 20])
def test_a_power_of_two_scale_changes_no_bit(k):
    """accumulate=2 with a clip norm that is active, three steps: parameters and Adam state equal the unscaled controlled
    steps exactly (2^k times a gradient is exact, and so is taking it out again)."""
    from tramba_amd import train
    x, m = _data()
    got, want = _Toy().double(), _Toy().double()
    og, ow = train.get_opt(1e-2, got), train.get_opt(1e-2, want)
    assert type(og) is torch.optim.Adam
    scaler = train.LossScale(init=2.0 ** k, min_scale=2.0 ** -8, max_scale=2.0 ** 20)
    cg = train.StepControl(accumulate=2, clip_norm=0.05, loss_scale=scaler)
    cw = train.StepControl(accumulate=2, clip_norm=0.05, skip_nonfinite=True)
    for step in range(3):
        xs = torch.roll(x, step, 0)
        lg = train.train_step(got, og, xs, m, control=cg)
        lw = train.train_step(want, ow, xs, m, control=cw)
        assert torch.equal(lg, lw)                                     # the returned loss stays unscaled
        assert torch.equal(cg.grad_norm, cw.grad_norm) and float(cw.grad_norm) > 0.05   # ... and so does the norm; clipping is on
        assert float(cg.loss_scale) == 2.0 ** k
    for a, b in zip(_state(got, og), _state(want, ow)):
        assert torch.equal(a, b)
    assert int(cg.skipped_steps) == 0 and int(cg.scale_backoffs) == 0


def _scripted_run(control, flags, model=None, opt=None):
    """one controlled step per flag (True: a batch with a NaN pixel); -> [(scale, good_steps, backoffs, skipped_steps)]"""
    from tramba_amd import train
    x, m = _data(4)
    bad = x.clone()
    bad[3, 1, 3, 3] = float("nan")
    model = model or _Toy().double()
    opt = opt or train.get_opt(1e-2, model)
    seen = []
    for nonfinite in flags:
        before = _state(model, opt)
        train.train_step(model, opt, bad if nonfinite else x, m, control=control)
        after = _state(model, opt)
        same = len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
        assert same == nonfinite                    # a skipped step moves nothing, every other step something
        sd = control.state_dict()
        assert sd["scale"] == float(control.loss_scale) and sd["backoffs"] == int(control.scale_backoffs)
        seen.append((sd["scale"], sd["good_steps"], sd["backoffs"], sd["skipped_steps"]))
    return seen, model, opt


# growth at the interval (twice), the upper clamp, five backoffs into the lower clamp, a backoff that resets a counter of 1
FLAGS = [False] * 7 + [True] * 5 + [False, True, False, False, False]
HYPER = dict(growth=2.0, backoff=0.5, growth_interval=2, min_scale=1.0, max_scale=16.0)


def _expected(flags, scale=4.0, good=0, backoffs=0, skipped=0):
    out = []
    for f in flags:
        scale, good, nb = _rule(scale, good, f, HYPER["growth"], HYPER["backoff"], HYPER["growth_interval"], HYPER["min_scale"],
                                HYPER["max_scale"])
        backoffs, skipped = backoffs + nb, skipped + int(f)
        out.append((scale, good, backoffs, skipped))
    return out


def test_scale_trajectory_follows_the_rule_and_survives_a_state_dict_round_trip():
    from tramba_amd import train
    want = _expected(FLAGS)
    scales = [w[0] for w in want]
    assert max(scales) == 16.0 and min(scales) == 1.0 and scales.count(16.0) >= 2 and scales.count(1.0) >= 2   # both clamps bite
    assert any(a[1] == 1 and b[1] == 0 and b[2] == a[2] + 1 for a, b in zip(want, want[1:]))    # a backoff resets the counter
    got, _, _ = _scripted_run(train.StepControl(accumulate=2, loss_scale=train.LossScale(init=4.0, **HYPER)), FLAGS)
    assert got == want
    # interrupted after 9 steps: a new control object continues from the state_dict
    first = train.StepControl(accumulate=2, loss_scale=train.LossScale(init=4.0, **HYPER))
    assert first.state_dict() == {"skipped_steps": 0, "scale": 4.0, "good_steps": 0, "backoffs": 0}
    head, model, opt = _scripted_run(first, FLAGS[:9])
    second = train.StepControl(accumulate=2, loss_scale=train.LossScale(init=4.0, **HYPER))
    second.load_state_dict(first.state_dict())            # before its first step
    assert second.state_dict() == first.state_dict()
    tail, _, _ = _scripted_run(second, FLAGS[9:], model, opt)
    assert head + tail == want
    second.load_state_dict({"skipped_steps": 2, "scale": 8.0, "good_steps": 1, "backoffs": 3})     # ... and after it
    assert second.state_dict() == {"skipped_steps": 2, "scale": 8.0, "good_steps": 1, "backoffs": 3}
    assert float(second.loss_scale) == 8.0 and int(second.skipped_steps) == 2
    with pytest.raises(ValueError):
        second.load_state_dict({"skipped_steps": 0})
    with pytest.raises(ValueError):
        second.load_state_dict({"skipped_steps": 0, "scale": 3.0, "good_steps": 0, "backoffs": 0})
    plain = train.StepControl(skip_nonfinite=True)
    assert plain.state_dict() == {"skipped_steps": 0}
    with pytest.raises(ValueError):
        plain.load_state_dict(first.state_dict())


def test_the_scale_changes_only_between_optimizer_steps():
    """accumulate=3, a scale that doubles after every step: the three micro-batches of a step see one scale"""
    from tramba_amd import train
    x, m = _data(6)
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(accumulate=3, loss_scale=train.LossScale(init=2.0, growth_interval=1, max_scale=64.0))
    model.watch = lambda: float(control.loss_scale)
    for _ in range(4):
        train.train_step(model, opt, x, m, control=control)
    assert model.seen == [2.0] * 3 + [4.0] * 3 + [8.0] * 3 + [16.0] * 3
    assert float(control.loss_scale) == 32.0


def test_resume_files(tmp_path):
    """without a scaler: the parent's three keys and nothing else; with one: its state under one extra key, which a
    control handed to load_resume continues from"""
    from tramba_amd import train
    x, m = _data(4)
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    for control in (None, train.StepControl(accumulate=2, skip_nonfinite=True)):
        path = train.save_resume(str(tmp_path), "plain", model, opt, 4, control=control)
        assert set(torch.load(path, weights_only=False)) == {"model", "optimizer", "epoch"}
    assert set(torch.load(train.save_resume(str(tmp_path), "plain", model, opt, 4), weights_only=False)) == {"model", "optimizer", "epoch"}
    control = train.StepControl(accumulate=2, loss_scale=train.LossScale(init=4.0, **HYPER))
    hist = train.fit(model, opt, lambda epoch: [(x[:2], m[:2]), (x[2:], m[2:])] * 3, 5, 1e-2, [], [], str(tmp_path), "scaled",
                     control=control)
    assert len(hist) == 5
    ck = torch.load(os.path.join(tmp_path, "scaled", "scaled_resume.pth"), weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "step_control"}
    assert ck["step_control"] == control.state_dict() == {"skipped_steps": 0, "scale": 16.0, "good_steps": 1, "backoffs": 0}
    again, model2 = train.StepControl(accumulate=2, loss_scale=train.LossScale(init=4.0, **HYPER)), _Toy().double()
    opt2 = train.get_opt(1e-2, model2)
    assert train.load_resume("last", str(tmp_path), "scaled", model2, opt2, control=again) == 5
    assert again.state_dict() == control.state_dict()
    # a file without the key leaves the control as it is; a control without a scaler ignores the key
    assert train.load_resume("last", str(tmp_path), "plain", model2, opt2, control=again) == 5
    assert again.state_dict() == control.state_dict()
    plain = train.StepControl(skip_nonfinite=True)
    assert train.load_resume("last", str(tmp_path), "scaled", model2, opt2, control=plain) == 5
    assert plain.state_dict() == {"skipped_steps": 0}
