"""Per-step learning-rate schedules and the weight EMA (train.LrSchedule, train.WeightEMA, StepControl(schedule=, ema=)):
the tables against closed forms restated here, the semantics on host tensors through torch's own functions against
hand-written loops, the state and checkpoint keys, `fit`, and the argument checks of the two library entries (no launch is
issued for a rejected call, so no device is needed)."""
import ctypes
import os
import re

import numpy as np
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

    def forward(self, x):
        y = self.encoder(x)
        return [nn.functional.avg_pool2d(y, 2), self.decoder(y)]


def _data(n=4):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, 3, 16, 16, generator=g, dtype=torch.float64)
    m = (torch.rand(n, 1, 16, 16, generator=g) > 0.7).double()
    return x, m


def _state(model, opt):
    out = [v.clone() for v in model.state_dict().values()]
    for st in opt.state.values():
        out += [torch.as_tensor(st[k]).clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


FACTORS = [1.0, 0.5, 0.3, 0.7, 0.11, 0.9, 0.25, 0.6]


# ----------------------------------------------------------------------------- 1. symbols and refusals
def test_new_symbols_are_exported_bound_and_refuse_bad_arguments():
    from tramba_amd import hip
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_\w+)\s*\(", header))
    for name in ("tramba_step_sched_advance", "tramba_adam_step_sched"):
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    body = re.search(r"typedef struct tramba_step_sched \{(.*?)\} tramba_step_sched;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|double|int32_t|int64_t)\s+(\w+);", body, re.M)
    assert fields == [("int64_t", "step"), ("double", "lr_factor"), ("float", "ema_weight"), ("int32_t", "reserved")]
    assert hip.STEP_SCHED_BYTES == 8 + 8 + 4 + 4

    buf = (ctypes.c_char * 64)()            # a plausible non-null address: a rejected call never touches it
    addr = ctypes.addressof(buf)

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        assert word in lib.tramba_last_error().decode(), lib.tramba_last_error().decode()

    adv = lib.tramba_step_sched_advance
    rejected(adv(None, addr, 4, addr, 3, None), "null")
    for n in (0, -1):
        rejected(adv(addr, addr, n, None, 0, None), "lr table")
        rejected(adv(addr, None, 0, addr, n, None), "ema table")
        rejected(adv(addr, addr, 4, addr, n, None), "ema table")

    ptrs, one = (ctypes.c_void_p * 1)(addr), (ctypes.c_int64 * 1)(1)
    nulls = (ctypes.c_void_p * 1)(None)
    st = lib.tramba_adam_step_sched
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    rejected(st(ptrs, ptrs, ptrs, ptrs, ptrs, one, 1, *hyper, None, None, ptrs, None, None), "schedule record")
    rejected(st(ptrs, ptrs, ptrs, ptrs, ptrs, one, 1, *hyper, None, None, nulls, addr, None), "null average")
    rejected(st(ptrs, ptrs, ptrs, ptrs, ptrs, one, 0, *hyper, None, None, None, addr, None), "empty")
    rejected(st(ptrs, nulls, ptrs, ptrs, ptrs, one, 1, *hyper, None, None, None, addr, None), "null pointer")
    rejected(st(ptrs, ptrs, ptrs, ptrs, ptrs, one, 1, -1.0, 0.9, 0.999, 1e-8, 0.0, None, None, None, addr, None), "hyper")
    rejected(st(ptrs, ptrs, ptrs, ptrs, ptrs, one, 0, *hyper, None, None, None, None, None), "empty")   # the _ctl path's check


# ----------------------------------------------------------------------------- 2. the tables
PI = np.longdouble("3.14159265358979323846264338327950288")


def _close(got, want, rel=1e-15):
    """`want` is an x87 extended-precision evaluation (64-bit significand) of the closed form"""
    assert np.finfo(np.longdouble).nmant >= 63
    return abs(np.longdouble(got) - want) <= rel * abs(want)


@pytest.mark.parametrize("total,warmup,floor", [(1, 0, 0.0), (10, 0, 0.0), (37, 5, 0.01), (1000, 100, 0.1), (257, 256, 0.0)])
def test_warmup_cosine_and_poly_match_their_closed_forms(total, warmup, floor):
    from tramba_amd import train
    ld = np.longdouble
    cos = train.LrSchedule.warmup_cosine(total, warmup=warmup, floor=floor)
    poly = train.LrSchedule.warmup_poly(total, warmup=warmup, power=0.9, floor=floor)
    sq = train.LrSchedule.warmup_poly(total, warmup=warmup, power=2.0, floor=floor)
    assert len(cos) == len(poly) == total + 1
    for t in range(total + 1):
        if t < warmup:
            want_c = want_p = want_s = ld(t + 1) / ld(warmup + 1)
        else:
            x = ld(t - warmup) / ld(total - warmup)                     # the fraction of the decay that has passed
            want_c = ld(floor) + (1 - ld(floor)) * (1 + np.cos(PI * x)) / 2
            want_p = ld(floor) + (1 - ld(floor)) * (1 - x) ** ld(0.9)
            want_s = ld(floor) + (1 - ld(floor)) * (1 - x) ** 2
        assert _close(cos.factor(t), want_c), (t, cos.factor(t), want_c)
        assert _close(poly.factor(t), want_p), (t, poly.factor(t), want_p)
        assert _close(sq.factor(t), want_s), (t, sq.factor(t), want_s)
    assert cos.factor(warmup) == poly.factor(warmup) == 1.0             # the decay starts at the full rate
    for s in (cos, poly):                                               # ... ends at the floor, and stays there
        assert s.factor(total) == s.factor(total + 1) == s.factor(10 ** 9) == floor
        assert s.factor(-3) == s.factor(0)
        assert all(0.0 <= f <= 1.0 for f in s.factors)
    if warmup:
        assert cos.factor(0) == 1 / (warmup + 1) and cos.factor(warmup - 1) == warmup / (warmup + 1)


def test_step_decay_is_the_epoch_rule_bit_for_bit():
    from tramba_amd import train
    base, spe, epochs = 3.7e-4, 3, 12
    decay_epochs, decay_factors = [4, 9, 7], [0.3, 0.01, 0.07]
    s = train.LrSchedule.step_decay(spe, epochs, decay_epochs, decay_factors)
    assert len(s) == spe * epochs
    opt = torch.optim.Adam([{"params": [nn.Parameter(torch.zeros(1))], "lr": base * 0.1},
                            {"params": [nn.Parameter(torch.zeros(1))], "lr": base}], base)
    for epoch in range(epochs):
        lr = train.adjust_learning_rate(opt, epoch, decay_epochs, base, decay_factors)
        for k in range(spe):
            assert base * s.factor(epoch * spe + k) == lr == opt.param_groups[1]["lr"], (epoch, k)
    assert s.factor(spe * epochs + 5) == 0.01
    assert train.LrSchedule.step_decay(2, 3, [], []).factors == (1.0,) * 6
    with pytest.raises(ValueError):
        train.LrSchedule.step_decay(2, 3, [1], [])


def test_tables_from_sequences_and_callables_and_what_is_refused():
    from tramba_amd import train
    import tramba_amd as ta
    assert ta.LrSchedule is train.LrSchedule and ta.WeightEMA is train.WeightEMA
    s = train.LrSchedule(FACTORS)
    assert s.factors == tuple(FACTORS) and len(s) == 8
    assert [s.factor(t) for t in range(8)] == FACTORS and s.factor(8) == s.factor(500) == FACTORS[-1]
    fn = lambda t: 1.0 / (1.0 + 0.37 * t)       # noqa: E731
    c = train.LrSchedule.from_callable(fn, 23)
    assert c.factors == tuple(fn(t) for t in range(23)) and c.factor(99) == fn(22)
    t = s.table("cpu")
    assert t.dtype == torch.float64 and t.tolist() == FACTORS and s.table("cpu") is t          # uploaded once
    for bad in ([], [1.0, -0.5], [float("nan")], [0.5, float("inf")], [-0.0 - 1e-300]):
        with pytest.raises(ValueError):
            train.LrSchedule(bad)
    with pytest.raises(ValueError):
        train.LrSchedule.from_callable(fn, 0)
    for kw in ({"total": 0}, {"total": 10, "warmup": 10}, {"total": 10, "warmup": -1}, {"total": 10, "floor": 1.5}, {"total": 10, "floor": -0.1}):
        with pytest.raises(ValueError):
            train.LrSchedule.warmup_cosine(**kw)
        with pytest.raises(ValueError):
            train.LrSchedule.warmup_poly(**kw)
    with pytest.raises(ValueError):
        train.LrSchedule.warmup_poly(10, power=0.0)
    with pytest.raises(TypeError):
        train.StepControl(schedule=[1.0, 0.5])
    with pytest.raises(TypeError):
        train.StepControl(ema=0.999)
    with pytest.raises(RuntimeError, match="neither"):
        train.StepControl().lr_factor
    with pytest.raises(RuntimeError, match="no step"):
        train.StepControl(schedule=s).sched_step


def test_ema_weight_table():
    from tramba_amd import train
    e = train.WeightEMA()
    assert (e.decay, e.warmup) == (0.999, True)
    ws = e.weights
    n = next(t for t in range(100000) if (1 + t) / (10 + t) >= 0.999)       # the first step at the final decay
    assert len(ws) == n + 1
    for t in (0, 1, 2, 17, 500, n - 1, n):
        assert ws[t] == float(np.float32(1.0 - min(0.999, (1 + t) / (10 + t)))), t
    assert ws[0] == float(np.float32(0.9)) and ws[-1] == float(np.float32(1.0 - 0.999)) == e.weight(n + 7)
    assert all(a >= b for a, b in zip(ws, ws[1:]))
    flat = train.WeightEMA(decay=0.9, warmup=False)
    assert flat.weights == (float(np.float32(1.0 - 0.9)),)
    assert flat.table("cpu").dtype == torch.float32 and flat.table("cpu").tolist() == list(flat.weights)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            train.WeightEMA(decay=bad)


# ----------------------------------------------------------------------------- 3. the fp64 host path
def test_scheduled_steps_equal_a_hand_written_loop():
    from tramba_amd import train
    x, m = _data()
    got, want = _Toy().double(), _Toy().double()
    og, ow = train.get_opt(1e-2, got), train.get_opt(1e-2, want)
    assert type(og) is torch.optim.Adam
    control = train.StepControl(schedule=train.LrSchedule(FACTORS))
    bases = [g["lr"] for g in ow.param_groups]
    for t in range(8):
        xs = torch.roll(x, t, 0)
        train.train_step(got, og, xs, m, control=control)
        for g, base in zip(ow.param_groups, bases):
            g["lr"] = base * FACTORS[t]
        ow.zero_grad(set_to_none=True)
        train.tramba_loss(want(xs), m).backward()
        ow.step()
        assert _same(_state(got, og), _state(want, ow)), t
        assert int(control.sched_step) == t + 1
        assert control.lr_factor.dtype == torch.float64 and control.lr_factor.dim() == 0
        assert float(control.lr_factor) == FACTORS[min(t + 1, 7)]              # the next step's
    # the factors did something: a run at the constant base rate ends elsewhere
    plain = _Toy().double()
    op = train.get_opt(1e-2, plain)
    cp = train.StepControl()
    for t in range(8):
        train.train_step(plain, op, torch.roll(x, t, 0), m, control=cp)
    assert not _same(_state(got, og), _state(plain, op))


def _ema_run(control, steps, bad_at=(), model=None, opt=None, start=0):
    """controlled steps with the averages checked against a by-hand lerp after every one; -> (model, opt, trace)"""
    from tramba_amd import train
    x, m = _data()
    bad = x.clone()
    bad[1, 2, 3, 3] = float("inf")
    model = model or _Toy().double()
    opt = opt or train.get_opt(1e-2, model)
    ema, trace = control.ema, []
    params = [p for g in opt.param_groups for p in g["params"]]
    for t in range(start, start + steps):
        before = None if not ema._order else [e.clone() for e in ema.tensors()]
        if before is None:                             # the first step lays the averages out: as the parameters before it,
            src = params if ema._pending is None else ema._pending       # or as load_state_dict left them
            before = [p.detach().clone() for p in src]
        skipped_before = 0 if control._key is None else int(control.skipped_steps)
        train.train_step(model, opt, torch.roll(bad if t in bad_at else x, t, 0), m, control=control)
        now = ema.tensors()
        assert len(now) == len(params)
        if t in bad_at:
            assert _same(now, before)
            assert int(control.skipped_steps) == skipped_before + 1
        else:
            want = [e.lerp(p.detach(), ema.weight(t)) for e, p in zip(before, params)]
            assert _same(now, want), t
            assert not _same(now, before)
        assert int(control.sched_step) == t + 1
        trace.append(_state(model, opt) + [e.clone() for e in now])
    return model, opt, trace


def test_host_ema_follows_a_hand_lerp_and_a_skipped_step_leaves_it():
    from tramba_amd import train
    control = train.StepControl(skip_nonfinite=True, schedule=train.LrSchedule(FACTORS), ema=train.WeightEMA(decay=0.9))
    assert len(control.ema.weights) > 8 and len(set(control.ema.weights[:8])) == 8          # a different weight at every step
    _ema_run(control, 8, bad_at=(3,))
    assert int(control.skipped_steps) == 1 and int(control.sched_step) == 8
    assert float(control.lr_factor) == FACTORS[-1]
    # an EMA alone keeps the record too; the rate stays the groups' own
    alone = train.StepControl(ema=train.WeightEMA(decay=0.9, warmup=False))
    model, opt, _ = _ema_run(alone, 3)
    assert float(alone.lr_factor) == 1.0 and [g["lr"] for g in opt.param_groups] == [1e-2 * 0.1, 1e-2]


def test_state_dict_round_trip_continues_the_trajectory():
    from tramba_amd import train
    make = lambda: train.StepControl(skip_nonfinite=True, schedule=train.LrSchedule(FACTORS), ema=train.WeightEMA(decay=0.9))   # noqa: E731
    _, _, want = _ema_run(make(), 8, bad_at=(2,))
    first = make()
    assert first.state_dict() == {"skipped_steps": 0, "sched_step": 0}
    model, opt, head = _ema_run(first, 5, bad_at=(2,))
    assert first.state_dict() == {"skipped_steps": 1, "sched_step": 5}
    second = make()
    second.load_state_dict(first.state_dict())                       # before its first step
    second.ema.load_state_dict(first.ema.state_dict())
    assert second.state_dict() == first.state_dict()
    _, _, tail = _ema_run(second, 3, model=model, opt=opt, start=5)
    assert len(head + tail) == len(want) and all(_same(a, b) for a, b in zip(head + tail, want))
    second.load_state_dict({"skipped_steps": 4, "sched_step": 2})    # ... and after it
    assert int(second.sched_step) == 2 and float(second.lr_factor) == FACTORS[2] and int(second.skipped_steps) == 4
    for bad in ({"skipped_steps": 0}, {"skipped_steps": 0, "sched_step": -1}, {"skipped_steps": 0, "sched_step": 1, "scale": 2.0}):
        with pytest.raises(ValueError):
            second.load_state_dict(bad)
    sd = second.ema.state_dict()
    assert set(sd) == {"decay", "warmup", "tensors"} and len(sd["tensors"]) == len(list(model.parameters()))
    with pytest.raises(ValueError):
        second.ema.load_state_dict({"decay": 0.9, "warmup": True, "tensors": sd["tensors"][:-1]})
    # a control without a schedule or EMA: exactly the keys it has always had
    plain = train.StepControl(skip_nonfinite=True)
    assert plain.state_dict() == {"skipped_steps": 0}
    plain.load_state_dict({"skipped_steps": 3})
    with pytest.raises(ValueError):
        plain.load_state_dict({"skipped_steps": 0, "sched_step": 0})
    scaled = train.StepControl(loss_scale=train.LossScale(init=4.0))
    assert scaled.state_dict() == {"skipped_steps": 0, "scale": 4.0, "good_steps": 0, "backoffs": 0}
    both = train.StepControl(loss_scale=train.LossScale(init=4.0), schedule=train.LrSchedule(FACTORS))
    assert both.state_dict() == {"skipped_steps": 0, "scale": 4.0, "good_steps": 0, "backoffs": 0, "sched_step": 0}


# ----------------------------------------------------------------------------- 4. files and fit
def test_resume_files(tmp_path):
    from tramba_amd import train
    x, m = _data()
    make = lambda: train.StepControl(schedule=train.LrSchedule(FACTORS), ema=train.WeightEMA(decay=0.9))   # noqa: E731
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    control = make()
    for t in range(3):
        train.train_step(model, opt, torch.roll(x, t, 0), m, control=control)
    path = train.save_resume(str(tmp_path), "both", model, opt, 4, control=control)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "step_control", "ema"}
    assert ck["step_control"] == {"skipped_steps": 0, "sched_step": 3}
    assert _same(ck["ema"]["tensors"], control.ema.tensors())
    only = train.StepControl(schedule=train.LrSchedule(FACTORS))
    ck = torch.load(train.save_resume(str(tmp_path), "sched", model, opt, 4, control=only), weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "step_control"} and ck["step_control"] == {"skipped_steps": 0, "sched_step": 0}
    # the loaded run continues as the first one does
    model2, again = _Toy().double(), make()
    opt2 = train.get_opt(1e-2, model2)
    assert train.load_resume("last", str(tmp_path), "both", model2, opt2, control=again) == 5
    assert again.state_dict() == control.state_dict()
    for t in range(3, 6):
        train.train_step(model, opt, torch.roll(x, t, 0), m, control=control)
        train.train_step(model2, opt2, torch.roll(x, t, 0), m, control=again)
    assert _same(_state(model, opt), _state(model2, opt2)) and _same(control.ema.tensors(), again.ema.tensors())
    assert int(again.sched_step) == 6
    # a file written without the features still loads, with or without a control that has them
    plain_path = train.save_resume(str(tmp_path), "plain", model, opt, 4, control=train.StepControl(skip_nonfinite=True))
    assert set(torch.load(plain_path, weights_only=False)) == {"model", "optimizer", "epoch"}
    fresh = make()
    assert train.load_resume("last", str(tmp_path), "plain", model2, opt2, control=fresh) == 5
    assert fresh.state_dict() == {"skipped_steps": 0, "sched_step": 0}
    assert train.load_resume("last", str(tmp_path), "both", model2, opt2, control=train.StepControl(skip_nonfinite=True)) == 5


def test_fit_with_a_schedule_and_an_ema(tmp_path):
    from tramba_amd import train
    x, m = _data()
    batches = lambda epoch: [(x[:2], m[:2]), (x[2:], m[2:])]        # noqa: E731  two optimizer steps per epoch
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    sched = train.LrSchedule(FACTORS[:6])
    with pytest.raises(ValueError, match="decay_epochs"):
        train.fit(model, opt, batches, 2, 1e-2, [1], [0.1], str(tmp_path), "m", control=train.StepControl(schedule=sched))
    control = train.StepControl(schedule=sched, ema=train.WeightEMA(decay=0.9))
    seen = []

    def evaluate(mod, epoch):
        # inside ema.applied: the model holds the averages; between steps the groups hold their base rates
        assert _same([p.detach() for p in mod.parameters()], control.ema.tensors())
        seen.append([g["lr"] for g in opt.param_groups])
        return 1.0 / (epoch + 1)

    live_ptrs = [p.data_ptr() for p in model.parameters()]
    hist = train.fit(model, opt, batches, 5, 1e-2, None, None, str(tmp_path), "m", control=control, evaluate=evaluate)
    assert [h["lr"] for h in hist] == [1e-2 * sched.factor(2 * e) for e in range(5)]
    assert seen == [[1e-2 * 0.1, 1e-2]] * 5
    assert [p.data_ptr() for p in model.parameters()] == live_ptrs
    assert not _same([p.detach() for p in model.parameters()], control.ema.tensors())         # the live weights are back
    best = torch.load(os.path.join(tmp_path, "m", "m_MAE_0.2_5.pth"), weights_only=False)
    assert list(best) == list(model.state_dict())
    assert _same([best[n] for n, _ in model.named_parameters()], control.ema.tensors())
    ck = torch.load(os.path.join(tmp_path, "m", "m_resume.pth"), weights_only=False)
    assert ck["step_control"] == {"skipped_steps": 0, "sched_step": 10} and len(ck["ema"]["tensors"]) == len(live_ptrs)


def test_fit_with_a_schedule_never_calls_the_epoch_rule(monkeypatch):
    from tramba_amd import train
    x, m = _data()
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(schedule=train.LrSchedule(FACTORS))
    called = []
    monkeypatch.setattr(train, "adjust_learning_rate", lambda *a, **k: called.append(a) or 0.0)
    hist = train.fit(model, opt, lambda e: [(x, m)], 3, 1e-2, [], [], "unused", "m", control=control, is_main=False)
    assert not called and [h["lr"] for h in hist] == [1e-2 * FACTORS[e] for e in range(3)]
    assert [g["lr"] for g in opt.param_groups] == [1e-2 * 0.1, 1e-2]
    # continued: the history starts from the control's step, not from zero
    hist = train.fit(model, opt, lambda e: [(x, m)], 5, 1e-2, [], [], "unused", "m", control=control, is_main=False, start_epoch=3)
    assert [h["lr"] for h in hist] == [1e-2 * FACTORS[3], 1e-2 * FACTORS[4]]
    # without a schedule the epoch rule runs as before
    train.fit(model, opt, lambda e: [(x, m)], 1, 1e-2, [], [], "unused", "m", control=train.StepControl(), is_main=False)
    assert len(called) == 1


# ----------------------------------------------------------------------------- 5. applied
def test_applied_swaps_content_not_pointers():
    from tramba_amd import train
    x, m = _data()
    model = _Toy().double()
    opt = train.get_opt(1e-2, model)
    control = train.StepControl(ema=train.WeightEMA(decay=0.9))
    with pytest.raises(RuntimeError, match="no parameter"):
        with control.ema.applied(model):
            pass
    for t in range(3):
        train.train_step(model, opt, torch.roll(x, t, 0), m, control=control)
    live = [p.detach().clone() for p in model.parameters()]
    ptrs = [p.data_ptr() for p in model.parameters()]
    versions = [p._version for p in model.parameters()]
    out_live = model(x)[1].detach().clone()
    with control.ema.applied(model) as inside:
        assert inside is model
        sd = model.state_dict()
        assert _same([sd[n] for n, _ in model.named_parameters()], control.ema.tensors())
        assert [p.data_ptr() for p in model.parameters()] == ptrs
        assert all(p._version > v for p, v in zip(model.parameters(), versions))
        mid = [p._version for p in model.parameters()]
        out_ema = model(x)[1].detach().clone()
    assert _same([p.detach() for p in model.parameters()], live)
    assert [p.data_ptr() for p in model.parameters()] == ptrs
    assert all(p._version > v for p, v in zip(model.parameters(), mid))
    assert torch.equal(model(x)[1], out_live) and not torch.equal(out_ema, out_live)
    # model_state_dict: the averages under the parameters' names, in a fresh model the same outputs
    other = _Toy().double()
    other.load_state_dict(control.ema.model_state_dict(model))
    assert torch.equal(other(x)[1], out_ema)
    with pytest.raises(ZeroDivisionError):             # an exception inside still puts the live weights back
        with control.ema.applied(model):
            1 / 0
    assert _same([p.detach() for p in model.parameters()], live)
