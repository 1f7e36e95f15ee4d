"""GPU tests of the per-step learning-rate schedule and the weight EMA: the two library entries (tramba_adam_step_sched,
tramba_step_sched_advance) against tramba_adam_step_ctl and against fp64 restatements, and the controlled step with a
schedule and an EMA -- eager against hand-set rates, captured against eager (no re-capture, a skipped replay, the next
factor), evaluation with the averaged weights in bf16."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [1, 3, 4, 5, 4095, 8191, 8192, 8193, 20000]      # the vector tail, the edges of a chunk of 8192, three chunks
MANY = [4] * 150                                          # more than two launches' worth in either argument struct
LAYOUTS = {"aligned": (SIZES, 4), "odd": (SIZES, 1), "many": (MANY, 4)}
EDGE_CYCLE = [1, 3, 4, 5, 8191, 8192, 8193]               # the sizes of a table filled to its last slot, and of one slot more


def edge_sizes(count):
    return [EDGE_CYCLE[i % len(EDGE_CYCLE)] for i in range(count)]
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
LR = 3.7e-4


class _Flat:
    """tensors as views of one flat buffer, each with at least four guard elements on either side.  `start` = 4: every view
    16-byte aligned; `start` = 1: every view one element past such an address (the scalar path)"""

    def __init__(self, sizes, start, fill):
        offs, off = [], start
        for n in sizes:
            offs.append(off)
            off += (n + 3) // 4 * 4 + 4
        self.flat = torch.full((off + 4,), 7.25, device=DEV)
        inside = torch.zeros(off + 4, dtype=torch.bool)
        self.views = []
        for n, o in zip(sizes, offs):
            v = self.flat[o:o + n]
            v.copy_(fill(n))
            assert v.data_ptr() % 16 == (0 if start == 4 else 4)
            self.views.append(v)
            inside[o:o + n] = True
        self.guard = (~inside).to(DEV)

    def guards_intact(self):
        return bool((self.flat[self.guard] == 7.25).all())


class _Set:
    """parameters, gradients, both moments and averages of one layout, and the step counters; the same seed gives the
    same bits"""

    def __init__(self, layout, seed=3):
        sizes, start = LAYOUTS[layout] if isinstance(layout, str) else layout
        self.sizes, self.start = sizes, start
        self.gen = torch.Generator().manual_seed(seed)
        rnd = lambda scale: (lambda n: torch.randn(n, generator=self.gen) * scale)     # noqa: E731
        self.p, self.g = _Flat(sizes, start, rnd(1.0)), _Flat(sizes, start, rnd(0.1))
        self.m = _Flat(sizes, start, rnd(0.05))
        self.v = _Flat(sizes, start, lambda n: torch.rand(n, generator=self.gen) * 1e-2)
        self.e = _Flat(sizes, start, lambda n: torch.zeros(n))
        self.e.flat[~self.e.guard] = self.p.flat[~self.p.guard]          # an average starts as its parameter
        self.steps_flat = torch.full((len(sizes),), 2.0, device=DEV)
        self.steps = [self.steps_flat[i] for i in range(len(sizes))]
        self.numel = (ctypes.c_int64 * len(sizes))(*sizes)

    def new_grads(self):
        for v in self.g.views:
            v.copy_(torch.randn(v.numel(), generator=self.gen) * 0.1)

    def bits(self):
        return [t.flat.clone() for t in (self.p, self.g, self.m, self.v, self.e)] + [self.steps_flat.clone()]

    def guards_intact(self):
        return all(t.guards_intact() for t in (self.p, self.g, self.m, self.v, self.e))

    def arrays(self):
        from tramba_amd import hip
        return [hip.pointer_array(t.views) for t in (self.p, self.g, self.m, self.v)] + [hip.pointer_array(self.steps), self.numel,
                                                                                        len(self.sizes)]

    def step_ctl(self, lr, gscale=None, skip=None):
        from tramba_amd import hip
        hip.adam_step_raw(*self.arrays(), lr, HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], gscale=gscale,
                          skip=skip)

    def step_sched(self, lr, gscale=None, skip=None, ema=False, sched=None):
        from tramba_amd import hip
        hip.adam_step_sched_raw(*self.arrays(), lr, HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"],
                                gscale=gscale, skip=skip, ema=hip.pointer_array(self.e.views) if ema else None, sched=sched)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _ctl(scale=0.5, skip=0):
    from tramba_amd import hip
    rec, f = hip.step_ctl_record(DEV)
    f["scale"].fill_(scale)
    f["skip"].fill_(skip)
    return rec, f


def _ema_misses(got, e_old, p_new, w):
    """elements of `got` further than 1 fp32 ulp from  e_old + w (p_new - e_old)  evaluated in fp64.  The difference is
    formed as the kernel forms it, in fp32 (exact wherever p_new and e_old lie within a factor of two of each other, which
    is where an average lives), the product and the sum in fp64: the stand-in for the kernel's fmaf, which it can differ
    from by a double rounding and by nothing else.  `w` is the fp32 weight as a Python float."""
    got, e_old, p_new = (t.detach().flatten().cpu().numpy() for t in (got, e_old, p_new))
    d = (p_new - e_old).astype(np.float64)                               # fp32 subtraction, then exact widening
    want = e_old.astype(np.float64) + np.float64(w) * d
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return int((np.abs(got.astype(np.float64) - want) > ulp).sum())


# ------------------------------------------------------------------------------------------------- 1. tramba_adam_step_sched
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_without_record_and_average_it_is_the_ctl_step(layout):
    a, b = _Set(layout), _Set(layout)
    assert _equal(a.bits(), b.bits())
    _, f = _ctl(0.5, 0)
    for _ in range(3):
        a.step_sched(LR, gscale=f["scale"], skip=f["skip"])
        b.step_ctl(LR, gscale=f["scale"], skip=f["skip"])
        a.new_grads()
        b.new_grads()
    torch.cuda.synchronize()
    assert _equal(a.bits(), b.bits()) and a.guards_intact()
    assert bool((a.steps_flat == 5.0).all())
    assert not torch.equal(a.p.flat, _Set(layout).p.flat)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_factor_is_a_double_product_into_the_rate_read_at_run_time(layout):
    from tramba_amd import hip
    a, b = _Set(layout), _Set(layout)
    _, f = _ctl(0.5, 0)
    rec, sf = hip.step_sched_record(DEV, lr_factor=0.3)
    for factor in (0.3, 1e-3):
        sf["lr_factor"].fill_(factor)                                    # written into the record between the steps
        a.step_sched(LR, gscale=f["scale"], skip=f["skip"], sched=rec)
        b.step_ctl(LR * factor, gscale=f["scale"], skip=f["skip"])
        torch.cuda.synchronize()
        assert _equal(a.bits(), b.bits()), factor
        a.new_grads()
        b.new_grads()
    assert a.guards_intact() and int(sf["step"]) == 0                    # the optimizer reads the record, it never writes it
    c = _Set(layout)                                                     # ... and the factor matters
    c.step_ctl(LR, gscale=f["scale"], skip=f["skip"])
    c.new_grads()
    c.step_ctl(LR, gscale=f["scale"], skip=f["skip"])
    assert not torch.equal(c.p.flat, a.p.flat)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_average_moves_in_the_same_pass(layout):
    from tramba_amd import hip
    a, b = _Set(layout), _Set(layout)
    w = float(np.float32(0.1))
    rec, sf = hip.step_sched_record(DEV, lr_factor=0.7, ema_weight=0.1)
    for k in range(5):
        e_old = a.e.flat.clone()
        a.step_sched(LR, sched=rec, ema=True)
        b.step_ctl(LR * 0.7)
        torch.cuda.synchronize()
        assert _equal(a.bits()[:4], b.bits()[:4]) and torch.equal(a.steps_flat, b.steps_flat), k      # p, g, m, v as without
        inside = ~a.e.guard
        assert _ema_misses(a.e.flat[inside], e_old[inside], a.p.flat[inside], w) == 0, k
        assert not torch.equal(a.e.flat[inside], e_old[inside])
        assert a.guards_intact(), k
        a.new_grads()
        b.new_grads()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_set_skip_flag_leaves_every_bit_and_the_record_still_advances(layout):
    from tramba_amd import hip
    a = _Set(layout)
    _, f = _ctl(0.5, 1)
    lr_table = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64, device=DEV)
    ema_table = torch.tensor([0.5, 0.125], dtype=torch.float32, device=DEV)
    rec, sf = hip.step_sched_record(DEV, lr_factor=1.0, ema_weight=0.5)
    before = a.bits()
    a.step_sched(LR, gscale=f["scale"], skip=f["skip"], sched=rec, ema=True)
    hip.step_sched_advance_raw(rec, lr_table, ema_table)
    torch.cuda.synchronize()
    assert _equal(a.bits(), before)
    assert (int(sf["step"]), float(sf["lr_factor"]), float(sf["ema_weight"])) == (1, 0.5, 0.125)
    f["skip"].fill_(0)                                                   # the same call moves everything once the flag is down
    a.step_sched(LR, gscale=f["scale"], skip=f["skip"], sched=rec, ema=True)
    torch.cuda.synchronize()
    after = a.bits()
    assert all(not torch.equal(x, y) for x, y in zip(after[:1] + after[2:], before[:1] + before[2:])) and a.guards_intact()


@pytest.mark.parametrize("count", [64, 65])                    # kAdamSchedTensors = 64 in csrc/loss_optim.hip
def test_a_full_argument_table_and_one_tensor_more(count):
    """64 tensors fill the one launch's table to its last slot (no padding, first[64] alone is the grid); 65 make two launches
    of 33 and 32.  With record and averages, at factor 1.0: p, g, m, v as the ctl step (one launch of its 72 slots) leaves
    them, every average moved, every tensor touched, nothing beside them."""
    from tramba_amd import hip
    layout = (edge_sizes(count), 4)
    a, b = _Set(layout), _Set(layout)
    w = float(np.float32(0.1))
    rec, _ = hip.step_sched_record(DEV, lr_factor=1.0, ema_weight=0.1)
    _, f = _ctl(0.5, 0)
    for k in range(2):
        old = {name: [v.clone() for v in getattr(a, name).views] for name in "pmve"}
        e_old = a.e.flat.clone()
        a.step_sched(LR, gscale=f["scale"], skip=f["skip"], sched=rec, ema=True)
        b.step_ctl(LR, gscale=f["scale"], skip=f["skip"])
        torch.cuda.synchronize()
        assert _equal(a.bits()[:4], b.bits()[:4]) and torch.equal(a.steps_flat, b.steps_flat), k
        assert bool((a.steps_flat == 3.0 + k).all())
        inside = ~a.e.guard
        assert _ema_misses(a.e.flat[inside], e_old[inside], a.p.flat[inside], w) == 0, k
        for name, views in old.items():
            same = [i for i, (x, y) in enumerate(zip(views, getattr(a, name).views)) if torch.equal(x, y)]
            assert not same, (k, name, same)
        assert a.guards_intact() and b.guards_intact(), k
        a.new_grads()
        b.new_grads()


# ------------------------------------------------------------------------------------------------- 2. tramba_step_sched_advance
def test_step_sched_advance_eagerly_and_replayed():
    from tramba_amd import hip
    lr_host, ema_host = [1.0, 0.37, 1e-3, 0.0], [float(np.float32(0.9)), float(np.float32(0.3)), float(np.float32(1e-3))]
    lr_table = torch.tensor(lr_host, dtype=torch.float64, device=DEV)
    ema_table = torch.tensor(ema_host, dtype=torch.float32, device=DEV)

    def read(sf):
        return int(sf["step"]), float(sf["lr_factor"]), float(sf["ema_weight"])

    want = [(t, lr_host[min(t, 3)], ema_host[min(t, 2)]) for t in range(1, 8)]
    rec, sf = hip.step_sched_record(DEV, lr_factor=lr_host[0], ema_weight=ema_host[0])
    assert read(sf) == (0, lr_host[0], ema_host[0])
    got = []
    for _ in range(7):
        hip.step_sched_advance_raw(rec, lr_table, ema_table)
        got.append(read(sf))
    assert got == want
    assert int(rec.view(torch.int32)[5]) == 0                            # nothing else is written
    # no tables: the factor is 1.0, the weight stays
    rec, sf = hip.step_sched_record(DEV, lr_factor=0.25, ema_weight=0.125)
    hip.step_sched_advance_raw(rec, None, None)
    assert read(sf) == (1, 1.0, 0.125)
    hip.step_sched_advance_raw(rec, lr_table, None)
    assert read(sf) == (2, lr_host[2], 0.125)
    hip.step_sched_advance_raw(rec, None, ema_table)
    assert read(sf) == (3, 1.0, ema_host[2])
    # captured once as a one-node graph: every replay moves the record on
    rec, sf = hip.step_sched_record(DEV, lr_factor=lr_host[0], ema_weight=ema_host[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.step_sched_advance_raw(rec, lr_table, ema_table)
    torch.cuda.synchronize()
    assert read(sf) == (0, lr_host[0], ema_host[0])                      # a capture executes nothing
    got = []
    for _ in range(7):
        graph.replay()
        got.append(read(sf))
    assert got == want


# ------------------------------------------------------------------------------------------------- the controlled step
class _Tiny(torch.nn.Module):
    """one decoder block + a per-channel head behind the interface train.train_step expects (the model of
    tests/test_gpu_loss_scale.py): 16-bit activations when compute_dtype is set, fp32 master weights"""

    def __init__(self, compute_dtype=None, drop_path=0.0):
        super().__init__()
        import tramba_amd as ta
        torch.manual_seed(11)
        self.encoder = ta.MultiScaleDecoderBlock(hidden_dim=32, drop_path=drop_path, channel_first=True)
        self.encoder_head = torch.nn.Parameter(torch.randn(32) * 0.2)
        self.encoder_bias = torch.nn.Parameter(torch.zeros(1))
        self.compute_dtype = compute_dtype

    def forward(self, z):
        if self.training:
            from tramba_amd.modules import model_mask_pool
            model_mask_pool(self).begin_step()
        h = self.encoder(z if self.compute_dtype is None else z.to(self.compute_dtype))
        w = self.encoder_head.to(h.dtype).view(1, -1, 1, 1)
        return [(h * w).sum(dim=1, keepdim=True) + self.encoder_bias.to(h.dtype).view(1, 1, 1, 1)]


def _tiny_data(n=2):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, 32, 24, 24, generator=g).to(DEV), (torch.rand(n, 1, 24, 24, generator=g) > 0.5).float().to(DEV)


FACTORS = [1.0, 0.5, 0.3, 0.7, 0.11, 0.9, 0.25, 0.6, 0.45]
STEPS = 6
BASE = 1e-3


def _control(**kw):
    from tramba_amd import train
    return train.StepControl(skip_nonfinite=True, schedule=train.LrSchedule(FACTORS), ema=train.WeightEMA(decay=0.9), **kw)


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _full_state(model, opt, control):
    out = _params(model)
    for st in opt.state.values():
        out += [st[k].clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out + [e.clone() for e in control.ema.tensors()]


def _rel_l2(got, want):
    want = want.detach().double()
    return float((got.detach().double() - want).norm() / want.norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def eager_run():
    """6 eager controlled steps with a schedule and an EMA; the averages are checked against the by-hand lerp on the way"""
    from tramba_amd import train
    x, y = _tiny_data()
    m = _Tiny().to(DEV).train()
    opt = train.get_opt(BASE, m)
    control = _control()
    assert len(set(control.ema.weights[:STEPS])) == STEPS and len(set(FACTORS[:STEPS])) == STEPS   # both differ at every step
    run = {"losses": [], "params": [], "emas": [], "factors": [], "misses": [], "lrs": []}
    e_old = _params(m)                                                   # the averages start as the parameters
    for k in range(STEPS):
        run["losses"].append(float(train.train_step(m, opt, torch.roll(x, k, 0), y, control=control)))
        now = [e.clone() for e in control.ema.tensors()]
        run["misses"].append(sum(_ema_misses(e, eo, p, control.ema.weight(k)) for e, eo, p in zip(now, e_old, m.parameters())))
        e_old = now
        run["params"].append(_params(m))
        run["emas"].append(now)
        run["factors"].append(float(control.lr_factor))
        run["lrs"].append([g["lr"] for g in opt.param_groups])
    run["sched_step"], run["skipped"] = int(control.sched_step), int(control.skipped_steps)
    return run


def test_eager_scheduled_step_equals_hand_set_rates(eager_run):
    from tramba_amd import train
    x, y = _tiny_data()
    m = _Tiny().to(DEV).train()
    opt = train.get_opt(BASE, m)
    control = train.StepControl(skip_nonfinite=True)
    bases = [g["lr"] for g in opt.param_groups]
    for k in range(STEPS):
        for g, base in zip(opt.param_groups, bases):
            g["lr"] = base * FACTORS[k]
        loss = float(train.train_step(m, opt, torch.roll(x, k, 0), y, control=control))
        assert loss == eager_run["losses"][k], k
        assert _equal(_params(m), eager_run["params"][k]), k
    assert eager_run["lrs"] == [bases] * STEPS                           # the scheduled run never wrote a group's rate
    assert eager_run["factors"] == FACTORS[1:STEPS + 1]                  # the read-out is the NEXT step's factor
    assert eager_run["sched_step"] == STEPS and eager_run["skipped"] == 0
    assert not _equal(eager_run["params"][0], eager_run["params"][-1])


def test_eager_averages_follow_the_hand_lerp(eager_run):
    assert eager_run["misses"] == [0] * STEPS
    assert all(not _equal(a, b) for a, b in zip(eager_run["emas"], eager_run["emas"][1:]))
    assert not _equal(eager_run["emas"][-1], eager_run["params"][-1])


@pytest.fixture(scope="module")
def graphed_run():
    import tramba_amd as ta
    from tramba_amd import train
    x, y = _tiny_data()
    m = _Tiny().to(DEV).train()
    opt = train.get_opt(BASE, m, capturable=True)
    control = _control()
    step = ta.GraphedTrainStep(m, opt, control=control)
    run = {"losses": [], "params": [], "emas": [], "factors": [], "lrs": [], "graphs": [], "m": m, "opt": opt, "control": control,
           "step": step}
    for k in range(STEPS):
        run["losses"].append(float(step(torch.roll(x, k, 0), y)))
        run["params"].append(_params(m))
        run["emas"].append([e.clone() for e in control.ema.tensors()])
        run["factors"].append(float(control.lr_factor))
        run["lrs"].append([g["lr"] for g in opt.param_groups])
        run["graphs"].append([g[0] for e in step._graphs.values() for g in ([e["mid"]] if e["mid"] else []) + list(e["update"].values())])
        if k == 0:          # the warm-up steps were undone: the record and the optimizer show exactly one step
            assert int(control.sched_step) == 1 and all(float(st["step"]) == 1.0 for st in opt.state.values())
    run["sched_step"], run["skipped"] = int(control.sched_step), int(control.skipped_steps)
    return run


def test_graphed_scheduled_step_never_recaptures_and_follows_the_eager_one(eager_run, graphed_run):
    got, eager = graphed_run, eager_run
    first = got["graphs"][0]
    assert len(first) == 1                                               # one micro-batch shape, accumulate=1: the update graph
    assert all(len(g) == len(first) and all(a is b for a, b in zip(g, first)) for g in got["graphs"])     # the same objects
    assert got["lrs"] == [[BASE * 0.1, BASE]] * STEPS
    assert got["factors"] == FACTORS[1:STEPS + 1]
    assert got["sched_step"] == STEPS and got["skipped"] == 0
    print("eager", eager["losses"], "graphed", got["losses"])
    # the criterion of test_graphed_step_with_a_scale_follows_the_eager_one: the first step to 1e-5, the trajectory to 3e-2
    assert got["losses"][0] == pytest.approx(eager["losses"][0], rel=1e-5)
    assert np.allclose(got["losses"], eager["losses"], rtol=3e-2)
    for name, key in (("parameters", "params"), ("averages", "emas")):
        first_err = max(_rel_l2(a, b) for a, b in zip(got[key][0], eager[key][0]))
        last_err = max(_rel_l2(a, b) for a, b in zip(got[key][-1], eager[key][-1]))
        print(name, "relative L2 against eager: first step", first_err, "last step", last_err)
        assert first_err <= 1e-5 and last_err <= 3e-2, (name, first_err, last_err)


def test_graphed_replay_with_an_inf_input_is_skipped_and_the_schedule_moves_on(graphed_run):
    run = graphed_run
    m, opt, control, step = run["m"], run["opt"], run["control"], run["step"]
    x, y = _tiny_data()
    done = int(control.sched_step)
    skipped = int(control.skipped_steps)
    assert float(control.lr_factor) == FACTORS[done]
    bad = x.clone()
    bad[1, 3, 5, 7] = float("inf")
    before = _full_state(m, opt, control)
    graphs = [g[0] for e in step._graphs.values() for g in e["update"].values()]
    step(bad, y)
    torch.cuda.synchronize()
    assert _equal(_full_state(m, opt, control), before)                  # no parameter, moment, counter or average bit
    assert int(control.skipped_steps) == skipped + 1 and int(control.sched_step) == done + 1
    assert float(control.lr_factor) == FACTORS[done + 1]                 # the skipped step used its entry up
    # the step after is taken, at the factor after next: the library's plain Adam step at that rate -- a Python product --
    # on copies of the state, with the gradients and the clip factor the replay left, gives the replay's parameters bit
    # for bit; at the skipped entry's rate it does not
    from tramba_amd import hip
    ps = [p for p in m.parameters()]
    group = opt.param_groups[0]
    assert len(group["params"]) == len(ps) and not opt.param_groups[1]["params"]
    state = [[opt.state[p][k].clone() for p in ps] for k in ("exp_avg", "exp_avg_sq", "step")]
    start = _params(m)
    step(x, y)
    torch.cuda.synchronize()
    assert int(control.skipped_steps) == skipped + 1 and int(control.sched_step) == done + 2
    assert float(control.lr_factor) == FACTORS[done + 2]
    assert not _equal(_params(m), start)
    grads = [p.grad.detach().clone() for p in ps]
    results = {}
    for which in (done + 1, done):
        cp, cm, cv, cs = ([t.clone() for t in ts] for ts in (start, state[0], state[1], state[2]))
        hip.adam_step_raw(hip.pointer_array(cp), hip.pointer_array(grads), hip.pointer_array(cm), hip.pointer_array(cv),
                          hip.pointer_array(cs), (ctypes.c_int64 * len(cp))(*[t.numel() for t in cp]), len(cp),
                          group["lr"] * FACTORS[which], *group["betas"], group["eps"], group["weight_decay"],
                          gscale=control._fields["scale"], skip=control._fields["skip"])
        torch.cuda.synchronize()
        results[which] = cp
    assert _equal(_params(m), results[done + 1])
    assert not any(torch.equal(a, b) for a, b in zip(_params(m), results[done]))
    assert [g[0] for e in step._graphs.values() for g in e["update"].values()] == graphs      # still no re-capture
    assert [g["lr"] for g in opt.param_groups] == [BASE * 0.1, BASE]


def test_bf16_evaluation_with_the_averages_refreshes_the_derived_weights():
    from tramba_amd import train
    x, y = _tiny_data()
    m = _Tiny(torch.bfloat16).to(DEV).train()
    opt = train.get_opt(1e-2, m)
    control = train.StepControl(ema=train.WeightEMA(decay=0.9))
    for k in range(3):
        train.train_step(m, opt, torch.roll(x, k, 0), y, control=control)
    m.eval()
    ptrs = [p.data_ptr() for p in m.parameters()]
    live = _params(m)
    with torch.no_grad():
        out_live = m(x)[0].clone()
        with control.ema.applied(m):
            assert _equal(_params(m), control.ema.tensors())
            out_ema = m(x)[0].clone()
        out_back = m(x)[0].clone()
        fresh = _Tiny(torch.bfloat16).to(DEV).eval()
        fresh.load_state_dict(control.ema.model_state_dict(m))
        out_fresh = fresh(x)[0].clone()
    assert out_ema.dtype == torch.bfloat16
    assert torch.equal(out_ema, out_fresh)                               # the shadows and packs inside were the averages'
    assert not torch.equal(out_ema, out_live)
    assert torch.equal(out_back, out_live)                               # ... and the live weights' again afterwards
    assert _equal(_params(m), live) and [p.data_ptr() for p in m.parameters()] == ptrs
    m.train()                                                            # the next training step runs on the live weights
    before = _params(m)
    train.train_step(m, opt, x, y, control=control)
    assert not _equal(_params(m), before) and int(control.sched_step) == 4
