#!/usr/bin/env python3
"""What the schedule record and the fused EMA cost and save, one process, one library -> JSON (--out, default
profiles/sched_ema_bench.json).  Nothing here is asserted.

  (a) optimizer: the parameter list of Tramba-V (384 x 384 build, random gradients), one optimizer step three ways, run
      alternately for ROUNDS rounds of STEPS steps under HIP events:
        fused     tramba_adam_step_sched with the averages (36 B per parameter, the launches of one Adam step)
        two_pass  tramba_adam_step, then torch._foreach_lerp_ over the same averages (28 + 12 B per parameter)
        adam      tramba_adam_step alone (28 B per parameter), for scale
  (b) the captured step (GraphedTrainStep) on the one-block model of tests/test_gpu_loss_scale.py at 2 x 32 x 24 x 24 in
      fp32 and on Tramba-V at batch 8 with bf16 activations (bench.py's training configuration): ms per step with a
      factor that differs at every step, with a constant factor, and the way the step had to be driven without the
      record -- the groups' lr written by hand before every step, which drops the graphs and captures again (warm-up
      steps, snapshot and restore included)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, STEPS = 6, 10


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def optimizer_rows(shapes):
    from tramba_amd import hip
    g = torch.Generator(device="cuda").manual_seed(1)
    ps = [torch.randn(s, device="cuda", generator=g) for s in shapes]
    gs = [torch.randn(s, device="cuda", generator=g) * 0.1 for s in shapes]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    es = [p.clone() for p in ps]
    steps = [torch.zeros((), device="cuda") for _ in ps]
    n = len(ps)
    arrays = [hip.pointer_array(t) for t in (ps, gs, ms, vs, steps)] + [(ctypes.c_int64 * n)(*[p.numel() for p in ps]), n]
    ema = hip.pointer_array(es)
    rec, _ = hip.step_sched_record("cuda", lr_factor=0.5, ema_weight=1e-3)
    hyper = (1e-4, 0.9, 0.999, 1e-8, 0.0)
    paths = {
        "fused": lambda: hip.adam_step_sched_raw(*arrays, *hyper, ema=ema, sched=rec),
        "two_pass": lambda: (hip.adam_step_raw(*arrays, *hyper), torch._foreach_lerp_(es, ps, 1e-3)),
        "adam": lambda: hip.adam_step_raw(*arrays, *hyper),
    }
    for fn in paths.values():
        fn()
        fn()
    t = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            t[k].append(timed(fn, STEPS))
    numel = sum(p.numel() for p in ps)
    bytes_per = {"fused": 36, "two_pass": 40, "adam": 28}
    rows = {"tensors": n, "parameters": numel, "rounds": ROUNDS, "steps_per_round": STEPS}
    for k in paths:
        ms_ = statistics.mean(t[k])
        rows[k] = {"ms": round(ms_, 4), "ms_min": round(min(t[k]), 4), "ms_max": round(max(t[k]), 4),
                   "bytes_per_parameter": bytes_per[k], "TB_per_s": round(numel * bytes_per[k] / ms_ / 1e9, 3)}
    rows["fused_over_two_pass"] = round(rows["fused"]["ms"] / rows["two_pass"]["ms"], 4)
    return rows


class Tiny(torch.nn.Module):
    """the one-block model of tests/test_gpu_loss_scale.py"""

    def __init__(self):
        super().__init__()
        import tramba_amd as ta
        torch.manual_seed(11)
        self.encoder = ta.MultiScaleDecoderBlock(hidden_dim=32, drop_path=0.0, channel_first=True)
        self.encoder_head = torch.nn.Parameter(torch.randn(32) * 0.2)
        self.encoder_bias = torch.nn.Parameter(torch.zeros(1))
        self.compute_dtype = None

    def forward(self, z):
        if self.training:
            from tramba_amd.modules import model_mask_pool
            model_mask_pool(self).begin_step()
        h = self.encoder(z)
        return [(h * self.encoder_head.view(1, -1, 1, 1)).sum(dim=1, keepdim=True) + self.encoder_bias.view(1, 1, 1, 1)]


def graphed_rows(make_model, x, y, replays, recaptures):
    import tramba_amd as ta
    from tramba_amd import train
    rows = {"replays": replays, "recaptured_steps": recaptures}
    tables = {"factor_differs_every_step": [1.0 / (1.0 + 0.01 * t) for t in range(4096)], "constant_factor": [0.5]}
    for tag, factors in tables.items():
        m = make_model()
        opt = train.get_opt(1e-4, m, capturable=True)
        control = train.StepControl(skip_nonfinite=True, schedule=train.LrSchedule(factors), ema=train.WeightEMA())
        step = ta.GraphedTrainStep(m, opt, control=control)
        t0 = time.perf_counter()
        step(x, y)
        torch.cuda.synchronize()
        rows[tag] = {"first_call_with_capture_ms": round((time.perf_counter() - t0) * 1e3, 1)}
        step(x, y)
        rows[tag]["ms_per_step"] = round(wall(lambda: step(x, y), replays), 4)
        rows[tag]["steps_taken"] = int(control.sched_step)
        rows[tag]["graphs_captured"] = sum(len(e["update"]) for e in step._graphs.values())
        del step, control, opt, m
    m = make_model()                                   # the record's absence: a rate written by hand drops the graphs
    opt = train.get_opt(1e-4, m, capturable=True)
    step = ta.GraphedTrainStep(m, opt, control=train.StepControl(skip_nonfinite=True))
    step(x, y)
    bases = [g["lr"] for g in opt.param_groups]
    k = [0]

    def by_hand():
        k[0] += 1
        for g, base in zip(opt.param_groups, bases):
            g["lr"] = base / (1.0 + 0.01 * k[0])
        step(x, y)
    rows["lr_written_by_hand_recaptures"] = {"ms_per_step": round(wall(by_hand, recaptures), 2)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_ema_bench.json"))
    ap.add_argument("--skip-model", action="store_true", help="leave the Tramba-V captured step out (the long part)")
    args = ap.parse_args()
    import tramba_amd as ta
    torch.manual_seed(1026)
    full = ta.bulid_model(use_pretrain=False, img_size=384).cuda().train()
    shapes = [tuple(p.shape) for p in full.parameters()]
    del full
    torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "timing": "HIP events (a), wall clock around synchronize (b)",
           "optimizer_tramba_v_parameter_list": optimizer_rows(shapes)}

    def dump():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    dump()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(2, 32, 24, 24, generator=g).cuda(), (torch.rand(2, 1, 24, 24, generator=g) > 0.5).float().cuda()
    out["graphed_step_one_block_2x32x24x24"] = graphed_rows(lambda: Tiny().cuda().train(), x, y, 50, 5)
    dump()
    if not args.skip_model:
        def tramba_v():
            torch.manual_seed(1026)
            m = ta.bulid_model(use_pretrain=False, img_size=384).cuda().train()
            m.compute_dtype = torch.bfloat16
            return m
        x = torch.randn(8, 3, 384, 384, generator=torch.Generator().manual_seed(100)).cuda()
        y = (torch.rand(8, 1, 384, 384, generator=torch.Generator().manual_seed(200)) > 0.7).float().cuda()
        out["graphed_step_tramba_v_batch8_bf16"] = graphed_rows(tramba_v, x, y, 10, 2)
        dump()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
