#!/usr/bin/env python3
"""Dynamic loss scaling (train.LossScale) on Tramba-V 384x384, batch 8, graphed: what the scaler costs and
what fp16 buys.  Writes profiles/loss_scale_bench.json.

  python scripts/bench_loss_scale.py [rounds] [out.json]
      (a) cost: the controlled bf16 step with skip_nonfinite=True (A), the same with a scaler (B) and a second capture of B on
          a model of its own (B2), in one process, replayed alternately `rounds` times, 20 steps per timing, device events
          (as scripts/bench_accum.py).  The scaler adds one one-lane launch and a 4-byte read per optimizer step; B counts as
          "not slower" if mean(B - A) is at most three times the A/A spread, the standard deviation of B - B2.
      (b) gradients: for fp16 + LossScale(init=65536) and for bf16, cosine and norm ratio of every parameter gradient of
          Tramba-V against the fp32 library gradients of the same batch (stochastic depth off); and the skips and the scale
          reached over 12 eager fp16 steps from init=65536."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "loss_scale_bench.json")


def fresh(dtype, capturable=True, drop=True):
    import torch
    import tramba_amd as ta
    from tramba_amd import train
    torch.manual_seed(1026)
    m = ta.bulid_model(use_pretrain=False, img_size=384).cuda().train()
    if not drop:
        for mod in m.modules():
            if isinstance(mod, ta.DropPath):
                mod.drop_prob = 0.0
    m.compute_dtype = dtype
    return m, train.get_opt(1e-4, m, capturable=capturable)


def data(n):
    import torch
    x = torch.randn(n, 3, 384, 384, generator=torch.Generator().manual_seed(0)).cuda()
    y = (torch.rand(n, 1, 384, 384, generator=torch.Generator().manual_seed(1)) > 0.7).float().cuda()
    return x, y


def cost(rounds):
    import torch
    import tramba_amd as ta
    from tramba_amd import train
    x, y = data(8)
    steps = 20

    def build(scaler):
        m, opt = fresh(torch.bfloat16)
        control = train.StepControl(skip_nonfinite=True) if scaler is None else train.StepControl(loss_scale=scaler)
        step = ta.GraphedTrainStep(m, opt, control=control)
        step(x, y)
        return (lambda: step(x, y)), (m, opt, step, control)

    variants = {"A": build(None), "B": build(train.LossScale()), "B2": build(train.LossScale())}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for name, (run, _keep) in variants.items():
            run()
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                run()
            e.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(e) / steps)
    diff = [b - p for b, p in zip(t["B"], t["A"])]
    aa = [b - b2 for b, b2 in zip(t["B"], t["B2"])]
    spread = statistics.pstdev(aa)
    control = variants["B"][1][3]
    return {"what": "Tramba-V 384x384 bf16 batch 8, graphed controlled step: A = skip_nonfinite, B = the same with "
                    "LossScale(), B2 = a second capture of B", "rounds": rounds, "steps_per_timing": steps,
            "ms_per_step": {k: statistics.mean(v) for k, v in t.items()}, "ms_per_step_by_round": t,
            "mean_B_minus_A_ms": statistics.mean(diff), "mean_B_minus_B2_ms": statistics.mean(aa), "aa_spread_ms": spread,
            "B_not_slower_than_A_by_more_than_3_spreads": statistics.mean(diff) <= 3 * spread,
            "loss_scale_after": float(control.loss_scale), "skipped_steps": int(control.skipped_steps)}


def gradients():
    import torch
    from tramba_amd import train
    x, y = data(8)
    ref, _ = fresh(None, capturable=False, drop=False)
    train.tramba_loss(ref(x), y).backward()
    want = {n: p.grad.detach().double() for n, p in ref.named_parameters() if p.grad is not None}
    del ref
    out = {}
    for tag, dtype, scaler in (("fp16_scaled", torch.float16, train.LossScale()), ("bf16", torch.bfloat16, None)):
        m, opt = fresh(dtype, capturable=False, drop=False)
        control = train.StepControl(skip_nonfinite=True) if scaler is None else train.StepControl(loss_scale=scaler)
        train.train_step(m, opt, x, y, control=control)
        inv = 1.0 if scaler is None else 1.0 / scaler.init
        rows = {}
        for n, p in m.named_parameters():
            if p.grad is None or n not in want:
                continue
            g, w = p.grad.detach().double() * inv, want[n]
            rows[n] = {"cosine": float((g * w).sum() / (g.norm() * w.norm() + 1e-300)), "norm_ratio": float(g.norm() / (w.norm() + 1e-300))}
        cos, ratio = [r["cosine"] for r in rows.values()], [r["norm_ratio"] for r in rows.values()]
        out[tag] = {"skipped_first_step": int(control.skipped_steps), "tensors": len(rows), "min_cosine": min(cos),
                    "median_cosine": statistics.median(cos), "min_norm_ratio": min(ratio), "max_norm_ratio": max(ratio),
                    "worst_by_cosine": sorted(rows.items(), key=lambda kv: kv[1]["cosine"])[:8], "per_tensor": rows}
        del m, opt
    m, opt = fresh(torch.float16, capturable=False)
    control = train.StepControl(loss_scale=train.LossScale())
    trail = []
    for _ in range(12):
        train.train_step(m, opt, x, y, control=control)
        trail.append(float(control.loss_scale))
    out["fp16_run_from_65536"] = {"steps": 12, "skipped_steps": int(control.skipped_steps), "scale_after_each_step": trail}
    return out


def main():
    args = [a for a in sys.argv[1:]]
    rounds = max(12, int(args[0])) if args else 12
    out_path = args[1] if len(args) > 1 else OUT
    doc = {"cost": cost(rounds)}
    print(json.dumps({k: v for k, v in doc["cost"].items() if k != "ms_per_step_by_round"}, indent=1), flush=True)
    doc["gradients"] = gradients()
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "per_tensor"} for k, v in doc["gradients"].items()}, indent=1))
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
