#!/usr/bin/env python3
"""What the controlled step (train.StepControl) costs: 64 images as 8 micro-batches of 8 and ONE Adam step,
against eight plain graphed steps at batch 8 (Tramba-V 384x384, bf16 activations, stochastic depth on).

  python scripts/bench_accum.py [rounds] [out.json]
      In one process: (A) the plain GraphedTrainStep at batch 8, replayed 8 times per figure; (B) the controlled graphs
      (accumulate=8, clip_norm, skip_nonfinite) on 8 x 8 images; (B2) a second capture of B on a model of its own.  The three
      are timed alternately, `rounds` times (>= 12), 20 optimizer steps of B (160 replays of A) per timing, device events.
      The A/A spread is the standard deviation over the rounds of B - B2; B counts as "not slower" if mean(B - A) is at
      most three times that (the rule of scripts/ab_parent.py).  Peak memory: the device memory each variant adds.
  python scripts/bench_accum.py --kernels
      A few EAGER controlled steps and nothing else, to be run under `rocprofv3 --kernel-trace --stats`.
  python scripts/bench_accum.py --summarize kernel_stats.csv PARAMETERS [out.json]
      (PARAMETERS: the count --kernels printed.)  Time of grad_accumulate_kernel, grad_norm_parts_kernel and adam_kernel in that trace against their algorithmic bytes
      (12 B per parameter and accumulate pass, 8 B on a step's first; 4 B; 28 B) and the HBM peak of 8 TB/s; merged into
      out.json under "kernels"."""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "accum_bench.json")
HBM_PEAK_TBS = 8.0
KERNEL_STEPS, KERNEL_MICRO = 6, 2          # what --kernels runs (and --summarize assumes)


def fresh(capturable=True):
    import torch
    import tramba_amd as ta
    from tramba_amd import train
    torch.manual_seed(1026)
    m = ta.bulid_model(use_pretrain=False, img_size=384).cuda().train()
    m.compute_dtype = torch.bfloat16
    return m, train.get_opt(1e-4, m, capturable=capturable)


def data(n):
    import torch
    x = torch.randn(n, 3, 384, 384, generator=torch.Generator().manual_seed(0)).cuda()
    y = (torch.rand(n, 1, 384, 384, generator=torch.Generator().manual_seed(1)) > 0.7).float().cuda()
    return x, y


def merge(path, update):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(update)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def bench(rounds, out_path):
    import torch
    import tramba_amd as ta
    from tramba_amd import train
    micro, steps = 8, 20
    x, y = data(8 * micro)
    xs, ys = list(x.chunk(micro)), list(y.chunk(micro))
    variants, memory = {}, {}

    def added(build):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_reserved()
        keep = build()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return keep, (torch.cuda.memory_reserved() - before) / 2 ** 20

    def plain():
        m, opt = fresh()
        step = ta.GraphedTrainStep(m, opt)
        step(xs[0], ys[0])

        def run():
            for a, b in zip(xs, ys):
                step(a, b)
        return run, (m, opt, step)

    def controlled():
        m, opt = fresh()
        control = train.StepControl(accumulate=micro, clip_norm=1.0, skip_nonfinite=True)
        step = ta.GraphedTrainStep(m, opt, control=control)
        step(xs, ys)
        return (lambda: step(xs, ys)), (m, opt, step, control)

    for name, build in (("A", plain), ("B", controlled), ("B2", controlled)):
        variants[name], memory[name] = added(build)
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
    cost = [b - p for b, p in zip(t["B"], t["A"])]
    aa = [b - b2 for b, b2 in zip(t["B"], t["B2"])]
    spread = statistics.pstdev(aa)
    control = variants["B"][1][3]
    res = {
        "what": "Tramba-V 384x384 bf16, 64 images: A = 8 plain graphed steps at batch 8 (8 Adam steps), B = one controlled step "
                "of 8 micro-batches of 8 (one Adam step, clip_norm 1.0, skip_nonfinite), B2 = a second capture of B",
        "rounds": rounds, "optimizer_steps_of_B_per_timing": steps,
        "ms_per_64_images": {k: statistics.mean(v) for k, v in t.items()},
        "ms_per_64_images_by_round": t,
        "aa_spread_ms": spread, "mean_B_minus_B2_ms": statistics.mean(aa), "mean_B_minus_A_ms": statistics.mean(cost),
        "B_not_slower_than_A_by_more_than_3_spreads": statistics.mean(cost) <= 3 * spread,
        "device_memory_added_mib": memory,
        "grad_norm_last_step": float(control.grad_norm), "skipped_steps": int(control.skipped_steps),
    }
    print(json.dumps({k: v for k, v in res.items() if k != "ms_per_64_images_by_round"}, indent=1))
    merge(out_path, {"timing": res})


def kernels():
    import torch
    from tramba_amd import train
    m, opt = fresh(capturable=False)
    x, y = data(8 * KERNEL_MICRO)
    control = train.StepControl(accumulate=KERNEL_MICRO, clip_norm=1.0, skip_nonfinite=True)
    for _ in range(KERNEL_STEPS):
        train.train_step(m, opt, x, y, control=control)
    torch.cuda.synchronize()
    n = sum(p.numel() for p in m.parameters() if p.grad is not None)
    print(json.dumps({"parameters_with_a_gradient": n, "steps": KERNEL_STEPS, "micro_batches": KERNEL_MICRO,
                      "grad_norm": float(control.grad_norm)}))


def summarize(stats_csv, out_path, nparams):
    total = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for key in ("grad_accumulate_kernel", "grad_norm_parts_kernel", "grad_norm_finish_kernel", "adam_kernel"):
                if key in row["Name"]:
                    calls, ns = total.get(key, (0, 0))
                    total[key] = (calls + int(row["Calls"]), ns + int(row["TotalDurationNs"]))
    per_step = {"grad_accumulate_kernel": 8 + 12 * (KERNEL_MICRO - 1), "grad_norm_parts_kernel": 4, "adam_kernel": 28}
    res = {"parameters": nparams, "steps": KERNEL_STEPS, "micro_batches_per_step": KERNEL_MICRO, "hbm_peak_tbs": HBM_PEAK_TBS}
    for key, (calls, ns) in total.items():
        ent = {"calls": calls, "ms_per_optimizer_step": ns / KERNEL_STEPS / 1e6}
        if key in per_step:
            ent["algorithmic_bytes_per_parameter_and_step"] = per_step[key]
            ent["tb_per_s"] = per_step[key] * nparams * KERNEL_STEPS / ns / 1e3
            ent["fraction_of_hbm_peak"] = ent["tb_per_s"] / HBM_PEAK_TBS
        res[key] = ent
    if "adam_kernel" in res:
        floor = res["adam_kernel"]["fraction_of_hbm_peak"] - 0.05
        res["bound_fraction_of_hbm_peak"] = floor
        res["bound_met"] = {k: res[k]["fraction_of_hbm_peak"] >= floor for k in ("grad_accumulate_kernel", "grad_norm_parts_kernel")
                            if k in res}
    print(json.dumps(res, indent=1))
    merge(out_path, {"kernels": res})


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--kernels":
        kernels()
    elif args and args[0] == "--summarize":
        summarize(args[1], args[3] if len(args) > 3 else OUT, int(args[2]))
    else:
        bench(int(args[0]) if args else 12, args[1] if len(args) > 1 else OUT)
