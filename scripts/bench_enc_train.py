#!/usr/bin/env python3
"""The encoders' training path on the library (`encoders.set_library_training`, csrc/patch_conv_bwd.hip) against the stock
autograd path it replaces, one process, one library -> JSON (--out, default profiles/enc_train_bench.json).  The protocol
of scripts/bench_attn_train.py:

  - models: Tramba-S and Tramba-P, bf16 activations, 384x384, batch 1 and 4, .train(): `train.train_step` as timed eager
    steps, three ways -- the switch on, the switch off (the parent's behaviour in the same build: the baseline), the switch
    on again for the A/A spread -- run alternately, ROUNDS rounds of STEPS steps under HIP events; then the same step as a
    `GraphedTrainStep` with the switch on (ms per replay).  With the switch off nothing is promised about capture: it is
    tried last, and its failure is recorded as such.
  - stages: one PVT block per stage shape, forward + backward, captured as one hipGraph per path and replayed alternately,
    and the two new entries alone (20 launches per graph).
  - `verdict_3x_rule`: a gain when mean(off - on) exceeds three times the standard deviation of on - on2, a loss when
    mean(on - off) does; `verdict` asks in addition that the difference exceed |mean(on - on2)|.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, STEPS, REPLAYS = 6, 5, 20
MODELS = (("Tramba-S", "Tramba-S-TSOD"), ("Tramba-P", "Tramba-P-TSOD"))
PVT_STAGES = ((9216, 1, 8, 8), (2304, 2, 4, 8), (576, 5, 2, 4), (144, 8, 1, 4))         # (N, heads, sr, mlp ratio) of PVTv2-b4


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def verdicts(t, n_key, n):
    gain = [s - f for s, f in zip(t["off"], t["on"])]
    aa = [f - f2 for f, f2 in zip(t["on"], t["on2"])]
    spread, offset, mean = statistics.pstdev(aa), abs(statistics.mean(aa)), statistics.mean(gain)
    bar = max(3 * spread, offset)
    row = dict(on_ms=round(statistics.mean(t["on"]), 4), off_ms=round(statistics.mean(t["off"]), 4),
               on2_ms=round(statistics.mean(t["on2"]), 4), mean_off_minus_on_ms=round(mean, 4),
               aa_spread_ms=round(spread, 4), aa_offset_ms=round(offset, 4),
               verdict_3x_rule="gain" if mean > 3 * spread else ("loss" if -mean > 3 * spread else "noise"),
               verdict="gain" if mean > bar else ("loss" if -mean > bar else "noise"), rounds=len(gain))
    row[n_key] = n
    return row


def model_rows(graphed):
    import tramba_amd as ta
    from tramba_amd import encoders, train
    rows = {}
    for tag, name in MODELS:
        for batch in (1, 4):
            torch.manual_seed(1026)
            m = ta.bulid_model_enc(name).cuda().train()
            m.compute_dtype = torch.bfloat16
            opt = train.get_opt(1e-4, m, capturable=True)
            gen = torch.Generator().manual_seed(batch)
            x = torch.randn(batch, 3, 384, 384, generator=gen).cuda()
            y = (torch.rand(batch, 1, 384, 384, generator=gen) > 0.5).float().cuda()

            def path(on):
                encoders.set_library_training(m, on)
                return lambda: train.train_step(m, opt, x, y)
            for on in (True, False):
                path(on)()
                path(on)()
            t = {"on": [], "off": [], "on2": []}
            for _ in range(ROUNDS):
                for key, on in (("on", True), ("off", False), ("on2", True)):
                    t[key].append(timed(path(on), STEPS))
            row = verdicts(t, "steps", STEPS)
            if graphed:
                for key, on in (("graphed_on_ms", True), ("graphed_off_ms", False)):
                    encoders.set_library_training(m, on)
                    try:
                        step = ta.GraphedTrainStep(m, opt)
                        step(x, y)
                        timed(lambda: step(x, y), 3)
                        row[key] = round(min(timed(lambda: step(x, y), 10) for _ in range(3)), 4)
                    except Exception as e:                         # (switch off: nothing is promised about capture)
                        row[key] = f"capture failed: {type(e).__name__}: {str(e)[:200]}"
                    step = None
            rows[f"{tag}_b{batch}"] = row
            print(f"{tag}_b{batch}", json.dumps(row), flush=True)
            del m, opt
            torch.cuda.empty_cache()
    return rows


def capture(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    torch.cuda.synchronize()
    return g


def block_row(blk, x, extra):
    from tramba_amd import encoders
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).cuda().to(x.dtype)
    xg = x.detach().requires_grad_()

    def step():
        blk.zero_grad(set_to_none=True)
        xg.grad = None
        blk(xg, *extra).backward(dy)
    graphs = {}
    for key, on in (("on", True), ("off", False), ("on2", True)):
        encoders.set_library_training(blk, on)
        graphs[key] = capture(step)
    t = {key: [] for key in graphs}
    for g in graphs.values():
        timed(g.replay, 3)
    for _ in range(ROUNDS):
        for key, g in graphs.items():
            t[key].append(timed(g.replay, REPLAYS))
    return verdicts(t, "replays", REPLAYS)


def entry_us(fn, inner=20):
    g = capture(lambda: [fn() for _ in range(inner)])
    timed(g.replay, 3)
    return round(min(timed(g.replay, 10) for _ in range(5)) / inner * 1e3, 2)


def stage_rows():
    from tramba_amd import encoders as E, hip
    rows = {}
    gen = torch.Generator().manual_seed(7)
    for batch in (1, 4):
        for n, heads, sr, ratio in PVT_STAGES:
            c = heads * 64
            side = int(n ** 0.5)
            blk = E._PvtBlock(c, heads, ratio, True, 0.0, sr, 1e-6).cuda().train()
            x = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            row = block_row(blk, x, (side, side))
            if sr > 1:
                xm = x.view(batch, side, side, c)
                wk = torch.randn(c, sr, sr, c, generator=gen).cuda().bfloat16()
                gy = torch.randn(batch, side // sr, side // sr, c, generator=gen).cuda().bfloat16()
                row["patch_conv_cl_us"] = entry_us(lambda: hip.patch_conv_cl(xm, wk, None))
                row["patch_conv_dgrad_cl_us"] = entry_us(lambda: hip.patch_conv_dgrad_cl(gy, wk, xm.shape))
                row["patch_conv_wgrad_cl_us"] = entry_us(lambda: hip.patch_conv_wgrad_cl(gy, xm, sr, want_bias=True))
                row["wgrad_split"] = hip.lib().tramba_patch_conv_wgrad_split(batch, side, side, c, c, sr)
            rows[f"pvt_n{n}_c{c}_sr{sr}_b{batch}"] = row
            print(f"pvt_n{n}_c{c}_sr{sr}_b{batch}", json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_train_bench.json"))
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--skip-graphed", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_enc_train.py measures the GPU path: it needs a device"
    res = dict(device=torch.cuda.get_device_name(0),
               what="bf16, 384x384; models: ms per timed eager train_step, and per GraphedTrainStep replay; stages: ms per "
                    "hipGraph replay of one PVT block's forward + backward; entries: us per launch",
               stages=stage_rows(), models={} if args.skip_models else model_rows(not args.skip_graphed))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
