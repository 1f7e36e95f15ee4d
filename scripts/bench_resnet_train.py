#!/usr/bin/env python3
"""The Tramba-R training path on the library (`encoders.set_library_training`, csrc/batchnorm.hip, the backward entries of
csrc/resnet_conv.hip), one process, one library -> JSON (--out, default profiles/resnet_train_bench.json).  The protocol of
scripts/bench_enc_train.py, as far as a baseline exists:

  - models: Tramba-R, 384x384, batch 1 and 4, .train(): `train.train_step` as timed eager steps three ways, run alternately,
    ROUNDS rounds of STEPS steps under HIP events -- the switch on with bf16 activations, the baseline, the switch on again
    for the A/A spread -- then the switch-on step as a `GraphedTrainStep` (ms per replay).  The baseline is the stock step of
    the same checkout with the switch off.  With fp32 master weights the stock ResNet does not take bf16 activations at all
    (nn.Conv2d refuses the mixed dtypes), so the stock step that exists is the fp32 one: that is what "off" measures, eagerly.
  - blocks: one layer1 and one layer3 bottleneck (the non-downsampling form), forward + backward, eagerly and alternately:
    the library path (fp32 masters, bf16 activations) on / on again, and the stock block cast to bf16 as "off"; then the
    library path as one hipGraph (ms per replay).
  - entries: each new entry alone at the workload's shapes as a hipGraph of INNER launches: us per call, with the bytes or
    flops the call must move, computed from the shape.  No stock op is timed beside them: see DESIGN 22.
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

ROUNDS, STEPS, REPLAYS, INNER = 6, 5, 10, 10
BF = torch.bfloat16


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def verdicts(t, n):
    gain = [s - f for s, f in zip(t["off"], t["on"])]
    aa = [f - f2 for f, f2 in zip(t["on"], t["on2"])]
    spread, offset, mean = statistics.pstdev(aa), abs(statistics.mean(aa)), statistics.mean(gain)
    bar = max(3 * spread, offset)
    return dict(on_ms=round(statistics.mean(t["on"]), 4), off_ms=round(statistics.mean(t["off"]), 4),
                on2_ms=round(statistics.mean(t["on2"]), 4), mean_off_minus_on_ms=round(mean, 4),
                aa_spread_ms=round(spread, 4), aa_offset_ms=round(offset, 4),
                verdict_3x_rule="gain" if mean > 3 * spread else ("loss" if -mean > 3 * spread else "noise"),
                verdict="gain" if mean > bar else ("loss" if -mean > bar else "noise"), rounds=len(gain), replays=n)


def alternate(fns, n):
    t = {key: [] for key in fns}
    for fn in fns.values():
        timed(fn, 3)
    for _ in range(ROUNDS):
        for key, fn in fns.items():
            t[key].append(timed(fn, n))
    return verdicts(t, n)


def model_rows():
    import tramba_amd as ta
    from tramba_amd import encoders, train
    rows = {}
    for batch in (1, 4):
        gen = torch.Generator().manual_seed(batch)
        x = torch.randn(batch, 3, 384, 384, generator=gen).cuda()
        y = (torch.rand(batch, 1, 384, 384, generator=gen) > 0.5).float().cuda()
        fns, keep = {}, []
        for key, on in (("on", True), ("off", False), ("on2", True)):
            torch.manual_seed(1026)
            m = ta.bulid_model_enc("Tramba-R-TSOD").cuda().train()
            m.compute_dtype = BF if on else None
            encoders.set_library_training(m, on)
            opt = train.get_opt(1e-4, m, capturable=True)
            fns[key] = (lambda mm, oo: lambda: train.train_step(mm, oo, x, y))(m, opt)
            keep.append((m, opt))
        row = alternate(fns, STEPS)
        row["paths"] = dict(on="bf16 activations, switch on, eager steps", off="fp32 stock step, eager steps")
        m, opt = keep[0]
        step = ta.GraphedTrainStep(m, opt)
        step(x, y)
        timed(lambda: step(x, y), 3)
        row["graphed_on_ms"] = round(min(timed(lambda: step(x, y), REPLAYS) for _ in range(3)), 4)
        rows[f"Tramba-R_b{batch}"] = row
        print(f"Tramba-R_b{batch}", json.dumps(row), flush=True)
        del fns, keep, step, m, opt
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


def block_rows():
    from tramba_amd import encoders, models
    rows = {}
    gen = torch.Generator().manual_seed(7)
    for tag, planes, side in (("layer1", 64, 96), ("layer3", 256, 24)):
        for batch in (1, 4):
            x = torch.randn(batch, side, side, planes * 4, generator=gen).clamp_min(0).cuda().to(BF)
            dy = torch.randn(batch, side, side, planes * 4, generator=gen).cuda().to(BF)
            steps = {}
            for key, on in (("on", True), ("off", False), ("on2", True)):
                torch.manual_seed(3)
                blk = models.Bottleneck(planes * 4, planes).cuda().train()
                if on:
                    encoders.set_library_training(blk, True)
                else:
                    blk = blk.to(BF)
                xg = x.detach().requires_grad_()

                def step(blk=blk, xg=xg, on=on):
                    blk.zero_grad(set_to_none=True)
                    xg.grad = None
                    out = blk.forward_cl(xg) if on else blk(xg.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
                    out.backward(dy)
                steps[key] = step
            row = alternate(steps, REPLAYS)
            row["paths"] = dict(on="fp32 masters, bf16 activations, switch on, eager", off="the block cast to bf16, stock ops, eager")
            g = capture(steps["on"])
            timed(g.replay, 3)
            row["graphed_on_ms"] = round(min(timed(g.replay, REPLAYS) for _ in range(3)), 4)
            rows[f"{tag}_bottleneck_{planes * 4}_{side}x{side}_b{batch}"] = row
            print(f"{tag}_b{batch}", json.dumps(row), flush=True)
    return rows


def entry_us(fn):
    g = capture(lambda: [fn() for _ in range(INNER)])
    timed(g.replay, 3)
    return round(min(timed(g.replay, 10) for _ in range(5)) / INNER * 1e3, 2)


def entry_rows():
    from tramba_amd import hip
    rows = {}
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda().to(BF)

    def rate(row, key, amount, unit):
        row[f"{key}_{unit}"] = round(amount / (row[f"{key}_us"] * 1e-6) / (1e12 if unit == "tflops" else 1e9), 2)
    for batch in (1, 4):
        for side, c in ((96, 64), (96, 256), (48, 512), (24, 256), (24, 1024)):            # batch norms of layer1..3
            x, dy, res = rnd(batch, side, side, c), rnd(batch, side, side, c), rnd(batch, side, side, c)
            gamma, beta = torch.ones(c).cuda(), torch.zeros(c).cuda()
            rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
            mean, rstd = hip.bn_stats_cl(x, 1e-5, rm, rv, 0.1)
            y = hip.bn_act_cl(x, mean, rstd, gamma, beta, res, True)
            nb = 2 * x.numel()
            row = dict(bn_stats_us=entry_us(lambda: hip.bn_stats_cl(x, 1e-5, rm, rv, 0.1)),
                       bn_act_res_relu_us=entry_us(lambda: hip.bn_act_cl(x, mean, rstd, gamma, beta, res, True)),
                       bn_act_bwd_res_relu_us=entry_us(lambda: hip.bn_act_bwd_cl(dy, x, y, mean, rstd, gamma, True, want_dres=True)))
            rate(row, "bn_stats", 2 * nb, "gbs")                        # x read twice
            rate(row, "bn_act_res_relu", 3 * nb, "gbs")                 # x, residual read; y written
            rate(row, "bn_act_bwd_res_relu", 8 * nb, "gbs")             # dy, x, y read twice; dx, dres written
            rows[f"bn_{side}x{side}x{c}_b{batch}"] = row
            print(f"bn_{side}x{side}x{c}_b{batch}", json.dumps(row), flush=True)
        x = rnd(batch, 192, 192, 64).clamp_min(0)
        gy = rnd(batch, 96, 96, 64)
        row = dict(maxpool_us=entry_us(lambda: hip.maxpool3s2_cl(x)), maxpool_bwd_us=entry_us(lambda: hip.maxpool3s2_bwd_cl(gy, x)))
        rate(row, "maxpool", 2 * (x.numel() + gy.numel()), "gbs")
        rate(row, "maxpool_bwd", 2 * (2 * x.numel() + gy.numel()), "gbs")
        rows[f"maxpool_192x192x64_b{batch}"] = row
        print(f"maxpool_b{batch}", json.dumps(row), flush=True)
        # (H, Cin, Cout, k, s): layer1 conv1 / conv2 / conv3 / the next block's conv1, layer2 conv2 + downsample, layer3 conv1 / conv2 / conv3
        for side, cin, cout, k, s in ((96, 64, 64, 1, 1), (96, 64, 64, 3, 1), (96, 64, 256, 1, 1), (96, 256, 64, 1, 1),
                                      (96, 128, 128, 3, 2), (96, 256, 512, 1, 2), (24, 1024, 256, 1, 1), (24, 256, 256, 3, 1),
                                      (24, 256, 1024, 1, 1)):
            x = rnd(batch, side, side, cin)
            wk = (torch.randn(cout, k, k, cin, generator=gen) * (cin * k * k) ** -0.5).cuda().to(BF)
            wt = hip.conv_transposed_weight(wk)
            so = hip.conv_out_size(side, k, s)
            gy = rnd(batch, so, so, cout)
            flop = 2.0 * batch * so * so * cout * cin * k * k
            row = dict(conv_fwd_us=entry_us(lambda: hip.conv_affine_cl(x, wk, None, None, None, False, ksize=k, stride=s)),
                       conv_dgrad_us=entry_us(lambda: hip.conv_dgrad_cl(gy, wt, x.shape, s)),
                       conv_wgrad_us=entry_us(lambda: hip.conv_wgrad_cl(gy, x, k, s)),
                       wgrad_split=hip.lib().tramba_conv_wgrad_split(batch, side, side, cin, cout, k, s))
            for key in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
                rate(row, key, flop, "tflops")
            rows[f"conv_{side}x{side}_{cin}to{cout}_k{k}s{s}_b{batch}"] = row
            print(f"conv_{side}x{side}_{cin}to{cout}_k{k}s{s}_b{batch}", json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_train_bench.json"))
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resnet_train.py measures the GPU path: it needs a device"
    res = dict(device=torch.cuda.get_device_name(0),
               what="bf16 activations, 384x384; models: ms per eager train_step (off: the fp32 stock step, see the script) and per "
                    "GraphedTrainStep replay with the switch on; blocks: ms per eager forward + backward of one bottleneck (off: the "
                    "stock block cast to bf16) and per hipGraph replay with the switch on; entries: us per call inside a hipGraph "
                    "of 10, with the bandwidth / rate over the bytes / flops the shape requires",
               entries=entry_rows(), blocks=block_rows(), models={} if args.skip_models else model_rows())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
