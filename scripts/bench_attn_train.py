#!/usr/bin/env python3
"""Attention backward on the library (csrc/attention_bwd.hip, `encoders.set_fused_attention_training`) against the stock
autograd path it replaces, one process, one library -> JSON (--out, default profiles/attn_train_bench.json).

  - models: Tramba-S and Tramba-P, bf16 activations, 384x384, batch 1 and 4, .train(): forward + loss + backward as timed
    eager steps, three ways -- the flag on, the flag off (the parent's behaviour in the same build: the baseline), the flag on
    again for the A/A spread -- run alternately, ROUNDS rounds of STEPS steps under HIP events.
  - stages: one encoder block per stage shape, forward + backward, captured as one hipGraph per path and replayed
    alternately (what the `*_train_supported` predicates would have to exclude, were a shape to lose), and the backward
    entry alone (20 launches per graph).
  - `verdict_3x_rule`: a gain when mean(stock - fused) exceeds three times the standard deviation of fused - fused2, a loss
    when mean(fused - stock) does; `verdict` asks in addition that the difference exceed |mean(fused - fused2)|, the offset
    between two runs / captures of the same code (the protocol of scripts/bench_attn.py).
  - `peak_mib`: torch.cuda.max_memory_allocated over one step of each path, from a reset counter.
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
# (H = W, heads) of Swin-B's stages at 384x384 (hd 32, ws 12; the last stage is one window) and (N, M, heads, sr) of PVTv2-b4's
SWIN_STAGES = ((96, 4), (48, 8), (24, 16), (12, 32))
PVT_STAGES = ((9216, 144, 1, 8), (2304, 144, 2, 4), (576, 144, 5, 2), (144, 144, 8, 1))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def verdicts(t, n_key, n):
    gain = [s - f for s, f in zip(t["stock"], t["fused"])]
    aa = [f - f2 for f, f2 in zip(t["fused"], t["fused2"])]
    spread, offset, mean = statistics.pstdev(aa), abs(statistics.mean(aa)), statistics.mean(gain)
    bar = max(3 * spread, offset)
    row = dict(fused_ms=round(statistics.mean(t["fused"]), 4), stock_ms=round(statistics.mean(t["stock"]), 4),
               fused2_ms=round(statistics.mean(t["fused2"]), 4), mean_stock_minus_fused_ms=round(mean, 4),
               aa_spread_ms=round(spread, 4), aa_offset_ms=round(offset, 4),
               verdict_3x_rule="gain" if mean > 3 * spread else ("loss" if -mean > 3 * spread else "noise"),
               verdict="gain" if mean > bar else ("loss" if -mean > bar else "noise"), rounds=len(gain))
    row[n_key] = n
    return row


def peak_mib(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)


def model_rows():
    import tramba_amd as ta
    from tramba_amd import encoders, train
    rows = {}
    for tag, name in MODELS:
        torch.manual_seed(1026)
        m = ta.bulid_model_enc(name).cuda().train()
        m.compute_dtype = torch.bfloat16
        for batch in (1, 4):
            gen = torch.Generator().manual_seed(batch)
            x = torch.randn(batch, 3, 384, 384, generator=gen).cuda()
            y = (torch.rand(batch, 1, 384, 384, generator=gen) > 0.5).float().cuda()

            def step():
                m.zero_grad(set_to_none=True)
                train.tramba_loss(m(x), y).backward()

            def path(on):
                encoders.set_fused_attention_training(m, on)
                return step
            for on in (True, False):
                path(on)()
                path(on)()
            t = {"fused": [], "stock": [], "fused2": []}
            for _ in range(ROUNDS):
                for key, on in (("fused", True), ("stock", False), ("fused2", True)):
                    t[key].append(timed(path(on), STEPS))
            row = verdicts(t, "steps", STEPS)
            row["peak_mib"] = {"fused": peak_mib(path(True)), "stock": peak_mib(path(False))}
            rows[f"{tag}_b{batch}"] = row
            print(f"{tag}_b{batch}", json.dumps(row), flush=True)
        del m
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
    for key, on in (("fused", True), ("stock", False), ("fused2", True)):
        encoders.set_fused_attention_training(blk, on)
        graphs[key] = capture(step)
    t = {key: [] for key in graphs}
    for g in graphs.values():
        timed(g.replay, 3)
    for _ in range(ROUNDS):
        for key, g in graphs.items():
            t[key].append(timed(g.replay, REPLAYS))
    row = verdicts(t, "replays", REPLAYS)
    peaks = {}
    for key, on in (("fused", True), ("stock", False)):
        encoders.set_fused_attention_training(blk, on)
        peaks[key] = peak_mib(step)
    row["peak_mib"] = peaks
    return row


def entry_us(fn, inner=20):
    g = capture(lambda: [fn() for _ in range(inner)])
    timed(g.replay, 3)
    return round(min(timed(g.replay, 10) for _ in range(5)) / inner * 1e3, 2)


def stage_rows():
    from tramba_amd import encoders as E, hip
    rows = {}
    gen = torch.Generator().manual_seed(7)
    for batch in (1, 4):
        for side, heads in SWIN_STAGES:
            c = heads * 32
            shift = 6 if side > 12 else 0
            blk = E.SwinTransformerBlock(c, (side, side), heads, 12, shift, 4.0, 0.0).cuda().train()
            x = torch.randn(batch, side * side, c, generator=gen).cuda().bfloat16()
            qkv = torch.randn(batch, side, side, 3 * c, generator=gen).cuda().bfloat16()
            dy = torch.randn(batch, side, side, c, generator=gen).cuda().bfloat16()
            table = blk.attn.relative_position_bias_table.detach().float()
            row = block_row(blk, x, ())
            row["window_attention_bwd_cl_us"] = entry_us(lambda: hip.window_attention_bwd_cl(qkv, table, dy, 12, shift, heads))
            row["window_attention_cl_us"] = entry_us(lambda: hip.window_attention_cl(qkv, table, 12, shift, heads))
            rows[f"swin_{side}x{side}_h{heads}_b{batch}"] = row
            print(f"swin_{side}x{side}_h{heads}_b{batch}", json.dumps(row), flush=True)
        for n, mk, heads, sr in PVT_STAGES:
            c = heads * 64
            side = int(n ** 0.5)
            blk = E._PvtBlock(c, heads, 4, True, 0.0, sr, 1e-6).cuda().train()
            x = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            q = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            kv = torch.randn(batch, mk, 2 * c, generator=gen).cuda().bfloat16()
            dy = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            row = block_row(blk, x, (side, side))
            row["kv_attention_bwd_cl_us"] = entry_us(lambda: hip.kv_attention_bwd_cl(q, kv, dy, heads))
            row["kv_attention_cl_us"] = entry_us(lambda: hip.kv_attention_cl(q, kv, heads))
            rows[f"pvt_n{n}_m{mk}_h{heads}_b{batch}"] = row
            print(f"pvt_n{n}_m{mk}_h{heads}_b{batch}", json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_train_bench.json"))
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_train.py measures the GPU path: it needs a device"
    res = dict(device=torch.cuda.get_device_name(0),
               what="bf16, 384x384, forward + backward; models: ms per timed eager step; stages: ms per hipGraph replay of one "
                    "block's forward + backward; entries: us per launch",
               stages=stage_rows(), models={} if args.skip_models else model_rows())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
