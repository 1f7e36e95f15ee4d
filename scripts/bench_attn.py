#!/usr/bin/env python3
"""Fused window / spatial-reduction attention (csrc/attention.hip) against the stock path it replaces, one process, one library.

default mode -> JSON (--out):
  - Tramba-S and Tramba-P, bf16, 384x384, batch 1 and 4, each captured as one hipGraph three ways: the fused path, the stock
    path (`SwinTransformerBlock._forward_stock` / `_PvtAttention._forward_stock` patched in here: no environment variable, no
    library knob), and the fused path again for the A/A spread.  The graphs are replayed alternately under HIP events, ROUNDS
    rounds of 20 replays.  `verdict_3x_rule`: a gain when mean(stock - fused) exceeds three times the standard deviation of
    fused - fused2 (the rule of scripts/ab_parent.py), a loss when mean(fused - stock) does.  `verdict` asks in addition that
    the difference exceed |mean(fused - fused2)|, the offset between two captures of the same code, which the standard
    deviation over rounds does not see: a difference below it is noise.
  - per stage shape: one encoder block captured fused and stock, timed the same way (what the `*_supported` predicates would
    have to exclude, were a shape to lose), and the attention entry alone (20 launches per graph).
--trace: one steady-state forward per (model, path) between marker launches (`col_sum_kernel`, which no inference path
  uses), to be run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_attn.py --trace`.
--summarize DIR --out FILE.csv: launches and kernel time per (model, path, kernel) of that trace.
"""
import argparse
import collections
import contextlib
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, REPLAYS = 12, 20
MODELS = (("Tramba-S", "Tramba-S-TSOD"), ("Tramba-P", "Tramba-P-TSOD"))
# (H = W, heads) of Swin-B's stages at 384x384 (hd 32, ws 12; the last stage is one window) and (N, M, heads) of PVTv2-b4's (hd 64)
SWIN_STAGES = ((96, 4), (48, 8), (24, 16), (12, 32))
PVT_STAGES = ((9216, 144, 1, 8), (2304, 144, 2, 4), (576, 144, 5, 2), (144, 144, 8, 1))


@contextlib.contextmanager
def stock_paths(on=True):
    from tramba_amd import encoders as E
    saved = E.SwinTransformerBlock.forward, E._PvtAttention.forward
    if on:
        E.SwinTransformerBlock.forward = E.SwinTransformerBlock._forward_stock
        E._PvtAttention.forward = E._PvtAttention._forward_stock
    try:
        yield
    finally:
        E.SwinTransformerBlock.forward, E._PvtAttention.forward = saved


def capture(fn, stock):
    with stock_paths(stock), torch.no_grad():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
    torch.cuda.synchronize()
    return g, out


def replay_ms(g, n=REPLAYS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def flat(out):
    return [out] if torch.is_tensor(out) else [t for o in out for t in flat(o)]


def aba(fn, rounds=ROUNDS, stock2=False):
    """fused / stock / fused2 graphs of fn, replayed alternately -> the row of numbers and the verdict by the 3 x rule"""
    graphs = {name: capture(fn, stock) for name, stock in (("fused", False), ("stock", True), ("fused2", False))}
    extra = {}
    if stock2:      # are two captures of the STOCK path bitwise equal? (what fused_equals_fused2 is to be read against)
        s2 = capture(fn, True)
        s2[0].replay()
        graphs["stock"][0].replay()
        torch.cuda.synchronize()
        extra["stock_equals_stock2"] = all(torch.equal(a, b) for a, b in zip(flat(graphs["stock"][1]), flat(s2[1])))
        del s2
    for g, _ in graphs.values():
        replay_ms(g, 3)
    t = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, (g, _) in graphs.items():
            t[name].append(replay_ms(g))
    gain = [s - f for s, f in zip(t["stock"], t["fused"])]
    aa = [f - f2 for f, f2 in zip(t["fused"], t["fused2"])]
    spread = statistics.pstdev(aa)
    offset = abs(statistics.mean(aa))       # two captures of the same code: where a capture's buffers land (cf. bench_loss.py)
    mean = statistics.mean(gain)
    bar = max(3 * spread, offset)
    outs = {name: [o.clone() for o in flat(out)] for name, (_, out) in graphs.items()}
    rel = max(float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
              for a, b in zip(outs["fused"], outs["stock"]))
    return dict(fused_ms=round(statistics.mean(t["fused"]), 4), stock_ms=round(statistics.mean(t["stock"]), 4),
                fused2_ms=round(statistics.mean(t["fused2"]), 4), mean_stock_minus_fused_ms=round(mean, 4),
                aa_spread_ms=round(spread, 4), capture_offset_ms=round(offset, 4),
                verdict_3x_rule="gain" if mean > 3 * spread else ("loss" if -mean > 3 * spread else "noise"),
                verdict="gain" if mean > bar else ("loss" if -mean > bar else "noise"),
                fused_equals_fused2=all(torch.equal(a, b) for a, b in zip(outs["fused"], outs["fused2"])),
                fused_vs_stock_rel_l2=rel, rounds=rounds, replays=REPLAYS, **extra)


def build(name):
    import tramba_amd as ta
    torch.manual_seed(1026)
    return ta.prepare_inference(ta.bulid_model_enc(name).cuda().eval(), torch.bfloat16)


def model_rows():
    rows = {}
    for tag, name in MODELS:
        m = build(name)
        for batch in (1, 4):
            x = torch.randn(batch, 3, 384, 384, generator=torch.Generator().manual_seed(batch)).cuda()
            rows[f"{tag}_b{batch}"] = aba(lambda: m(x), stock2=True)
            print(f"{tag}_b{batch}", json.dumps(rows[f"{tag}_b{batch}"]), flush=True)
        del m
        torch.cuda.empty_cache()
    return rows


def entry_us(fn, inner=20):
    g, _ = capture(lambda: [fn() for _ in range(inner)], False)
    replay_ms(g, 3)
    return round(min(replay_ms(g, 10) for _ in range(5)) / inner * 1e3, 2)


def stage_rows():
    from tramba_amd import encoders as E, hip
    rows = {}
    gen = torch.Generator().manual_seed(7)
    for batch in (1, 4):
        for side, heads in SWIN_STAGES:
            c = heads * 32
            shift = 6 if side > 12 else 0
            blk = E.SwinTransformerBlock(c, (side, side), heads, 12, shift, 4.0, 0.0).cuda().eval()
            x = torch.randn(batch, side * side, c, generator=gen).cuda().bfloat16()
            qkv = torch.randn(batch, side, side, 3 * c, generator=gen).cuda().bfloat16()
            table = blk.attn.relative_position_bias_table.detach().float()
            row = aba(lambda: blk(x), rounds=6)
            row["window_attention_cl_us"] = entry_us(lambda: hip.window_attention_cl(qkv, table, 12, shift, heads))
            rows[f"swin_{side}x{side}_h{heads}_b{batch}"] = row
            print(f"swin_{side}x{side}_h{heads}_b{batch}", json.dumps(row), flush=True)
        for n, mk, heads, sr in PVT_STAGES:
            c = heads * 64
            side = int(n ** 0.5)
            blk = E._PvtBlock(c, heads, 4, True, 0.0, sr, 1e-6).cuda().eval()
            x = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            q = torch.randn(batch, n, c, generator=gen).cuda().bfloat16()
            kv = torch.randn(batch, mk, 2 * c, generator=gen).cuda().bfloat16()
            row = aba(lambda: blk(x, side, side), rounds=6)
            row["kv_attention_cl_us"] = entry_us(lambda: hip.kv_attention_cl(q, kv, heads))
            rows[f"pvt_n{n}_m{mk}_h{heads}_b{batch}"] = row
            print(f"pvt_n{n}_m{mk}_h{heads}_b{batch}", json.dumps(row), flush=True)
    return rows


def trace():
    from tramba_amd import hip
    mark = torch.zeros(2, 8, device="cuda")
    for tag, name in MODELS:
        m = build(name)
        x = torch.randn(1, 3, 384, 384, generator=torch.Generator().manual_seed(1)).cuda()
        for stock in (False, True):
            with stock_paths(stock), torch.no_grad():
                for _ in range(2):
                    m(x)
                hip.slab_sum(mark)
                m(x)
                hip.slab_sum(mark)
            torch.cuda.synchronize()
        del m


def summarize(src, out):
    rows = []
    for f in glob.glob(src + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if "col_sum_kernel" in r["Kernel_Name"]]
    segments = [(tag, path) for tag, _ in MODELS for path in ("fused", "stock")]
    assert len(cuts) == 2 * len(segments), f"{len(cuts)} markers in the trace, expected {2 * len(segments)}"
    with open(out, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Model", "Path", "Name", "Calls", "TotalUs", "Library"])
        for k, (tag, path) in enumerate(segments):
            acc = collections.OrderedDict()
            for r in rows[cuts[2 * k] + 1:cuts[2 * k + 1]]:
                e = acc.setdefault(r["Kernel_Name"], [0, 0.0])
                e[0] += 1
                e[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            lib = lambda n: "tramba::" in n                                        # noqa: E731
            n_all, n_lib = sum(v[0] for v in acc.values()), sum(v[0] for kk, v in acc.items() if lib(kk))
            t_all = sum(v[1] for v in acc.values())
            w.writerow([tag, path, "ALL LAUNCHES OF ONE FORWARD", n_all, f"{t_all:.1f}", ""])
            w.writerow([tag, path, "LIBRARY LAUNCHES", n_lib, f"{sum(v[1] for kk, v in acc.items() if lib(kk)):.1f}", 1])
            w.writerow([tag, path, "LAUNCHES OUTSIDE THE LIBRARY", n_all - n_lib,
                        f"{sum(v[1] for kk, v in acc.items() if not lib(kk)):.1f}", 0])
            print(f"{tag} {path}: {n_all} launches ({n_lib} library, {n_all - n_lib} outside), kernel time {t_all / 1e3:.3f} ms")
            for kk, v in sorted(acc.items(), key=lambda kv: -kv[1][1]):
                w.writerow([tag, path, kk[:160], v[0], f"{v[1]:.1f}", int(lib(kk))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)
    assert torch.cuda.is_available(), "bench_attn.py measures the GPU path: it needs a device"
    if args.trace:
        return trace()
    res = dict(device=torch.cuda.get_device_name(0), what="bf16, 384x384; ms per forward of one hipGraph replay",
               models=model_rows(), stages=stage_rows())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
