#!/usr/bin/env python3
"""The forward's launches that were still on register-staged GEMM forms or on a merge geometry sized for a larger map, hipGraph-timed
(20 launches per replay, forms interleaved, min of 3 rounds), at batch 4 and batch 1 (the two largest merges at batch 8 too):
  * the four 3x3 / stride-2 convolutions (stem conv 2, three downsamples) and the three two-source GEMM shapes (decoder
    concat_back_dim: bias; FreqSS2Dv6 gate: sigmoid gate), TRAMBA_TUNE_GEMM_TILE 18 (linear_tiled_kernel<.., CONV> /
    linear_lean_kernel) against the rule (linear_pc_kernel with the conv / two-source loaders);
  * merge + out_norm + GELU of the K = 4 maps at 96x96 / 48x48 / 24x24 and of the Helix K = 8 maps, streaming form at
    TRAMBA_TUNE_MERGE_PW 4 / 8 / 16 (K = 8: TRAMBA_TUNE_MERGE_FORM 2, the rule runs one wave per pixel there) and the rule.
Results must be bit-identical across forms (`DIFF` otherwise).
usage: python scripts/bench_stragglers.py [out.txt]   (profiles/stragglers_forms.txt)"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import hip
dev = torch.device("cuda")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stragglers_forms.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns):
    """every fn captured as a graph of 20 launches; replayed alternately, 3 rounds: min us per launch"""
    graphs, outs = [], []
    for fn in fns:
        for _ in range(3):
            y = fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                keep = fn()
        g.replay()
        torch.cuda.synchronize()
        graphs.append(g)
        outs.append(y)
    best = [1e9] * len(fns)
    for _ in range(3):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); g.replay(); e1.record(); torch.cuda.synchronize()
            best[i] = min(best[i], e0.elapsed_time(e1) / 40 * 1e3)
    return best, outs


def tuned(pairs, fn):
    def run():
        for knob, v in pairs:
            hip.tune_set(knob, v)
        try:
            return fn()
        finally:
            for knob, _ in pairs:
                hip.tune_set(knob, 0)
    return run


def ab(label, fn, forms, ref=0):
    us, ys = timed([tuned(pairs, fn) for _, pairs in forms])
    line = f"{label} |"
    for i, ((name, _), u, y) in enumerate(zip(forms, us, ys)):
        line += f"  {name} {u:6.1f}{'' if i < ref or torch.equal(y, ys[ref]) else ' DIFF'}"
    say(line)
    return us


GEMM_FORMS = [("knob18", [(hip.TUNE_GEMM_TILE, 18)]), ("rule", [])]
CONVS = [(192, 64, 128), (96, 128, 256), (48, 256, 512), (24, 512, 1024)]         # input side, Cin, Cout
TWO = [(24, 512, 512, 512), (48, 256, 256, 256), (96, 128, 128, 128)]             # map side, N, K1, K2
MERGES = [("raster", 96, 256), ("raster", 48, 512), ("window", 48, 512), ("raster", 24, 1024), ("helix", 96, 256), ("helix", 48, 512)]
tot = {}


def merges(batch, cases):
    say(f"--- batch {batch}: merge + out_norm + GELU, bf16 ys, us per launch (rule first)")
    for fam, h, d in cases:
        order = hip.scan_order(fam, h, h, dev)
        ys = torch.randn(batch, order.k, h * h, d, device=dev).bfloat16()
        lw, lb = torch.ones(d, device=dev), torch.zeros(d, device=dev)
        form = [(hip.TUNE_MERGE_FORM, 2)] if order.k > 4 else []
        forms = [("rule", [])] + [(f"pw{p}", form + [(hip.TUNE_MERGE_PW, p)]) for p in (4, 8, 16)]
        mb = (ys.numel() + batch * h * h * d) * 2 / 1e6
        # (K = 8: the rule is another kernel, one wave per pixel -- the streaming forms are compared among themselves)
        ab(f"merge {fam:8s} {h:2d}x{h:2d} D={d:4d} K={order.k} pixels {batch * h * h:6d} {mb:6.1f} MB",
           lambda: hip.ss2d_merge_norm_cl(ys, order, lw, lb, 1e-5, 2, torch.bfloat16), forms, ref=1 if order.k > 4 else 0)


for batch in (4, 1):
    say(f"--- batch {batch}: 3x3 / stride-2 convolutions as implicit GEMMs, us per launch")
    for h, cin, cout in CONVS:
        x = torch.randn(batch, h, h, cin, device=dev).bfloat16()
        w = (torch.randn(cout, 9 * cin, device=dev) * (9 * cin) ** -0.5).bfloat16()
        b = torch.randn(cout, device=dev)
        m = batch * (h // 2) ** 2
        us = ab(f"conv  M={m:6d} N={cout:5d} K={9 * cin:5d} tiles {-(-m // 64) * -(-cout // 64):5d}", lambda: hip.conv3x3s2_cl(x, w, b), GEMM_FORMS)
        for (name, _), u in zip(GEMM_FORMS, us):
            tot[("conv", batch, name)] = tot.get(("conv", batch, name), 0.0) + u
    say(f"--- batch {batch}: two-source GEMMs (bias / sigmoid gate), us per launch")
    for h, n, k1, k2 in TWO:
        m = batch * h * h
        x1 = torch.randn(m, k1, device=dev).bfloat16()
        x2 = torch.randn(m, k2, device=dev).bfloat16()
        w = (torch.randn(n, k1 + k2, device=dev) * (k1 + k2) ** -0.5).bfloat16()
        b = torch.randn(n, device=dev)
        r = torch.randn(m, n, device=dev).bfloat16()
        for kind, fn in (("bias", lambda: hip.linear2_cl(x1, x2, w, b)), ("gate", lambda: hip.linear2_cl(x1, x2, w, None, r, hip.ACT_SIGMOID_GATE))):
            us = ab(f"two-source {kind}  M={m:6d} N={n:5d} K={k1:4d}+{k2:4d} tiles {-(-m // 64) * -(-n // 64):5d}", fn, GEMM_FORMS)
            for (name, _), u in zip(GEMM_FORMS, us):
                tot[("two", batch, name)] = tot.get(("two", batch, name), 0.0) + u
    merges(batch, MERGES)
merges(8, MERGES[:2])      # where the largest maps stop gaining from fewer pixels per wave
for batch in (4, 1):
    say(f"batch {batch}: sum of the four convolutions, us: knob18 {tot[('conv', batch, 'knob18')]:.1f} rule {tot[('conv', batch, 'rule')]:.1f};  "
        f"of the six two-source GEMMs: knob18 {tot[('two', batch, 'knob18')]:.1f} rule {tot[('two', batch, 'rule')]:.1f}")
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
