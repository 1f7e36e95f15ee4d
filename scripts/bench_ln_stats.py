#!/usr/bin/env python3
"""The model's LayerNorm-folded GEMM shapes (norm -> in_proj: N = 2C, norm2 -> fc1: N = 4C) at batch 4 and batch 1, timed in
the manner of scripts/bench_gemm_pc.py (hipGraph of 20 launches per form, forms replayed alternately, min of 3 rounds):

  today      tramba_linear_ln_cl under the rule: the block derives its rows' statistics in the K loop
  s13 s14    the row statistics SUPPLIED (tramba_linear_ln_rowstat_cl) on linear_dma_kernel, 2 / 3 stages
  s16 s17    supplied, on linear_pc_kernel, 3 / 4 stages
  s0         supplied, under the rule (ln_stat_rule, csrc/linear.hip)
  ws         linear_ws_kernel as it is (knob 19; derives its own statistics) where it can run

and, second table, what the slab costs its producer: the block-output GEMMs (out_proj: K = 2C, fc2: K = 4C, both + residual)
with and without the row-partial output.  Output: profiles/lnstats_forms.txt."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tramba_amd import hip
dev = torch.device("cuda")
STAGES = [(96, 128), (48, 256), (24, 512), (12, 1024)]          # (map side, channels) of Tramba-V at 384 x 384


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


def with_form(form, fn):
    def run():
        hip.tune_set(hip.TUNE_GEMM_TILE, form)
        try:
            return fn()
        finally:
            hip.tune_set(hip.TUNE_GEMM_TILE, 0)
    return run


def main():
    print("LayerNorm-folded GEMMs, us per launch")
    for batch in (4, 1):
        for side, c in STAGES:
            m = batch * side * side
            for n in (2 * c, 4 * c):
                k = c
                x = torch.randn(m, k, device=dev).bfloat16()
                w = (torch.randn(n, k, device=dev) * k ** -0.5).bfloat16()
                b = torch.randn(n, device=dev)
                cs = w.float().sum(dim=1).contiguous()
                x64 = x.float().view(m, k // 64, 64)
                slab = torch.stack((x64.sum(-1), (x64 * x64).sum(-1)), -1).contiguous()
                act = 2 if n == 4 * c else 0
                own = lambda: hip.linear_ln_cl(x, w, cs, b, 1e-5, None, act)
                sup = lambda: hip.linear_ln_cl(x, w, cs, b, 1e-5, None, act, rowstat=slab)
                cols = [("today", with_form(0, own))] + [(f"s{f}", with_form(f, sup)) for f in (13, 14, 16, 17, 0)]
                if k in (128, 256) and n % 128 == 0 and m >= 64:
                    cols.append(("ws", with_form(19, own)))
                us, ys = timed([fn for _, fn in cols])
                line = f"B={batch} M={m:6d} N={n:5d} K={k:5d} tiles {-(-m // 64) * -(-n // 64):5d} |"
                for (name, _), u, y in zip(cols, us, ys):
                    ok = float((y.float() - ys[0].float()).abs().max()) <= 0.07
                    line += f" {name} {u:5.1f}{'' if ok else ' DIFF'}"
                print(line, flush=True)
    print("producers (plain GEMM + residual), us per launch: without / with the row-partial output")
    for batch in (4, 1):
        for side, c in STAGES:
            m = batch * side * side
            for k in (2 * c, 4 * c):
                n = c
                x = torch.randn(m, k, device=dev).bfloat16()
                w = (torch.randn(n, k, device=dev) * k ** -0.5).bfloat16()
                b = torch.randn(n, device=dev)
                r = torch.randn(m, n, device=dev).bfloat16()
                us, ys = timed([lambda: hip.linear_cl(x, w, b, r, 0), lambda: hip.linear_cl(x, w, b, r, 0, rowstat=True)])
                note = "" if torch.equal(ys[0], ys[1]) else " DIFF"
                if not hasattr(ys[1], "_tramba_rowstat"):
                    note += "  (no slab: its consumer runs the weight-stationary form)"
                print(f"B={batch} M={m:6d} N={n:5d} K={k:5d} | {us[0]:5.1f} {us[1]:5.1f}{note}", flush=True)


if __name__ == "__main__":
    main()
