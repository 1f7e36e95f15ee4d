#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_scan_memory.py: every launch of that file (the cases, regimes and fp64 references of
tests/golden/scan_memory_cases.py) with, per case, output and regime, E32 (what a plain fp32 evaluation of the same formulas
loses against fp64, position by position and tile-wise), the bound the test holds the kernel to (8 x E32, plus the rounding
unit of a 16-bit output) and the kernel's measured error, on the max-relative and the RMS-relative measure.
usage: python scripts/measure_scan_memory_parity.py [--out profiles/scan_memory_parity.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import scan_memory_cases as smc  # noqa: E402  (the cases, references and bounds the tests use)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
RING, SEGMENT, LDS_DMA = 1, 2, 3


def forward_launches():
    """(case, regime, input dtype, form, a_log, forced W values) as tests/test_gpu_scan_memory.py runs them"""
    for dtype in (F32, BF16):
        for regime in ("slow", "undamped", "init"):
            yield "raster37", regime, dtype, RING, regime == "init", (0, 1, 2, 4) if regime != "init" else (0,)
            yield "raster37", regime, dtype, SEGMENT, False, (0,)
    for regime in ("slow", "undamped"):
        yield "helix37_wide", regime, BF16, SEGMENT, False, (0,)
        yield "helix37_d576", regime, BF16, LDS_DMA, False, (0,)
    for r in (8, 16, 32):
        for dtype in (BF16, F16):
            for regime in ("slow", "undamped", "init"):
                yield f"helix40_r{r}", regime, dtype, LDS_DMA, regime == "init", (0,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_scan_memory_parity.py needs a device"
    from tramba_amd import hip as H
    dev = torch.device("cuda")
    recs = []
    for name, regime, dtype, form, a_log, ws in forward_launches():
        c, ref, e = smc.fwd_e32(name, regime, dtype, a_log, segment=form == SEGMENT)
        for w in ws:
            for ys_dtype in ((F32,) if dtype == F32 else (F32, dtype)):
                ys = smc.run_scan(H, c, dev, form, ys_dtype, w)
                recs.append(smc.record(f"fwd {name} {regime} in={str(dtype)[6:]} form={form} W={w}", "ys", ys, ref["ys"], e["ys"], ys_dtype))
        if form != SEGMENT and name in ("raster37", "helix40_r8"):
            _, states = smc.run_scan(H, c, dev, form, dtype, states=True)
            recs.append(smc.record(f"fwd {name} {regime} in={str(dtype)[6:]} form={form}", "states", states, ref["states"], e["states"]))
    for name, (_, _, _, _, _, dtypes) in smc.BWD_CASES.items():
        for dtype in dtypes:
            for regime in ("slow", "init"):
                for a_log in (False, True):
                    recs += smc.bwd_records(H, dev, name, regime, dtype, a_log)
    for regime in ("slow", "undamped"):
        for n in (1, 4):
            for dtype in (F32, BF16):
                recs += smc.boundary_records(H, dev, regime, n, dtype)
    for r in recs:
        print(" ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()), flush=True)
    worst = max(r["err_max"] / r["bound_max"] for r in recs if r.get("out_dtype", "float32") == "float32")
    res = dict(device=torch.cuda.get_device_name(0), factor=smc.FACTOR, all_within_bounds=all(r["ok"] for r in recs),
               worst_fp32_error_over_bound=worst, records=recs)
    print(f"{len(recs)} records, all within bounds: {res['all_within_bounds']}, worst fp32 error / bound {worst:.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
