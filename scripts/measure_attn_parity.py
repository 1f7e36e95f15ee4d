#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_attn.py's block-level parity check: one bf16 Swin block and one bf16 PVT block (the
blocks and inputs of tests/golden/attn_blocks.py), fused attention against the stock path, each as the relative L2 error to the fp32
stock forward, over SEEDS seeds.  Both paths are 16-bit roundings of the same math and differ only in where P is rounded,
so the margin the test allows the fused path is the stock path's own seed-to-seed spread:
    m = (largest stock error / smallest stock error) - 1.
usage: python scripts/measure_attn_parity.py [--seeds 16] [--out profiles/attn_parity.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import attn_blocks  # noqa: E402  (the blocks, inputs and error the test uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_attn_parity.py needs a device"
    res = dict(device=torch.cuda.get_device_name(0), seeds=args.seeds, error="relative L2 against the fp32 stock forward")
    for kind in ("swin", "pvt"):
        pairs = [attn_blocks.block_errors(kind, seed) for seed in range(args.seeds)]
        fused, stock = [p[0] for p in pairs], [p[1] for p in pairs]
        res[kind] = dict(fused=fused, stock=stock, m=max(stock) / min(stock) - 1.0,
                         worst_fused_over_stock=max(f / s for f, s in pairs))
        print(kind, json.dumps(res[kind]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
