#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_resnet_train.py's block-level gradient parity check: a layer1-type and a layer2-type
bottleneck in .train() (the blocks and inputs of tests/golden/resnet_train_blocks.py), the gradients of the input and of
every block parameter with the library training switch (`encoders.set_library_training`) on and on the stock 16-bit path,
each as the relative L2 error to the fp32 stock gradients, over SEEDS seeds.  The margin the test allows the library path
is, per gradient tensor, the stock path's own seed-to-seed spread:
    m_t = (largest stock error / smallest stock error) - 1.
A tensor whose stock spread is not narrow (m_t >= 1) is listed under "left_out": the test skips it.
usage: python scripts/measure_resnet_train_parity.py [--seeds 16] [--out profiles/resnet_train_parity.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import resnet_train_blocks  # noqa: E402  (the blocks, inputs and errors the test uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_resnet_train_parity.py needs a device"
    res = dict(device=torch.cuda.get_device_name(0), seeds=args.seeds,
               error="relative L2 of a 16-bit bottleneck's gradients against the fp32 stock gradients")
    for kind in resnet_train_blocks.KINDS:
        per_seed = [resnet_train_blocks.block_errors(kind, seed) for seed in range(args.seeds)]
        names = list(per_seed[0])
        lib = {n: [e[n][0] for e in per_seed] for n in names}
        stock = {n: [e[n][1] for e in per_seed] for n in names}
        m = {n: max(stock[n]) / min(stock[n]) - 1.0 for n in names}
        res[kind] = dict(m=m, left_out=sorted(n for n in names if not m[n] < 1.0),
                         worst_library_over_stock={n: max(f / s for f, s in zip(lib[n], stock[n])) for n in names},
                         library=lib, stock=stock)
        for n in names:
            print(f"{kind} {n}: m {m[n]:.4f} worst library / stock {res[kind]['worst_library_over_stock'][n]:.4f} "
                  f"stock {min(stock[n]):.3e}..{max(stock[n]):.3e} library {min(lib[n]):.3e}..{max(lib[n]):.3e}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
