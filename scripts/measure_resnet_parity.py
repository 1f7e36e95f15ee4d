#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_resnet_conv.py's whole-model accuracy check: the bf16 Tramba-R model of
tests/golden/resnet_parity.py, library convolutions against the stock path, each as the relative L2 error to the fp32 forward
of the same weights, for the encoder's three features and the model's three outputs, over SEEDS input seeds and at 384 x 384
and 256 x 256.  Both paths are 16-bit roundings of the same math and differ in where they round, so the margin the test allows
the library path is the stock path's own seed-to-seed spread, per quantity:
    m = (largest stock error / smallest stock error) - 1.
usage: python scripts/measure_resnet_parity.py [--seeds 8] [--out profiles/resnet_parity.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import resnet_parity  # noqa: E402  (the model, inputs and error the test uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--sizes", default="384,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_resnet_parity.py needs a device"
    res = dict(device=torch.cuda.get_device_name(0), seeds=args.seeds,
               error="relative L2 against the fp32 stock forward of the same weights")
    for size in (int(s) for s in args.sizes.split(",")):
        m, ref = resnet_parity.models(size)
        per_seed = [resnet_parity.errors(m, ref, resnet_parity.image(seed, size)) for seed in range(args.seeds)]
        rows = {}
        for name in resnet_parity.NAMES:
            lib, stock = [e[name][0] for e in per_seed], [e[name][1] for e in per_seed]
            rows[name] = dict(library=lib, stock=stock, m=max(stock) / min(stock) - 1.0,
                              worst_library_over_stock=max(a / b for a, b in zip(lib, stock)))
            print(size, name, json.dumps(rows[name]), flush=True)
        res[str(size)] = rows
        del m, ref
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
