#!/usr/bin/env python3
"""Kernel launches of ONE Tramba-S / -P training step with `encoders.set_library_training` on, by source: the to-do list of
what still runs outside the library.  Two traced runs that differ by one step, so that model construction, the
first step's lazy caches and the teardown cancel:

    rocprofv3 --kernel-trace --stats --output-format csv -d A -- python scripts/enc_train_launches.py run Tramba-P-TSOD 2
    rocprofv3 --kernel-trace --stats --output-format csv -d B -- python scripts/enc_train_launches.py run Tramba-P-TSOD 3
    python scripts/enc_train_launches.py diff A B [--out profiles/enc_train_launches_P.json]
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# first match wins
SOURCES = (("library", r"tramba::"),
           ("framework GEMM (rocBLAS / hipBLASLt)", r"Cijk_|rocblas|hipblaslt|gemm"),
           ("framework convolution (MIOpen)", r"miopen|MIOpen|Conv|conv|igemm|Im2|Col2|naive_"),
           ("framework element-wise / cast / copy", r"elementwise|vectorized|copy|Copy|fill|Fill|CatArray|cat_"),
           ("framework reduction", r"reduce|Reduce|sum|Sum"),
           ("framework random", r"random|philox|distribution|bernoulli"))


def run(name, steps):
    import torch
    import tramba_amd as ta
    from tramba_amd import encoders, train
    torch.manual_seed(0)
    m = ta.bulid_model_enc(name).cuda().train()
    m.compute_dtype = torch.bfloat16
    encoders.set_library_training(m)
    opt = train.get_opt(1e-4, m)
    x = torch.randn(1, 3, 384, 384).cuda()
    y = (torch.rand(1, 1, 384, 384) > 0.5).float().cuda()
    for _ in range(steps):
        train.train_step(m, opt, x, y)
    torch.cuda.synchronize()


def calls(folder):
    out = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
    assert out, f"no *kernel_stats.csv under {folder}"
    return out


def diff(a, b, out=None):
    ca, cb = calls(a), calls(b)
    per_step = {k: cb.get(k, 0) - ca.get(k, 0) for k in set(ca) | set(cb)}
    per_step = {k: v for k, v in per_step.items() if v}
    groups = {}
    for name, n in per_step.items():
        src = next((s for s, pat in SOURCES if re.search(pat, name)), "other")
        g = groups.setdefault(src, dict(launches=0, kernels={}))
        g["launches"] += n
        g["kernels"][name[:120]] = g["kernels"].get(name[:120], 0) + n
    total = sum(g["launches"] for g in groups.values())
    res = dict(launches_per_step=total, by_source={})
    for src, g in sorted(groups.items(), key=lambda kv: -kv[1]["launches"]):
        top = sorted(g["kernels"].items(), key=lambda kv: -kv[1])[:12]
        res["by_source"][src] = dict(launches=g["launches"], top=top)
        print(f"{src}: {g['launches']}")
        for k, n in top:
            print(f"    {n:6d}  {k}")
    print("total", total)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    else:
        diff(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--out" else None)
