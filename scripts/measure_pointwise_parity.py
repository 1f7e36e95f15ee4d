#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_pointwise.py: the host numbers of tests/golden/pointwise_cases.py (E32 of every documented
formula over the sweep, the factor by which every injected fault exceeds 8 x E32) and, from one run of that test file on the
device, the records its cases append (kernel, form, dtype, function, worst x, error, bound), the worst one per kernel, form,
function and output width.
usage: python scripts/measure_pointwise_parity.py [--out profiles/pointwise_parity.json]"""
import argparse
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import pointwise_cases as pc  # noqa: E402  (the sweep, references, emulations and bounds the tests use)


def _num(v, digits):
    """rounded for the file; None where not finite (standard JSON has no inf)"""
    return float(f"{v:.{digits}g}") if v == v and abs(v) != float("inf") else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_pointwise_parity.py needs a device"
    host = pc.host_profile()
    for name, v in host["e32"].items():
        print(f"E32 {name}: {v['e32']:.3e} at x = {v['worst_x']:.6g}")
    for name, f in host["faults"].items():
        print(f"fault {name}: {f['factor']} x the bound, non-finite: {f['nonfinite']}")
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_pointwise.py")])
    cases = sys.modules["test_gpu_pointwise"].RECORDS
    # one record per (kernel, form, function, fp32 or narrower output): the worst case of that group (pieces of the sweep, input
    # dtypes and the oracle / closed-form pair of one probe fall together), with the input dtypes it covers
    groups = {}
    for r in cases:
        key = (r["kernel"], r["form"], r["function"].replace(" closed form", ""), r["out_dtype"] if r["out_dtype"] == "float32" else "narrow")
        ratio = r["error"] / r["bound"] if r["bound"] else float(r["error"] > 0)
        g = groups.setdefault(key, dict(ratio=-1.0, dtypes=set(), ok=True, cases=0))
        g["dtypes"].add(r["dtype"])
        g["ok"] = g["ok"] and r["ok"]
        g["cases"] += 1
        if ratio > g["ratio"]:
            g.update(ratio=ratio, worst=r)
    recs = []
    for (kernel, form, function, _), g in sorted(groups.items()):
        w = g["worst"]
        recs.append(dict(kernel=kernel, form=form, dtype=",".join(sorted(g["dtypes"])), function=function, out_dtype=w["out_dtype"],
                         worst_x=_num(w["worst_x"], 7), error=_num(w["error"], 4), bound=_num(w["bound"], 4),
                         variant=w["variant"], cases=g["cases"], ok=g["ok"]))
    worst = {}
    for r in recs:
        key = f"{r['kernel']} | {r['function']} | {'fp32' if r['out_dtype'] == 'float32' else r['out_dtype'] if r['bound'] == 0 else '16-bit'} out"
        ratio = float("inf") if r["error"] is None else r["error"] / r["bound"] if r["bound"] else float(r["error"] > 0)
        if ratio >= worst.get(key, (-1.0,))[0]:
            worst[key] = (ratio, r["error"], r["bound"], r["form"], r["dtype"], r["worst_x"])
    for key in sorted(worst):
        ratio, e, b, form, dtype, x = worst[key]
        print(f"{key}: worst error / bound {ratio:.3f} ({e} / {b}) {form} {dtype} at x = {x}")
    ok = all(r["ok"] for r in cases) and rc == 0
    head = dict(device=torch.cuda.get_device_name(0), pytest_exit_code=int(rc), all_within_bounds=ok, cases=len(cases), host=host,
                note="`form` names the knob the test requested; the tests assert or state that the library honours it at that shape")
    print(f"{len(cases)} cases in {len(recs)} records, all within bounds: {ok}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                     # one record per line
            f.write(json.dumps(head, allow_nan=False)[:-1] + ', "records": [\n' + ",\n".join(json.dumps(r, allow_nan=False) for r in recs) + "\n]}\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
