#!/usr/bin/env python3
"""Generate tests/golden/golden_loss.npz by loading the reference's utils/loss.py BY PATH (torch only, nothing stubbed) and
running its structure_loss and wbce in fp64, with autograd for the input gradients, on the closed-form cases of loss_cases.py.

    python tests/golden/make_golden_loss.py            # TRAMBA_REFERENCE=/root/reference

Run in the build container only; the fixture (numbers only) is what travels.  Per case and loss: `<loss>/<case>/value`,
`.../grad_sample` (every GRAD_STRIDE-th element of the flattened gradient), `.../grad_sum`, `.../grad_norm`."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_cases  # noqa: E402

REF = os.environ.get("TRAMBA_REFERENCE", "/root/reference")


def main():
    spec = importlib.util.spec_from_file_location("reference_utils_loss", os.path.join(REF, "utils", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name in loss_cases.CASES:
        pred, mask, weight = loss_cases.case(name)
        calls = {"structure": lambda p: ref.structure_loss(p, mask) if weight is None else ref.structure_loss(p, mask, weight)}
        if weight is None:
            calls["wbce"] = lambda p: ref.wbce(p, mask)
        for loss, fn in calls.items():
            p = pred.clone().requires_grad_()
            value = fn(p)
            value.backward()
            d = loss_cases.digest(p.grad)
            out[f"{loss}/{name}/value"] = np.float64(value.item())
            out[f"{loss}/{name}/grad_sample"] = d["sample"].numpy()
            out[f"{loss}/{name}/grad_sum"] = np.float64(d["sum"])
            out[f"{loss}/{name}/grad_norm"] = np.float64(d["norm"])
            print(f"{loss:9s} {name:9s} {value.item():.10f}")
    path = os.path.join(HERE, "golden_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
