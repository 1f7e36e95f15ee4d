"""Closed-form cases of the structure-loss / weighted-BCE fixtures (make_golden_loss.py writes them, the tests rebuild them):
every tensor is a function of the case name through synth.py, so the fixture holds results only."""
import numpy as np
import torch

import synth

GRAD_STRIDE = 11    # the fixture keeps every 11th gradient element (flattened) plus the gradient's sum and L2 norm


def _blob_label(tag, shape):
    """0/1 labels: a few smooth blobs per plane, thresholded"""
    b, c, h, w = shape
    rs = synth._rs("loss_label:" + tag)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros(shape)
    for i in range(b):
        for j in range(c):
            z = np.zeros((h, w))
            for _ in range(3):
                cy, cx = rs.uniform(0.1, 0.9) * h, rs.uniform(0.1, 0.9) * w
                sy, sx = rs.uniform(0.08, 0.3) * h, rs.uniform(0.08, 0.3) * w
                z += rs.uniform(0.5, 1.5) * np.exp(-((yy - cy) ** 2 / (2 * sy * sy) + (xx - cx) ** 2 / (2 * sx * sx)))
            out[i, j] = z > 0.6
    return torch.from_numpy(out)


# name: (shape, label kind, with a caller's weight)
CASES = {
    "blob": ((2, 1, 48, 48), "blob", False),
    "soft": ((2, 1, 48, 48), "soft", False),              # labels anywhere in [0, 1], as gt / 255 yields
    "zeros": ((1, 1, 40, 40), "zeros", False),
    "ones": ((1, 1, 40, 40), "ones", False),
    "rect": ((2, 1, 37, 45), "blob", False),
    "small": ((2, 1, 16, 16), "blob", False),             # smaller than the 31 window
    "channels": ((2, 3, 36, 40), "blob", False),
    "weight": ((2, 1, 40, 40), "blob", True),             # structure_loss(pred, mask, weight)
}


def case(name):
    """-> (pred, mask, weight or None), fp64 host tensors"""
    shape, kind, with_weight = CASES[name]
    pred = synth.synth_input(f"wloss_{name}_pred", shape, scale=3.0).double()
    if kind == "blob":
        mask = _blob_label(name, shape)
    elif kind == "soft":
        mask = torch.sigmoid(4.0 * synth.synth_input(f"wloss_{name}_mask", shape).double())
        mask = (mask * 255).round() / 255
    else:
        mask = torch.full(shape, 1.0 if kind == "ones" else 0.0, dtype=torch.float64)
    weight = torch.sigmoid(synth.synth_input(f"wloss_{name}_weight", shape).double()) if with_weight else None
    return pred, mask, weight


def digest(grad):
    g = grad.detach().double().reshape(-1)
    return {"sample": g[::GRAD_STRIDE].clone(), "sum": float(g.sum()), "norm": float(g.norm())}
