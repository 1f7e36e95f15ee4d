"""Errors of the fused channels-last SS2D scan at d_state 3 and 16 (hip.ss2d_scan_n_cl) and of the plugin path's scan
(hip.selective_scan_fwd behind a framework einsum) on the same operands, against the fp64 recurrence, in the `slow` and
`undamped` regimes where the state outlives all 36 segments of a 48 x 48 helix map -- the records that
tests/test_gpu_ss2d_dstate.py::test_state_outlives_the_segments asserts on, kept as a file.
Writes profiles/ss2d_dstate_parity.json (or the path given as the first argument)."""
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ss2d_dstate_cases as sdc  # noqa: E402
import scan_memory_cases as smc  # noqa: E402
from tramba_amd import hip  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ss2d_dstate_parity.json")
    dev = torch.device("cuda")
    recs = []
    for regime in ("slow", "undamped"):
        for n in (3, 16):
            for dtype in (torch.float32, torch.bfloat16):
                recs += sdc.memory_records(hip, dev, regime, n, dtype)
    torch.cuda.synchronize()
    hip.device_error()
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               rule=f"fused: both relative measures within {smc.FACTOR:g} x E32; a 16-bit ys adds the elementwise rounding allowance "
                    "u = 2^-8 (bf16); the plugin path is recorded, not judged",
               shape=dict(family=sdc.MEMORY_SHAPE[0], H=sdc.MEMORY_SHAPE[1], D=sdc.MEMORY_SHAPE[2], R=sdc.MEMORY_SHAPE[3], B=1),
               all_fused_ok=all(r["ok"] for r in recs if r["path"] == "fused"), records=recs)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
