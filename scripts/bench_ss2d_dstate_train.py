"""Forward + backward of the SS2D op under autograd per d_state: the fused channels-last training path
(tramba_amd.fused_dstate_training(True): SS2D._forward_train_cl on _SS2DInnerCL, hip.ss2d_scan_n_cl and the state-looped scan
backward) against the plugin path on the same module in the same process -- as it runs by default (fp32 atomics in the scan
backward) and under deterministic_scan(True).  bf16, N in {2, 4, 8, 16}, the shape classes of scripts/bench_ss2d_dstate.py:
  helix96   B = 4, 96 x 96, D = 256, R = 8, K = 8        raster96  the same map, K = 4
  helix48   B = 4, 48 x 48, D = 512, R = 16, K = 8       batch1    B = 1, 96 x 96, D = 256, R = 8, K = 8
Protocol of that script: one process, warm-up, HIP events around back-to-back calls, the samples of the three paths
alternating; median and inter-quartile range of 15 samples.  `verdict` is "fused" only where the fused median plus the largest
inter-quartile range is still below the FASTER of the two plugin medians.  The scan-backward launches (hip.ss2d_scan_bwd_cl on
the module's own operands) are timed the same way on their own, and torch.cuda.max_memory_allocated of one forward + backward
is recorded per path.
Writes profiles/ss2d_dstate_train_bench.json (or the path given as the first argument; the second names the commit where the
tree runs without its git metadata)."""
import json
import os
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tramba_amd as ta  # noqa: E402
from tramba_amd import hip  # noqa: E402
import bench_ss2d_dstate as base  # noqa: E402

SHAPES = base.SHAPES
DSTATES = (2, 4, 8, 16)
base.PER_SAMPLE = 2


def step(m, x, g, fused, det):
    def run():
        xg = x.detach().requires_grad_()
        with ta.fused_dstate_training(fused), ta.deterministic_scan(det):
            y = m._forward_cl(xg)
            y.backward(g)
        m.zero_grad(set_to_none=True)
    return run


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def scan_bwd_alone(m, x, n):
    b, h, w, _ = x.shape
    d = m.d_inner
    order = hip.scan_order(m.scan._tramba_family, h, w, x.device)
    xs = torch.randn(b, h * w, d, generator=torch.Generator().manual_seed(1)).to(x.device, x.dtype)
    xdbl = hip.linear_cl(xs, m._padded_x_proj(x.dtype), out_dtype=torch.float32)
    dt_w, dt_b, a_neg, ds = m._scan_params()
    gym = torch.randn(b, h * w, d, generator=torch.Generator().manual_seed(2)).to(x.device, x.dtype)
    rec = base.timed(lambda: hip.ss2d_scan_bwd_cl(xs, xdbl, order, dt_w, dt_b, a_neg, ds, gym, bc_partials=True))[0]
    nt, nseg = hip.ss2d_scan_n_bwd_plan(b, h * w, d, m.k_group, n)
    rec["plan"] = dict(tiles_per_segment=nt, segments=nseg)
    rec["workspace_bytes"] = int(hip.lib().tramba_ss2d_scan_n_bwd_workspace(b, h * w, d, m.k_group, n, hip.dt(xs)))
    return rec


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ss2d_dstate_train_bench.json")
    commit = sys.argv[2] if len(sys.argv) > 2 else ""
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    dev = torch.device("cuda")
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), commit=commit or "unknown (no git metadata)",
               io="bfloat16", measured="forward + backward of SS2D._forward_cl under autograd",
               protocol=dict(samples=base.SAMPLES, calls_per_sample=base.PER_SAMPLE, warmup=base.WARMUP, interleaved=True),
               shapes={k: dict(B=v[0], H=v[1], W=v[1], D=v[2], R=v[3], family=v[4]) for k, v in SHAPES.items()}, cells={})
    for sname, (b, h, d, r, fam) in SHAPES.items():
        x = torch.randn(b, h, h, d // 2, generator=torch.Generator().manual_seed(h + d)).to(dev, torch.bfloat16)
        g = torch.randn(b, h, h, d // 2, generator=torch.Generator().manual_seed(h + d + 1)).to(dev, torch.bfloat16)
        for n in DSTATES:
            m = base.module(d, r, fam, n, dev).train()
            with ta.fused_dstate_training(True):
                assert m._train_fused_n_ok(x)
            runs = dict(fused=step(m, x, g, True, False), plugin=step(m, x, g, False, False),
                        plugin_deterministic=step(m, x, g, False, True))
            cell = dict(zip(runs, base.timed(*runs.values())))
            for name, fn in runs.items():
                cell[name]["peak_bytes"] = int(peak(fn))
            cell["scan_backward_alone"] = scan_bwd_alone(m, x, n)
            best = min(cell["plugin"]["median_us"], cell["plugin_deterministic"]["median_us"])
            spread = max(cell[k_]["iqr_us"] for k_ in runs)
            cell["speedup_over_the_faster_plugin_form"] = best / cell["fused"]["median_us"]
            cell["verdict"] = "fused" if cell["fused"]["median_us"] + spread < best else "plugin"
            res["cells"][f"{sname}/N={n}"] = cell
            hip.device_error()
            print(f"{sname:9s} N={n:2d} fused {cell['fused']['median_us']:9.1f} us (iqr {cell['fused']['iqr_us']:6.1f}, peak "
                  f"{cell['fused']['peak_bytes'] >> 20} MiB)  plugin {cell['plugin']['median_us']:9.1f} us (iqr "
                  f"{cell['plugin']['iqr_us']:6.1f}, peak {cell['plugin']['peak_bytes'] >> 20} MiB)  deterministic "
                  f"{cell['plugin_deterministic']['median_us']:9.1f} us  x{cell['speedup_over_the_faster_plugin_form']:.2f} -> "
                  f"{cell['verdict']};  scan backward alone {cell['scan_backward_alone']['median_us']:.1f} us "
                  f"{cell['scan_backward_alone']['plan']}", flush=True)
            del m, runs
            torch.cuda.empty_cache()
    res["plugin_cells"] = sorted(k for k, v in res["cells"].items() if v["verdict"] == "plugin")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("cells where the faster plugin form is not beaten beyond the spread:", res["plugin_cells"] or "none")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
