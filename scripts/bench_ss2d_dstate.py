"""The SS2D inference core -- x_proj + scan + merge / out_norm / GELU -- per d_state, fused channels-last path
(SS2D._core_fused_cl: one GEMM, hip.ss2d_scan_cl at N = 1 / hip.ss2d_scan_n_cl beyond, one merge kernel) against the plugin
path on the same module in the same process (SS2D._core_plugin_cl: NCHW copy, K-fold gather, two framework einsums, the
reference-layout scan, merge, LayerNorm + GELU).  bf16, N in {1, 2, 4, 8, 16}, four shape classes:
  helix96   B = 4, 96 x 96, D = 256, R = 8, K = 8        raster96  the same map, K = 4
  helix48   B = 4, 48 x 48, D = 512, R = 16, K = 8       batch1    B = 1, 96 x 96, D = 256, R = 8, K = 8
Protocol (scripts/bench_scan_dstate.py): one process, warm-up, HIP events around back-to-back calls; here the samples of the
two paths alternate, so that a drift of the machine lands on both.  Median and inter-quartile range per path; `verdict` is
"fused" only where the fused median plus the larger of the two inter-quartile ranges is still below the plugin median.
The parts of the fused path are timed the same way on their own: the x_proj GEMM, the scan's reduce launch and its replay
launch (knob TUNE_SCAN_N_PASS launches one of them alone), the merge kernel.
Writes profiles/ss2d_dstate_bench.json (or the path given as the first argument; the second names the commit where the tree
runs without its git metadata)."""
import json
import os
import socket
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tramba_amd as ta  # noqa: E402
from tramba_amd import hip, ops  # noqa: E402
from tramba_amd.modules import _f32  # noqa: E402

SHAPES = {          # name: (B, H, D, R, family)
    "helix96": (4, 96, 256, 8, "helix"),
    "raster96": (4, 96, 256, 8, "raster"),
    "helix48": (4, 48, 512, 16, "helix"),
    "batch1": (1, 96, 256, 8, "helix"),
}
DSTATES = (1, 2, 4, 8, 16)
SAMPLES, PER_SAMPLE, WARMUP = 15, 3, 3


def _sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(PER_SAMPLE):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / PER_SAMPLE * 1e3


def _stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), iqr_us=q[2] - q[0], samples=len(us))


def timed(*fns):
    """interleaved samples of several callables -> one statistics record each"""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(SAMPLES):
        for i, fn in enumerate(fns):
            us[i].append(_sample(fn))
    return [_stats(u) for u in us]


def module(d, r, fam, n, dev):
    torch.manual_seed(n)
    kw = dict(scan=ops.CrossScan_Line, merge=ops.CrossMerge_Line, k_group=8) if fam == "helix" else {}
    m = ta.SS2D(d_model=d // 2, d_state=n, ssm_ratio=2.0, dt_rank=r, channel_first=True, **kw)
    return m.to(dev, torch.bfloat16).eval()


def parts(m, x, n):
    """the launches of _core_fused_cl, one by one, on the module's own cached operands"""
    b, h, w, d = x.shape
    order = hip.scan_order(m.scan._tramba_family, h, w, x.device)
    xf = x.view(b, h * w, d)
    wp = m._padded_x_proj(x.dtype)
    dt_w, dt_b, a_neg, ds = m._scan_params()
    xdbl = hip.linear_cl(xf, wp, out_dtype=torch.float32)
    lw, lb = _f32(m.out_norm.weight), _f32(m.out_norm.bias)
    scan = (lambda: hip.ss2d_scan_cl(xf, xdbl, order, dt_w, dt_b, a_neg, ds, x.dtype)) if n == 1 else \
        (lambda: hip.ss2d_scan_n_cl(xf, xdbl, order, dt_w, dt_b, a_neg, ds, x.dtype))
    ys = scan()
    out = {}
    out["x_proj"], out["scan"], out["merge_norm_gelu"] = timed(
        lambda: hip.linear_cl(xf, wp, out_dtype=torch.float32), scan,
        lambda: hip.ss2d_merge_norm_cl(ys, order, lw, lb, m.out_norm.eps, hip.ACT_GELU, x.dtype))
    if n > 1:
        nt, nseg = hip.ss2d_scan_n_plan(b, h * w, d, m.k_group, n)
        out["plan"] = dict(tiles_per_segment=nt, segments=nseg)
        for name, knob in (("scan_reduce", 1), ("scan_replay", 2)):
            if nseg == 1 and knob == 1:
                continue
            try:
                hip.tune_set(hip.TUNE_SCAN_N_PASS, knob)
                out[name] = timed(scan)[0]
            finally:
                hip.tune_set(hip.TUNE_SCAN_N_PASS, 0)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ss2d_dstate_bench.json")
    commit = sys.argv[2] if len(sys.argv) > 2 else ""
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    dev = torch.device("cuda")
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), commit=commit or "unknown (no git metadata)",
               io="bfloat16", protocol=dict(samples=SAMPLES, calls_per_sample=PER_SAMPLE, warmup=WARMUP, interleaved=True),
               shapes={k: dict(B=v[0], H=v[1], W=v[1], D=v[2], R=v[3], family=v[4]) for k, v in SHAPES.items()}, cells={})
    for sname, (b, h, d, r, fam) in SHAPES.items():
        x = torch.randn(b, h, h, d, generator=torch.Generator().manual_seed(h + d)).to(dev, torch.bfloat16)
        for n in DSTATES:
            m = module(d, r, fam, n, dev)
            with torch.no_grad():
                assert m._fused_ok(x)
                fused, plugin = timed(lambda: m._core_fused_cl(x), lambda: m._core_plugin_cl(x))
                a, p = m._core_fused_cl(x).float(), m._core_plugin_cl(x).float()
                cell = dict(fused=fused, plugin=plugin, parts=parts(m, x, n),
                            max_abs_difference_of_the_two_outputs=float((a - p).abs().max()))
            spread = max(fused["iqr_us"], plugin["iqr_us"])
            cell["speedup"] = plugin["median_us"] / fused["median_us"]
            cell["verdict"] = "fused" if fused["median_us"] + spread < plugin["median_us"] else "plugin"
            res["cells"][f"{sname}/N={n}"] = cell
            hip.device_error()
            pr = cell["parts"]
            print(f"{sname:9s} N={n:2d} fused {fused['median_us']:9.1f} us (iqr {fused['iqr_us']:6.1f})  plugin "
                  f"{plugin['median_us']:9.1f} us (iqr {plugin['iqr_us']:6.1f})  x{cell['speedup']:.2f} -> {cell['verdict']};  x_proj "
                  f"{pr['x_proj']['median_us']:.1f}  scan {pr['scan']['median_us']:.1f}"
                  + (f" (reduce {pr['scan_reduce']['median_us']:.1f} + replay {pr['scan_replay']['median_us']:.1f})"
                     if "scan_reduce" in pr else "") + f"  merge {pr['merge_norm_gelu']['median_us']:.1f}", flush=True)
            del m
            torch.cuda.empty_cache()
    res["plugin_cells"] = sorted(k for k, v in res["cells"].items() if v["verdict"] == "plugin")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("cells where the plugin path is not beaten beyond the spread:", res["plugin_cells"] or "none")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
