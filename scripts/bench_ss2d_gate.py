"""The price of SS2D's z gate (disable_z=False) and the routing of the gated module: the SS2D op in bf16, inference and
forward + backward, per cell
  helix96   B = 4, 96 x 96, d_model 128 (Di 256), K = 8, N in {1, 16}      raster96  the same map, K = 4, N = 1
  helix48   B = 4, 48 x 48, d_model 256 (Di 512), K = 8, N = 1             batch1    B = 1 of helix96, N in {1, 16}
in three variants that alternate in one process (the protocol of scripts/bench_ss2d_dstate_train.py: warm-up, HIP events around
back-to-back calls, median and inter-quartile range of 15 samples):
  fused_gated     the module as it routes itself (gate in the merge kernel / the dual-store LayerNorm + tramba_gelu_gate_bwd_cl)
  plugin_gated    the same module with its fused predicates turned off: reference graph, the gate in framework ops
  fused_ungated   the disable_z=True module of the same shape: what the gate costs
`fused_gated` is sampled twice (A/A): the difference of the two medians is the spread a verdict has to clear, their mean what
is compared.  A cell where fused_gated loses to plugin_gated by more than three times that spread is listed under
"route_to_plugin".  The merge launch alone is timed with and without the gate on the module's own operands (by bytes the gate
adds one Di-wide read to a launch that reads K and writes one: +11 % at K = 8, +20 % at K = 4), and so is the extra in_proj
half.
Writes profiles/ss2d_gate_bench.json (or the path given as the first argument; the second names the commit where the tree runs
without its git metadata)."""
import contextlib
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
from tramba_amd import hip, ops  # noqa: E402
import bench_ss2d_dstate as base  # noqa: E402

CELLS = [("helix96", 1), ("helix96", 16), ("raster96", 1), ("helix48", 1), ("batch1", 1), ("batch1", 16)]
base.PER_SAMPLE = 2


def module(d, r, fam, n, gated, dev):
    torch.manual_seed(n)
    kw = dict(scan=ops.CrossScan_Line, merge=ops.CrossMerge_Line, k_group=8) if fam == "helix" else {}
    m = ta.SS2D(d_model=d // 2, d_state=n, ssm_ratio=2.0, dt_rank=r, channel_first=False, disable_z=not gated, **kw)
    return m.to(dev, torch.bfloat16)


@contextlib.contextmanager
def plugin_path(m, on):
    """the module with its three fused predicates answering no (instance attributes in front of the methods)"""
    names = ("_fused_ok", "_train_path_ok", "_train_fused_ok") if on else ()
    for nm in names:
        setattr(m, nm, lambda x: False)
    try:
        yield
    finally:
        for nm in names:
            delattr(m, nm)


def infer(m, x, plugin):
    def run():
        with torch.no_grad(), plugin_path(m, plugin):
            m._forward_cl(x)
    return run


def train(m, x, g, plugin):
    def run():
        xg = x.detach().requires_grad_()
        with ta.fused_dstate_training(True), plugin_path(m, plugin):
            m._forward_cl(xg).backward(g)
        m.zero_grad(set_to_none=True)
    return run


def verdict(cell):
    aa = abs(cell["fused_gated"]["median_us"] - cell["fused_gated_again"]["median_us"])
    fused = 0.5 * (cell["fused_gated"]["median_us"] + cell["fused_gated_again"]["median_us"])   # (neither sample is favoured)
    cell["fused_gated_mean_us"] = fused
    cell["aa_spread_us"] = aa
    cell["fused_over_plugin"] = cell["plugin_gated"]["median_us"] / fused
    cell["gate_price"] = fused / cell["fused_ungated"]["median_us"]
    cell["verdict"] = "plugin" if fused - cell["plugin_gated"]["median_us"] > 3 * aa else "fused"


def launches_alone(m, x):
    """the merge launch with and without the gate, and one half of the gated in_proj, on the module's own operands"""
    b, h, w, _ = x.shape
    d = m.d_inner
    order = hip.scan_order(m.scan._tramba_family, h, w, x.device)
    ys = torch.randn(b, m.k_group, h * w, d, generator=torch.Generator().manual_seed(1)).to(x.device, x.dtype)
    z = torch.randn(b, h * w, d, generator=torch.Generator().manual_seed(2)).to(x.device, x.dtype)
    lw, lb = hip._f32(m.out_norm.weight), hip._f32(m.out_norm.bias)
    wz = m.in_proj.weight.detach()[d:]
    out = dict(zip(("merge_ungated", "merge_gated", "in_proj_half"), base.timed(
        lambda: hip.ss2d_merge_norm_cl(ys, order, lw, lb, m.out_norm.eps, hip.ACT_GELU, x.dtype),
        lambda: hip.ss2d_merge_norm_gate_cl(ys, order, lw, lb, z, m.out_norm.eps, hip.ACT_GELU, x.dtype),
        lambda: hip.linear_cl(x, wz))))
    out["merge_gated_over_ungated"] = out["merge_gated"]["median_us"] / out["merge_ungated"]["median_us"]
    out["merge_bytes_gated_over_ungated"] = (m.k_group + 2) / (m.k_group + 1)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ss2d_gate_bench.json")
    commit = sys.argv[2] if len(sys.argv) > 2 else ""
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    dev = torch.device("cuda")
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), commit=commit or "unknown (no git metadata)",
               io="bfloat16", measured="SS2D._forward_cl: inference (no_grad) and forward + backward under autograd",
               protocol=dict(samples=base.SAMPLES, calls_per_sample=base.PER_SAMPLE, warmup=base.WARMUP, interleaved=True),
               cells={})
    for sname, n in CELLS:
        b, h, d, r, fam = base.SHAPES[sname]
        x = torch.randn(b, h, h, d // 2, generator=torch.Generator().manual_seed(h + d)).to(dev, torch.bfloat16)
        g = torch.randn(b, h, h, d // 2, generator=torch.Generator().manual_seed(h + d + 1)).to(dev, torch.bfloat16)
        mg, mu = module(d, r, fam, n, True, dev), module(d, r, fam, n, False, dev)
        cell = dict(shape=dict(B=b, H=h, W=h, d_model=d // 2, d_inner=d, R=r, family=fam, K=mg.k_group, N=n))
        names = ("fused_gated", "plugin_gated", "fused_ungated", "fused_gated_again")
        mg.eval(), mu.eval()
        inf = dict(zip(names, base.timed(infer(mg, x, False), infer(mg, x, True), infer(mu, x, False), infer(mg, x, False))))
        verdict(inf)
        inf["launches_alone"] = launches_alone(mg, x)
        mg.train(), mu.train()
        with ta.fused_dstate_training(True):
            assert mg._train_path_ok(x.detach().requires_grad_())
        trn = dict(zip(names, base.timed(train(mg, x, g, False), train(mg, x, g, True), train(mu, x, g, False),
                                         train(mg, x, g, False))))
        verdict(trn)
        cell["inference"], cell["training"] = inf, trn
        res["cells"][f"{sname}/N={n}"] = cell
        hip.device_error()
        for kind, c in (("inference", inf), ("training", trn)):
            print(f"{sname:9s} N={n:2d} {kind:9s} fused-gated {c['fused_gated']['median_us']:9.1f} us (A/A {c['aa_spread_us']:6.1f})  "
                  f"plugin-gated {c['plugin_gated']['median_us']:9.1f} us  fused-ungated {c['fused_ungated']['median_us']:9.1f} us  "
                  f"fused/plugin x{c['fused_over_plugin']:.2f}  gate price x{c['gate_price']:.3f} -> {c['verdict']}", flush=True)
        la = inf["launches_alone"]
        print(f"{'':12s} merge alone {la['merge_ungated']['median_us']:.1f} -> {la['merge_gated']['median_us']:.1f} us "
              f"(x{la['merge_gated_over_ungated']:.3f}, by bytes x{la['merge_bytes_gated_over_ungated']:.3f}); in_proj half "
              f"{la['in_proj_half']['median_us']:.1f} us", flush=True)
        del mg, mu
        torch.cuda.empty_cache()
    res["route_to_plugin"] = sorted(f"{k} {kind}" for k, v in res["cells"].items() for kind in ("inference", "training")
                                    if v[kind]["verdict"] == "plugin")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("cells routed back to the plugin path:", res["route_to_plugin"] or "none")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
