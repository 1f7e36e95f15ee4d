"""The two backward forms of the reference-layout selective scan at the shape of bench_scan_dstate.py: (B, KD, L) =
(4, 1024, 9216), K = 4, bf16 in, N in {1, 4, 8, 16}.
  atomic         hip.selective_scan_bwd as it runs by default: zero-filling the (ncopy, B, K, N, L) dB / dC copies and the small
                 outputs, the kernel with its fp32 atomics, and the two sums over the copies;
  deterministic  hip.selective_scan_bwd(..., deterministic=True): the two small fills, the scan kernel that stores one partial
                 row per slab, and the sum pass -- both launches.
Protocol of bench_scan_dstate.py: one process, warm-up, HIP events around 5 back-to-back calls, 24 such samples per form, median
and spread (min, max, inter-quartile range); the samples of the two forms ALTERNATE, so that a drift of the clocks lands on both.
The workspace bytes of each form are recorded with the times.  Writes profiles/scan_det_bench.json (or the path given as the
first argument; the second names the commit where the tree runs without its git metadata)."""
import json
import os
import socket
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import hip  # noqa: E402

NB, KD, K, L = 4, 1024, 4, 9216
DSTATES = (1, 4, 8, 16)
SAMPLES, PER_SAMPLE, WARMUP = 24, 5, 5


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(PER_SAMPLE):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / PER_SAMPLE * 1e3


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), iqr_us=q[2] - q[0], samples=len(us))


def timed_alternating(forms):
    """{name: fn} -> {name: stats}; sample i of every form is taken before sample i + 1 of any"""
    for fn in forms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in forms}
    for _ in range(SAMPLES):
        for name, fn in forms.items():
            us[name].append(sample(fn))
    return {name: stats(v) for name, v in us.items()}


def case(n, dev):
    g = torch.Generator().manual_seed(n)
    r = lambda *s: torch.randn(*s, generator=g)
    u, delta = r(NB, KD, L).to(dev, torch.bfloat16), (0.5 * r(NB, KD, L)).to(dev, torch.bfloat16)
    A = -(torch.rand(KD, n, generator=g) + 0.5).to(dev)
    B, C = r(NB, K, n, L).to(dev, torch.bfloat16), r(NB, K, n, L).to(dev, torch.bfloat16)
    D, bias = torch.ones(KD, device=dev), torch.full((KD,), -3.0, device=dev)
    dout = r(NB, KD, L).to(dev)
    return u, delta, A, B, C, D, bias, dout


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scan_det_bench.json")
    dev = torch.device("cuda")
    commit = sys.argv[2] if len(sys.argv) > 2 else ""      # where the tree travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), commit=commit or "unknown (no git metadata)",
               shape=dict(B=NB, KD=KD, K=K, L=L, io="bfloat16"),
               protocol=dict(samples=SAMPLES, launches_per_sample=PER_SAMPLE, warmup=WARMUP, alternated=True), bwd={})
    for n in DSTATES:
        *args, dout = case(n, dev)
        _, ckpt = hip.selective_scan_fwd(*args, True, True, want_ckpt=True)
        t = timed_alternating({
            "atomic": lambda: hip.selective_scan_bwd(*args, dout, ckpt, True),
            "deterministic": lambda: hip.selective_scan_bwd(*args, dout, ckpt, True, deterministic=True)})
        hip.device_error()
        ncopy = hip.scan_bc_copies(KD, K, n)
        t["atomic"].update(ncopy=ncopy, workspace_bytes=2 * ncopy * NB * K * n * L * 4)
        t["deterministic"].update(workspace_bytes=hip.selective_scan_bwd_det_work(NB, KD, K, n, L, torch.bfloat16))
        # the two forms agree (dB: the output the forms differ in most)
        a = hip.selective_scan_bwd(*args, dout, ckpt, True)
        d = hip.selective_scan_bwd(*args, dout, ckpt, True, deterministic=True)
        rel = [float((x.double() - y.double()).norm() / y.double().norm()) for x, y in zip(d, a)]
        res["bwd"][n] = dict(t, deterministic_over_atomic=t["deterministic"]["median_us"] / t["atomic"]["median_us"],
                             rel_l2_deterministic_vs_atomic=max(rel))
        print(f"N={n:2d} atomic {t['atomic']['median_us']:9.1f} us (iqr {t['atomic']['iqr_us']:.1f}, {t['atomic']['workspace_bytes'] / 2**20:.1f} MiB)"
              f"  deterministic {t['deterministic']['median_us']:9.1f} us (iqr {t['deterministic']['iqr_us']:.1f}, "
              f"{t['deterministic']['workspace_bytes'] / 2**20:.1f} MiB)  rel L2 {max(rel):.1e}", flush=True)
        del args, dout, ckpt, a, d, t
        torch.cuda.empty_cache()
    res["deterministic_faster_at_every_n"] = all(v["deterministic_over_atomic"] < 1.0 for v in res["bwd"].values())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
