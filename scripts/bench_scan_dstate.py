"""selective_scan_fwd / _bwd per d_state at the shape of `roofline_boundary`: (B, KD, L) = (4, 1024, 9216), K = 4, bf16 in, fp32
out, N in {1, 2, 4, 8, 16}.  Protocol of bench_boundary.py: one process, warm-up, HIP events around back-to-back launches;
here 24 samples of 5 launches each per (direction, N), median and spread (min, max, inter-quartile range).  What the
state-looped kernels (N = 8, 16) are measured against is the N = 4 instantiation in the same process: the targets are
time(16) <= 4 x time(4) and time(8) <= 2 x time(4), i.e. no worse per state, with 10 % slack for the spread of short launches.
The backward is timed as hip.selective_scan_bwd runs it: zero-filling the (ncopy, B, K, N, L) dB / dC copies, the kernel, and
the sum over the copies; `bwd_kernel_only` times the kernel alone on pre-allocated buffers (accumulating into them).
Writes profiles/scan_dstate_bench.json (or the path given as the first argument; the second names the commit where the
tree runs without its git metadata)."""
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
DSTATES = (1, 2, 4, 8, 16)
SAMPLES, PER_SAMPLE, WARMUP = 24, 5, 5


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(PER_SAMPLE):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / PER_SAMPLE * 1e3)
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), iqr_us=q[2] - q[0], samples=len(us))


def case(n, dev):
    g = torch.Generator().manual_seed(n)
    r = lambda *s: torch.randn(*s, generator=g)
    u, delta = r(NB, KD, L).to(dev, torch.bfloat16), (0.5 * r(NB, KD, L)).to(dev, torch.bfloat16)
    A = -(torch.rand(KD, n, generator=g) + 0.5).to(dev)
    B, C = r(NB, K, n, L).to(dev, torch.bfloat16), r(NB, K, n, L).to(dev, torch.bfloat16)
    D, bias = torch.ones(KD, device=dev), torch.full((KD,), -3.0, device=dev)
    dout = r(NB, KD, L).to(dev)
    return u, delta, A, B, C, D, bias, dout


def bwd_kernel_only(args, dout, ckpt, n):
    u, delta, A, B, C, D, bias = args
    ncopy = hip.scan_bc_copies(KD, K, n)
    du, dd = torch.empty_like(u), torch.empty_like(delta)
    dA = torch.zeros(KD, n, device=u.device)
    dB = torch.zeros(ncopy, NB, K, n, L, device=u.device)
    dC, dD, db = torch.zeros_like(dB), torch.zeros(KD, device=u.device), torch.zeros(KD, device=u.device)
    p = lambda t: t.data_ptr()

    def launch():
        hip._check(hip.lib().tramba_selective_scan_bwd(
            p(u), p(delta), p(A), p(B), p(C), p(D), p(bias), p(dout), p(ckpt), p(du), p(dd), p(dA), p(dB), p(dC), p(dD), p(db),
            NB, KD, K, n, L, hip.dt(u), 1, ncopy, hip._stream()), "selective_scan_bwd")
    return launch, ncopy


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scan_dstate_bench.json")
    dev = torch.device("cuda")
    commit = sys.argv[2] if len(sys.argv) > 2 else ""      # where the tree travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), commit=commit or "unknown (no git metadata)",
               shape=dict(B=NB, KD=KD, K=K, L=L, io="bfloat16", out="float32"),
               protocol=dict(samples=SAMPLES, launches_per_sample=PER_SAMPLE, warmup=WARMUP), fwd={}, bwd={}, bwd_kernel_only={})
    for n in DSTATES:
        *args, dout = case(n, dev)
        res["fwd"][n] = timed(lambda: hip.selective_scan_fwd(*args, True, True, want_ckpt=True))
        _, ckpt = hip.selective_scan_fwd(*args, True, True, want_ckpt=True)
        res["bwd"][n] = timed(lambda: hip.selective_scan_bwd(*args, dout, ckpt, True))
        launch, ncopy = bwd_kernel_only(args, dout, ckpt, n)
        res["bwd_kernel_only"][n] = dict(timed(launch), ncopy=ncopy)
        hip.device_error()
        print(f"N={n:2d} fwd {res['fwd'][n]['median_us']:9.1f} us  bwd {res['bwd'][n]['median_us']:9.1f} us  "
              f"bwd kernel {res['bwd_kernel_only'][n]['median_us']:9.1f} us (ncopy {ncopy})", flush=True)
        del args, dout, ckpt, launch
        torch.cuda.empty_cache()
    ratios = {}
    for key in ("fwd", "bwd", "bwd_kernel_only"):
        t = {n: res[key][n]["median_us"] for n in DSTATES}
        ratios[key] = {"t8_over_t4": t[8] / t[4], "target_8": 2.0, "t16_over_t4": t[16] / t[4], "target_16": 4.0,
                       "slack": 0.10, "met": t[8] <= 2.2 * t[4] and t[16] <= 4.4 * t[4],
                       "us_per_state": {n: t[n] / n for n in DSTATES}}
    res["ratios"] = ratios
    print(json.dumps(ratios, indent=1))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
