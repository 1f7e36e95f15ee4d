#!/usr/bin/env python3
"""The device train transform (tramba_amd/augment.py) against the host one it replaces, same box, seeded 1080x1920 pairs
(smooth content plus noise, JPEG image + PNG mask on disk), S = 384, batch 8:
  - tramba_augment_batch alone by HIP events over back-to-back batches (25 distinct packed batches of recorded draws,
    cycled), with the bytes it must move (from the shapes) per second against the HBM peak;
  - the upload of one packed batch (pinned, non_blocking) by HIP events;
  - host CPU per sample, one process: decode + draws (the device loader's worker) against decode + get_transform (the
    host loader's worker);
  - samples/s delivered on the device by device_batches(train_loader(...)) and device_train_batches(...) at a few worker
    counts (wall clock, synchronised at the end).
usage: python scripts/bench_augment.py [--out FILE.json] [--reps N] [--quick]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import augment, data, hip  # noqa: E402

H, W, S, B = 1080, 1920, 384, 8
HBM_PEAK = 8.0e12           # MI355X HBM3E, spec


def pair(seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (np.sin(yy / 37.0)[..., None] * 60 + np.cos(xx / 53.0)[..., None] * 60 + 128).astype(np.float64)
    img = np.clip(base + rs.randint(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)
    gt = ((((yy - H / 2) / H) ** 2 + ((xx - W / 2) / W) ** 2) < 0.08).astype(np.uint8) * 255
    return img, gt


def write_folder(root, n):
    for sub in ("image", "mask"):
        os.makedirs(os.path.join(root, "Train", sub), exist_ok=True)
    for i in range(n):
        img, gt = pair(i % 8)
        Image.fromarray(img).save(os.path.join(root, "Train", "image", f"f{i}.jpg"), quality=90)
        Image.fromarray(gt).save(os.path.join(root, "Train", "mask", f"f{i}.png"))


def device_transform(reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    pairs = [pair(i) for i in range(B)]
    rec = augment.DrawRecorder(np.random.RandomState(1026))
    batches = []
    for _ in range(25):
        batch = augment.pack([(img, gt, rec(S)) for img, gt in pairs], S)
        desc = augment.bind(augment.descriptors(batch), S, dev).copy()
        batches.append((batch["packed"].to(dev), desc))
    for packed, desc in batches[:3]:
        augment.transform(packed, desc, S)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        packed, desc = batches[i % len(batches)]
        augment.transform(packed, desc, S)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    # bytes the chain must move: the sources once, the (S, S, 4) stages written and read (A, G, the enhancer ping-pong
    # counted once), the bicubic rows of the scaled samples, the f32 outputs
    src = B * H * W * 4
    stages = B * S * S * 4 * 2 * 3
    rows = sum(int(d[augment._D_R]) for _, dd in batches for d in dd) / len(batches) * S * 4 * 2
    outs = B * S * S * 4 * 4
    nbytes = src + stages + rows + outs
    # the upload of one packed batch
    host = batches[0][0].cpu().pin_memory()
    dst = torch.empty_like(batches[0][0])
    for _ in range(3):
        dst.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        dst.copy_(host, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    up = e0.elapsed_time(e1) / 20
    return {"transform_ms_per_batch": ms, "transform_bytes": int(nbytes), "transform_hbm_frac": nbytes / (ms * 1e-3) / HBM_PEAK,
            "packed_bytes": int(host.numel()), "upload_ms_per_batch": up, "upload_GBps": host.numel() / (up * 1e-3) / 1e9,
            "reps": reps}


def host_cpu(root, n):
    ds = data.RGB_Dataset(root, ["Train"], S, "train")
    pds = augment.PairDataset(root, ["Train"], S)
    np.random.seed(1026)
    best = {}
    for name, get in (("decode_plus_draws", lambda i: pds[i]), ("decode_plus_get_transform", lambda i: ds[i])):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            for i in range(n):
                get(i % len(ds))
            ts.append((time.perf_counter() - t0) / n * 1e3)
        best[name + "_ms"] = min(ts)
    t0 = time.perf_counter()
    for i in range(n):
        with Image.open(ds.images[i % len(ds)]) as a, Image.open(ds.gts[i % len(ds)]) as b:
            a.convert("RGB"), b.convert("L")
    best["decode_only_ms"] = (time.perf_counter() - t0) / n * 1e3
    return best


def loaders(root, workers, nbatch):
    out = {}
    for nw in workers:
        for name, make in (("host", lambda: data.device_batches(data.train_loader(root, S, batch_size=B, num_workers=nw))),
                           ("device", lambda: augment.device_train_batches(root, S, batch_size=B, num_workers=nw))):
            np.random.seed(1026)
            torch.manual_seed(1026)
            batches = make()
            it = batches(0)
            next(it)                                        # workers started, tables built
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for img, lab in it:
                n += img.shape[0]
                if n >= nbatch * B:
                    break
            torch.cuda.synchronize()
            out[f"{name}_w{nw}_samples_per_s"] = n / (time.perf_counter() - t0)
            del it, batches
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--quick", action="store_true", help="the device transform only (for a kernel trace)")
    args = ap.parse_args()
    res = {"shape": {"source": [H, W], "S": S, "batch": B}, "device": torch.cuda.get_device_name(0)}
    res["device_transform"] = device_transform(args.reps)
    print(json.dumps(res["device_transform"]), flush=True)
    if not args.quick:
        with tempfile.TemporaryDirectory() as root:
            write_folder(root, 96)
            res["host_cpu_per_sample"] = host_cpu(root, 16)
            print(json.dumps(res["host_cpu_per_sample"]), flush=True)
            res["host_cpu_per_sample"]["cpus"] = len(os.sched_getaffinity(0))
            res["loaders"] = loaders(root, [0, 4, 8], 10)
            print(json.dumps(res["loaders"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
