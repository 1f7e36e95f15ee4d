#!/usr/bin/env python3
"""The weighted F-measure (Evaluation/metrics.py:379-441) on the GPU against the reference's host path (scipy
distance_transform_edt + convolve), same box, same seeded maps:
  - tramba_feature_transform alone and feature transform + weighted-F sums, by HIP events over back-to-back launches;
  - WeightedFmeasure.step from device tensors (GPU, result read back) and WeightedFmeasure(host=True).step from host
    arrays (one thread, warm), per image, at 384x384 batch 1 and 4 and at 1080x1920;
  - test_one_epoch wall time on Tramba-V 384x384 bf16 over synthetic batches of 4: weighted=False, weighted=True on the
    GPU, weighted=True on the host path.
usage: python scripts/bench_wfm.py [--out FILE.json] [--batches N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import evaluate as E, hip  # noqa: E402


def blob_pair(h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = np.zeros((h, w))
    for _ in range(3):
        cy, cx = rs.uniform(0.15, 0.85) * h, rs.uniform(0.15, 0.85) * w
        sy, sx = rs.uniform(0.05, 0.2) * h, rs.uniform(0.05, 0.2) * w
        z += rs.uniform(0.5, 1.5) * np.exp(-((yy - cy) ** 2 / (2 * sy * sy) + (xx - cx) ** 2 / (2 * sx * sx)))
    pred = 1.0 / (1.0 + np.exp(-(6.0 * (z - 0.55) + 1.2 * rs.standard_normal((h, w)))))
    return pred.astype(np.float32), z > 0.55


def events_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def metric_rows():
    rows = []
    for h, w, b, reps, host_reps in ((384, 384, 1, 200, 20), (384, 384, 4, 200, 5), (1080, 1920, 1, 50, 3)):
        pairs = [blob_pair(h, w, s) for s in range(b)]
        pred = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
        gt = torch.from_numpy(np.stack([g for _, g in pairs])).cuda()
        ft = events_ms(lambda: hip.feature_transform(gt), reps)
        sums = events_ms(lambda: hip.weighted_f_sums(pred, gt), reps)

        def gpu_step():
            m = E.WeightedFmeasure()
            m.step(pred, gt)
            E._memo["key"] = None          # a fresh (pred, gt) every call, as in an evaluation loop
            return m.weighted_fms

        def host_step():
            m = E.WeightedFmeasure(host=True)
            for p, g in pairs:
                m.step(p, g)
            return m.weighted_fms

        gpu = wall_ms(gpu_step, reps)
        host = wall_ms(host_step, host_reps)
        diff = max(abs(a - c) for a, c in zip(gpu_step(), host_step()))
        rows.append(dict(shape=[b, h, w], feature_transform_ms=round(ft, 4), ft_plus_sums_ms=round(sums, 4),
                         gpu_step_ms=round(gpu, 4), host_step_ms=round(host, 3),
                         host_per_image_ms=round(host / b, 3), speedup=round(host / gpu, 1), max_abs_diff_wfm=diff))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def epoch_rows(nbatch):
    import tramba_amd as ta
    torch.manual_seed(1026)
    model = ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=384, dims=128, depths=[2, 2, 2, 2])
    model = ta.prepare_inference(model.cuda(), torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    batches = []
    for i in range(nbatch):
        img = torch.nn.functional.avg_pool2d(torch.randn(4, 3, 384, 384, generator=g), 9, 1, 4)
        mask = np.stack([blob_pair(384, 384, 100 + 4 * i + j)[1] for j in range(4)])
        batches.append({"image": img, "gt": torch.from_numpy(mask[:, None].astype(np.float32))})
    host_cls = E.WeightedFmeasure
    out = {}
    for name, weighted, host in (("unweighted", False, False), ("weighted_gpu", True, False),
                                 ("weighted_host", True, True), ("weighted_gpu_2", True, False)):
        if host:
            E.WeightedFmeasure = lambda: host_cls(host=True)
        try:
            E.test_one_epoch(model, batches[:1], weighted=weighted)      # warm
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = E.test_one_epoch(model, batches, weighted=weighted)
            torch.cuda.synchronize()
            out[name] = dict(ms_total=round((time.perf_counter() - t) * 1e3, 2), Wmeasure_r=None if r["Wmeasure_r"] is None
                             else float(r["Wmeasure_r"]))
        finally:
            E.WeightedFmeasure = host_cls
        print(name, json.dumps(out[name]), flush=True)
    out["images"] = 4 * nbatch
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wfm.py measures the GPU path: it needs a device"
    res = dict(device=torch.cuda.get_device_name(0), threads=torch.get_num_threads(), metric=metric_rows(),
               test_one_epoch_tramba_v_384_bf16_b4=epoch_rows(args.batches))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
