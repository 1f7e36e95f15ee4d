#!/usr/bin/env python3
"""The deployment pipeline (tramba_amd/infer.py) against the host pipeline it replaces, same box, seeded 1080x1920 uint8
frames, Tramba-V 384x384 bf16 (random init: the weights do not change the time):
  - host pipeline: data.get_transform(384, "Test") per frame on the host (PIL resize + numpy normalisation), upload,
    GraphedForward, then save_predictions' torch sequence per image (F.interpolate, sigmoid, *255, .to(uint8));
  - device pipeline: FramePredictor, graphed (preprocess + forward + postprocess as one hipGraph; the frames' upload
    before the replay);
  both from frames in host memory to uint8 maps on the device, wall clock over a synchronised loop, per frame, at batch 1
  and 4;
  - tramba_frames_to_input and tramba_logits_to_u8 alone by HIP events over back-to-back launches, with the bytes they
    must move (from the shapes) per second against the HBM peak;
  - the host transform alone, per frame.
usage: python scripts/bench_frames.py [--out FILE.json] [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import data, hip, infer  # noqa: E402

H, W, S = 1080, 1920, 384
HBM_PEAK = 8.0e12           # MI355X HBM3E, spec
HBM_ACHIEVABLE = 6.29e12    # float4 copy, measured (MI355X_MICROARCH: HBM)


def frames_for(b, seed=0):
    rs = np.random.RandomState(seed)
    # smooth content plus noise: a random-noise frame and a camera frame cost the same to resize, not to compress
    yy, xx = np.mgrid[0:H, 0:W]
    base = (np.sin(yy / 37.0)[..., None] * 60 + np.cos(xx / 53.0)[..., None] * 60 + 128).astype(np.float64)
    return np.stack([np.clip(base + rs.randint(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8) for _ in range(b)])


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
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def bandwidth(nbytes, ms):
    bps = nbytes / (ms * 1e-3)
    return dict(bytes=int(nbytes), GBps=round(bps / 1e9, 1), share_of_hbm_peak=round(bps / HBM_PEAK, 3),
                share_of_hbm_achievable=round(bps / HBM_ACHIEVABLE, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames.py measures the device pipeline: it needs a GPU"
    import tramba_amd as ta
    from PIL import Image
    dev = torch.device("cuda", 0)
    torch.manual_seed(1026)
    model = ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=S, dims=128, depths=[2, 2, 2, 2])
    model = ta.prepare_inference(model.to(dev), torch.bfloat16).eval()
    tf = data.get_transform(S, "Test")
    res = dict(device=torch.cuda.get_device_name(0), torch_threads=torch.get_num_threads(), frame=[H, W], img_size=S,
               model="Tramba-V 384 bf16 (random init)", hbm_peak_Bps=HBM_PEAK, hbm_achievable_Bps=HBM_ACHIEVABLE, rows=[])

    # the host transform alone: one frame on one core, as each loader worker runs it
    one = frames_for(1, seed=7)[0]
    t = time.perf_counter()
    n = 20
    for _ in range(n):
        tf({"image": Image.fromarray(one)})
    res["host_transform_ms_per_frame"] = round((time.perf_counter() - t) / n * 1e3, 3)
    print("host transform", res["host_transform_ms_per_frame"], "ms / frame", flush=True)

    for b in (1, 4):
        frames = frames_for(b, seed=b)
        gf = ta.GraphedForward(model, strict=True)
        fp = infer.FramePredictor(model, S, graph=True, strict=True)

        def host_pipeline():
            x = torch.stack([tf({"image": Image.fromarray(f)})["image"] for f in frames]).to(dev)
            r = gf(x)[-1].float()
            return [(torch.sigmoid(F.interpolate(r[i:i + 1], size=(H, W), mode="bilinear", align_corners=False))[0, 0]
                     * 255).to(torch.uint8) for i in range(b)]

        def device_pipeline():
            return fp(frames)

        same = all(torch.equal(m, d) for m, d in zip(host_pipeline(), device_pipeline()))
        host_ms = wall_ms(host_pipeline, max(3, args.reps // 3))
        dev_ms = wall_ms(device_pipeline, args.reps)

        dframes = torch.from_numpy(frames).to(dev)
        table = infer.resize_table(H, W, S, dev)
        pre_ms = events_ms(lambda: hip.frames_to_input(dframes, table, S, S), 200)
        logits = torch.randn(b, 1, S, S, device=dev)
        post_ms = events_ms(lambda: hip.logits_to_u8(logits, H, W), 200)
        row = dict(batch=b, maps_identical=same,
                   host_pipeline_ms_per_frame=round(host_ms / b, 3), device_pipeline_ms_per_frame=round(dev_ms / b, 3),
                   speedup=round(host_ms / dev_ms, 2),
                   frames_to_input_us=round(pre_ms * 1e3, 2),
                   frames_to_input_bw=bandwidth(b * H * W * 3 + b * 3 * S * S * 4, pre_ms),
                   logits_to_u8_us=round(post_ms * 1e3, 2),
                   logits_to_u8_bw=bandwidth(b * S * S * 4 + b * H * W, post_ms))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
