#!/usr/bin/env python3
"""The mixed-size frame path (tramba_amd/infer.py on lists of frames) against what such a set cost before it, same box, one
process, Tramba-V 384x384 bf16 (random init: the weights do not change the time), the protocol of bench_frames.py:
  - pipeline, ms per frame, on 64 seeded frames of 16 distinct sizes between 300x400 and 1080x1920, from frames in host
    memory to uint8 maps on the device, wall clock over synchronised passes: `FramePredictor` on lists of 4 and of 8 frames
    (graphed: one graph per bucket) against `FramePredictor` one frame at a time, graphed (a capture per new size, at most
    MAX_GRAPHS kept) and eager;
  - the two ragged kernels against their uniform counterparts on equal-sized 1080x1920 frames, batch 1 and 4, by HIP events
    over 200 back-to-back launches, five such measurements each: the ratio and the uniform kernel's run-to-run spread;
  - `evaluate_dataset` against `predict_folder` + `evaluate_folder` on one seeded set of 24 pairs, wall clock.
usage: python scripts/bench_frames_ragged.py [--out FILE.json] [--passes N]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tramba_amd import evaluate, hip, infer  # noqa: E402

S = 384
SIZES = [(300, 400), (375, 500), (480, 640), (640, 480), (427, 640), (333, 500), (600, 800), (768, 1024), (720, 1280),
         (1080, 1920), (1024, 768), (500, 375), (540, 960), (400, 300), (900, 1200), (681, 1024)]


def frame(h, w, seed, noise=40):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(yy / 37.0) * 60 + np.cos(xx / 53.0) * 60 + 128)[..., None]
    return np.clip(base + rs.randint(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def events_us(fn, reps=200):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def pass_ms(fn, frames, passes):
    """ms per frame of `fn(frames)` over synchronised passes, after one warm pass"""
    fn(frames)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(passes):
        fn(frames)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / passes / len(frames) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_ragged_bench.json"))
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames_ragged.py measures the device pipeline: it needs a GPU"
    import tramba_amd as ta
    from PIL import Image
    dev = torch.device("cuda", 0)
    torch.manual_seed(1026)
    model = ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=S, dims=128, depths=[2, 2, 2, 2])
    model = ta.prepare_inference(model.to(dev), torch.bfloat16).eval()
    res = dict(device=torch.cuda.get_device_name(0), torch_threads=torch.get_num_threads(), img_size=S,
               model="Tramba-V 384 bf16 (random init)", sizes=SIZES)

    # ---- pipeline on a mixed-size set
    order = np.random.RandomState(3).permutation(64)
    frames = [frame(*SIZES[i % len(SIZES)], seed=int(i)) for i in order]
    pipe = {}
    for b in (4, 8):
        pred = infer.FramePredictor(model, S, graph=True, strict=True)

        def ragged(fs, pred=pred, b=b):
            for i in range(0, len(fs), b):
                pred(fs[i:i + b])
        pipe[f"ragged_graphed_batch{b}_ms_per_frame"] = round(pass_ms(ragged, frames, args.passes), 3)
        pipe[f"ragged_graphed_batch{b}_graphs"] = len(pred._graphs)
    for b in (4, 8):
        pred = infer.FramePredictor(model, S, graph=False)

        def ragged_eager(fs, pred=pred, b=b):
            for i in range(0, len(fs), b):
                pred(fs[i:i + b])
        pipe[f"ragged_eager_batch{b}_ms_per_frame"] = round(pass_ms(ragged_eager, frames, args.passes), 3)
    for name, graph in (("one_at_a_time_eager", False), ("one_at_a_time_graphed", True)):
        pred = infer.FramePredictor(model, S, graph=graph, strict=True)

        def single(fs, pred=pred):
            for f in fs:
                pred(f)
        pipe[f"{name}_ms_per_frame"] = round(pass_ms(single, frames, 1 if graph else args.passes), 3)
    res["pipeline_64_frames_16_sizes"] = pipe
    print(json.dumps(pipe), flush=True)

    # ---- kernels on equal-sized frames
    H, W = 1080, 1920
    rows = []
    for b in (1, 4):
        fs = [frame(H, W, seed=100 + k) for k in range(b)]
        batch = infer.pack_frames(fs, S)
        desc = infer.descriptors(batch)
        packed = batch["packed"].to(dev)
        dframes = torch.from_numpy(np.stack(fs)).to(dev)
        table = infer.resize_table(H, W, S, dev)
        logits = torch.randn(b, 1, S, S, device=dev)
        out = torch.empty(infer.output_bytes(desc), dtype=torch.uint8, device=dev)
        same_in = torch.equal(hip.frames_to_input_ragged(packed, desc, S), hip.frames_to_input(dframes, table, S, S))
        same_out = torch.equal(torch.stack(infer._map_views(hip.logits_to_u8_ragged(logits, packed, desc, out), desc)),
                               hip.logits_to_u8(logits, H, W))
        t = {k: [] for k in ("in_uniform", "in_ragged", "out_uniform", "out_ragged")}
        for _ in range(5):                                   # alternating, so drift hits both alike
            t["in_uniform"].append(events_us(lambda: hip.frames_to_input(dframes, table, S, S)))
            t["in_ragged"].append(events_us(lambda: hip.frames_to_input_ragged(packed, desc, S)))
            t["out_uniform"].append(events_us(lambda: hip.logits_to_u8(logits, H, W)))
            t["out_ragged"].append(events_us(lambda: hip.logits_to_u8_ragged(logits, packed, desc, out)))
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = dict(batch=b, results_identical=bool(same_in and same_out),
                   frames_to_input_us=round(med["in_uniform"], 2), frames_to_input_ragged_us=round(med["in_ragged"], 2),
                   frames_to_input_ratio=round(med["in_ragged"] / med["in_uniform"], 3),
                   frames_to_input_uniform_spread=round((max(t["in_uniform"]) - min(t["in_uniform"])) / med["in_uniform"], 3),
                   logits_to_u8_us=round(med["out_uniform"], 2), logits_to_u8_ragged_us=round(med["out_ragged"], 2),
                   logits_to_u8_ratio=round(med["out_ragged"] / med["out_uniform"], 3),
                   logits_to_u8_uniform_spread=round((max(t["out_uniform"]) - min(t["out_uniform"])) / med["out_uniform"], 3),
                   all_us={k: [round(x, 2) for x in v] for k, v in t.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    res["kernels_1080x1920"] = rows

    # ---- evaluate_dataset against predict_folder + evaluate_folder
    with tempfile.TemporaryDirectory() as tmp:
        for sub in ("image", "mask"):
            os.makedirs(os.path.join(tmp, "Test", sub))
        n = 24
        for k in range(n):
            h, w = SIZES[k % len(SIZES)]
            Image.fromarray(frame(h, w, seed=700 + k, noise=4)).save(os.path.join(tmp, "Test", "image", f"i{k:03d}.png"),
                                                                     compress_level=1)
            yy, xx = np.mgrid[0:h, 0:w]
            m = ((yy - h / 2) ** 2 + (xx - w / 3) ** 2 < (min(h, w) / 3) ** 2).astype(np.uint8) * 255
            Image.fromarray(m).save(os.path.join(tmp, "Test", "mask", f"i{k:03d}.png"), compress_level=1)
        ev = {"pairs": n}
        for b in (1, 4):
            for rep in range(2):                             # the second repetition is the one recorded (warm files, warm kernels)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                infer.predict_folder(model, os.path.join(tmp, "Test", "image"), os.path.join(tmp, f"p{b}"), S, batch=b)
                t1 = time.perf_counter()
                two = evaluate.evaluate_folder(os.path.join(tmp, f"p{b}"), os.path.join(tmp, "Test", "mask"))
                t2 = time.perf_counter()
                one = evaluate.evaluate_dataset(model, tmp, S, batch=b)
                t3 = time.perf_counter()
            ev[f"batch{b}"] = dict(predict_folder_s=round(t1 - t0, 3), evaluate_folder_s=round(t2 - t1, 3),
                                   two_step_s=round(t2 - t0, 3), evaluate_dataset_s=round(t3 - t2, 3),
                                   results_identical=all(np.array_equal(one[k], two[k]) for k in two))
        res["evaluate_24_pairs"] = ev
        print(json.dumps(ev), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
