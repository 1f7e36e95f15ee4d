#!/usr/bin/env python3
"""ResNet-50 encoder convolutions on the library (csrc/resnet_conv.hip, `encoders.set_library_convolutions` on a Tramba-R model)
against the conv2d + batch_norm + relu + max_pool2d path they replace, one process, one library; the protocol of
scripts/bench_enc_convs.py / bench_attn.py.

Every row captures its function as three hipGraphs -- switch on, switch off, switch on again for the A/A spread -- and replays
them alternately under HIP events.  `verdict`: a gain when mean(off - on) exceeds both three times the standard deviation of
on - on2 and |mean(on - on2)|, the offset between two captures of the same code; a loss when mean(on - off) does; noise
otherwise.  The switch-off path of this build is the parent's behaviour.

rows (bf16, 384 x 384, batch 1 and 4):
  models   Tramba-R, one forward per replay; `on_equals_on2` / `off_equals_off2`: are two captures bitwise equal?
  encoder  the encoder alone (on: features_cl, layer4 not run; off: the stock forward with its to_cl copies)
  entries  each distinct (shape, ksize, stride) of the 42 conv_affine_cl launches, and the stem, alone, 20 calls per graph,
           against the stock conv + bn (+ shortcut) + relu of the same module; us per call
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_attn import build  # noqa: E402
from scripts.bench_enc_convs import aba  # noqa: E402


def model_rows(m, batches):
    rows = {}
    for batch in batches:
        x = torch.randn(batch, 3, 384, 384, generator=torch.Generator().manual_seed(batch)).cuda()
        rows[f"Tramba-R_b{batch}"] = aba(lambda: m(x), m, twice=True)
        print(f"Tramba-R_b{batch} (ms)", json.dumps(rows[f"Tramba-R_b{batch}"]), flush=True)
    return rows


def _encoder(enc, x):
    from tramba_amd.modules import to_cl
    if enc.library_convolutions:
        return enc.features_cl(x)
    return [to_cl(o) for o in enc(x.contiguous(memory_format=torch.channels_last))[1:-1][::-1]]


def encoder_rows(m, batches):
    rows = {}
    for batch in batches:
        x = torch.randn(batch, 3, 384, 384, generator=torch.Generator().manual_seed(batch)).cuda().bfloat16()
        rows[f"encoder_b{batch}"] = aba(lambda: _encoder(m.encoder, x), m, twice=True)
        print(f"encoder_b{batch} (ms)", json.dumps(rows[f"encoder_b{batch}"]), flush=True)
    return rows


def _launches(enc, side):
    """(key, owner, name, conv, bn, input side, with residual, relu) of the distinct launches of layer1..3 on a side x side
    stem output, in forward order"""
    seen, out = set(), []
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            mid = (side + 2 - 3) // blk.conv2.stride[0] + 1
            calls = [("conv1", blk.conv1, blk.bn1, side, False, True), ("conv2", blk.conv2, blk.bn2, side, False, True)]
            if blk.downsample is not None:
                calls.append(("downsample", blk.downsample[0], blk.downsample[1], side, False, False))
            calls.append(("conv3", blk.conv3, blk.bn3, mid, True, True))
            for name, conv, bn, s, res, relu in calls:
                k, st = conv.kernel_size[0], conv.stride[0]
                key = f"{name}_{s}x{s}_{conv.in_channels}to{conv.out_channels}_k{k}s{st}"
                if key not in seen:
                    seen.add(key)
                    out.append((key, blk, name, conv, bn, s, res, relu))
            side = mid
    return out


def entry_rows(m, batches, inner=20):
    from tramba_amd import models as M
    from tramba_amd.modules import from_cl, to_cl
    enc = m.encoder
    rows = {}
    gen = torch.Generator().manual_seed(11)
    per = 1e3 / inner

    def row(key, lib, stock):
        fn = lambda: [lib() if enc.library_convolutions else stock() for _ in range(inner)]
        rows[key] = aba(fn, m, rounds=6, per=per)
        print(key, "(us)", json.dumps(rows[key]), flush=True)

    for batch in batches:
        img = torch.randn(batch, 3, 384, 384, generator=gen).cuda().bfloat16()
        w, scale, shift = M._conv_bn_params(enc, "stem", enc.conv1, enc.bn1, img.dtype, kmajor=False)
        row(f"stem_b{batch}", lambda: M.hip.stem7_affine_relu_pool(img, w, scale, shift, img.dtype),
            lambda: to_cl(F.max_pool2d(F.relu(enc.bn1(enc.conv1(img))), 3, 2, 1)))
        for key, blk, name, conv, bn, side, with_res, relu in _launches(enc, 96):
            x = torch.randn(batch, side, side, conv.in_channels, generator=gen).cuda().bfloat16()
            res = None
            if with_res:
                res = torch.randn(batch, side, side, conv.out_channels, generator=gen).cuda().bfloat16()

            def stock(conv=conv, bn=bn, x=x, res=res, relu=relu):
                y = bn(conv(from_cl(x)))
                if res is not None:
                    y = y + from_cl(res)
                return to_cl(F.relu(y) if relu else y)
            row(f"{key}_b{batch}", lambda: M._conv_bn_cl(blk, name, conv, bn, x, res, relu), stock)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="models,encoder,entries")
    ap.add_argument("--batches", default="1,4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resnet_convs.py measures the GPU path: it needs a device"
    batches = [int(b) for b in args.batches.split(",")]
    res = dict(device=torch.cuda.get_device_name(0),
               what="bf16, 384x384; switch on / off / on again as hipGraphs; models and encoder in ms per replay, entries in us "
                    "per call")
    m = build("Tramba-R-TSOD")
    for part, fn in (("models", model_rows), ("encoder", encoder_rows), ("entries", entry_rows)):
        if part in args.only.split(","):
            res[part] = fn(m, batches)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
