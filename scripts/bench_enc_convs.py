#!/usr/bin/env python3
"""Encoder convolutions on the library (csrc/patch_conv.hip, `encoders.set_library_convolutions`) against the `F.conv2d` path
they replace, one process, one library; the protocol of scripts/bench_attn.py.

Every row captures its function as three hipGraphs -- switch on, switch off, switch on again for the A/A spread -- and replays
them alternately under HIP events, ROUNDS rounds of 20 replays.  `verdict`: a gain when mean(off - on) exceeds both three times
the standard deviation of on - on2 and |mean(on - on2)|, the offset between two captures of the same code; a loss when
mean(on - off) does; noise otherwise.  The switch-off path of this build is the parent's behaviour.

rows (bf16, 384 x 384, batch 1 and 4):
  models   Tramba-P and Tramba-S, one forward per replay; `on_equals_on2` / `off_equals_off2`: are two captures bitwise equal?
  blocks   one PVT block per stage shape with a spatial-reduction conv
  entries  each module that the switch flips, alone, 20 calls per graph: `sr` (patch_conv_cl), PVT's four patch embeddings
           (patch_embed_ln; conv3x3s2_cl + LayerNorm) and Swin's (patch_embed_ln); us per call
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_attn import REPLAYS, ROUNDS, build, flat, replay_ms  # noqa: E402

MODELS = (("Tramba-P", "Tramba-P-TSOD"), ("Tramba-S", "Tramba-S-TSOD"))
# (map side, C, heads, sr) of PVTv2-b4's stages with a spatial-reduction conv at 384 x 384
PVT_SR_STAGES = ((96, 64, 1, 8), (48, 128, 2, 4), (24, 320, 5, 2))
# (patch, stride, Cin, Cout, input side) of PVT's patch embeddings
PVT_EMBEDS = ((7, 4, 3, 64, 384), (3, 2, 64, 128, 96), (3, 2, 128, 320, 48), (3, 2, 320, 512, 24))


def capture(fn, root, on):
    from tramba_amd import encoders as E
    E.set_library_convolutions(root, on)
    with torch.no_grad():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
    torch.cuda.synchronize()
    return g, out


def aba(fn, root, rounds=ROUNDS, twice=False, per=1.0):
    """on / off / on2 graphs of fn (root: the module whose switch is flipped), replayed alternately"""
    graphs = {name: capture(fn, root, on) for name, on in (("on", True), ("off", False), ("on2", True))}
    extra = {}
    if twice:
        o2 = capture(fn, root, False)
        o2[0].replay()
        graphs["off"][0].replay()
        torch.cuda.synchronize()
        extra["off_equals_off2"] = all(torch.equal(a, b) for a, b in zip(flat(graphs["off"][1]), flat(o2[1])))
        del o2
    for g, _ in graphs.values():
        replay_ms(g, 3)
    t = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, (g, _) in graphs.items():
            t[name].append(replay_ms(g) * per)
    gain = [s - f for s, f in zip(t["off"], t["on"])]
    aa = [f - f2 for f, f2 in zip(t["on"], t["on2"])]
    spread, offset, mean = statistics.pstdev(aa), abs(statistics.mean(aa)), statistics.mean(gain)
    bar = max(3 * spread, offset)
    outs = {name: [o.clone() for o in flat(out)] for name, (_, out) in graphs.items()}
    rel = max(float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
              for a, b in zip(outs["on"], outs["off"]))
    return dict(on=round(statistics.mean(t["on"]), 4), off=round(statistics.mean(t["off"]), 4),
                on2=round(statistics.mean(t["on2"]), 4), mean_off_minus_on=round(mean, 4), aa_spread=round(spread, 4),
                capture_offset=round(offset, 4), verdict="gain" if mean > bar else ("loss" if -mean > bar else "noise"),
                on_equals_on2=all(torch.equal(a, b) for a, b in zip(outs["on"], outs["on2"])), on_vs_off_rel_l2=rel,
                rounds=rounds, replays=REPLAYS, **extra)


def model_rows(batches):
    rows = {}
    for tag, name in MODELS:
        m = build(name)
        for batch in batches:
            x = torch.randn(batch, 3, 384, 384, generator=torch.Generator().manual_seed(batch)).cuda()
            rows[f"{tag}_b{batch}"] = aba(lambda: m(x), m, twice=True)
            print(f"{tag}_b{batch} (ms)", json.dumps(rows[f"{tag}_b{batch}"]), flush=True)
        del m
        torch.cuda.empty_cache()
    return rows


def _lowp(module):
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d) and m.groups == 1:
            m.weight.data = m.weight.data.bfloat16()
            m.bias.data = m.bias.data.bfloat16()
    return module.cuda().eval()


def block_rows(batches):
    from tramba_amd import encoders as E
    rows = {}
    gen = torch.Generator().manual_seed(7)
    for batch in batches:
        for side, c, heads, sr in PVT_SR_STAGES:
            blk = _lowp(E._PvtBlock(c, heads, 4, True, 0.0, sr, 1e-6))
            x = torch.randn(batch, side * side, c, generator=gen).cuda().bfloat16()
            key = f"pvt_block_{side}x{side}_c{c}_sr{sr}_b{batch}"
            rows[key] = aba(lambda: blk(x, side, side), blk, rounds=6)
            print(key, "(ms)", json.dumps(rows[key]), flush=True)
    return rows


def entry_rows(batches, inner=20):
    """us per call of each switched module alone"""
    from tramba_amd import encoders as E
    rows = {}
    gen = torch.Generator().manual_seed(11)
    per = 1e3 / inner

    def row(key, fn, root):
        rows[key] = aba(lambda: [fn() for _ in range(inner)], root, rounds=6, per=per)
        print(key, "(us)", json.dumps(rows[key]), flush=True)

    for batch in batches:
        for side, c, heads, sr in PVT_SR_STAGES:
            attn = _lowp(E._PvtAttention(c, heads, True, sr))
            x = torch.randn(batch, side * side, c, generator=gen).cuda().bfloat16()
            # `_ln` takes a contiguous tensor: the stock path's transpose back is a copy of its own
            row(f"sr_{side}x{side}_c{c}_r{sr}_b{batch}", lambda: attn._reduce(x, side, side).contiguous(), attn)
        for s, (patch, stride, cin, cout, side) in enumerate(PVT_EMBEDS):
            emb = _lowp(E._OverlapPatchEmbed(patch, stride, cin, cout))
            x = torch.randn((batch, 3, side, side) if s == 0 else (batch, side, side, cin), generator=gen).cuda().bfloat16()
            row(f"pvt_patch_embed{s + 1}_b{batch}", lambda: emb(x, channels_last=s > 0)[0], emb)
        emb = _lowp(E._SwinPatchEmbed(384, 4, 3, 128))
        x = torch.randn(batch, 3, 384, 384, generator=gen).cuda().bfloat16()
        row(f"swin_patch_embed_b{batch}", lambda: emb(x), emb)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="models,blocks,entries")
    ap.add_argument("--batches", default="1,4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_enc_convs.py measures the GPU path: it needs a device"
    batches = [int(b) for b in args.batches.split(",")]
    res = dict(device=torch.cuda.get_device_name(0),
               what="bf16, 384x384; switch on / off / on again as hipGraphs; models and blocks in ms per replay, entries in us per call")
    for part, fn in (("models", model_rows), ("blocks", block_rows), ("entries", entry_rows)):
        if part in args.only.split(","):
            res[part] = fn(batches)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
