#!/usr/bin/env python3
"""What the weighted losses (structure_loss / wbce) cost on the device, at the training shapes: batch 8,
384 x 384 labels, deep-supervision outputs at 24 / 48 / 96 / 384.

  python scripts/bench_loss.py [rounds] [out.json]
      Loss forward + backward (gradients of all four outputs), device events, `rounds` (>= 8) timings, the variants timed
      alternately after a warm-up of every one of them; the calls per timing are chosen per variant from a pilot so that a
      timed window is about WINDOW_S of work:
        (a) bce_iou               the existing device loss (tramba_loss)
        (b) structure / wbce      the new kernels, both readings of the BCE term
        (c) composed:<loss>       the same losses composed from framework ops on the GPU (interpolate, avg_pool2d, sigmoid,
                                  products, reductions and their autograd backward)
      twice: "eager" (each call enqueued from Python: what train_step pays, the host's launches included) and "graph" (the
      same forward + backward captured once and replayed: what the device pays inside a GraphedTrainStep; the ratio to set
      against the byte model).  Every call clears the outputs' .grad first, so each call -- and each replay, from the
      graph's own pool -- also runs autograd's node that copies a fresh gradient into .grad, one small copy per output:
      the figures of (a), (b) and (c) all include it, and the ratios are read with that in mind.
      Then the weight-map kernel by itself (k = 31, k = 15), GRAPH_LAUNCHES launches into one
      preallocated map captured as one graph: time per launch inside a graph (the gaps between graph nodes included; not a
      kernel-trace figure) against its algorithmic bytes (one read and one write of the map, which at this size stay in the
      last-level cache: a rate, not an HBM bandwidth).
      Then the full Tramba-V step (bf16 activations, stochastic depth on) as ONE hipGraph with the default loss, with the
      structure loss, with the default loss captured a second time and -- when the parent commit's library has been built
      into tramba_amd/_lib_parent/ (untracked, as scripts/ab_parent.py uses it) -- with the default loss on the parent's
      library, captured twice as well, all replayed alternately in one process.  aa_spread_ms is the round-to-round
      spread of default - default2; capture_spread_ms is the distance between the means of two captures of the same
      code, the larger of the two and the one a difference between libraries or losses is read against.
      Written to profiles/loss_bench.json, section by section.

  python scripts/bench_loss.py --ab [rounds] [out.json]
      This tree's library against the parent commit's (tramba_amd/_lib_parent/, required), `hip._lib` swapped between them
      in one process:
        bits   every LOSS_CASES entry of tests/test_gpu_step_ends.py, hard and soft labels, bce_iou and the four weighted
               forms through the bindings: `torch.equal` of the loss, the coefficient table and every output's gradient
               (incoming gradient 0.37) between the two libraries; all_equal says whether every one of them is True
        loss   forward + backward of bce_iou and structure/reference at the training shapes, captured on each library TWICE
               and replayed alternately: mean of new - parent per variant against capture_spread_ms, the larger distance
               between the means of two captures of the same code (within_3x_spread)
        step   the whole-step section above
      Written to profiles/loss_unify_ab.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "loss_bench.json")
OUT_AB = os.path.join(ROOT, "profiles", "loss_unify_ab.json")
PARENT = os.path.join(ROOT, "tramba_amd", "_lib_parent", "libtramba_hip.so")
BATCH, SIZE, OUTS = 8, 384, (24, 48, 96, 384)
WINDOW_S, GRAPH_LAUNCHES, STEP_REPLAYS = 0.3, 200, 10


def composed(kind, per_pixel):
    """the loss from framework ops only: utils/loss.py:15-42 after train.py:78-79's resize"""
    import torch
    import torch.nn.functional as F
    k, eps, iou = {"structure": (31, 0.001, True), "wbce": (15, 0.0, False)}[kind]

    def loss(outs, label):
        weit = 1 + 5 * torch.abs(F.avg_pool2d(label, kernel_size=k, stride=1, padding=k // 2) - label)
        total = None
        for o in outs:
            if o.shape[-2:] != label.shape[-2:]:
                o = F.interpolate(o, label.shape[-2:], mode="bilinear")
            bce = F.binary_cross_entropy_with_logits(o, (1 - eps) * label + eps / 2, reduction="none" if per_pixel else "mean")
            term = ((weit * bce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))).mean()
            if iou:
                p = torch.sigmoid(o)
                inter = ((p * label) * weit).sum(dim=(2, 3))
                union = ((p + label) * weit).sum(dim=(2, 3))
                term = term + (1 - (inter + 1) / (union - inter + 1)).mean()
            total = term if total is None else total + term
        return total
    return loss


def timed(runs, rounds, calls=None):
    """{name: fn} -> ({name: [ms per call, one per round]}, {name: calls per timing}), the variants alternating within a
    round.  calls=None: per variant, from a pilot of 10 calls, as many as make a window of WINDOW_S."""
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, n):
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / n

    t = {k: [] for k in runs}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    n = {k: calls or max(10, min(20000, int(1e3 * WINDOW_S / max(window(fn, 10), 1e-3)))) for k, fn in runs.items()}
    for _ in range(rounds):
        for name, fn in runs.items():
            t[name].append(window(fn, n[name]))
    return t, n


def stats(timings):
    t, n = timings
    return {k: {"mean_ms": statistics.mean(v), "std_ms": statistics.pstdev(v), "min_ms": min(v), "calls_per_timing": n[k]}
            for k, v in t.items()}


def graphed(fn, times=1):
    """fn() `times` over captured as one hipGraph (after eager runs that warm it up); returns the replay"""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(times):
            fn()
    torch.cuda.synchronize()
    return g.replay


def ratios(t):
    base = t["bce_iou"]["mean_ms"]
    return {"ms_per_call": t,
            "ratio_to_bce_iou": {k: v["mean_ms"] / base for k, v in t.items()},
            "device_over_composed": {k: t[k]["mean_ms"] / t["composed:" + k]["mean_ms"] for k in t if "/" in k and ":" not in k}}


def bench_losses(rounds):
    import torch
    from tramba_amd import hip, train
    g = torch.Generator().manual_seed(0)
    outs = [(3.0 * torch.randn(BATCH, 1, s, s, generator=g)).cuda().requires_grad_() for s in OUTS]
    blobs = torch.nn.functional.avg_pool2d(torch.randn(BATCH, 1, SIZE, SIZE, generator=g), 25, 1, 12)
    label = (blobs > 0.02).float().cuda()

    def fwd_bwd(loss_fn):
        def run():
            for o in outs:
                o.grad = None
            loss_fn(outs, label).backward()
        return run

    runs = {"bce_iou": fwd_bwd(train.tramba_loss)}
    for kind in ("structure", "wbce"):
        for bce in ("reference", "pixel"):
            runs[f"{kind}/{bce}"] = fwd_bwd(train.SodLoss(kind, bce))
            runs[f"composed:{kind}/{bce}"] = fwd_bwd(composed(kind, bce == "pixel"))
    eager = stats(timed(runs, rounds))
    keep = {k: graphed(fn) for k, fn in runs.items()}      # one graph per variant, all alive while they alternate
    graph = stats(timed(keep, rounds))
    # the composition and the kernels compute the same thing (fp32 both): the figure that says so
    agree = {}
    for kind in ("structure", "wbce"):
        for bce in ("reference", "pixel"):
            with torch.no_grad():
                got, want = float(train.SodLoss(kind, bce)(outs, label)), float(composed(kind, bce == "pixel")(outs, label))
            agree[f"{kind}/{bce}"] = {"device": got, "composed": want}
    weit = torch.empty_like(label)
    planes = label.numel() // (SIZE * SIZE)

    def launch(k):
        def run():
            hip._check(hip.lib().tramba_loss_weight_map(label.data_ptr(), weit.data_ptr(), planes, SIZE, SIZE, k, hip._stream()),
                       "loss_weight_map")
        return run

    maps = stats(timed({f"k={k}": graphed(launch(k), GRAPH_LAUNCHES) for k in (31, 15)}, rounds))
    nbytes = 2 * 4 * label.numel()
    for v in maps.values():
        v["ms_per_launch_in_graph"] = v["mean_ms"] / GRAPH_LAUNCHES
        v["algorithmic_bytes"] = nbytes
        v["gb_per_s_in_graph"] = nbytes / v["ms_per_launch_in_graph"] / 1e6
    return {
        "what": f"loss forward + backward, batch {BATCH}, label {SIZE}x{SIZE}, outputs {list(OUTS)}, fp32, {rounds} rounds, "
                f"windows of about {WINDOW_S} s (calls_per_timing); eager: enqueued from Python, host launches included; "
                f"graph: the same calls captured once and replayed",
        "eager": ratios(eager),
        "graph": ratios(graph),
        "loss_values": agree,
        "weight_map_kernel": {"what": f"{GRAPH_LAUNCHES} launches into one map captured as one graph; mean_ms is per replay",
                              **maps},
    }


def ab_bits(rounds):
    import torch
    from tramba_amd import hip
    from ab_lib import load
    from test_gpu_losses import FORMS, LOSS_CASES, _label
    import synth
    libs = {"parent": load(PARENT), "new": hip.lib()}
    gscale = torch.tensor(0.37, device="cuda")

    def run(lib, form, outs, lab):
        """(loss, coefs, gradient of every output) of one form through the bindings on one library"""
        hip._lib = lib
        if form == "bce_iou":
            loss, coefs = hip.sod_loss(outs, lab)
            grads = [hip.sod_loss_grad(o, lab, coefs[i], gscale) for i, o in enumerate(outs)]
        else:
            kind, bce = form.split("/")
            k, eps, iou = FORMS[kind]
            wmap = hip.loss_weight_map(lab, k)
            loss, coefs = hip.sod_wloss(outs, lab, wmap, eps=eps, per_pixel=bce == "pixel", with_iou=iou)
            grads = [hip.sod_wloss_grad(o, lab, wmap, coefs[i], gscale, eps=eps) for i, o in enumerate(outs)]
        torch.cuda.synchronize()
        return loss, coefs, grads

    forms = ["bce_iou"] + [f"{kind}/{bce}" for kind in FORMS for bce in ("reference", "pixel")]
    res = {}
    try:
        for name, (b, c, (hh, ww), sizes) in LOSS_CASES.items():
            outs = [synth.synth_input(f"loss_{name}_{i}", (b, c, h, w), scale=3.0).cuda() for i, (h, w) in enumerate(sizes)]
            for soft in (False, True):
                lab = _label(f"wloss_{name}", (b, c, hh, ww), soft).cuda()
                for form in forms:
                    (lp, cp, gp), (ln, cn, gn) = (run(libs[k], form, outs, lab) for k in ("parent", "new"))
                    res[f"{name}/{'soft' if soft else 'hard'}/{form}"] = {
                        "loss": torch.equal(lp, ln), "coefs": torch.equal(cp, cn),
                        "grads": [torch.equal(p, n) for p, n in zip(gp, gn)], "loss_value": float(ln)}
    finally:
        hip._lib = libs["new"]
    return {"what": "torch.equal(parent library, this library) of the loss, the coefficient table and each output's gradient",
            "all_equal": all(v["loss"] and v["coefs"] and all(v["grads"]) for v in res.values()), "cases": res}


def ab_loss(rounds):
    import torch
    from tramba_amd import hip, train
    from ab_lib import load
    libs = {"parent": load(PARENT), "new": hip.lib()}
    g = torch.Generator().manual_seed(0)
    outs = [(3.0 * torch.randn(BATCH, 1, s, s, generator=g)).cuda().requires_grad_() for s in OUTS]
    blobs = torch.nn.functional.avg_pool2d(torch.randn(BATCH, 1, SIZE, SIZE, generator=g), 25, 1, 12)
    label = (blobs > 0.02).float().cuda()
    specs = {"bce_iou": train.tramba_loss, "structure/reference": train.SodLoss("structure", "reference")}

    def fwd_bwd(loss_fn):
        def run():
            for o in outs:
                o.grad = None
            loss_fn(outs, label).backward()
        return run

    keep = {}
    try:
        for tag in ("parent", "new", "parent2", "new2"):          # a graph holds the kernels of the library it was captured on
            hip._lib = libs[tag.rstrip("2")]
            for name, fn in specs.items():
                keep[f"{name}:{tag}"] = graphed(fwd_bwd(fn))
    finally:
        hip._lib = libs["new"]
    t, n = timed(keep, rounds)
    mean = {k: statistics.mean(v) for k, v in t.items()}
    res = {"what": f"loss forward + backward captured once per (loss, library, capture) and replayed alternately, batch {BATCH}, "
                   f"label {SIZE}x{SIZE}, outputs {list(OUTS)}, {rounds} rounds, windows of about {WINDOW_S} s",
           "ms_per_call": stats((t, n))}
    for name in specs:
        m = {tag: mean[f"{name}:{tag}"] for tag in ("parent", "new", "parent2", "new2")}
        spread = max(abs(m["parent"] - m["parent2"]), abs(m["new"] - m["new2"]))
        diff = (m["new"] + m["new2"] - m["parent"] - m["parent2"]) / 2
        res[name] = {"mean_new_minus_parent_ms": diff, "capture_spread_ms": spread, "within_3x_spread": abs(diff) <= 3 * spread,
                     "not_slower_beyond_3x_spread": diff <= 3 * spread}
    return res


def bench_step(rounds):
    import torch
    import tramba_amd as ta
    from tramba_amd import hip, train
    from ab_lib import load
    new, parent_path = hip.lib(), PARENT
    # two captures of the same code differ by more than the rounds of one capture do (where a capture's buffers land), so
    # every library is captured twice, the libraries alternating: capture_spread_ms is what a difference is read against
    variants = [("default", None, new), ("structure", train.SodLoss("structure"), new), ("default2", None, new)]
    if os.path.exists(parent_path):
        parent = load(parent_path)
        variants = [("parent", None, parent)] + variants[:2] + [("parent2", None, parent)] + variants[2:]
    x = torch.randn(BATCH, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).cuda()
    y = (torch.rand(BATCH, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(1)) > 0.7).float().cuda()
    keep, runs, first = [], {}, {}
    for name, spec, lib in variants:
        hip._lib = lib
        torch.manual_seed(1026)
        m = ta.bulid_model(use_pretrain=False, img_size=SIZE).cuda().train()
        m.compute_dtype = torch.bfloat16
        step = ta.GraphedTrainStep(m, train.get_opt(1e-4, m, capturable=True), loss=spec)
        first[name] = float(step(x, y))
        keep.append((m, step))
        runs[name] = lambda step=step: step(x, y)
    hip._lib = new
    t, n = timed(runs, rounds, STEP_REPLAYS)
    aa = [p - q for p, q in zip(t["default"], t["default2"])]
    cost = [p - q for p, q in zip(t["structure"], t["default"])]
    res = {
        "what": f"Tramba-V {SIZE}x{SIZE} bf16, batch {BATCH}, the whole step as one hipGraph, {STEP_REPLAYS} replays per timing, "
                f"{rounds} rounds, {len(runs)} captures replayed alternately in one process",
        "ms_per_step": stats((t, n)),
        "first_step_loss": first,
        "aa_spread_ms": statistics.pstdev(aa), "mean_default_minus_default2_ms": statistics.mean(aa),
        "mean_structure_minus_default_ms": statistics.mean(cost),
    }
    mean = {k: statistics.mean(v) for k, v in t.items()}
    res["capture_spread_ms"] = {"default": abs(mean["default"] - mean["default2"])}
    if "parent" in t:
        res["capture_spread_ms"]["parent"] = abs(mean["parent"] - mean["parent2"])
        res["mean_parent_minus_default_ms"] = (mean["parent"] + mean["parent2"] - mean["default"] - mean["default2"]) / 2
        res["parent_first_step_loss_equal"] = first["parent"] == first["default"] == first["parent2"]
    return res


def main():
    args = sys.argv[1:]
    ab = args[:1] == ["--ab"]
    args = args[1:] if ab else args
    rounds = int(args[0]) if args else 8
    out_path = args[1] if len(args) > 1 else (OUT_AB if ab else OUT)
    import torch
    assert torch.cuda.is_available(), "bench_loss.py measures on the GPU"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sections = (("losses", bench_losses), ("step", bench_step))
    if ab:
        assert os.path.exists(PARENT), f"--ab needs the parent commit's library at {PARENT}"
        sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]      # the tests' cases and labels
        sections = (("bits", ab_bits), ("loss", ab_loss), ("step", bench_step))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    doc = {}
    for name, section in sections:
        doc[name] = section(rounds)
        print(json.dumps(doc[name], indent=1), flush=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
