#!/usr/bin/env python3
"""Same-box A/B of the LayerNorm family's row kernels (csrc/norm_conv.hip, csrc/train_fused.hip; the rows form of csrc/norm.h)
between the PARENT commit's library and this tree's, in the manner of scripts/ab_step_kernels.py:
  * `parent`  tramba_amd/_lib_parent/libtramba_hip.so, built from the parent commit (untracked, never shipped)
  * `new`     the current library
  * `new2`    the current library timed a second time: the spread between two runs of identical code
One process, hip._lib swapped between the calls, no graph captured anywhere:
  1. every public entry of the family -- layernorm_cl, shuffle_norm_cl, shuffle_norm_head_cl, add_layernorm_cl (with and
     without y, mask, dual and gate), layernorm_bwd_cl, layernorm_bwd_res_cl, shuffle_norm_bwd_cl, shuffle_norm_head_bwd_cl,
     rowdot_cl, rowdot_bwd_cl -- under each library on the same inputs: every output and every partial table (the raw entries,
     tables sized by the library's own query) must be torch.equal.  Shapes: the sweep of tests/test_gpu_row_forms.py (fp32 and
     bf16, C = VM * {1 .. 64, 3, 25}, 37 and 4609 rows, p = 2 on (1, 3, 3) / (1, 1, 1153), p = 4 on (1, 1, 2)) and the four
     (rows, C) pairs of Tramba-V's stages at 384 x 384, batch 4, bf16.  The first difference ends the script (exit status 1):
     nothing further is started on the device.
  2. each entry at those four shapes timed alternately parent / new / new2 under HIP events, ROUNDS rounds of STEPS calls (the
     order rotates from round to round, after one round that is timed and dropped).  The A/A spread is the standard deviation
     over the rounds of new - new2; an entry counts as slower if the mean of new - parent exceeds three times that.
     Reported, not asserted.
usage: python scripts/ab_row_forms.py [out.txt]   (profiles/row_forms_ab.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tramba_amd import hip                                 # noqa: E402
from ab_lib import load                                    # noqa: E402
from bench_sched_ema import ROUNDS, STEPS, timed           # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MULTS = (1, 2, 4, 8, 16, 32, 64, 3, 25)
STAGES = ((36864, 128, 48), (9216, 256, 24), (2304, 512, 12), (576, 1024, 6))      # rows, C, side of the p = 2 input map (batch 4)


class Case:
    """the operands of every entry for a (B, rows / B, C) map and, with `shuffle` = (p, B, H, W), a (B, H, W, p*p*C) one"""

    def __init__(self, dtype, rows, c, batch, shuffle):
        g = torch.Generator(device=DEV).manual_seed(rows * 131 + c)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)                                        # noqa: E731
        self.dtype, self.rows, self.c, self.shuffle = dtype, rows, c, shuffle
        self.x = (rnd(batch, rows // batch, c) * 1.5 + 0.3).to(dtype)
        self.y, self.dy, self.gres, self.gate = (rnd(batch, rows // batch, c).to(dtype) for _ in range(4))
        self.w, self.b, self.hw = 1 + 0.2 * rnd(c), 0.1 * rnd(c), rnd(c) * c ** -0.5
        self.gy = rnd(batch, rows // batch)
        self.mask = torch.tensor(([2.0, 0.0, 1.25, 0.5] * batch)[:batch], device=DEV)
        p, b, h, w = shuffle
        self.sx = (rnd(b, h, w, p * p * c) * 1.5 + 0.3).to(dtype)
        self.sdy = rnd(b, h * p, w * p, c).to(dtype)
        self.sg = rnd(b, h * p, w * p)
        self.tag = f"{str(dtype).split('.')[-1]} {rows}x{c} shuffle p={p} {b}x{h}x{w}"


def _table(parts, width):
    return torch.full((parts, width), float("nan"), device=DEV)


def ln_bwd_tables(k):
    """the raw partial tables of the LayerNorm backward, plain and through the shuffle"""
    lib, d, st, out = hip.lib(), hip.dt(k.x), hip._stream(), []
    p, b, h, w = k.shuffle
    for x, dy, rows, geom in ((k.x, k.dy, k.rows, (1, 1, 1)), (k.sx, k.sdy, b * h * w * p * p, (p, h, w))):
        t, dx = _table(lib.tramba_layernorm_bwd_parts(rows, k.c, d), 2 * k.c), torch.empty_like(x)
        hip._check(lib.tramba_layernorm_bwd_any_cl(hip._ptr(x), hip._ptr(dy), hip._ptr(k.w), hip._ptr(dx), hip._ptr(t), None, None,
                                                   0, None, rows, k.c, 1e-5, *geom, d, st), "layernorm_bwd_any_cl")
        out += [t, dx]
    return out


def rowdot_bwd_table(k):
    lib, d = hip.lib(), hip.dt(k.x)
    t, gx = _table(lib.tramba_rowdot_bwd_parts(k.rows, k.c, d), k.c + 4), torch.empty_like(k.x)
    hip._check(lib.tramba_rowdot_bwd_cl(hip._ptr(k.x), hip._ptr(k.gy), hip._ptr(k.hw), hip._ptr(gx), hip._ptr(t), k.rows, k.c, d,
                                        hip._stream()), "rowdot_bwd_cl")
    return [t, gx]


def head_bwd(k):
    dx, part = hip.shuffle_norm_head_bwd_cl(k.sx, k.sg, k.w, k.hw, k.shuffle[0])
    return [dx, part[:, :k.c + 1]]                         # (three pad slots behind slot C: nothing writes or reads them)


def add_ln(with_y, with_m, dual, with_gate):
    def run(k):
        out = hip.add_layernorm_cl(k.x, k.y if with_y else None, k.mask if with_m else None, k.w, k.b, 1e-5,
                                   hip.ACT_GELU if dual else hip.ACT_NONE, dual=dual, gate=k.gate if with_gate else None)
        return [t for t in out if t is not None]
    return run


ENTRIES = {
    "layernorm_cl": lambda k: [hip.layernorm_cl(k.x, k.w, k.b), hip.layernorm_cl(k.x, k.w, k.b, 1e-5, hip.ACT_GELU)],
    "shuffle_norm_cl": lambda k: [hip.shuffle_norm_cl(k.sx, k.w, k.b, k.shuffle[0])],
    "shuffle_norm_head_cl": lambda k: [hip.shuffle_norm_head_cl(k.sx, k.w, k.b, k.hw, -0.21, k.shuffle[0])],
    "add_layernorm_cl": add_ln(False, False, False, False),
    "add_layernorm_cl y": add_ln(True, False, False, False),
    "add_layernorm_cl y mask dual": add_ln(True, True, True, False),
    "add_layernorm_cl y mask dual gate": add_ln(True, True, True, True),
    "layernorm_bwd_cl": lambda k: list(hip.layernorm_bwd_cl(k.x, k.dy, k.w)),
    "layernorm_bwd_res_cl": lambda k: list(hip.layernorm_bwd_res_cl(k.x, k.dy, k.w, gres=k.gres, mask=k.mask, want_masked=True)),
    "shuffle_norm_bwd_cl": lambda k: list(hip.shuffle_norm_bwd_cl(k.sx, k.sdy, k.w, k.shuffle[0])),
    "layernorm_bwd tables": ln_bwd_tables,
    "shuffle_norm_head_bwd_cl": head_bwd,
    "rowdot_cl": lambda k: [hip.rowdot_cl(k.x, k.hw, 0.37)],
    "rowdot_bwd_cl": lambda k: list(hip.rowdot_bwd_cl(k.x, k.gy, k.hw)) + rowdot_bwd_table(k),
}
ROWS_FORM_ONLY = ("shuffle_norm_head_cl", "shuffle_norm_head_bwd_cl", "rowdot_bwd_cl")    # C <= 64 * VM; others take any C here


def served(name, k):
    vm = 4 if k.dtype == F32 else 8
    return name not in ROWS_FORM_ONLY or k.c // vm <= 64


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "row_forms_ab.txt")
    libs = {"parent": load(os.path.join(ROOT, "tramba_amd", "_lib_parent", "libtramba_hip.so")), "new": hip.lib()}
    lines = [f"{torch.cuda.get_device_name(0)}; the LayerNorm family's entries, parent library / this tree's"]

    def finish(code):
        hip._lib = libs["new"]
        print("\n".join(lines))
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(code)

    def cases():
        for dtype in (F32, BF16):
            vm = 4 if dtype == F32 else 8
            for m in MULTS:
                yield Case(dtype, 37, vm * m, 1, (2, 1, 3, 3))
                yield Case(dtype, 4609, vm * m, 11, (2, 1, 1, 1153))
                yield Case(dtype, 37, vm * m, 1, (4, 1, 1, 2))
        for rows, c, side in STAGES:
            yield Case(BF16, rows, c, 4, (2, 4, side, side))

    compared = 0
    for k in cases():
        for name, run in ENTRIES.items():
            if not served(name, k):
                continue
            got = {}
            for lib_name, lib in libs.items():
                hip._lib = lib
                got[lib_name] = run(k)
            torch.cuda.synchronize()
            same = [torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all().item() and torch.equal(a.nan_to_num(), b.nan_to_num())
                    for a, b in zip(got["parent"], got["new"])]
            compared += len(same)
            if len(got["parent"]) != len(got["new"]) or not all(same):
                lines.append(f"{name} at {k.tag}: outputs {[i for i, s in enumerate(same) if not s]} are NOT bit-identical: stopped here")
                finish(1)
    lines.append(f"every entry at every shape of the sweep and at the four stage shapes: {compared} tensors (outputs and partial "
                 "tables), all torch.equal between the parent's library and the new one")

    variants = (("parent", libs["parent"]), ("new", libs["new"]), ("new2", libs["new"]))
    lines.append(f"ms per call under HIP events (bf16, batch 4), {ROUNDS} rounds of {STEPS} calls, parent / new / new2 alternately; "
                 "the order rotates from round to round and a first round is timed and dropped")
    for rows, c, side in STAGES:
        k = Case(BF16, rows, c, 4, (2, 4, side, side))
        for name, run in ENTRIES.items():
            if not served(name, k):
                continue
            fn = lambda: run(k)                                                                          # noqa: E731
            for _, lib in variants:
                hip._lib = lib
                fn()
                fn()
            t = {n: [] for n, _ in variants}
            for r in range(-1, ROUNDS):
                for n, lib in variants[r % 3:] + variants[:r % 3]:
                    hip._lib = lib
                    ms = timed(fn, STEPS)
                    if r >= 0:
                        t[n].append(ms)
            diff = [a - b for a, b in zip(t["new"], t["parent"])]
            spread = statistics.pstdev([a - b for a, b in zip(t["new"], t["new2"])])
            verdict = "SLOWER" if statistics.mean(diff) > 3 * spread else "not slower"
            lines.append(f"{rows:6d} x {c:4d}  {name:34s} parent {statistics.mean(t['parent']):.4f}  new {statistics.mean(t['new']):.4f}  "
                         f"new2 {statistics.mean(t['new2']):.4f}   mean of new - parent {statistics.mean(diff):+.4f}   "
                         f"A/A spread {spread:.4f}   {verdict} by the 3 x rule")
    finish(0)


if __name__ == "__main__":
    main()
