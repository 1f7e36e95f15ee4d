#!/usr/bin/env python3
"""Same-box A/B of the optimizer-step kernels (csrc/loss_optim.hip) between the PARENT commit's library and this tree's, in
the manner of scripts/ab_parent.py:
  * `parent`  tramba_amd/_lib_parent/libtramba_hip.so, built from the parent commit (untracked, never shipped)
  * `new`     the current library
  * `new2`    the current library timed a second time: the spread between two runs of identical code
On the parameter list of Tramba-V (384 x 384 build; the tensors and seeds of scripts/bench_sched_ema.py's optimizer rows), one
process, hip._lib swapped between the calls:
  1. three steps of  grad_accumulate (two micro-batches), grad_norm with a clip, adam_step_ctl on the accumulated gradients
     with the record's scale and skip flag, adam_step_sched with averages  under each library on identically seeded state;
     after every step every parameter, moment, average, accumulator, counter and record must be torch.equal between the
     two.  The first difference ends the script (exit status 1): nothing further is started on the device.
  2. the four operations timed alternately parent / new / new2 under HIP events, ROUNDS rounds of STEPS calls (the order
     rotates from round to round, after one round that is timed and dropped).  The A/A
     spread is the standard deviation over the rounds of new - new2; an operation counts as slower if the mean of
     new - parent exceeds three times that.  Reported, not asserted.
usage: python scripts/ab_step_kernels.py [out.txt]   (profiles/step_kernels_ab.txt)"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tramba_amd as ta                                    # noqa: E402
from tramba_amd import hip                                 # noqa: E402
from ab_lib import load                                    # noqa: E402
from bench_sched_ema import ROUNDS, STEPS, timed           # noqa: E402

HYPER = (1e-4, 0.9, 0.999, 1e-8, 1e-2)


class State:
    """everything the four operations read and write; the same shapes give the same bits"""

    def __init__(self, shapes):
        g = torch.Generator(device="cuda").manual_seed(1)
        new = lambda scale=1.0: [torch.randn(s, device="cuda", generator=g) * scale for s in shapes]     # noqa: E731
        self.micro = [new(0.1) for _ in range(6)]                       # two micro-batches for each of three steps
        self.acc = [torch.full(s, float("nan"), device="cuda") for s in shapes]
        self.ctl, self.f = hip.step_ctl_record("cuda")
        self.sched, _ = hip.step_sched_record("cuda", lr_factor=0.5, ema_weight=1e-3)
        self.sets = []                                                  # [0]: adam_step_ctl's, [1]: adam_step_sched's
        for _ in range(2):
            ps = new()
            self.sets.append({"p": ps, "m": [torch.zeros_like(p) for p in ps], "v": [torch.zeros_like(p) for p in ps],
                              "e": [p.clone() for p in ps], "t": [torch.zeros((), device="cuda") for _ in ps]})
        self.n = len(shapes)
        self.numel = (ctypes.c_int64 * self.n)(*[a.numel() for a in self.acc])
        self.acc_ptrs = hip.pointer_array(self.acc)
        self.ws = torch.empty((hip.grad_norm_workspace(self.numel, self.n) + 7) // 8, dtype=torch.float64, device="cuda")
        self.total = sum(a.numel() for a in self.acc)

    def grad_accumulate(self, k=0):
        hip.grad_accumulate_raw(self.acc_ptrs, hip.pointer_array(self.micro[k]), self.numel, self.n, self.ctl)

    def grad_norm(self):
        hip.grad_norm_raw(self.acc_ptrs, self.numel, self.n, 0.5, 1.0, True, self.ctl, self.ws)

    def _adam(self, which, **kw):
        s = self.sets[which]
        hip.adam_step_raw(hip.pointer_array(s["p"]), self.acc_ptrs, hip.pointer_array(s["m"]), hip.pointer_array(s["v"]),
                          hip.pointer_array(s["t"]), self.numel, self.n, *HYPER, **kw)

    def adam_step_ctl(self):
        self._adam(0, gscale=self.f["scale"], skip=self.f["skip"])

    def adam_step_sched(self):
        self._adam(1, gscale=self.f["scale"], skip=self.f["skip"], ema=hip.pointer_array(self.sets[1]["e"]), sched=self.sched)

    def step(self, k):
        self.grad_accumulate(2 * k)
        self.grad_accumulate(2 * k + 1)
        self.grad_norm()                                                # (the record's micro counter returns to 0)
        self.adam_step_ctl()
        self.adam_step_sched()

    def tensors(self):
        out = {"accumulator": self.acc, "step_ctl record": [self.ctl], "step_sched record": [self.sched]}
        for tag, s in zip(("ctl", "sched"), self.sets):
            out.update({f"{tag} parameter": s["p"], f"{tag} exp_avg": s["m"], f"{tag} exp_avg_sq": s["v"], f"{tag} counter": s["t"]})
        out["sched average"] = self.sets[1]["e"]
        return out


OPS = ("grad_accumulate", "grad_norm", "adam_step_ctl", "adam_step_sched")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "step_kernels_ab.txt")
    libs = {"parent": load(os.path.join(ROOT, "tramba_amd", "_lib_parent", "libtramba_hip.so")), "new": hip.lib()}
    torch.manual_seed(1026)
    full = ta.bulid_model(use_pretrain=False, img_size=384).cuda().train()
    shapes = [tuple(p.shape) for p in full.parameters()]
    del full
    torch.cuda.empty_cache()
    states = {name: State(shapes) for name in libs}
    lines = [f"{torch.cuda.get_device_name(0)}; {states['new'].n} tensors, {states['new'].total} elements (Tramba-V, 384 x 384 build)"]

    def finish(code):
        hip._lib = libs["new"]
        print("\n".join(lines))
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(code)

    for k in range(3):
        before = [s["p"][0].clone() for s in states["new"].sets]       # (a step that changed nothing would compare equal too)
        for name, lib in libs.items():
            hip._lib = lib
            states[name].step(k)
        torch.cuda.synchronize()
        a, b = states["parent"].tensors(), states["new"].tensors()
        differ = {what: sum(not torch.equal(x, y) for x, y in zip(a[what], b[what])) for what in a}
        moved = all(not torch.equal(x, y) for x, y in zip(before, (b["ctl parameter"][0], b["sched parameter"][0])))
        lines.append(f"step {k}: tensors that differ between parent and new, torch.equal per tensor: {differ}; "
                     f"norm {float(states['new'].f['norm'])!r} scale {float(states['new'].f['scale'])!r} "
                     f"skip {int(states['new'].f['skip'])}")
        if any(differ.values()) or not moved:
            lines.append("NOT bit-identical (or a step that moved nothing): stopped here")
            finish(1)
    lines.append("three steps of every operation: bit-identical between the parent's library and the new one")

    st = states["new"]
    variants = (("parent", libs["parent"]), ("new", libs["new"]), ("new2", libs["new"]))
    lines.append(f"ms per call under HIP events, {ROUNDS} rounds of {STEPS} calls, parent / new / new2 alternately; the order "
                 "rotates from round to round and a first round is timed and dropped (the first window after a pause runs "
                 "faster, whichever library it holds)")
    for op in OPS:
        fn = getattr(st, op)
        for _, lib in variants:
            hip._lib = lib
            fn()
            fn()
        t = {name: [] for name, _ in variants}
        for r in range(-1, ROUNDS):
            for name, lib in variants[r % 3:] + variants[:r % 3]:
                hip._lib = lib
                ms = timed(fn, STEPS)
                if r >= 0:
                    t[name].append(ms)
        diff = [n - p for n, p in zip(t["new"], t["parent"])]
        aa = [n - n2 for n, n2 in zip(t["new"], t["new2"])]
        spread = statistics.pstdev(aa)
        verdict = "SLOWER" if statistics.mean(diff) > 3 * spread else "not slower"
        lines.append(f"{op:16s} parent {statistics.mean(t['parent']):.4f}  new {statistics.mean(t['new']):.4f}  "
                     f"new2 {statistics.mean(t['new2']):.4f}   mean of new - parent {statistics.mean(diff):+.4f}   "
                     f"A/A spread (std of new - new2) {spread:.4f}   {verdict} by the 3 x rule")
        lines.append(f"{'':16s} rounds, parent: {[round(x, 4) for x in t['parent']]}  new: {[round(x, 4) for x in t['new']]}  "
                     f"new2: {[round(x, 4) for x in t['new2']]}")
    finish(0)


if __name__ == "__main__":
    main()
