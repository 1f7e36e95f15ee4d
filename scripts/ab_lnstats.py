#!/usr/bin/env python3
"""Same-box A/B of the Tramba-V 384x384 batch-4 bf16 forward for the row-statistics hand-over (modules.ROW_STATS), by the
protocol of scripts/ab_parent.py:
  * `parent`  tramba_amd/_lib_parent/libtramba_hip.so, built from the parent commit (untracked, never shipped), with the switch
              off -- the parent's library has no row-statistics entries, and with the switch off this tree's Python issues the
              parent's calls
  * `new`     the current library, switch on
  * `new2`    the same, captured a second time: the spread between two graphs of identical code
  * `off`     the current library, switch off (the cost of the change where it is not used)
Every variant is one hipGraph in ONE process; the graphs are replayed alternately, 20 replays per timing.  The A/A spread is
the standard deviation over the rounds of new - new2; the change counts as a gain if the mean of parent - new exceeds three
times that.  The outputs are no longer bit-identical to the parent's (the same sums in another fp32 order): their maximum and
RMS difference is printed per map, relative to the map's RMS.
usage: python scripts/ab_lnstats.py [rounds] [out.txt]   (profiles/lnstats_ab.txt)"""
import os, sys, statistics, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tramba_amd as ta
from tramba_amd import hip, modules
from ab_lib import load, capture
from ab_parent import _flat


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lnstats_ab.txt")
    new = hip.lib()
    parent = load(os.path.join(ROOT, "tramba_amd", "_lib_parent", "libtramba_hip.so"))
    torch.manual_seed(0)
    m = ta.prepare_inference(ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=384).cuda().eval(), torch.bfloat16)
    x = torch.randn(4, 3, 384, 384, device="cuda")
    graphs, outs = {}, {}
    try:
        for name, l, on in (("parent", parent, False), ("new", new, True), ("new2", new, True), ("off", new, False)):
            hip._lib, modules.ROW_STATS = l, on
            with torch.no_grad():
                outs[name] = [o.clone() for o in _flat(m(x))]
            graphs[name] = capture(m, x)
    finally:
        hip._lib, modules.ROW_STATS = new, True
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            g.replay()
            torch.cuda.synchronize()
            a.record()
            for _ in range(20):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(e) / 20)
    lines = ["forward, ms per replay (20 replays per figure), graphs replayed alternately",
             "round   parent      new     new2      off   parent-new  new-new2"]
    for i in range(rounds):
        lines.append(f"{i:5d}  {t['parent'][i]:7.4f}  {t['new'][i]:7.4f}  {t['new2'][i]:7.4f}  {t['off'][i]:7.4f}   "
                     f"{t['parent'][i] - t['new'][i]:+8.4f}  {t['new'][i] - t['new2'][i]:+8.4f}")
    gain = [p - n for p, n in zip(t["parent"], t["new"])]
    aa = [n - n2 for n, n2 in zip(t["new"], t["new2"])]
    spread = statistics.pstdev(aa)
    lines.append("mean " + "  ".join(f"{k} {statistics.mean(v):.4f}" for k, v in t.items()))
    lines.append(f"A/A spread (std of new - new2 over {rounds} rounds): {spread:.4f} ms;  mean of new - new2: {statistics.mean(aa):+.4f} ms")
    lines.append(f"mean of parent - new: {statistics.mean(gain):+.4f} ms = {statistics.mean(gain) / max(spread, 1e-9):.1f} x the A/A spread "
                 f"({'a gain' if statistics.mean(gain) > 3 * spread else 'inside the noise'} by the 3 x rule)")
    lines.append(f"mean of parent - off: {statistics.mean(p - o for p, o in zip(t['parent'], t['off'])):+.4f} ms")
    lines.append(f"outputs of one eager forward, parent against off, torch.equal per tensor: "
                 f"{[torch.equal(p, o) for p, o in zip(outs['parent'], outs['off'])]}")
    for i, (p, n) in enumerate(zip(outs["parent"], outs["new"])):
        d, rms = (p.double() - n.double()), float(p.double().square().mean().sqrt())
        lines.append(f"output {i} {tuple(p.shape)}: parent against new, max |d| {float(d.abs().max()) / rms:.2e}  RMS {float(d.square().mean().sqrt()) / rms:.2e} "
                     f"of the map's RMS")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
