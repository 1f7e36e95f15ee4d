#!/usr/bin/env python3
"""Same-box A/B of the Tramba-V 384x384 batch-4 bf16 forward (BASELINE config 2) between the PARENT commit's library and this
tree's, in the manner of scripts/ab_lib.py:
  * `parent`  tramba_amd/_lib_parent/libtramba_hip.so, built from the parent commit (untracked, never shipped)
  * `new`     the current library
  * `new2`    the current library captured a second time: the spread between two graphs of identical code
Every variant is captured as one hipGraph in ONE process; the graphs are replayed alternately, 20 replays per timing.  The A/A
spread is the standard deviation over the rounds of new - new2; the change counts as a gain if the mean of parent - new exceeds
three times that.  The outputs of the parent's and the new graph are compared bit for bit.
usage: python scripts/ab_parent.py [rounds] [out.txt]   (profiles/stragglers_ab.txt)"""
import os, sys, statistics, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tramba_amd as ta
from tramba_amd import hip
from ab_lib import load, capture


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stragglers_ab.txt")
    new = hip.lib()
    parent = load(os.path.join(ROOT, "tramba_amd", "_lib_parent", "libtramba_hip.so"))
    torch.manual_seed(0)
    m = ta.prepare_inference(ta.bulid_model(deep_supervision=True, use_pretrain=False, img_size=384).cuda().eval(), torch.bfloat16)
    x = torch.randn(4, 3, 384, 384, device="cuda")
    graphs, outs = {}, {}
    for name, l in (("parent", parent), ("new", new), ("new2", new)):
        hip._lib = l
        with torch.no_grad():
            outs[name] = [o.clone() for o in _flat(m(x))]
        graphs[name] = capture(m, x)
    hip._lib = new
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
    lines = ["forward, ms per replay (20 replays per figure), graphs replayed alternately", "round   parent      new     new2   parent-new  new-new2"]
    for i in range(rounds):
        lines.append(f"{i:5d}  {t['parent'][i]:7.4f}  {t['new'][i]:7.4f}  {t['new2'][i]:7.4f}   {t['parent'][i] - t['new'][i]:+8.4f}  {t['new'][i] - t['new2'][i]:+8.4f}")
    gain = [p - n for p, n in zip(t["parent"], t["new"])]
    aa = [n - n2 for n, n2 in zip(t["new"], t["new2"])]
    spread = statistics.pstdev(aa)
    lines.append(f"mean parent {statistics.mean(t['parent']):.4f}  new {statistics.mean(t['new']):.4f}  new2 {statistics.mean(t['new2']):.4f}")
    lines.append(f"A/A spread (std of new - new2 over {rounds} rounds): {spread:.4f} ms;  mean of new - new2: {statistics.mean(aa):+.4f} ms")
    lines.append(f"mean of parent - new: {statistics.mean(gain):+.4f} ms = {statistics.mean(gain) / max(spread, 1e-9):.1f} x the A/A spread "
                 f"({'a gain' if statistics.mean(gain) > 3 * spread else 'inside the noise'} by the 3 x rule)")
    same = [torch.equal(p, n) for p, n in zip(outs["parent"], outs["new"])]
    lines.append(f"outputs of one eager forward, parent library against new, torch.equal per tensor: {same}")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for it in o for t in _flat(it)]


if __name__ == "__main__":
    main()
