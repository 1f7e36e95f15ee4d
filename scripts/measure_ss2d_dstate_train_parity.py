"""Accuracy records of the fused channels-last SS2D training path at d_state 2..16, kept as a file:
  kernel    per case, dtype and gradient of hip.ss2d_scan_bwd_cl (gu, graw, dB, dC, dA_logs, dD, dbias): E32 (the fp32
            restatement's own max-relative error against fp64), the bound tests/test_gpu_ss2d_dstate_train.py asserts, and the
            kernel's measured error; the core cases and the long-memory cases (`slow`, `undamped`, N = 3 and 16);
  module    SS2D (helix, d_state 16) in bf16 under autograd: each parameter gradient's relative L2 error, cosine and norm
            ratio against the fp32 oracle gradient, on the fused path and on the plugin path, same module and inputs.
Writes profiles/ss2d_dstate_train_parity.json (or the path given as the first argument)."""
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scan_memory_cases as smc  # noqa: E402
import ss2d_dstate_cases as sdc  # noqa: E402
import ss2d_dstate_train_cases as tc  # noqa: E402
import tramba_amd as ta  # noqa: E402
from oracle import model as om  # noqa: E402
from tramba_amd import hip, ops  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def kernel_records(dev):
    recs = []

    def add(label, c, gym, ref, e32, dtype, long_memory):
        got, _ = tc.run_bwd(hip, c, gym, dev)
        for out in tc.OUTPUTS:
            bnd = tc.bound(out, dtype, e32[out], stored16=out in ("gu", "graw"), long_memory=long_memory)
            err = smc.rel_errors(got[out], ref[out])[0]
            recs.append(dict(case=label, dtype=str(dtype)[6:], output=out, e32_max=e32[out], bound=bnd, err_max=err, ok=err <= bnd))

    for name in tc.KERNEL_CASES:
        b, h, d, r, fam, n = tc.CORE_CASES[name]
        nt, nseg = hip.ss2d_scan_n_bwd_plan(b, h * h, d, sdc.k_of(fam), n)
        for dtype in (F32, BF16, F16):
            c, gym, ref, e32 = tc.core_e32(name, dtype, F32, nt)
            add(f"{name} N={n} nseg={nseg}", c, gym, ref, e32, dtype, False)
    fam, h, d, r = sdc.MEMORY_SHAPE
    for regime in ("slow", "undamped"):
        for n in (3, 16):
            nt, nseg = hip.ss2d_scan_n_bwd_plan(1, h * h, d, sdc.k_of(fam), n)
            for dtype in (F32, BF16):
                c, gym, ref, e32 = tc.memory_e32(regime, n, dtype, nt)
                add(f"{regime} N={n} helix48 D=32 nseg={nseg}", c, gym, ref, e32, dtype, True)
    return recs


def module_records(dev):
    torch.manual_seed(11)
    m = ta.SS2D(d_model=16, d_state=16, channel_first=True, scan=ops.CrossScan_Line, merge=ops.CrossMerge_Line, k_group=8)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    x16 = torch.randn(1, 16, 24, 24, generator=g).to(BF16)
    leaves = {k_: v.detach().clone().requires_grad_() for k_, v in m.state_dict().items()}
    want = om.ss2d(om.SD(leaves), x16.float(), "helix")
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(13))
    (want * gy).sum().backward()
    m.to(dev)
    recs = []
    for path, on in (("fused", True), ("plugin", False)):
        m.zero_grad(set_to_none=True)
        with ta.fused_dstate_training(on):
            ta.modules.refresh_lowp_shadows(m, BF16)
            (m(x16.to(dev)).float() * gy.to(dev)).sum().backward()
        for name, p in m.named_parameters():
            a, w = p.grad.double().cpu().reshape(-1), leaves[name].grad.double().reshape(-1)
            recs.append(dict(path=path, parameter=name, rel_l2=float((a - w).norm() / w.norm()),
                             cosine=float(a @ w / (a.norm() * w.norm())), norm_ratio=float(a.norm() / w.norm())))
    return recs


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ss2d_dstate_train_parity.json")
    dev = torch.device("cuda")
    kr, mr = kernel_records(dev), module_records(dev)
    torch.cuda.synchronize()
    hip.device_error()
    for r in kr + mr:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    fused = {r["parameter"]: r["rel_l2"] for r in mr if r["path"] == "fused"}
    plugin = {r["parameter"]: r["rel_l2"] for r in mr if r["path"] == "plugin"}
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               rule="kernel: max |got - want| / max |want| within the N = 1 kernel's bounds (3e-4 gu, 5e-4 others in fp32; 3e-2 / "
                    "5e-2 in 16 bit) where E32 uses at most half of them, else and for the long-memory cases 8 x E32 (+ u for a "
                    "16-bit gu / graw); module: fused rel L2 <= 2 x plugin rel L2, cosine >= 0.998, norm ratio within 4 %",
               all_kernel_ok=all(r["ok"] for r in kr),
               worst_fused_over_plugin=max(fused[k_] / plugin[k_] for k_ in fused), kernel=kr, module=mr)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
