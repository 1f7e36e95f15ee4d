"""Host side of SS2D's default configuration (z gate, channels-last interface): construction and state_dict names, the fp64
closed forms of the gate's backward against autograd, and the pointwise bound the GPU tests hold the gate kernels to
(tests/golden/ss2d_gate_cases.py).  No kernel is launched."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointwise_cases as pc
import ss2d_gate_cases as gc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: v if isinstance(v, str) else str(v)[6:]


def _shapes(m, prefix=""):
    return {k[len(prefix):]: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(prefix)}


def test_default_and_gated_configurations_construct_with_the_reference_state_dict():
    import tramba_amd as ta
    from tramba_amd import modules as M
    m = ta.SS2D()                                                     # d_model 96, d_state 16, channels-last, no gate
    assert not m.channel_first and m.disable_z
    assert _shapes(m) == gc.expected_state_dict(96, 16, 4, gated=False)
    assert isinstance(m.in_proj, nn.Linear) and isinstance(m.out_norm, nn.LayerNorm)
    g = ta.SS2D(d_model=32, d_state=3, channel_first=False, disable_z=False, k_group=8, scan=ta.CrossScan_Line,
                merge=ta.CrossMerge_Line)
    assert _shapes(g) == gc.expected_state_dict(32, 3, 8, gated=True)
    assert g.in_proj.weight.shape == (128, 32) and g.out_proj.weight.shape == (32, 64)
    gb = ta.SS2D(d_model=32, d_state=1, channel_first=True, disable_z=False, bias=True, conv_bias=True)
    assert _shapes(gb) == gc.expected_state_dict(32, 1, 4, gated=True, bias=True, conv_bias=True)
    assert type(gb.in_proj) is M.Linear2d and type(g.in_proj) is M.LinearLast and type(g.out_norm) is M.LayerNormLast
    blk = ta.VSSBlock(32, channel_first=False, norm_layer=nn.LayerNorm)
    assert not blk.op.channel_first and blk.op.disable_z and type(blk.norm) is M.LayerNormLast
    want = {"norm.weight": (32,), "norm.bias": (32,), "norm2.weight": (32,), "norm2.bias": (32,),
            "mlp.fc1.weight": (128, 32), "mlp.fc1.bias": (128,), "mlp.fc2.weight": (32, 128), "mlp.fc2.bias": (32,)}
    want.update({"op." + k: v for k, v in gc.expected_state_dict(32, 1, 4, gated=False).items()})
    assert _shapes(blk) == want
    mlp = ta.Mlp(32, 64, channels_first=False)
    assert type(mlp.fc1) is M.LinearLast and _shapes(mlp) == {"fc1.weight": (64, 32), "fc1.bias": (64,), "fc2.weight": (32, 64),
                                                              "fc2.bias": (32,)}
    # what was accepted before is what it was
    old = ta.SS2D(d_model=32, d_state=1, channel_first=True)
    assert type(old.in_proj) is M.Linear2d and type(old.out_norm) is M.LayerNorm2d and old.in_proj.weight.shape == (64, 32)


def test_no_cpu_fallback_in_the_new_layout():
    import tramba_amd as ta
    with pytest.raises(RuntimeError, match="HIP device"):
        ta.SS2D(d_model=16)(torch.zeros(1, 4, 4, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ta.SS2D(d_model=16).in_proj(torch.zeros(1, 4, 4, 16))


def test_closed_forms_of_the_gate_backward_equal_autograd():
    """gn = gp silu(z) gelu'(n), gz = gp gelu(n) silu'(z) in fp64 against autograd through gelu(n) * silu(z) in double, on the
    pair sweep restricted to |x| <= 30 (beyond it both sides are 0 or the identity to the last bit anyway)"""
    n, z = gc.pairs(F32)
    keep = (np.abs(n) <= 30) & (np.abs(z) <= 30)
    n, z = torch.from_numpy(n[keep]).double().requires_grad_(), torch.from_numpy(z[keep]).double().requires_grad_()
    gp = torch.linspace(-2, 2, n.numel(), dtype=torch.float64)
    (F.gelu(n) * F.silu(z) * gp).sum().backward()
    with torch.no_grad():
        gn = gp * gc.FORMULAS["gate_gn"][1](n, z)
        gz = gp * gc.FORMULAS["gate_gz"][1](n, z)
        fwd = gc.FORMULAS["gate_fwd"][1](n, z)
        assert float(pc.err(fwd, F.gelu(n) * F.silu(z)).max()) <= 1e-13
    assert float(pc.err(gn, n.grad).max()) <= 1e-13 and float(pc.err(gz, z.grad).max()) <= 1e-13


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
@pytest.mark.parametrize("formula", list(gc.FORMULAS))
def test_pointwise_rule_on_the_pair_sweep(formula, dtype):
    """the float32 emulation of the documented formula, stored in `dtype`, meets the rule; at most 5 % of the sweep is skipped
    (in fp16 only gelu(1e4) against silu(30) leaves the range); the sigmoid-for-silu fault does not meet it"""
    emu, ref = gc.FORMULAS[formula]
    n, z = gc.pairs(dtype)
    assert len(n) % 8 != 0 and len(n) >= 2 * len(gc.HELD) * len(pc.sweep_for(dtype))
    for t in (n, z):
        assert torch.equal(torch.from_numpy(t).to(dtype).float(), torch.from_numpy(t))
    want = ref(n, z)
    share = gc.skipped_share(formula, dtype)
    assert share <= gc.MAX_SKIPPED, share
    dead = ~torch.isfinite(want.float().to(dtype).float())
    if dtype == F16 and formula == "gate_fwd":
        d = dead.numpy()                              # +1e4 against 30 in either role: 3e5 is past fp16's 65504
        assert bool(dead.any()) and set(zip(n[d].tolist(), z[d].tolist())) == {(1e4, 30.0), (30.0, 1e4)}
    else:
        assert not bool(dead.any())
    with np.errstate(all="ignore"):
        got = torch.from_numpy(np.asarray(emu(n, z), np.float32)).to(dtype)
    res = gc.check(got, want, formula, dtype)
    print(formula, IDS(dtype), f"E32 {gc.e32(formula):.2e} error {res['error']:.2e} bound {res['bound']:.2e} skipped {res['skipped']:.4f}")
    assert res["ok"], res
    if formula == "gate_fwd":
        with np.errstate(all="ignore"):
            bad = torch.from_numpy(np.asarray(gc.fault_sigmoid_gate(n, z), np.float32)).to(dtype)
        assert not gc.check(bad, want, formula, dtype)["ok"]


def test_merge_cases_reach_their_forms_by_the_launchers_rule():
    """the selection rule of csrc/ss2d_fused.hip merge_launch restated: each case lands on the form it is named for, at fp32
    and at 16-bit rows alike"""
    for name, (form, fam, k, b, h, d) in gc.MERGE_CASES.items():
        for ys_f32 in (True, False):
            npix, v = b * h * h, 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1
            need = -(-d // (64 * v))
            nit = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8
            stream = nit <= 2 and k <= 4 and npix >= 8192
            split = not stream and (ys_f32 or k <= 4) and nit >= 4 and npix <= 16384
            assert ("stream" if stream else "split" if split else "deep") == form, (name, ys_f32)
