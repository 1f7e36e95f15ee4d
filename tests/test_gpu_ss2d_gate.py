"""SS2D in its default configuration on the device: the z gate (disable_z=False) and the channels-last interface
(channel_first=False).  Kernel level: the gated merge + out_norm + GELU in its three forms, the gated dual-store LayerNorm and
the gate backward, held to the pointwise rule of tests/golden/ss2d_gate_cases.py (sized in tests/test_ss2d_gate_host.py).
Module level: forward and gradients against the oracle composition (oracle.ops + F.silu / F.gelu), 16-bit parity of the fused
path against the plugin path, reproducibility, graph capture, and the launches the gate adds."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import pointwise_cases as pc
import ss2d_gate_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: v if isinstance(v, str) else str(v)[6:]
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
WRITE = os.environ.get("TRAMBA_WRITE_PROFILES") == "1"
EPS = 1e-5


def hip():
    from tramba_amd import hip as h
    return h


def _update_profile(name, fn):
    path = os.path.join(PROFILES, name)
    rec = json.load(open(path)) if os.path.exists(path) else {}
    fn(rec)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


def _kernels_of(fn):
    """(result, kernel names launched by fn())"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [ev.key for ev in prof.key_averages() if not ev.key.startswith("hip")]


# ----------------------------------------------------------------------------- kernel 1a
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
@pytest.mark.parametrize("name", list(gc.MERGE_CASES))
def test_gated_merge_in_each_form(name, dtype):
    """y = gelu(LayerNorm(merge(ys))) * silu(zpre) against n32 * silu64(zpre), n32 = the UNGATED kernel's fp32 output on the same
    operand values (ys on multiples of 1/32: exact in every dtype, sums exact in any order): the epilogue alone, by the
    pointwise rule.  The kernel that ran is the gated one of the form the case is named for.  fp32: with zpre = 64 the gate is
    exactly 64 (exp(-64) vanishes against 1), so y / 64 must equal n32 bit for bit -- same form, same order."""
    H = hip()
    form, fam, k, b, h, d = gc.MERGE_CASES[name]
    ys, ln_w, ln_b, zpre = gc.merge_operands(name, dtype)
    order = H.scan_order(fam, h, h, torch.device(DEV))
    assert order.k == k
    w, bb = ln_w.to(DEV), ln_b.to(DEV)
    n32 = H.ss2d_merge_norm_cl(ys.to(DEV), order, w, bb, EPS, H.ACT_GELU, F32)
    ys_d, z_d = ys.to(DEV, dtype), zpre.to(DEV, dtype)
    assert torch.equal(ys_d.float().cpu(), ys) and torch.equal(z_d.float().cpu(), zpre)
    got, names = _kernels_of(lambda: H.ss2d_merge_norm_gate_cl(ys_d, order, w, bb, z_d, EPS, H.ACT_GELU, dtype))
    H.device_error()
    assert got.dtype == dtype and got.shape == (b, h * h, d)
    assert len(names) == 1 and f"ss2d_merge_norm_{form}_gate_kernel" in names[0], names
    want = n32.double().cpu() * pc.ref_silu(zpre)
    res = gc.check(got, want, "gate_fwd", dtype)
    print(name, IDS(dtype), f"error {res['error']:.2e} bound {res['bound']:.2e} skipped {res['skipped']:.4f}")
    assert res["ok"] and res["skipped"] <= gc.MAX_SKIPPED, res
    if dtype == F32:
        n_again, ungated = _kernels_of(lambda: H.ss2d_merge_norm_cl(ys_d, order, w, bb, EPS, H.ACT_GELU, F32))
        assert len(ungated) == 1 and f"ss2d_merge_norm_{form}_kernel" in ungated[0], ungated
        assert torch.equal(n_again, n32)
        got64 = H.ss2d_merge_norm_gate_cl(ys_d, order, w, bb, torch.full_like(z_d, 64.0), EPS, H.ACT_GELU, F32)
        assert torch.equal(got64 / 64, n32)
        H.device_error()


def test_gated_merge_rejects_what_it_does_not_do():
    H = hip()
    order = H.scan_order("raster", 12, 12, torch.device(DEV))
    ys = torch.zeros(1, 4, 144, 32, device=DEV)
    w = torch.ones(32, device=DEV)
    z = torch.zeros(1, 144, 32, device=DEV)
    with pytest.raises(H.TrambaHipError, match="merge-only"):
        H.ss2d_merge_norm_gate_cl(ys, order, w, w, z, -1.0, H.ACT_GELU, F32)
    with pytest.raises(H.TrambaHipError, match="gate"):
        H.ss2d_merge_norm_gate_cl(ys, order, w, w, z.to(BF16), EPS, H.ACT_GELU, F32)
    with pytest.raises(H.TrambaHipError, match="gate"):
        H.ss2d_merge_norm_gate_cl(ys, order, w, w, z[:, :100].contiguous(), EPS, H.ACT_GELU, F32)
    with pytest.raises(H.TrambaHipError):
        H.gelu_gate_bwd_cl(z, z, z.to(BF16))
    with pytest.raises(H.TrambaHipError, match="dual"):
        H.add_layernorm_cl(z, None, None, w, w, EPS, H.ACT_GELU, dual=False, gate=z)


# ----------------------------------------------------------------------------- kernels 1b, 1c
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
def test_gate_backward_on_the_pair_sweep(dtype):
    """gn and gz of tramba_gelu_gate_bwd_cl on every (n, z) pair of the sweep, count % 8 != 0, incoming gradient 2 (exact)"""
    H = hip()
    n, z = gc.pairs(dtype)
    assert len(n) % 8 != 0
    nd, zd = torch.from_numpy(n).to(DEV, dtype), torch.from_numpy(z).to(DEV, dtype)
    gn, gz = H.gelu_gate_bwd_cl(torch.full_like(nd, 2.0), nd, zd)
    H.device_error()
    for got, formula in ((gn, "gate_gn"), (gz, "gate_gz")):
        res = gc.check(got, 2.0 * gc.FORMULAS[formula][1](n, z), formula, dtype)
        print(formula, IDS(dtype), f"error {res['error']:.2e} bound {res['bound']:.2e} at n = {n[res['worst']]} z = {z[res['worst']]}")
        assert res["ok"] and res["skipped"] <= gc.MAX_SKIPPED, (formula, res)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
def test_gated_dual_store_layernorm(dtype):
    """the gated form of add_layernorm_cl: with a zero LayerNorm weight n IS the bias, so p = gelu(bias[c]) * silu(z[row, c])
    covers the pair sweep in both roles (a row as wide as the sweep: the wave form; 48 channels: the rows form); and with
    random operands, a residual add and a mask, xsum and n equal the ungated launch's bit for bit while the second output is
    gelu(n) * silu(z) of the n that was stored"""
    H = hip()
    sw = pc.sweep_for(dtype)
    held = np.asarray(gc.HELD, np.float32)
    g = torch.Generator().manual_seed(5)
    roles = [(torch.from_numpy(sw), torch.from_numpy(held)[:, None].expand(len(held), len(sw))),
             (torch.from_numpy(np.resize(held, 48)), torch.from_numpy(sw)[:, None].expand(len(sw), 48))]
    for bias, z in roles:
        rows, c = z.shape
        x = torch.randn(rows, c, generator=g).to(DEV, dtype)
        zd = z.contiguous().to(DEV, dtype)
        w0 = torch.zeros(c, device=DEV)
        _, n, p = H.add_layernorm_cl(x, None, None, w0, bias.to(DEV), EPS, H.ACT_GELU, dual=True, gate=zd)
        _, n0, _ = H.add_layernorm_cl(x, None, None, w0, bias.to(DEV), EPS, H.ACT_GELU, dual=True)
        H.device_error()
        assert torch.equal(n, n0) and torch.equal(n.float().cpu(), bias[None].expand(rows, c))
        res = gc.check(p, gc.FORMULAS["gate_fwd"][1](bias[None].expand(rows, c).numpy(), z.numpy()), "gate_fwd", dtype)
        print(IDS(dtype), c, f"error {res['error']:.2e} bound {res['bound']:.2e} skipped {res['skipped']:.4f}")
        assert res["ok"] and res["skipped"] <= gc.MAX_SKIPPED, res
    for c in (40, 316):
        x, y = (torch.randn(3, 7, c, generator=g).to(DEV, dtype) for _ in range(2))
        z = torch.randn(3, 7, c, generator=g).mul(2).to(DEV, dtype)
        w, b = (1 + 0.2 * torch.randn(c, generator=g)).to(DEV), (0.3 * torch.randn(c, generator=g)).to(DEV)
        mask = torch.tensor([1.25, 0.0, 1.25], device=DEV)
        xs, n, p = H.add_layernorm_cl(x, y, mask, w, b, EPS, H.ACT_GELU, dual=True, gate=z)
        xs0, n0, a0 = H.add_layernorm_cl(x, y, mask, w, b, EPS, H.ACT_GELU, dual=True)
        H.device_error()
        assert torch.equal(xs, xs0) and torch.equal(n, n0)
        # (from n as stored, in fp64: the ungated second output carries a rounding of its own)
        res = gc.check(p, gc.FORMULAS["gate_fwd"][1](n.float().cpu().numpy(), z.float().cpu().numpy()), "gate_fwd", dtype)
        assert res["ok"], res
        assert gc.check(a0, pc.ref_gelu(n.float().cpu().numpy()), "gate_fwd", dtype)["ok"]


# ----------------------------------------------------------------------------- module forward
@functools.lru_cache(maxsize=None)
def _forward_reference(n, family, gated):
    m = gc.make_ss2d(n, family, True, gated)
    x = gc.make_input()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return sd, x, gc.oracle_ss2d(sd, x, family)


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
@pytest.mark.parametrize("family", ["raster", "helix"])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_forward_matches_the_oracle_in_both_layouts(n, family, gated):
    """fp32 inference, d_model 32, 12 x 12, batch 2: rtol 1e-3 / atol 1e-4 against the oracle composition; the channels-last
    module's output is the channel-first module's, permuted, bit for bit; a direct call of in_proj / out_norm / out_proj has
    the last-dim semantics of nn.Linear / nn.LayerNorm"""
    import torch.nn.functional as F
    sd, x, want = _forward_reference(n, family, gated)
    outs = {}
    for cf in (True, False):
        m = gc.make_ss2d(n, family, cf, gated)
        m.load_state_dict(sd)
        m.to(DEV).eval()
        xin = x.to(DEV) if cf else x.permute(0, 2, 3, 1).contiguous().to(DEV)
        with torch.no_grad():
            out = m(xin)
        outs[cf] = out if cf else out.permute(0, 3, 1, 2)
        assert out.shape == xin.shape
        if not cf:
            with torch.no_grad():
                t = m.in_proj(xin)
                assert t.shape == xin.shape[:-1] + ((2 if gated else 1) * m.d_inner,)
                np.testing.assert_allclose(t.cpu().numpy(), F.linear(xin.cpu(), sd["in_proj.weight"]).numpy(), rtol=1e-3, atol=1e-4)
                u = t[..., :m.d_inner].contiguous()
                np.testing.assert_allclose(m.out_norm(u).cpu().numpy(),
                                           F.layer_norm(u.cpu(), (m.d_inner,), sd["out_norm.weight"], sd["out_norm.bias"]).numpy(),
                                           rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(m.out_proj(u).cpu().numpy(), F.linear(u.cpu(), sd["out_proj.weight"]).numpy(),
                                           rtol=1e-3, atol=1e-4)
    hip().device_error()
    np.testing.assert_allclose(outs[True].cpu().numpy(), want.numpy(), rtol=1e-3, atol=1e-4)
    assert torch.equal(outs[False], outs[True])


def test_vssblock_and_mlp_channels_last():
    """VSSBlock(channel_first=False, norm_layer=nn.LayerNorm) and Mlp(channels_first=False) equal their channel-first twins on
    the permuted map, bit for bit (fp32 and bf16 inference), and train"""
    import tramba_amd as ta
    x = gc.make_input()
    for dtype in (F32, BF16):
        torch.manual_seed(3)
        a = ta.VSSBlock(32, channel_first=True, ssm_d_state=16).to(DEV, dtype).eval()
        b = ta.VSSBlock(32, channel_first=False, norm_layer=torch.nn.LayerNorm, ssm_d_state=16).to(DEV, dtype).eval()
        b.load_state_dict(a.state_dict())
        xc = x.to(DEV, dtype)
        xl = xc.permute(0, 2, 3, 1).contiguous()
        with torch.no_grad():
            assert torch.equal(b(xl).permute(0, 3, 1, 2), a(xc))
            assert torch.equal(b.mlp(xl).permute(0, 3, 1, 2), a.mlp(xc))
    b.train()
    xg = xl.clone().requires_grad_()
    b(xg).float().square().mean().backward()
    assert xg.grad.shape == xl.shape and bool(torch.isfinite(xg.grad.float()).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in b.parameters())
    hip().device_error()


# ----------------------------------------------------------------------------- gradients
class _Spy:
    def __init__(self, monkeypatch, owner, name, fail=False, static=False):
        self.calls = 0
        orig = getattr(owner, name)

        def wrapped(*a, **kw):
            self.calls += 1
            if fail:
                raise AssertionError(f"{name} was called")
            return orig(*a, **kw)

        monkeypatch.setattr(owner, name, staticmethod(wrapped) if static else wrapped)


def _run_gated(m, x_cl, gy_cl, switch):
    import tramba_amd as ta
    m.zero_grad(set_to_none=True)
    xg = x_cl.clone().requires_grad_()
    with ta.fused_dstate_training(switch):
        out = m(xg)
        (out.float() * gy_cl).sum().backward()
    grads = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}
    grads["x"] = xg.grad.detach().float().cpu().permute(0, 3, 1, 2)
    return out.detach().float().cpu().permute(0, 3, 1, 2), grads


GRAD_CASES = {"plugin_n3": ("plugin", 3, "raster"), "fused_n1": ("fused", 1, "helix"), "fused_n3": ("fused", 3, "raster"),
              "fused_n16": ("fused", 16, "helix")}


@pytest.mark.parametrize("case", list(GRAD_CASES))
def test_gradients_match_autograd_through_the_oracle(case, monkeypatch):
    """fp32, the gated channels-last module: the output to rtol 1e-3 / atol 1e-4, the input gradient and every parameter
    gradient (in_proj.weight's x half and z half separately) to a relative L2 of 1e-3 -- on the plugin path (N = 3, switch off),
    on the fused path at N = 1, and at N = 3 / 16 with the switch on (SelectiveScanOflex.apply patched to raise there)"""
    from tramba_amd import ops
    path, n, family = GRAD_CASES[case]
    m = gc.make_ss2d(n, family, False, True)
    x = gc.make_input()
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(13))
    want, wgrads = gc.oracle_with_grads(m, x, family, gy)
    m.to(DEV)
    plugin = _Spy(monkeypatch, ops.SelectiveScanOflex, "apply", fail=path == "fused", static=True)
    gate_bwd = _Spy(monkeypatch, hip(), "gelu_gate_bwd_cl")
    got, grads = _run_gated(m, x.permute(0, 2, 3, 1).contiguous().to(DEV), gy.permute(0, 2, 3, 1).contiguous().to(DEV),
                            switch=path == "fused")
    hip().device_error()
    assert (plugin.calls, gate_bwd.calls) == ((1, 0) if path == "plugin" else (0, 1))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-4)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    di = m.d_inner
    g, w = gc.split_in_proj(grads, di), gc.split_in_proj(wgrads, di)
    assert set(g) == set(w)
    errs = {k: rel(g[k], w[k]) for k in w}
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-3, errs


# ----------------------------------------------------------------------------- 16 bit
@pytest.mark.parametrize("dtype", [BF16, F16], ids=IDS)
@pytest.mark.parametrize("n", [1, 16])
def test_sixteen_bit_parity_of_the_fused_and_plugin_paths(n, dtype, monkeypatch):
    """16-bit activations, fp32 parameters, fp32 oracle on the rounded input (helix K = 8).  The plugin-gated path meets the
    project's bf16 criteria on the output and on every gradient (cosine >= 0.998, norm within 4 %); the fused-gated path's
    relative L2 error is at most twice the plugin-gated path's on the output and on every parameter gradient.  (N = 1 has no
    switch: the plugin path is reached there by turning the module's two fused-path predicates off.)"""
    import tramba_amd as ta
    from tramba_amd import modules as M
    family = "helix"
    m = gc.make_ss2d(n, family, False, True)
    x16 = gc.make_input().to(dtype)
    gy = torch.randn(x16.shape, generator=torch.Generator().manual_seed(13))
    want, wgrads = gc.oracle_with_grads(m, x16.float(), family, gy)
    m.to(DEV)
    xd, gd = x16.permute(0, 2, 3, 1).contiguous().to(DEV), gy.permute(0, 2, 3, 1).contiguous().to(DEV)
    stats = {}
    for path in ("fused", "plugin"):
        with monkeypatch.context() as mp:
            if path == "plugin":
                mp.setattr(M.SS2D, "_train_path_ok", lambda self, x: False)
                mp.setattr(M.SS2D, "_train_fused_ok", lambda self, x: False)
            spy = _Spy(mp, hip(), "gelu_gate_bwd_cl")
            ta.modules.refresh_lowp_shadows(m, dtype)
            out, grads = _run_gated(m, xd, gd, switch=path == "fused")
            assert spy.calls == (1 if path == "fused" else 0)
        grads["out"], ref = out, dict(wgrads, out=want)
        stats[path] = {}
        for k, w in ref.items():
            g, w = grads[k].double().reshape(-1), w.double().reshape(-1)
            stats[path][k] = (float((g - w).norm() / w.norm()), float(g @ w / (g.norm() * w.norm())), float(g.norm() / w.norm()))
    hip().device_error()
    ratios = {k: stats["fused"][k][0] / stats["plugin"][k][0] for k in stats["fused"] if k != "x"}
    for k in stats["fused"]:
        f, p = stats["fused"][k], stats["plugin"][k]
        print(n, IDS(dtype), k, f"fused rel L2 {f[0]:.2e} cos {f[1]:.5f} norm {f[2]:.4f}; plugin rel L2 {p[0]:.2e} cos {p[1]:.5f} norm {p[2]:.4f}")
    if WRITE:
        _update_profile("ss2d_gate_parity.json", lambda rec: rec.setdefault("cases", {}).update({f"{IDS(dtype)}_n{n}": dict(
            fused={k: v[0] for k, v in stats["fused"].items()}, plugin={k: v[0] for k, v in stats["plugin"].items()},
            ratio=ratios, plugin_cosine={k: v[1] for k, v in stats["plugin"].items()},
            plugin_norm={k: v[2] for k, v in stats["plugin"].items()})}))
    bad = {k: v for k, v in stats["plugin"].items() if v[1] < 0.998 or abs(v[2] - 1) > 0.04}
    assert not bad, ("plugin", bad)
    assert max(ratios.values()) <= 2.0, ratios


# ----------------------------------------------------------------------------- reproducibility and capture
def _gated_block(dim, n, seed):
    import tramba_amd as ta
    torch.manual_seed(seed)
    blk = ta.VSSBlock(hidden_dim=dim, ssm_d_state=n, channel_first=True, drop_path=0.0)
    blk.op = ta.SS2D(d_model=dim, d_state=n, channel_first=True, disable_z=False)
    return blk


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
def test_fused_gated_steps_are_bitwise_reproducible(dtype, monkeypatch):
    """two forward + backward passes of a gated VSSBlock (N = 16, switch on: the deferred residual stream, unchanged) from the
    same state give equal outputs and gradients bit for bit, every parameter with a finite gradient, no plugin path"""
    import tramba_amd as ta
    from tramba_amd import ops
    m = _gated_block(32, 16, 21).to(DEV, dtype)
    x = gc.make_input(22).to(DEV, dtype)
    _Spy(monkeypatch, ops.SelectiveScanOflex, "apply", fail=True, static=True)
    runs = []
    with ta.fused_dstate_training(True):
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_()
            y = m(xg)
            y.float().square().mean().backward()
            for name, p in m.named_parameters():
                assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad.float()).all()), name
            runs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    hip().device_error()


def test_graphed_forward_of_a_gated_stack_equals_eager():
    import tramba_amd as ta
    m = torch.nn.Sequential(_gated_block(32, 16, 23), _gated_block(32, 1, 24)).to(DEV, BF16).eval()
    x = gc.make_input(25, h=24).to(DEV, BF16)
    with torch.no_grad():
        eager = m(x).clone()
    graphed = ta.GraphedForward(m, strict=True)
    first = graphed(x).clone()
    second = graphed(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(eager, first) and torch.equal(first, second) and bool(torch.isfinite(eager.float()).all())
    hip().device_error()


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 32, 1)
        self.block = _gated_block(32, 16, 61)
        self.head = torch.nn.Conv2d(32, 1, 1)
        self.compute_dtype = BF16

    def forward(self, x):
        return [self.head(self.block(self.stem(x).to(BF16)).float())]


def test_graphed_train_step_with_a_gated_block():
    """GraphedTrainStep captures a model holding a gated block (bf16, N = 16, switch on); its first loss equals the eager
    step's to rel 1e-5, and two captures from the same state replay to equal losses"""
    import tramba_amd as ta
    from tramba_amd import train
    x = torch.randn(2, 3, 24, 24, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = (torch.rand(2, 1, 24, 24, generator=torch.Generator().manual_seed(1)) > 0.6).float().to(DEV)
    state = {k: v.clone() for k, v in _Tiny().state_dict().items()}

    def fresh():
        m = _Tiny().to(DEV).train()
        m.load_state_dict(state)
        return m

    with ta.fused_dstate_training(True):
        m = fresh()
        eager = float(train.train_step(m, train.get_opt(1e-3, m), x, y))
        runs = []
        for _ in range(2):
            m = fresh()
            step = ta.GraphedTrainStep(m, train.get_opt(1e-3, m, capturable=True))
            runs.append([float(step(x, y)) for _ in range(2)])
            torch.cuda.synchronize()
    print("eager", eager, "graphed", runs)
    assert abs(runs[0][0] - eager) <= 1e-5 * abs(eager) and runs[0] == runs[1]
    hip().device_error()


# ----------------------------------------------------------------------------- launches
LAUNCH_PROFILE = os.path.join(PROFILES, "ss2d_gate_launches.json")


@functools.lru_cache(maxsize=None)
def _launches(case, gated):
    import tramba_amd as ta
    with ta.fused_dstate_training(True):
        return gc.module_launches(gc.LAUNCH_CASES[case], gated, DEV)


@pytest.mark.parametrize("case", list(gc.LAUNCH_CASES))
def test_launches_the_gate_adds(case):
    """one forward + backward of the gated fused module against the ungated one (bf16): every kernel NAME only the gated run
    launches is the library's own (no matrix multiply, mul, silu, sigmoid or add of the framework); at most 7 more launches
    outside the copy and fill classes (the z-half GEMM, the gate backward, a weight-gradient GEMM and partial sums), at most
    2 more copies and 1 more fill"""
    got, base = _launches(case, True), _launches(case, False)
    for name in sorted(got):
        print(case, got[name], base.get(name, 0), name[:160])
    new = [k for k in got if k not in base]
    assert new and all("tramba::" in k for k in new), new
    assert any("gelu_gate_bwd_kernel" in k for k in new) and any("add_ln_" in k and "_gate_kernel" in k for k in new)
    by_class = lambda c: {cls: sum(v for k, v in c.items() if gc.launch_class(k) == cls) for cls in ("copy", "fill", "other")}  # noqa: E731
    g, b = by_class(got), by_class(base)
    if WRITE:
        _update_profile("ss2d_gate_launches.json", lambda rec: rec.setdefault("head", {}).update(
            {case: dict(gated=got, ungated=base, gated_by_class=g, ungated_by_class=b)}))
    assert g["other"] - b["other"] <= 7 and g["copy"] - b["copy"] <= 2 and g["fill"] - b["fill"] <= 1, (g, b)


@pytest.mark.parametrize("case", list(gc.LAUNCH_CASES))
def test_ungated_launches_equal_the_parent_commits(case):
    """the ungated module's launches, name by name, are what the same counting code gave on the parent commit
    (profiles/ss2d_gate_launches.json, "parent")"""
    with open(LAUNCH_PROFILE) as f:
        want = json.load(f)["parent"][case]
    got = _launches(case, False)
    assert got == want, {k: (got.get(k, 0), want.get(k, 0)) for k in set(got) | set(want) if got.get(k, 0) != want.get(k, 0)}
