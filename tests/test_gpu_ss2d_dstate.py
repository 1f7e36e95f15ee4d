"""The fused channels-last SS2D scan at d_state N = 2..16 (hip.ss2d_scan_n_cl, ss2d_seg_n_kernel) and the modules that now
reach it under torch.no_grad(), against the fp64 oracle.  tests/test_ss2d_dstate_host.py shows, on the CPU and on these very
inputs, that fp32 arithmetic in the kernel's documented form uses at most 0.37 of the core tolerances (rtol = atol = 2e-4 for
fp32, 4e-2 for 16-bit, measured after merge + out_norm + GELU as tests/test_gpu_kernels.py::test_ss2d_fused_core does).

The core cases decay by 0.6 .. 0.9 per position: the state dies inside a tile, and a lost segment carry would go unseen there.
test_state_outlives_the_segments uses the `slow` and `undamped` regimes of tests/golden/scan_memory_cases.py with A and (B, C)
extended to N columns, where the state crosses all 36 segments, under that module's rule: an fp32 output within 8 x E32 of the
fp64 reference on the max- and the RMS-relative measure, a 16-bit output with every element within u |want| + (that bound)
max |want|."""
import numpy as np
import pytest
import torch

import buffer_cases as bc
import ss2d_dstate_cases as sdc
from oracle import model as om

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: v if isinstance(v, str) else str(v)[6:]


def hip():
    from tramba_amd import hip as h
    return h


def _core_args(c, dev):
    H = hip()
    order = H.scan_order(c.fam, c.h, c.h, dev)
    xc = c.x.permute(0, 2, 3, 1).contiguous().view(c.b, c.l, c.d).to(dev)
    xdbl = H.linear_cl(xc, H.pad_x_proj_weight(c.wx.to(dev), c.n), out_dtype=F32)
    return xc, xdbl, order, c.wdt.to(dev), c.dtb.reshape(-1).to(dev), c.a_neg.to(dev), c.ds.to(dev)


# ----------------------------------------------------------------------------- kernel against oracle
def test_the_cases_reach_the_paths_they_are_named_for():
    H = hip()
    plans = {name: H.ss2d_scan_n_plan(b, h * h, d, sdc.k_of(fam), n) for name, (b, h, d, r, fam, n) in sdc.CORE_CASES.items()}
    tiles = {name: (h * h + 31) // 32 for name, (b, h, d, r, fam, n) in sdc.CORE_CASES.items()}
    assert plans["single_launch"][1] == 1 and plans["single_launch"][0] > tiles["single_launch"]     # one launch, a padding tile
    assert plans["rank40"][1] == 1
    assert 1 < plans["segments_k8"][1] and sdc.CORE_CASES["segments_k8"][2] > 32                      # two channel tiles
    assert plans["d40_window"][1] > 1 and plans["d40_dilation"][1] > 1
    nt, nseg = plans["ragged_r1"]
    assert nseg > 1 and nt * nseg > tiles["ragged_r1"] and 14 * 14 % 32 != 0      # the last segment ends in a padding tile
    assert plans["fold_unrolled"][1] > 16                                         # two rounds of the 8-wide fold and a remainder
    assert plans["rank64"][1] > 1
    for name, (b, h, d, r, fam, n) in sdc.CORE_CASES.items():
        assert (r + 15) // 16 == {"rank40": 3, "rank64": 4}.get(name, 1), name


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
@pytest.mark.parametrize("name", list(sdc.CORE_CASES), ids=IDS)
def test_scan_against_the_oracle(name, dtype):
    """per-direction ys against oracle.ops.ss2d_core(merge=False) in fp64, then merge + out_norm + GELU: rtol = atol = 2e-4
    (fp32) / 4e-2 (16-bit activations, 16-bit and fp32 ys)"""
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_case(sdc.CORE_CASES[name], dtype)
    args = _core_args(c, dev)
    tol = sdc.CORE_TOL[dtype]
    scale = float(c.ys_want.abs().max())
    for ys_dtype in ([F32] if dtype == F32 else [F32, dtype]):
        ys = H.ss2d_scan_n_cl(*args, ys_dtype)
        assert ys.dtype == ys_dtype and ys.shape == (c.b, c.k, c.l, c.d)
        out = H.ss2d_merge_norm_cl(ys, args[2], c.lw.to(dev), c.lb.to(dev), 1e-5, 2, dtype)
        torch.cuda.synchronize()
        H.device_error()
        err = float((ys.cpu().double() - c.ys_want).abs().max()) / scale
        got = out.view(c.b, c.h, c.h, c.d).cpu().double()
        print(name, IDS(dtype), "ys", IDS(ys_dtype), f"ys max err / max |ys| {err:.2e}; share of the tolerance used "
              f"{sdc.tolerance_share(got, c.want, tol):.3f}")
        assert bool(torch.isfinite(ys.float()).all())
        if dtype != F32:      # ys itself, the figure of test_ss2d_lds_dma_scan_at_the_benchmarked_launches for 16-bit maps
            assert err <= 2e-2
        np.testing.assert_allclose(got.numpy(), c.want.numpy(), rtol=tol, atol=tol)


def test_shape_checks_name_the_layout():
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_case(sdc.SINGLE_PASS, F32)
    xc, xdbl, order, wdt, dtb, a_neg, ds = _core_args(c, dev)
    with pytest.raises(H.TrambaHipError, match=r"K\*RG\(R, N\)"):
        H.ss2d_scan_n_cl(xc, xdbl[..., :-4].contiguous(), order, wdt, dtb, a_neg, ds)
    with pytest.raises(H.TrambaHipError, match="ss2d_scan_cl"):
        H.ss2d_scan_n_cl(xc, xdbl, order, wdt, dtb, a_neg[:, :1].contiguous(), ds)        # N = 1 belongs to the other entry
    with pytest.raises(H.TrambaHipError, match=r"\(K\*D, N\)"):
        H.ss2d_scan_n_cl(xc, xdbl, order, wdt, dtb, a_neg.reshape(-1), ds)


# ----------------------------------------------------------------------------- state outlives the segments
@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_state_outlives_the_segments(regime, n, dtype):
    """helix 48 x 48, D = 32: 72 tiles in 36 segments.  fp32 ys within 8 x E32 on both relative measures, 16-bit ys with the
    elementwise rounding allowance on top.  The plugin path's scan on the same operands is run for the record (it is not the
    reference, and the new path is not asked to beat it)."""
    H = hip()
    recs = sdc.memory_records(H, torch.device(DEV), regime, n, dtype)
    torch.cuda.synchronize()
    H.device_error()
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    assert sum(r["path"] == "fused" for r in recs) == (1 if dtype == F32 else 2)
    for r in recs:
        if r["path"] == "fused":
            assert r["ok"], r


# ----------------------------------------------------------------------------- workspace and torch.empty
def test_nothing_depends_on_the_workspace_or_on_torch_empty():
    """the several-segment case: twice; after the stream's workspace was filled with NaN bytes and with 0xFF; after it grew
    and moved; on a second stream; and with torch.empty handing back NaN, zeros and noise (tests/golden/buffer_cases.py), for
    `ys` and for a workspace first allocated under that fill on a fresh stream"""
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_case(sdc.MULTI_SEG, BF16)
    assert H.ss2d_scan_n_plan(c.b, c.l, c.d, c.k, c.n)[1] > 1
    args = _core_args(c, dev)
    run = lambda: H.ss2d_scan_n_cl(*args, BF16)
    first = run()
    assert bool(torch.isfinite(first.float()).all()) and torch.equal(first, run())
    ws = H._scan_workspace(first.device, 1)
    assert ws.numel() >= H.lib().tramba_ss2d_scan_n_workspace(c.b, c.l, c.d, c.k, c.n)
    nan_bytes = torch.full((ws.numel() // 4,), float("nan"), device=first.device).view(torch.uint8)
    for fill in (nan_bytes, 0xFF):
        if isinstance(fill, int):
            ws.fill_(fill)
        else:
            ws[:fill.numel()].copy_(fill)
        assert H._scan_workspace(first.device, 1).data_ptr() == ws.data_ptr()
        assert torch.equal(first, run())
    grown = H._scan_workspace(first.device, ws.numel() + (3 << 20) + 8)
    assert grown.data_ptr() != ws.data_ptr() and grown.numel() > ws.numel()
    assert torch.equal(first, run())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(first, on_side)
    # what torch.empty hands back: `ys` itself, and a workspace allocated under the fill (a new stream has none yet)
    for fill in bc.FILLS:
        fresh = torch.cuda.Stream()
        fresh.wait_stream(torch.cuda.current_stream())
        with bc.poisoned_allocations(fill) as st, torch.cuda.stream(fresh):
            got = run()
            fresh.synchronize()
        assert any(f == "hip.py" for f, _ in st.device_sites)
        torch.cuda.current_stream().wait_stream(fresh)
        assert torch.equal(first, got), fill
    H.device_error()


# ----------------------------------------------------------------------------- modules
def _ss2d(case):
    """the two modules of tests/test_gpu_scan_dstate.py::test_ss2d_at_the_default_dstate"""
    import tramba_amd as ta
    from tramba_amd import ops
    torch.manual_seed(11)
    if case == "default":      # the constructor's own d_state: raster, K = 4
        m, shape, family = ta.SS2D(d_model=16, channel_first=True), (2, 16, 12, 12), "raster"
    else:                      # helix, K = 8
        m = ta.SS2D(d_model=16, d_state=16, channel_first=True, scan=ops.CrossScan_Line, merge=ops.CrossMerge_Line, k_group=8)
        shape, family = (1, 16, 24, 24), "helix"
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    return m, torch.randn(*shape, generator=g), family


class _Spy:
    """counts the calls of an attribute while it is patched; `fail`: raise instead of calling through"""

    def __init__(self, monkeypatch, owner, name, fail=False, static=False):
        self.calls, self.name = 0, name
        orig = getattr(owner, name)

        def wrapped(*a, **kw):
            self.calls += 1
            if fail:
                raise AssertionError(f"{name} was called")
            return orig(*a, **kw)

        monkeypatch.setattr(owner, name, staticmethod(wrapped) if static else wrapped)


@pytest.mark.parametrize("case", ["default", "helix"])
def test_ss2d_inference_takes_the_fused_path_and_matches_the_oracle(case, monkeypatch):
    """no_grad forward of SS2D at d_state 16: fp32 within rtol 1e-3 / atol 1e-4 of oracle.model.ss2d, bf16 within 4e-2 of the
    map's largest magnitude (the figures of test_ss2d_at_the_default_dstate), through hip.ss2d_scan_n_cl"""
    H = hip()
    m, x, family = _ss2d(case)
    assert m.d_state == 16
    sd = {k_: v.detach().clone() for k_, v in m.state_dict().items()}
    fused = _Spy(monkeypatch, H, "ss2d_scan_n_cl")
    m.to(DEV).eval()
    with torch.no_grad():
        want = om.ss2d(om.SD(sd), x, family)
        got = m(x.to(DEV))
    assert fused.calls == 1 and got.dtype == F32
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-3, atol=1e-4)
    m16 = m.to(BF16)
    sd16 = {k_: v.detach().cpu().float() for k_, v in m16.state_dict().items()}
    x16 = x.to(BF16)
    with torch.no_grad():
        got16 = m16(x16.to(DEV)).float().cpu()
        want16 = om.ss2d(om.SD(sd16), x16.float(), family)
    assert fused.calls == 2 and bool(torch.isfinite(got16).all())
    err16 = float((got16 - want16).abs().max()) / float(want16.abs().max())
    print(case, f"bf16 forward: {err16:.2e} of the largest magnitude")
    assert err16 <= 4e-2


def _blocks():
    import tramba_amd as ta
    torch.manual_seed(21)
    return [("ss2d", ta.SS2D(d_model=16, channel_first=True)),
            ("vssblock", ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0)),
            ("decoder", ta.MultiScaleDecoderBlock(hidden_dim=16, drop_path=0.0, channel_first=True, ssm_d_state=16))]


def test_inference_at_dstate_16_needs_neither_the_reference_layout_scan_nor_an_einsum(monkeypatch):
    """with SelectiveScanOflex.apply, hip.selective_scan_fwd and torch.einsum patched to raise, the no_grad forwards of SS2D,
    VSSBlock(ssm_d_state=16) and MultiScaleDecoderBlock(ssm_d_state=16) complete: one x_proj GEMM, the fused scan, the fused
    merge + out_norm + GELU.  With gradients enabled (and nothing patched to raise) the same modules still take the plugin
    path -- the fused training path stays d_state == 1 -- and every parameter gets a gradient."""
    from tramba_amd import ops
    H = hip()
    blocks = _blocks()
    x = torch.randn(2, 16, 12, 12, generator=torch.Generator().manual_seed(22)).to(DEV)
    with monkeypatch.context() as mp:
        _Spy(mp, ops.SelectiveScanOflex, "apply", fail=True, static=True)
        _Spy(mp, H, "selective_scan_fwd", fail=True)
        _Spy(mp, torch, "einsum", fail=True)
        fused = _Spy(mp, H, "ss2d_scan_n_cl")
        for name, m in blocks:
            m.to(DEV).eval()
            with torch.no_grad():
                y = m(x)
            assert y.shape == x.shape and bool(torch.isfinite(y).all()), name
        assert fused.calls == len(blocks)
    with monkeypatch.context() as mp:
        plugin = _Spy(mp, ops.SelectiveScanOflex, "apply", static=True)
        fused = _Spy(mp, H, "ss2d_scan_n_cl")
        fused1 = _Spy(mp, H, "ss2d_scan_cl")
        for i, (name, m) in enumerate(blocks):
            m.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_()
            m(xg).square().mean().backward()
            assert plugin.calls == i + 1, name
            assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()), name
            for pname, p in m.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (name, pname)
        assert fused.calls == 0 and fused1.calls == 0


def test_graphed_forward_at_dstate_16():
    """GraphedForward over VSSBlock(ssm_d_state=16) in bf16: the replay equals the eager forward bit for bit, and so does a
    second replay after an unrelated allocation"""
    import tramba_amd as ta
    torch.manual_seed(23)
    m = ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0).to(DEV, BF16).eval()
    x = torch.randn(2, 16, 24, 24, device=DEV, dtype=BF16)         # 18 tiles: several segments, two launches per scan
    assert hip().ss2d_scan_n_plan(2, 576, m.op.d_inner, m.op.k_group, 16)[1] > 1
    with torch.no_grad():
        eager = m(x).clone()
    graphed = ta.GraphedForward(m, strict=True)
    first = graphed(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(eager, first)
    junk = torch.full((1 << 20,), float("nan"), device=DEV)          # an unrelated allocation between the replays
    second = graphed(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(first, second) and bool(torch.isnan(junk).all())
    hip().device_error()


def test_dstate_1_dispatch_is_undisturbed():
    """SS2D(d_state=1): the module's no_grad output equals, bit for bit, the same forward with the scan forced through
    hip.ss2d_scan_cl by hand -- same padded weight, same parameters, same launches"""
    import tramba_amd as ta
    from tramba_amd import modules as M
    H = hip()
    torch.manual_seed(24)
    m = ta.SS2D(d_model=16, d_state=1, channel_first=True).to(DEV).eval()
    x = torch.randn(2, 16, 12, 12, device=DEV)
    with torch.no_grad():
        got = m(x)
        xc = M.to_cl(x)
        xi = m.in_proj._forward_cl(xc)
        wt, bt = H.dw_pack(m.conv2d.weight, m.conv2d.bias)
        xi = H.dwconv_cl(xi, wt, bt, H.ACT_SILU)
        b, h, w, d = xi.shape
        order = H.scan_order("raster", h, w, xi.device)
        xf = xi.view(b, h * w, d)
        wp = H.pad_x_proj_weight(m.x_proj_weight.detach())
        assert wp.shape == (4 * H.ss2d_group_stride(m.dt_rank), d)
        xdbl = H.linear_cl(xf, wp.contiguous(), out_dtype=F32)
        ys = H.ss2d_scan_cl(xf, xdbl, order, m.dt_projs_weight.detach().float().contiguous(),
                            m.dt_projs_bias.detach().float().reshape(-1).contiguous(),
                            (-torch.exp(m.A_logs.detach().float())).reshape(-1).contiguous(), m.Ds.detach().float(), xi.dtype)
        y = H.ss2d_merge_norm_cl(ys, order, m.out_norm.weight.detach().float(), m.out_norm.bias.detach().float(),
                                 m.out_norm.eps, H.ACT_GELU, xi.dtype).view(b, h, w, d)
        want = M.from_cl(m.out_proj._forward_cl(y, residual=None, gelu_in=False))
    assert torch.equal(got, want)
