"""The fused channels-last SS2D TRAINING path at d_state N = 2..16 (opt-in, tramba_amd.set_fused_dstate_training): the
state-looped scan backward (hip.ss2d_scan_bwd_cl with a (K*D, N) `A`: ss2d_seg_n_bwd_kernel), the glue around it, the
_SS2DInnerCL Function and the modules that reach it, against fp64.

Kernel level: every output against the fp64 adjoint of tests/golden/ss2d_dstate_train_cases.py, which
tests/test_ss2d_dstate_train_host.py holds against autograd through oracle.ops.ss2d_core + cross_merge.  The bounds are the
project's for the N = 1 kernel (max |got - want| / max |want| <= 3e-4 for gu, 5e-4 for the other gradients in fp32; 3e-2 / 5e-2
in 16 bit), and the host file shows that fp32 arithmetic in the kernel's documented form uses at most half of each on these
inputs.  The long-memory cases (A = 0: the adjoint, like the state, crosses all segments undamped) use 8 x E32 (+ u for an
output stored in 16 bits) throughout."""
import json
import os

import numpy as np
import pytest
import torch

import buffer_cases as bc
import scan_memory_cases as smc
import ss2d_dstate_cases as sdc
import ss2d_dstate_train_cases as tc
from oracle import model as om

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = lambda v: v if isinstance(v, str) else str(v)[6:]


def hip():
    from tramba_amd import hip as h
    return h


def _plan(cfg):
    b, h, d, r, fam, n = cfg
    return hip().ss2d_scan_n_bwd_plan(b, h * h, d, sdc.k_of(fam), n)


# ----------------------------------------------------------------------------- kernel level
def test_the_cases_reach_the_paths_they_are_named_for():
    plans = {name: _plan(tc.CORE_CASES[name]) for name in tc.KERNEL_CASES}
    tiles = {name: (tc.CORE_CASES[name][1] ** 2 + 31) // 32 for name in tc.KERNEL_CASES}
    assert plans["single_launch"] == (tiles["single_launch"], 1) and 12 * 12 % 32 != 0     # one launch, a ragged last tile
    assert plans["rank40"][1] == 1
    nt, nseg = plans["segments_k8"]
    assert nseg > 2 and nt > 1 and tc.CORE_CASES["segments_k8"][2] > 32                  # several tiles per segment, two channel tiles
    assert plans["d40_window"][1] > 1 and tc.CORE_CASES["d40_window"][2] % 32 == 8
    nt, nseg = plans["ragged_r1"]
    assert nseg > 1 and nt * nseg > tiles["ragged_r1"] and 14 * 14 % 32 != 0             # the last segment is short and ends ragged
    assert plans["fold_unrolled"][1] > 16                                                # both folds: two 8-wide rounds + remainder
    for name in tc.KERNEL_CASES:
        nt, nseg = plans[name]
        assert nt * tc.CORE_CASES[name][5] <= 160, name                                  # the tile-entry states fit the LDS rows
        assert (tc.CORE_CASES[name][3] + 15) // 16 == {"rank40": 3}.get(name, 1), name


KERNEL_DTYPES = [(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]


@pytest.mark.parametrize("dtypes", KERNEL_DTYPES, ids=lambda v: "-".join(IDS(t) for t in v))
@pytest.mark.parametrize("name", tc.KERNEL_CASES, ids=IDS)
def test_scan_backward_against_fp64(name, dtypes):
    """gu, graw, dB_n, dC_n, dA_logs, dD, dbias of hip.ss2d_scan_bwd_cl against the fp64 adjoint; gym in fp32 and in the
    activation dtype.  Rows and columns past D (d40_window) are outside the outputs' shapes: the allocation has no room for them."""
    H = hip()
    dtype, gdtype = dtypes
    nt, nseg = _plan(tc.CORE_CASES[name])
    c, gym, ref, e32 = tc.core_e32(name, dtype, gdtype, nt)
    got, raw = tc.run_bwd(H, c, gym, torch.device(DEV))
    torch.cuda.synchronize()
    H.device_error()
    gu, graw, bpart, cpart, gpar = raw
    ct = (c.d + 31) // 32
    assert gu.dtype == graw.dtype == dtype and gu.shape == graw.shape == (c.b, c.k, c.l, c.d)
    assert bpart.shape == cpart.shape == (c.b, c.k, ct, c.n, c.l) and gpar.shape == (c.b * nseg, c.k * c.d * (c.n + 2))
    bad = {}
    for out in tc.OUTPUTS:
        assert bool(torch.isfinite(got[out]).all()), out
        err = smc.rel_errors(got[out], ref[out])[0]
        bnd = tc.bound(out, dtype, e32[out], stored16=out in ("gu", "graw"))
        print(name, IDS(dtype), "gym", IDS(gdtype), out, f"err {err:.2e} E32 {e32[out]:.2e} bound {bnd:.2e}")
        if err > bnd:
            bad[out] = (err, bnd)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS)
@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_state_and_adjoint_outlive_the_segments(regime, n, dtype):
    """helix 48 x 48, D = 32: 72 tiles; with A = 0 neither the state nor the adjoint decays, so a lost segment hand-over in
    either direction moves every gradient.  8 x E32 on the max-relative measure (+ u for the 16-bit gu / graw)."""
    H = hip()
    fam, h, d, r = sdc.MEMORY_SHAPE
    nt, nseg = H.ss2d_scan_n_bwd_plan(1, h * h, d, sdc.k_of(fam), n)
    assert nseg > 8
    c, gym, ref, e32 = tc.memory_e32(regime, n, dtype, nt)
    got, _ = tc.run_bwd(H, c, gym, torch.device(DEV))
    torch.cuda.synchronize()
    H.device_error()
    bad = {}
    for out in tc.OUTPUTS:
        err = smc.rel_errors(got[out], ref[out])[0]
        bnd = tc.bound(out, dtype, e32[out], stored16=out in ("gu", "graw"), long_memory=True)
        print(regime, n, IDS(dtype), out, f"err {err:.2e} E32 {e32[out]:.2e} bound {bnd:.2e}")
        if not err <= bnd:
            bad[out] = (err, bnd)
    assert not bad, bad


@pytest.mark.parametrize("name", ["d40_window", "ragged_r1"])
def test_nothing_is_written_outside_the_outputs(name):
    """D % 32 != 0 (the second channel tile is 8 channels wide) and L % 32 != 0 (a ragged last tile): the entry is called on
    outputs that sit between guard zones of a sentinel; the guards stay intact, every element between them is written, and
    the outputs equal the wrapper's bit for bit"""
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_as_scan_case(sdc.core_case(tc.CORE_CASES[name], BF16))
    assert c.d % 32 != 0 or c.l % 32 != 0
    x, xdbl, order, dt_w, dt_b, A, ds = sdc.device_args(H, c, dev)
    gym = tc.gym_of(c).to(dev)
    want = H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, A, ds, gym, bc_partials=True)
    guard = 4096                                                       # elements on either side, 16-byte multiples
    bufs, views = [], []
    for t in want:
        sentinel = -7.0 if t.dtype == BF16 else float("nan")
        buf = torch.full((t.numel() + 2 * guard,), sentinel, dtype=t.dtype, device=dev)
        bufs.append((buf, sentinel))
        views.append(buf[guard:guard + t.numel()].view(t.shape))
    ws_bytes = H.lib().tramba_ss2d_scan_n_bwd_workspace(c.b, c.l, c.d, c.k, c.n, H.dt(x))
    ws = H._scan_workspace(dev, ws_bytes)
    rc = H.lib().tramba_ss2d_scan_n_bwd_cl(x.data_ptr(), xdbl.data_ptr(), order.table.data_ptr(), dt_w.data_ptr(),
                                           dt_b.data_ptr(), A.data_ptr(), ds.data_ptr(), gym.data_ptr(), *[v.data_ptr() for v in views],
                                           ws.data_ptr(), ws_bytes, c.b, c.l, c.d, c.k, c.r, c.n, H.dt(x), H.dt(gym), H._stream())
    assert rc == 0, H.lib().tramba_last_error()
    torch.cuda.synchronize()
    H.device_error()
    for (buf, sentinel), v, t in zip(bufs, views, want):
        for zone in (buf[:guard], buf[guard + t.numel():]):
            assert bool(torch.isnan(zone).all()) if sentinel != sentinel else bool((zone == sentinel).all())
        assert bool(torch.isfinite(v.float()).all()) and torch.equal(v, t)


def test_shape_checks_name_the_layout():
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_as_scan_case(sdc.core_case(tc.CORE_CASES["single_launch"], F32))
    x, xdbl, order, dt_w, dt_b, A, ds = sdc.device_args(H, c, dev)
    gym = tc.gym_of(c).to(dev)
    with pytest.raises(H.TrambaHipError, match=r"K\*RG\(R, N\)"):
        H.ss2d_scan_bwd_cl(x, xdbl[..., :-4].contiguous(), order, dt_w, dt_b, A, ds, gym, bc_partials=True)
    with pytest.raises(H.TrambaHipError, match="bc_partials"):
        H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, A, ds, gym)
    with pytest.raises(H.TrambaHipError, match=r"\(K\*D, N\)"):
        H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, A[:4].contiguous(), ds, gym, bc_partials=True)
    gu, graw, bpart, cpart, gpar = H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, A, ds, gym, bc_partials=True)
    with pytest.raises(H.TrambaHipError, match="CT, 2, L"):
        H.ss2d_bwd_prep(xdbl, order, bpart[:, :, :, 0].contiguous(), cpart[:, :, :, 0].contiguous(), c.r, F32, c.n)
    with pytest.raises(H.TrambaHipError, match=r"RG\(r, n\)"):
        H.ss2d_bwd_assemble(torch.zeros(c.b, c.k, c.l, 16, device=dev), order, c.r, F32, c.n)


# ----------------------------------------------------------------------------- reproducibility
def test_every_output_is_bitwise_reproducible():
    """the several-segment case: run to run; on a second stream; with the stream's workspace filled with NaN and with 0xFF
    bytes; after the workspace grew and moved; and with torch.empty handing back NaN, zeros and noise"""
    H = hip()
    dev = torch.device(DEV)
    c = sdc.core_as_scan_case(sdc.core_case(tc.CORE_CASES["segments_k8"], BF16))
    assert _plan(tc.CORE_CASES["segments_k8"])[1] > 1
    x, xdbl, order, dt_w, dt_b, A, ds = sdc.device_args(H, c, dev)
    gym = tc.gym_of(c).to(dev)

    def run():
        gu, graw, bpart, cpart, gpar = H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, A, ds, gym, bc_partials=True)
        ranks, gseq = H.ss2d_bwd_prep(xdbl, order, bpart, cpart, c.r, BF16, c.n)
        r8 = sdc.rank_pad(c.r)
        return gu, graw, bpart, cpart, gpar, ranks, gseq[..., r8:].contiguous()

    same = lambda a, b: all(torch.equal(p, q) for p, q in zip(a, b))
    first = run()
    assert all(bool(torch.isfinite(t.float()).all()) for t in first) and same(first, run())
    ws = H._scan_workspace(x.device, 1)
    assert ws.numel() >= H.lib().tramba_ss2d_scan_n_bwd_workspace(c.b, c.l, c.d, c.k, c.n, H.dt(x))
    nan_bytes = torch.full((ws.numel() // 4,), float("nan"), device=x.device).view(torch.uint8)
    for fill in (nan_bytes, 0xFF):
        if isinstance(fill, int):
            ws.fill_(fill)
        else:
            ws[:fill.numel()].copy_(fill)
        assert H._scan_workspace(x.device, 1).data_ptr() == ws.data_ptr()
        assert same(first, run())
    grown = H._scan_workspace(x.device, ws.numel() + (3 << 20) + 8)
    assert grown.data_ptr() != ws.data_ptr() and grown.numel() > ws.numel()
    assert same(first, run())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, on_side)
    for fill in bc.FILLS:
        fresh = torch.cuda.Stream()
        fresh.wait_stream(torch.cuda.current_stream())
        with bc.poisoned_allocations(fill) as st, torch.cuda.stream(fresh):
            got = run()
            fresh.synchronize()
        assert any(f == "hip.py" for f, _ in st.device_sites)
        torch.cuda.current_stream().wait_stream(fresh)
        assert same(first, got), fill
    H.device_error()


# ----------------------------------------------------------------------------- Function level
def _function_inputs(o, dtype, dev):
    cc = o.case
    z = cc.x.permute(0, 2, 3, 1).reshape(cc.b, cc.l, cc.d).contiguous().to(dtype).to(dev).requires_grad_()
    xs = torch.nn.functional.silu(z.detach().float()).to(dtype)
    pars = [cc.wx.float().to(dev).requires_grad_(), cc.wdt.to(dev).requires_grad_(), cc.dtb.to(dev).requires_grad_(),
            cc.a_logs.to(dev).requires_grad_(), cc.ds.to(dev).requires_grad_()]
    return z, xs, pars


@pytest.mark.parametrize("name", ["segments_k8", "d40_window"])
def test_function_against_fp64_autograd(name):
    """_SS2DInnerCL in fp32: the merged output within 2e-4 and the gradients of z (through the SiLU), the x_proj weight, dt_w,
    dt_bias, A_logs and Ds within 3e-4 / 5e-4 of autograd through oracle.ops.ss2d_core + cross_merge (max-relative); its
    forward equals the same launches made by hand bit for bit"""
    from tramba_amd import modules as M
    H = hip()
    dev = torch.device(DEV)
    o = tc.oracle_grads(name, F32, True)
    cc = o.case
    z, xs, pars = _function_inputs(o, F32, dev)
    order = H.scan_order(cc.fam, cc.h, cc.h, dev)
    ym = M._SS2DInnerCL.apply(z, xs, *pars, order)
    wa = H.pad_x_proj_weight(pars[0].detach(), cc.n).contiguous()
    xdbl = H.linear_cl(xs, wa, out_dtype=F32)
    a_neg = -torch.exp(pars[3].detach())
    ys = H.ss2d_scan_n_cl(xs, xdbl, order, pars[1].detach().contiguous(), pars[2].detach().reshape(-1).contiguous(), a_neg,
                          pars[4].detach(), F32)
    assert torch.equal(ym.detach(), H.ss2d_merge_sum_cl(ys, order, F32))
    assert smc.rel_errors(ym.detach().cpu(), o.y)[0] <= tc.BASE_TOL[F32][0]
    (ym * o.gym.to(dev)).sum().backward()
    torch.cuda.synchronize()
    H.device_error()
    got = dict(x=z.grad, wx=pars[0].grad, dt_w=pars[1].grad, dt_b=pars[2].grad, a_logs=pars[3].grad, ds=pars[4].grad)
    bad = {}
    for k_, g in got.items():
        assert g is not None and g.shape == o.grads[k_].shape, k_
        err = smc.rel_errors(g.cpu(), o.grads[k_])[0]
        print(name, k_, f"{err:.2e}")
        if err > tc.base_tol(k_, F32):
            bad[k_] = err
    assert not bad, bad


def test_function_at_dstate_1_is_undisturbed():
    """_SS2DInnerCL at N = 1: output and gradients equal, bit for bit, the parent code path's launches made by hand"""
    from tramba_amd import modules as M
    H = hip()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(41)
    b, h, d, r, k = 2, 12, 40, 3, 4
    l = h * h
    order = H.scan_order("raster", h, h, dev)
    z = torch.randn(b, l, d, generator=g).to(BF16).to(dev).requires_grad_()
    xs = torch.nn.functional.silu(z.detach().float()).to(BF16)
    xw = (torch.randn(k, r + 2, d, generator=g) * d ** -0.5).to(dev).requires_grad_()
    dtw = (torch.randn(k, d, r, generator=g) * r ** -0.5).to(dev).requires_grad_()
    dtb = (torch.randn(k, d, generator=g) * 0.5 - 2).to(dev).requires_grad_()
    al = torch.log(0.5 + torch.rand(k * d, 1, generator=g)).to(dev).requires_grad_()
    ds = (1 + 0.1 * torch.randn(k * d, generator=g)).to(dev).requires_grad_()
    gym = torch.randn(b, l, d, generator=g).to(BF16).to(dev)
    ym = M._SS2DInnerCL.apply(z, xs, xw, dtw, dtb, al, ds, order)
    ym.backward(gym)
    # by hand, as the Function stood before it had a sibling
    wa = H.pad_x_proj_weight(xw.detach().to(BF16)).contiguous()
    assert torch.equal(wa, M._xproj_padded(xw, BF16)[0]) and torch.equal(wa, M._xproj_padded(xw, BF16, 1)[0])
    xdbl = H.linear_cl(xs, wa, out_dtype=F32)
    f = lambda t: t.detach().float().contiguous()
    states = H.ss2d_scan_states(xs, order)
    ys = H.ss2d_scan_cl(xs, xdbl, order, f(dtw), f(dtb).reshape(-1), f(al).reshape(-1), f(ds), BF16, states=states, a_log=True)
    assert torch.equal(ym.detach(), H.ss2d_merge_sum_cl(ys, order, BF16))
    gu, graw, bpart, cpart, gpar = H.ss2d_scan_bwd_cl(xs, xdbl, order, f(dtw), f(dtb).reshape(-1), f(al).reshape(-1), f(ds),
                                                     gym, states=states, a_log=True, bc_partials=True)
    ranks, gseq = H.ss2d_bwd_prep(xdbl, order, bpart, cpart, r, BF16)
    rg = H.ss2d_group_stride(r)
    assert ranks.shape[-1] == rg - 4 and bool((gseq[..., rg - 2:] == 0).all())
    assert bpart.shape == (b, k, 2, l) and torch.equal(gseq[..., rg - 4], bpart[:, :, 0] + bpart[:, :, 1])
    assert torch.equal(gseq[..., rg - 3], cpart[:, :, 0] + cpart[:, :, 1])
    gp = H.slab_sum(gpar)
    assert torch.equal(dtb.grad, gp[2].reshape(k, d)) and torch.equal(al.grad, gp[0].reshape(k * d, 1))
    assert torch.equal(ds.grad, gp[1].reshape(-1))
    g_dtw = H.wgrad_grouped_cl(graw, ranks)[..., :r]
    assert torch.equal(dtw.grad, g_dtw)
    H.rows_gemm_cl(graw.view(b * k, l, d), f(dtw).transpose(1, 2).to(BF16).contiguous(), gseq.view(b * k, l, rg), r)
    g_xd = H.ss2d_bwd_assemble(gseq, order, r, BF16).view(b * l, k * rg)
    t = M._dgrad(g_xd, wa, None).view(b, l, d)
    assert torch.equal(z.grad, H.ss2d_merge_grad_cl(gu, order, t, z.detach()))
    H.device_error()


# ----------------------------------------------------------------------------- the one Function against its two parents
def _inner_inputs(n_kind, dtype, dev):
    """(order, n, gym, [z, xs, x_proj weight, dt_w, dt_bias, A_logs, Ds]) for _SS2DInnerCL.apply, fresh leaves: "n1" the raster
    shape of test_function_at_dstate_1_is_undisturbed, "n16" CORE_CASES["segments_k8"] (helix, K = 8, 9 segments)"""
    H = hip()
    if n_kind == "n1":
        g = torch.Generator().manual_seed(41)
        b, h, d, r, k, n = 2, 12, 40, 3, 4, 1
        order = H.scan_order("raster", h, h, dev)
        z = torch.randn(b, h * h, d, generator=g).to(dtype)
        pars = [torch.randn(k, r + 2, d, generator=g) * d ** -0.5, torch.randn(k, d, r, generator=g) * r ** -0.5,
                torch.randn(k, d, generator=g) * 0.5 - 2, torch.log(0.5 + torch.rand(k * d, 1, generator=g)),
                1 + 0.1 * torch.randn(k * d, generator=g)]
        gym = torch.randn(b, h * h, d, generator=g).to(dtype)
    else:
        cc = sdc.core_case(tc.CORE_CASES["segments_k8"], dtype)
        n = cc.n
        order = H.scan_order(cc.fam, cc.h, cc.h, dev)
        z = cc.x.permute(0, 2, 3, 1).reshape(cc.b, cc.l, cc.d).contiguous()
        pars = [t.float() for t in (cc.wx, cc.wdt, cc.dtb, cc.a_logs, cc.ds)]
        gym = tc.gym_of(sdc.core_as_scan_case(cc)).to(dtype)
    z = z.to(dev).requires_grad_()
    xs = torch.nn.functional.silu(z.detach().float()).to(dtype)
    return order, n, gym.to(dev), [z, xs] + [p.to(dev).requires_grad_() for p in pars]


@pytest.mark.parametrize("n_kind,dtype", [("n1", F16), ("n1", F32), ("n16", F16)], ids=IDS)
def test_wide_routes_equal_the_parents_launches(n_kind, dtype):
    """graw in fp32 (fp16 activations, fp32 validation mode): the output and the gradients of z, the x_proj weight, dt_w,
    dt_bias, A_logs and Ds equal, bit for bit, the launches of the two Functions this one replaced, made by hand -- fp32
    copies of xs / gym into the scan backward for fp16, ss2d_bwd_prep in fp32, the three split passes with passes two and
    three written to a SEPARATE scratch tensor (the Function writes them into the dead fp32 rank rows)"""
    from tramba_amd import modules as M
    H = hip()
    dev = torch.device(DEV)
    order, n, gym, (z, xs, xw, dtw, dtb, al, ds) = _inner_inputs(n_kind, dtype, dev)
    b, l, d = xs.shape
    k, r = order.k, dtw.shape[-1]
    ym = M._SS2DInnerCL.apply(z, xs, xw, dtw, dtb, al, ds, order)
    ym.backward(gym)
    f = lambda t: t.detach().float().contiguous()        # noqa: E731
    rg, r8 = H.ss2d_group_stride(r, n), (r + 7) & ~7
    wa = H.pad_x_proj_weight(xw.detach().to(dtype), n).contiguous()
    xdbl = H.linear_cl(xs, wa, out_dtype=F32)
    if n == 1:
        a, states = f(al).reshape(-1), H.ss2d_scan_states(xs, order)
        ys = H.ss2d_scan_cl(xs, xdbl, order, f(dtw), f(dtb).reshape(-1), a, f(ds), dtype, states=states, a_log=True)
        kw = dict(states=states, a_log=True, bc_partials=True)
    else:
        a = torch.exp(f(al).reshape(-1, n)).neg_()
        ys = H.ss2d_scan_n_cl(xs, xdbl, order, f(dtw), f(dtb).reshape(-1), a, f(ds), dtype)
        kw = dict(bc_partials=True)
    assert torch.equal(ym.detach(), H.ss2d_merge_sum_cl(ys, order, dtype))
    x32, g32 = (xs.float(), gym.float()) if dtype == F16 else (xs, gym)
    gu, graw, bpart, cpart, gpar = H.ss2d_scan_bwd_cl(x32, xdbl, order, f(dtw), f(dtb).reshape(-1), a, f(ds), g32, **kw)
    gu = gu.to(dtype)
    assert graw.dtype == F32
    ranks, gseq = H.ss2d_bwd_prep(xdbl, order, bpart, cpart, r, F32, n)
    assert ranks.shape == (b, k, l, r8) and ranks.dtype == F32 and ranks.is_contiguous()
    gh, gl = M._split16(graw)
    rh, rl = M._split16(ranks)
    wh, wl = M._split16(f(dtw).transpose(1, 2).contiguous())
    g_dtw = H.wgrad_grouped_cl(gh, rh) + H.wgrad_grouped_cl(gh, rl) + H.wgrad_grouped_cl(gl, rh)
    assert torch.equal(dtw.grad, g_dtw[..., :r].contiguous())
    tmp = torch.zeros_like(gseq)
    H.rows_gemm_cl(gh.view(b * k, l, d), wh, gseq.view(b * k, l, rg), r)
    for ga_, wa_ in ((gh, wl), (gl, wh)):
        H.rows_gemm_cl(ga_.view(b * k, l, d), wa_, tmp.view(b * k, l, rg), r)
        gseq[..., :r] += tmp[..., :r]
    g_xd = H.ss2d_bwd_assemble(gseq, order, r, dtype, n).view(b * l, k * rg)
    t = M._dgrad(g_xd, wa, None).view(b, l, d)
    assert torch.equal(z.grad, H.ss2d_merge_grad_cl(gu, order, t, z.detach()))
    if dtype != F32:
        segs = [s_ for g in range(k) for s_ in ((g * rg, r), (g * rg + r8, 2 * n))]
        gxw = H.wgrad_rows_cl(g_xd, xs.view(b * l, d), segs).view(k, r + 2 * n, d)
    else:
        gp_ = M._wgrad(g_xd, xs.view(b * l, d))[0].view(k, rg, d)
        gxw = torch.cat((gp_[:, :r], gp_[:, r8:r8 + 2 * n]), dim=1)
    assert torch.equal(xw.grad, gxw)
    gp, kd = H.slab_sum(gpar).reshape(-1), k * d
    assert torch.equal(dtb.grad, gp[kd * (n + 1):].reshape(k, d)) and torch.equal(al.grad, gp[:kd * n].reshape(kd, n))
    assert torch.equal(ds.grad, gp[kd * n:kd * (n + 1)])
    for t_ in (ym, z.grad, xw.grad, dtw.grad, dtb.grad, al.grad, ds.grad):
        assert bool(torch.isfinite(t_.float()).all())
    H.device_error()


def test_the_scan_backward_call_at_dstate_1(monkeypatch):
    """_SS2DInnerCL at N = 1 hands hip.ss2d_scan_bwd_cl exactly the keywords states, a_log, bc_partials, and with them its own
    tensors, untouched, for bf16 and fp32 activations (same storage, same dtypes) and fp32 copies for fp16 alone; graw comes
    back in the activation dtype for bf16 and in fp32 otherwise"""
    from tramba_amd import modules as M
    H = hip()
    dev = torch.device(DEV)
    real, calls = H.ss2d_scan_bwd_cl, []

    def spy(x, xdbl, order, dt_w, dt_b, a, ds, gym, **kw):
        res = real(x, xdbl, order, dt_w, dt_b, a, ds, gym, **kw)
        calls.append((x, gym, a, kw, res[1].dtype))
        return res

    monkeypatch.setattr(H, "ss2d_scan_bwd_cl", spy)
    for dtype in (BF16, F32, F16):
        order, n, gym, (z, xs, xw, dtw, dtb, al, ds) = _inner_inputs("n1", dtype, dev)
        del calls[:]
        M._SS2DInnerCL.apply(z, xs, xw, dtw, dtb, al, ds, order).backward(gym)
        assert len(calls) == 1
        x, gy, a, kw, graw_dtype = calls[0]
        assert set(kw) == {"states", "a_log", "bc_partials"} and kw["a_log"] is True and kw["bc_partials"] is True
        assert kw["states"].dtype == torch.uint8 and kw["states"].numel() == H.ss2d_scan_states(xs, order).numel()
        assert a.data_ptr() == al.data_ptr() and a.dtype == F32 and a.shape == (al.numel(),)      # A_logs itself
        if dtype == F16:
            assert x.dtype == gy.dtype == graw_dtype == F32 and torch.equal(x, xs.float()) and torch.equal(gy, gym.float())
        else:
            assert x.data_ptr() == xs.data_ptr() and x.dtype == dtype and gy.data_ptr() == gym.data_ptr() and gy.dtype == dtype
            assert graw_dtype == (BF16 if dtype == BF16 else F32)
    H.device_error()


LAUNCH_CASES = {"bf16_n1": ("n1", BF16), "bf16_n16": ("n16", BF16), "fp16_n1": ("n1", F16), "fp16_n16": ("n16", F16)}
LAUNCH_PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ss2d_inner_launches.json")


def inner_launches(function, n_kind, dtype):
    """{kernel name: launches} of one forward + backward of `function` called directly (fresh leaves, no shadows), counted with
    torch.profiler as tests/test_gpu_step_control.py::_kernel_counts does, after one call that is not counted (the shared
    zero constants, the scan order's tables)"""
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)

    def once():
        order, n, gym, args = _inner_inputs(n_kind, dtype, dev)
        torch.cuda.synchronize()
        return lambda: function.apply(*args, order).backward(gym)

    once()()
    run = once()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    counts = {}
    for ev in prof.key_averages():
        if not ev.key.startswith("hip"):        # (the runtime's own calls -- hipLaunchKernel, hipDeviceSynchronize -- are no kernels)
            counts[ev.key] = counts.get(ev.key, 0) + ev.count
    return counts


def _launch_class(name):
    """the framework's copy / cast kernels, its fills, everything else (the library's kernels among it)"""
    return "copy" if "copy" in name.lower() else "fill" if "fill" in name.lower() else "other"


@pytest.mark.parametrize("case", list(LAUNCH_CASES))
def test_launches_equal_the_parent_commits(case):
    """one forward + backward of the Function makes the launches the parent commit's pair of Functions made, name by name
    (profiles/ss2d_inner_launches.json, "parent": this counting code run on the parent commit; TRAMBA_WRITE_PROFILES=1 writes
    this tree's counts beside them as "head").  Two differences are allowed, both at N > 1 and both a launch LESS: the
    fallback transposed dt_projs_weight of the 16-bit route is one transposing cast, as the parent's N = 1 Function made it
    (there: a cast, then a transposing copy), so the copy / cast kernels are one fewer in all and the only name that may gain
    a launch is one the parent's N = 1 record of that dtype holds; and a wide route has one fill fewer (no zeroed scratch).
    Every other name, and everything at N = 1, equals the record."""
    from tramba_amd import modules as M
    n_kind, dtype = LAUNCH_CASES[case]
    got = inner_launches(M._SS2DInnerCL, n_kind, dtype)
    with open(LAUNCH_PROFILE) as f:
        record = json.load(f)
    for name in sorted(got):
        print(case, got[name], name)
    if os.environ.get("TRAMBA_WRITE_PROFILES") == "1":
        record.setdefault("head", {})[case] = got
        with open(LAUNCH_PROFILE, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
    want = record["parent"][case]
    wide = dtype != BF16
    fewer = {"copy": int(n_kind != "n1" and not wide), "fill": int(n_kind != "n1" and wide), "other": 0}
    by_class = lambda c: {cls: sum(v for k_, v in c.items() if _launch_class(k_) == cls) for cls in fewer}   # noqa: E731
    assert {cls: v + fewer[cls] for cls, v in by_class(got).items()} == by_class(want), (by_class(got), by_class(want))
    n1_record = record["parent"][case.replace("n16", "n1")]
    for name in set(got) | set(want):
        g, w, cls = got.get(name, 0), want.get(name, 0), _launch_class(name)
        if not fewer[cls]:
            assert g == w, (name, g, w)
        elif cls == "copy":
            assert g <= w + 1 and (g <= w or name in n1_record), (name, g, w)
        else:
            assert g <= w, (name, g, w)
    assert sum(max(got.get(k_, 0) - want.get(k_, 0), 0) for k_ in got) <= fewer["copy"]


# ----------------------------------------------------------------------------- module level
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


def _forbid_the_plugin_path(mp):
    from tramba_amd import ops
    H = hip()
    _Spy(mp, ops.SelectiveScanOflex, "apply", fail=True, static=True)
    _Spy(mp, H, "selective_scan_fwd", fail=True)
    _Spy(mp, H, "selective_scan_bwd", fail=True)
    _Spy(mp, torch, "einsum", fail=True)


@pytest.mark.parametrize("case", ["default", "helix"])
def test_ss2d_with_the_switch_on_matches_the_oracle(case, monkeypatch):
    """SS2D at d_state 16 under autograd, switch on, fp32: forward rtol 1e-3 / atol 1e-4, every parameter gradient and the
    input gradient to a relative L2 of 1e-3 against oracle.model.ss2d with autograd through it -- without the plugin path"""
    import tramba_amd as ta
    m, x, family = _ss2d(case)
    sd = {k_: v.detach().clone() for k_, v in m.state_dict().items()}
    leaves = {k_: v.clone().requires_grad_() for k_, v in sd.items()}
    xo = x.clone().requires_grad_()
    want = om.ss2d(om.SD(leaves), xo, family)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(13))
    (want * gy).sum().backward()
    m.to(DEV)
    xg = x.to(DEV).requires_grad_()
    fused = _Spy(monkeypatch, hip(), "ss2d_scan_n_cl")
    _forbid_the_plugin_path(monkeypatch)
    with ta.fused_dstate_training(True):
        got = m(xg)
        (got * gy.to(DEV)).sum().backward()
    assert fused.calls == 1 and not ta.get_fused_dstate_training()
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-3, atol=1e-4)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    errs = {"x": rel(xg.grad.cpu(), xo.grad)}
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        errs[name] = rel(p.grad.cpu(), leaves[name].grad)
    print(case, {k_: f"{v:.2e}" for k_, v in errs.items()})
    assert max(errs.values()) <= 1e-3, errs
    hip().device_error()


def _blocks():
    import tramba_amd as ta
    torch.manual_seed(21)
    return [("vssblock", ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0)),
            ("decoder", ta.MultiScaleDecoderBlock(hidden_dim=16, drop_path=0.0, channel_first=True, ssm_d_state=16))]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=IDS)
def test_blocks_train_at_dstate_16_without_the_plugin_path(dtype, monkeypatch):
    """VSSBlock(ssm_d_state=16) and MultiScaleDecoderBlock(ssm_d_state=16), switch on: forward + backward complete with
    SelectiveScanOflex.apply, hip.selective_scan_fwd / _bwd and torch.einsum patched to raise; every parameter gets a finite
    gradient of its own shape, and two backward passes from the same state give equal gradients bit for bit.  With the switch
    off the same call reaches SelectiveScanOflex.apply."""
    import tramba_amd as ta
    from tramba_amd import ops
    x = torch.randn(2, 16, 12, 12, generator=torch.Generator().manual_seed(22)).to(DEV, dtype)
    for name, m in _blocks():
        m.to(DEV, dtype)
        grads = []
        with monkeypatch.context() as mp, ta.fused_dstate_training(True):
            _forbid_the_plugin_path(mp)
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                xg = x.clone().requires_grad_()
                y = m(xg)
                assert y.shape == x.shape
                y.float().square().mean().backward()
                assert bool(torch.isfinite(xg.grad.float()).all()), name
                for pname, p in m.named_parameters():
                    assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad.float()).all()), (name, pname)
                grads.append([xg.grad.clone()] + [p.grad.clone() for p in m.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*grads)), name
        with monkeypatch.context() as mp:
            plugin = _Spy(mp, ops.SelectiveScanOflex, "apply", static=True)
            m(x.clone().requires_grad_()).float().square().mean().backward()
            assert plugin.calls == 1, name
    hip().device_error()


def test_configurations_out_of_scope_keep_the_plugin_path(monkeypatch):
    """an SS2D without depth-wise conv, or with dropout, at N = 16 takes the plugin path with the switch on"""
    import tramba_amd as ta
    from tramba_amd import ops
    torch.manual_seed(31)
    x = torch.randn(1, 16, 12, 12, device=DEV)
    plugin = _Spy(monkeypatch, ops.SelectiveScanOflex, "apply", static=True)
    fused = _Spy(monkeypatch, hip(), "ss2d_scan_n_cl")
    with ta.fused_dstate_training(True):
        for i, kw in enumerate((dict(d_conv=1), dict(dropout=0.1))):
            m = ta.SS2D(d_model=16, channel_first=True, **kw).to(DEV)
            m(x.clone().requires_grad_()).square().mean().backward()
            assert plugin.calls == i + 1 and fused.calls == 0, kw


def test_bf16_gradients_are_no_worse_than_the_plugin_path():
    """bf16 activations, fp32 oracle gradients: each parameter gradient's relative L2 error on the fused path may exceed the
    plugin path's, on the same module and inputs, by at most a factor of 2; and it stays inside the project's bf16 figures
    (cosine >= 0.998, norm ratio within 4 %)"""
    import tramba_amd as ta
    m, x, family = _ss2d("helix")
    sd = {k_: v.detach().clone() for k_, v in m.state_dict().items()}
    leaves = {k_: v.clone().requires_grad_() for k_, v in sd.items()}
    x16 = x.to(BF16)
    xo = x16.float().requires_grad_()
    want = om.ss2d(om.SD(leaves), xo, family)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(13))
    (want * gy).sum().backward()
    m.to(DEV)
    errs = {}
    for path, on in (("fused", True), ("plugin", False)):
        m.zero_grad(set_to_none=True)
        with ta.fused_dstate_training(on):
            ta.modules.refresh_lowp_shadows(m, BF16)
            (m(x16.to(DEV)).float() * gy.to(DEV)).sum().backward()
        errs[path] = {}
        for name, p in m.named_parameters():
            g, w = p.grad.double().cpu().reshape(-1), leaves[name].grad.double().reshape(-1)
            errs[path][name] = (float((g - w).norm() / w.norm()), float(g @ w / (g.norm() * w.norm())), float(g.norm() / w.norm()))
    for name in errs["fused"]:
        f, p = errs["fused"][name], errs["plugin"][name]
        print(name, f"fused rel L2 {f[0]:.2e} cos {f[1]:.5f} ratio {f[2]:.4f}; plugin rel L2 {p[0]:.2e}")
    bad = {n: (errs["fused"][n], errs["plugin"][n][0]) for n in errs["fused"]
           if errs["fused"][n][0] > 2 * errs["plugin"][n][0] or errs["fused"][n][1] < 0.998 or abs(errs["fused"][n][2] - 1) > 0.04}
    assert not bad, bad


def test_stochastic_depth_on_the_deferred_stream():
    """drop_path > 0 on the deferred residual stream runs with the switch on; fed the same mask table (same seed, the pool's
    rows already assigned by a warm-up forward), output and input gradient agree with the switch-off (plugin) path within the
    project's bf16 figures: cosine >= 0.998, norm ratio within 4 %"""
    import tramba_amd as ta
    torch.manual_seed(51)
    m = ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.5).to(DEV, BF16).train()
    x = torch.randn(4, 16, 12, 12, device=DEV, dtype=BF16)
    pool = ta.modules.model_mask_pool(m)
    with ta.fused_dstate_training(True):
        m(x.clone().requires_grad_())                    # assigns the two mask rows of the block's DropPath
    res, masks = {}, {}
    for on in (True, False):
        torch.cuda.manual_seed(52)
        pool.begin_step()
        xg = x.clone().requires_grad_()
        with ta.fused_dstate_training(on):
            y = m(xg)
            y.float().square().mean().backward()
        masks[on] = pool.buf32.clone()
        res[on] = (y.detach().double().reshape(-1), xg.grad.double().reshape(-1))
        assert bool(torch.isfinite(res[on][0]).all()) and bool(torch.isfinite(res[on][1]).all())
    assert torch.equal(masks[True], masks[False]) and bool((masks[True] == 0).any()) and bool((masks[True] != 0).any())
    for a, b in zip(res[True], res[False]):
        cos, ratio = float(a @ b / (a.norm() * b.norm())), float(a.norm() / b.norm())
        print(f"fused against plugin, same masks: cosine {cos:.5f} norm ratio {ratio:.4f}")
        assert cos >= 0.998 and abs(ratio - 1) <= 0.04


# ----------------------------------------------------------------------------- graph
class _Tiny(torch.nn.Module):
    def __init__(self):
        import tramba_amd as ta
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 16, 1)
        self.block = ta.VSSBlock(hidden_dim=16, ssm_d_state=16, channel_first=True, drop_path=0.0)
        self.head = torch.nn.Conv2d(16, 1, 1)
        self.compute_dtype = BF16

    def forward(self, x):
        return [self.head(self.block(self.stem(x).to(BF16)).float())]


def test_graphed_train_step_at_dstate_16():
    """GraphedTrainStep over a tiny model holding one VSSBlock(ssm_d_state=16) in bf16, switch on, several segments: it
    captures; the first loss equals the eager step's to rel 1e-5; three replays' losses follow the eager steps' (rtol 3e-2);
    two captures from the same state replay to equal losses bit for bit"""
    import tramba_amd as ta
    from tramba_amd import train
    assert hip().ss2d_scan_n_bwd_plan(2, 576, 32, 4, 16)[1] > 1
    x = torch.randn(2, 3, 24, 24, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = (torch.rand(2, 1, 24, 24, generator=torch.Generator().manual_seed(1)) > 0.6).float().to(DEV)
    torch.manual_seed(61)
    state = {k_: v.clone() for k_, v in _Tiny().state_dict().items()}

    def fresh():
        m = _Tiny().to(DEV).train()
        m.load_state_dict(state)
        return m

    with ta.fused_dstate_training(True):
        m = fresh()
        assert m.block.op.d_inner == 32 and m.block.op.k_group == 4
        opt = train.get_opt(1e-3, m)
        eager = [float(train.train_step(m, opt, x, y)) for _ in range(3)]
        runs = []
        for _ in range(2):
            m = fresh()
            step = ta.GraphedTrainStep(m, train.get_opt(1e-3, m, capturable=True))
            runs.append([float(step(x, y)) for _ in range(3)])
            torch.cuda.synchronize()
    print("eager", eager, "graphed", runs)
    assert abs(runs[0][0] - eager[0]) <= 1e-5 * abs(eager[0])
    np.testing.assert_allclose(runs[0], eager, rtol=3e-2)
    assert runs[0] == runs[1]
    hip().device_error()
