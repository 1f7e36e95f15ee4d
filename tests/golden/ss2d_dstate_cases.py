"""Inputs, fp64 references and an fp32 restatement of the kernel arithmetic for the fused channels-last SS2D scan at d_state
N = 2..16 (hip.ss2d_scan_n_cl; tests/test_ss2d_dstate_host.py, tests/test_gpu_ss2d_dstate.py,
scripts/measure_ss2d_dstate_parity.py).

Two families of inputs:
  core cases    drawn as tests/test_gpu_kernels.py::test_ss2d_fused_core draws them (dt_bias ~ N(-2, 0.5), A in -[0.5, 1.5]),
                with x_proj_weight (K, R + 2N, D) and A_logs (K*D, N); the reference is oracle.ops.ss2d_core in fp64.
  memory cases  the `slow` and `undamped` regimes of scan_memory_cases.make, A and (B, C) extended to N columns (A per
                state as make_boundary draws it); x_dbl is built on the host, pre-rounded as that module explains, and the
                reference is the fp64 recurrence position by position.
The fp32 restatement (terms32) is ScanWave's documented form: the dt_proj operands rounded to bf16 (hi + lo split without
the lo * lo product for fp32 activations), t = med3(log2(1 + exp2(x')), x', 128), a_n = exp2(t A_n), bb_n = t (B_n ln2) u.
It exists to size tolerances, never to stand in for the kernel."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

import scan_memory_cases as smc
from oracle import ops as oo
from oracle import scan_tables as st

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TILE = 32

# (b, h, D, R, family, N): the smallest shapes that reach each code path of ss2d_seg_n_kernel (asserted through the plan query)
CORE_CASES = {
    "single_launch": (1, 12, 32, 2, "raster", 2),        # 5 tiles: one segment of 6 (one padding tile), PASS 1 alone
    "segments_k8": (1, 24, 64, 4, "helix", 16),          # 18 tiles in 9 segments of 2, K = 8, two channel tiles
    "d40_window": (1, 16, 40, 3, "window", 3),           # D % 32 != 0: the second channel tile is 8 channels wide
    "d40_dilation": (1, 16, 40, 3, "dilation", 3),
    "ragged_r1": (1, 14, 32, 1, "helix", 5),             # L = 196: 7 tiles, the last 4 positions wide; the last segment's second
                                                         # tile is padding; R = 1
    "fold_unrolled": (2, 48, 32, 8, "helix", 8),         # 36 segments: the 8-wide unrolled fold and its remainder, two batches
    "rank40": (1, 12, 96, 40, "raster", 16),             # three MFMA rank blocks
    "rank64": (1, 24, 32, 64, "raster", 12),             # four
}
SINGLE_PASS = CORE_CASES["single_launch"]
MULTI_SEG = CORE_CASES["segments_k8"]
MANY_SEG = CORE_CASES["fold_unrolled"]
CORE_TOL = {F32: 2e-4, BF16: 4e-2, F16: 4e-2}       # rtol = atol after merge + out_norm + GELU (test_ss2d_fused_core's figures)


def k_of(fam):
    return 8 if fam == "helix" else 4


def rank_pad(r):
    return (r + 7) & ~7


def group_stride(r, n):
    return rank_pad(r) + ((2 * n + 3) & ~3)


def table_of(fam, h):
    return torch.from_numpy(np.ascontiguousarray(st.table(fam, h, h))).long()


def pad_weight(wx, n):
    """(K, R + 2N, D) -> (K * RG, D), the documented layout (restated here, so that the library's is tested against it)"""
    k, c, d = wx.shape
    r = c - 2 * n
    rg, r8 = group_stride(r, n), rank_pad(r)
    w = wx.new_zeros(k, rg, d)
    w[:, :r] = wx[:, :r]
    w[:, r8:r8 + 2 * n] = wx[:, r:]
    return w.reshape(k * rg, d)


# ----------------------------------------------------------------------------- core cases
@functools.lru_cache(maxsize=None)
def core_case(cfg, dtype):
    """-> namespace with the drawn tensors, the fp64 per-direction `ys_want` (B, K, L, D) and `want` (B, H, W, D) after
    merge + out_norm + GELU"""
    b, h, d, r, fam, n = cfg
    k = k_of(fam)
    g = torch.Generator().manual_seed(h * d + k + 31 * n)
    x = torch.randn(b, d, h, h, generator=g).to(dtype)
    wx = (torch.randn(k, r + 2 * n, d, generator=g) * d ** -0.5).to(dtype)
    wdt = torch.randn(k, d, r, generator=g) * r ** -0.5
    dtb = torch.randn(k, d, generator=g) * 0.5 - 2.0
    a_logs = torch.log(0.5 + torch.rand(k * d, n, generator=g))
    ds = 1 + 0.1 * torch.randn(k * d, generator=g)
    lw, lb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ys_want = oo.ss2d_core(x.double(), wx.double(), wdt.double(), dtb.double(), a_logs.double(), ds.double(), fam, merge=False)
    y = oo.cross_merge(ys_want.permute(0, 1, 3, 2), fam, h, h).reshape(b, d, h, h)
    want = F.gelu(oo.layernorm2d(y, lw.double(), lb.double())).permute(0, 2, 3, 1).contiguous()
    return types.SimpleNamespace(cfg=cfg, b=b, h=h, d=d, r=r, fam=fam, n=n, k=k, l=h * h, dtype=dtype, x=x, wx=wx, wdt=wdt,
                                 dtb=dtb, a_logs=a_logs, a_neg=-torch.exp(a_logs), ds=ds, lw=lw, lb=lb, ys_want=ys_want, want=want)


def core_as_scan_case(c):
    """a core case in the layout of the memory cases (x channels-last, x_dbl from an fp32 GEMM on the padded weight)"""
    xc = c.x.permute(0, 2, 3, 1).reshape(c.b, c.l, c.d).contiguous()
    xdbl = xc.float() @ pad_weight(c.wx, c.n).float().t()
    return types.SimpleNamespace(b=c.b, h=c.h, d=c.d, r=c.r, k=c.k, l=c.l, n=c.n, rg=group_stride(c.r, c.n), fam=c.fam,
                                 dtype=c.dtype, table=table_of(c.fam, c.h), x=xc, xdbl=xdbl, dt_w=c.wdt,
                                 dt_b=c.dtb.reshape(-1), A=c.a_neg, ds=c.ds)


# ----------------------------------------------------------------------------- memory cases
MEMORY_SHAPE = ("helix", 48, 32, 4)      # family, h, D, R: L = 2304 = 72 tiles, K = 8, one channel tile: 36 segments of 2


@functools.lru_cache(maxsize=None)
def memory_case(regime, n, dtype, seed=0):
    fam, h, d, r = MEMORY_SHAPE
    b = 1
    tbl = table_of(fam, h)
    k, l = tbl.shape
    rg, r8 = group_stride(r, n), rank_pad(r)
    g = torch.Generator().manual_seed(1000 * seed + 7 * h + d + r + k + 100 * n)
    x = torch.randn(b, l, d, generator=g).to(dtype)
    ranks = 0.5 * torch.randn(b, l, k, r, generator=g)
    bc = torch.randn(b, l, k, 2 * n, generator=g)
    dt_w = torch.randn(k, d, r, generator=g) * r ** -0.5
    ds = 1 + 0.1 * torch.randn(k, d, generator=g)
    if regime == "slow":
        dt_b = torch.randn(k, d, generator=g) * 0.5 - 1.0
        a = torch.stack([smc._slow_a(g, k, d, specials=True) for _ in range(n)], -1)
    elif regime == "undamped":
        dt_b = torch.randn(k, d, generator=g) * 0.3 - 3.0
        a = torch.zeros(k, d, n)
    else:
        raise ValueError(regime)
    if dtype != F32:
        ranks, dt_w, dt_b = smc._bf16(ranks), smc._prescaled_bf16(dt_w), smc._prescaled_hilo(dt_b)
    xdbl = torch.zeros(b, l, k, rg)
    xdbl[..., :r] = ranks
    xdbl[..., r8:r8 + 2 * n] = bc
    return types.SimpleNamespace(regime=regime, b=b, h=h, d=d, r=r, k=k, l=l, n=n, rg=rg, fam=fam, dtype=dtype, table=tbl, x=x,
                                 xdbl=xdbl.view(b, l, k * rg), dt_w=dt_w.contiguous(), dt_b=dt_b.reshape(-1).contiguous(),
                                 A=a.reshape(k * d, n).contiguous(), ds=ds.reshape(-1).contiguous())


# ----------------------------------------------------------------------------- the terms of image i, (L, S = K*D, N)
def _gather(c, i, dt):
    tbl, k, l, d, r, n, rg = c.table, c.k, c.l, c.d, c.r, c.n, c.rg
    r8 = rank_pad(r)
    u = c.x[i].to(dt)[tbl].permute(1, 0, 2).reshape(l, k * d)
    rows = torch.stack([c.xdbl[i].view(l, k, rg)[tbl[j], j] for j in range(k)]).to(dt)         # (K, L, RG)
    spread = lambda v: v.permute(1, 0, 2).reshape(l, k, 1, n).expand(l, k, d, n).reshape(l, k * d, n)
    return u, rows[..., :r], spread(rows[..., r8:r8 + n]), spread(rows[..., r8 + n:r8 + 2 * n])


def terms64(c, i):
    u, ranks, bv, cv = _gather(c, i, torch.float64)
    raw = torch.einsum("klr,kdr->lkd", ranks, c.dt_w.double()).reshape(c.l, -1)
    dt = F.softplus(raw + c.dt_b.double())[..., None]
    return dict(a=torch.exp(dt * c.A.double()), bb=dt * bv * u[..., None], C=cv, Du=c.ds.double() * u)


def terms32(c, i):
    u, ranks, bv, cv = _gather(c, i, torch.float32)
    w2 = c.dt_w * smc.LOG2E_F
    mm = lambda p, q: torch.einsum("klr,kdr->lkd", p, q).reshape(c.l, -1)
    if c.dtype == F32:
        (rh, rl), (wh, wl) = smc._hilo(ranks), smc._hilo(w2)
        x2 = mm(rh, wh) + mm(rh, wl) + mm(rl, wh)
    else:
        x2 = mm(smc._bf16(ranks), smc._bf16(w2))
    x2 = x2 + c.dt_b * smc.LOG2E_F
    t = torch.log2(1.0 + torch.exp2(x2))
    t = torch.maximum(torch.minimum(t, x2), torch.minimum(torch.maximum(t, x2), torch.tensor(128.0)))[..., None]   # v_med3_f32
    return dict(a=torch.exp2(t * c.A), bb=t * ((bv * smc.LN2_F) * u[..., None]), C=cv, Du=c.ds * u)


def _ys(c, outs):
    return torch.stack([o["y"].reshape(c.l, c.k, c.d).permute(1, 0, 2) for o in outs])       # (B, K, L, D)


def reference(c):
    """fp64, position by position -> ys (B, K, L, D)"""
    return _ys(c, [smc._sequential(terms64(c, i), False) for i in range(c.b)])


def emulate(c, nt_seg=None):
    """fp32 in the kernel's arithmetic: position by position, or tile-wise with the aggregates folded by segments of nt_seg tiles"""
    if nt_seg is None:
        return _ys(c, [smc._sequential(terms32(c, i), False) for i in range(c.b)])
    return _ys(c, [smc._tiled(terms32(c, i), False, nt_seg) for i in range(c.b)])


@functools.lru_cache(maxsize=None)
def memory_e32(regime, n, dtype, nt_seg):
    """-> (case, fp64 ys, E32 = (max-relative, rms-relative)): the larger error of the two fp32 evaluations, as smc.e32"""
    c = memory_case(regime, n, dtype)
    ref = reference(c)
    errs = [smc.rel_errors(ev, ref) for ev in (emulate(c), emulate(c, nt_seg))]
    return c, ref, tuple(max(e[m] for e in errs) for m in (0, 1))


@functools.lru_cache(maxsize=None)
def _core_emulated_ys(cfg, dtype, nt_seg):
    return emulate(core_as_scan_case(core_case(cfg, dtype)), nt_seg)


def core_emulated(c, ys_dtype, nt_seg):
    """the fp32 evaluation of a core case carried to the tested output: ys rounded to ys_dtype, fp32 merge + out_norm + GELU,
    rounded to the activation dtype -> (B, H, W, D) float64"""
    ys = _core_emulated_ys(c.cfg, c.dtype, nt_seg).to(ys_dtype).float()
    y = oo.cross_merge(ys.permute(0, 1, 3, 2), c.fam, c.h, c.h).reshape(c.b, c.d, c.h, c.h)
    out = F.gelu(oo.layernorm2d(y, c.lw, c.lb)).permute(0, 2, 3, 1)
    return out.to(c.dtype).double()


def tolerance_share(got, want, tol):
    """max |got - want| / (atol + rtol |want|): <= 1 passes np.testing.assert_allclose(rtol = atol = tol)"""
    return float(((got.double() - want).abs() / (tol + tol * want.abs())).max())


# ----------------------------------------------------------------------------- device runs (H = tramba_amd.hip)
def device_args(H, c, dev):
    if not hasattr(c, "dev"):
        order = H.scan_order(c.fam, c.h, c.h, dev)
        assert torch.equal(order.table.cpu().long(), c.table), "the library's scan table is not the oracle's"
        c.dev = (c.x.to(dev), c.xdbl.to(dev), order, c.dt_w.to(dev), c.dt_b.to(dev), c.A.to(dev), c.ds.to(dev))
    return c.dev


def plugin_scan(H, c, dev):
    """what SS2D._core_plugin_cl does with the same operands: K-fold gather, dts by a framework einsum, the reference-layout
    scan (hip.selective_scan_fwd) -> ys (B, K, L, D) f32"""
    tbl, k, l, d, r, n, rg = c.table.to(dev), c.k, c.l, c.d, c.r, c.n, c.rg
    r8 = rank_pad(r)
    xs = c.x.to(dev)[:, tbl]                                          # (B, K, L, D)
    rows = torch.stack([c.xdbl.to(dev).view(c.b, l, k, rg)[:, tbl[j], j] for j in range(k)], 1)      # (B, K, L, RG)
    dts = torch.einsum("bklr,kdr->bkdl", rows[..., :r].to(c.dtype), c.dt_w.to(dev).to(c.dtype))
    bs = rows[..., r8:r8 + n].permute(0, 1, 3, 2).to(c.dtype).contiguous()
    cs = rows[..., r8 + n:r8 + 2 * n].permute(0, 1, 3, 2).to(c.dtype).contiguous()
    u = xs.permute(0, 1, 3, 2).reshape(c.b, k * d, l).contiguous()
    out, _ = H.selective_scan_fwd(u, dts.reshape(c.b, k * d, l).contiguous(), c.A.to(dev), bs, cs, c.ds.to(dev), c.dt_b.to(dev),
                                  True, True)
    return out.view(c.b, k, d, l).permute(0, 1, 3, 2).float()


def memory_records(H, dev, regime, n, dtype):
    """the rule of scan_memory_cases.check on the new path (both ys dtypes of a 16-bit input) and, for the record, the
    plugin path's error on the same operands"""
    nt, nseg = H.ss2d_scan_n_plan(1, MEMORY_SHAPE[1] ** 2, MEMORY_SHAPE[2], 8, n)
    c, ref, e = memory_e32(regime, n, dtype, nt)
    args = device_args(H, c, dev)
    label = f"{regime} N={n} {str(dtype)[6:]} helix48 D=32 nseg={nseg}"
    recs = []
    for ys_dtype in ([F32] if dtype == F32 else [F32, dtype]):
        ys = H.ss2d_scan_n_cl(*args, ys_dtype)
        recs.append(dict(smc.record(label, "ys", ys, ref, e, ys_dtype), path="fused"))
    pe = smc.rel_errors(plugin_scan(H, c, dev).cpu(), ref)
    recs.append(dict(case=label, output="ys", out_dtype="float32", path="plugin", e32_max=e[0], e32_rms=e[1], err_max=pe[0],
                     err_rms=pe[1]))
    return recs
