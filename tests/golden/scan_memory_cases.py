"""Selective-scan inputs whose recurrence state outlives many 32-position tiles, an fp64 reference of the fused scan, and an
fp32 emulation of the kernels' arithmetic that exists ONLY to size tolerances and to show that the tests have teeth
(tests/test_scan_memory_host.py, tests/test_gpu_scan_memory.py, scripts/measure_scan_memory_parity.py).

Regimes (every tensor is a function of (regime, shape, dtype, seed)):
  slow      dt_bias ~ N(-1, 0.5) (dt ~ 0.3, softplus well conditioned), A log-uniform in -[0.002, 0.05]: a decay of 0.985 ..
            0.9994 per position, a memory of 70 .. 1600 positions.  Where A is passed as a negative value (not as A_logs) the
            first channels of every direction have A = 0 (undamped) and the next ones A = -30 (the state dies within one
            position, exp2 underflows, A_tile == 0): 4 + 4 channels, or a quarter + a quarter of a direction narrower than 16.
  undamped  A = 0, dt_bias ~ N(-3, 0.3): h = cumsum(dt B u), every lost or doubled hand-over shifts the rest of the sequence.
  init      Dt_init / A_log_init of tramba_amd/modules.py (dt 1e-3 .. 1e-1, A = -1, passed as A_logs): where training starts.
  existing  the recipe of the older scan tests (dt_bias ~ N(-2, 0.5), A in -[0.5, 1.5], unit-variance rank rows): the state
            dies inside one tile.  Only test_scan_memory_host.py uses it, to document why this file exists.

Exact inputs.  x_dbl is built on the host.  The 16-bit kernels (ScanWave<.., SPLIT = false>) round two operands to bf16 before
the dt_proj MFMA, for fp16 activations too: the dt-rank rows of x_dbl, and dt_w * log2(e).  Both are pre-rounded here (dt_w is
chosen so that fl32(dt_w * log2e) IS a bf16 value), so that the in-kernel rounding is a no-op.  The LDS-DMA kernel at padded
rank 8 also feeds dt_bias * log2(e) to the MFMA as a bf16 (hi, lo) pair; dt_bias is chosen so that the pair holds it to an fp32 ulp.
x (and the incoming gradient) are rounded to the activation dtype; B, C, A, D stay fp32.  fp32 activations are not pre-rounded:
that path splits both MFMA operands into bf16 hi + lo and drops the lo * lo product, which the emulation restates."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import scan_tables as st
from oracle import selective_scan as oss

TILE = 32
LOG2E_F = float(np.float32(1.44269504088896))
LN2_F = float(np.float32(0.693147180559945))
LOG2E = 1.4426950408889634
U_ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # elementwise allowance of a 16-bit output
FACTOR = 8.0      # bound = FACTOR * E32: hardware exp2 / log2 (<= 1 ulp each), fold order of the aggregates, MFMA summation order
# Outputs whose fp32 bound needs more than FACTOR * E32, with the reason (tests/test_gpu_scan_memory.py docstrings repeat it).
# gA (dL/dA or dL/dA_logs of the fused backward): both of its factors, the state h and the adjoint gh, are sums over the whole
# memory of a channel, so an error of the per-position decay a = exp2(t A) enters it twice.  Where the decay is slow that error
# is not noise: near a = 1 one ulp of a is 1e-4 of log(a) at A = -0.002, and the hardware exp2 is within an ulp but not
# correctly rounded.  With a decay that is off by up to one ulp in ONE direction the emulation moves gA 2.4 times as far as ys
# and the other gradients (test_scan_memory_host.py::test_ga_is_the_output_most_sensitive_to_the_decay asserts 2 .. 2.5), and
# the kernel's gA, the largest element of which belongs to the slowest channel, sits at 9 x E32 where its ys sits at 3.6 x.
FACTOR_FOR = {"gA": 2.5 * FACTOR}


def group_stride(r):
    return ((r + 7) & ~7) + 4


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _prescaled_bf16(v):
    """fp32 w with fl32(w * log2e) exactly the bf16 value nearest v * log2e"""
    target = _bf16(v.float() * LOG2E_F)
    w = (target.double() / LOG2E).float()
    assert torch.equal(_bf16(w * LOG2E_F), target)
    return w


def _prescaled_hilo(v):
    """fp32 b whose fl32(b * log2e) a bf16 (hi, lo) pair holds to within an fp32 ulp"""
    b2 = v.float() * LOG2E_F
    hi = _bf16(b2)
    target = hi + _bf16(b2 - hi)
    b = (target.double() / LOG2E).float()
    got = b * LOG2E_F
    h2 = _bf16(got)
    assert bool(((h2 + _bf16(got - h2) - got).abs() <= 2.0 ** -22 * got.abs()).all())
    return b


def n_special(dper):
    return 4 if dper >= 16 else dper // 4


def _slow_a(gen, k, d, specials):
    a = -torch.exp(torch.rand(k, d, generator=gen) * (math.log(0.05) - math.log(0.002)) + math.log(0.002))
    if specials:
        ns = n_special(d)
        a[:, :ns] = 0.0
        a[:, ns:2 * ns] = -30.0
    return a


def make(regime, fam, h, b, d, r, dtype, seed=0, a_log=False):
    """-> namespace: x, gym (B, L, D) `dtype`; xdbl (B, L, K*RG) f32; dt_w (K, D, R), dt_b, A, ds (K*D) f32 (A is A_logs when
    a_log), table (K, L) int64, k, l, r, rg"""
    tbl = torch.from_numpy(np.ascontiguousarray(st.table(fam, h, h))).long()
    k, l = tbl.shape
    rg = group_stride(r)
    g = torch.Generator().manual_seed(1000 * seed + 7 * h + d + r + k)
    lowp = dtype != torch.float32
    x = torch.randn(b, l, d, generator=g).to(dtype)
    gym = torch.randn(b, l, d, generator=g).to(dtype)
    ranks = (1.0 if regime == "existing" else 0.5) * torch.randn(b, l, k, r, generator=g)
    bc = torch.randn(b, l, k, 2, generator=g)
    dt_w = torch.randn(k, d, r, generator=g) * r ** -0.5
    ds = 1 + 0.1 * torch.randn(k, d, generator=g)
    if regime == "slow":
        dt_b = torch.randn(k, d, generator=g) * 0.5 - 1.0
        a = _slow_a(g, k, d, specials=not a_log)
    elif regime == "undamped":
        assert not a_log, "A = 0 has no A_logs"
        dt_b = torch.randn(k, d, generator=g) * 0.3 - 3.0
        a = torch.zeros(k, d)
    elif regime == "existing":
        dt_b = torch.randn(k, d, generator=g) * 0.5 - 2.0
        a = -(0.5 + torch.rand(k, d, generator=g))
    elif regime == "init":
        from tramba_amd import modules as M
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(g.initial_seed())
            projs = [M.Dt_init(r, d) for _ in range(k)]
            a_logs = M.A_log_init(1, d, copies=k).detach().reshape(k, d)
        dt_w = torch.stack([p.weight.detach() for p in projs])
        dt_b = torch.stack([p.bias.detach() for p in projs])
        a = -torch.exp(a_logs)
    else:
        raise ValueError(regime)
    if lowp:
        ranks, dt_w, dt_b = _bf16(ranks), _prescaled_bf16(dt_w), _prescaled_hilo(dt_b)
    xdbl = torch.zeros(b, l, k, rg)
    xdbl[..., :r] = ranks
    xdbl[..., rg - 4:rg - 2] = bc
    A = torch.log(-a) if a_log else a
    return types.SimpleNamespace(regime=regime, fam=fam, h=h, b=b, d=d, r=r, k=k, l=l, rg=rg, dtype=dtype, a_log=a_log, table=tbl,
                                 x=x, gym=gym, xdbl=xdbl.view(b, l, k * rg), dt_w=dt_w.contiguous(),
                                 dt_b=dt_b.reshape(-1).contiguous(), A=A.reshape(-1).contiguous(), ds=ds.reshape(-1).contiguous())


def make_boundary(regime, nb, k, dper, n, l, dtype, seed=0):
    """operands of the boundary op selective_scan_fwd / _bwd: u, delta (nb, KD, L), B, C (nb, K, N, L) in `dtype`; A (KD, N), D,
    delta_bias (KD) f32; dout (nb, KD, L) f32"""
    g = torch.Generator().manual_seed(1000 * seed + l + 10 * n + k * dper)
    kd = k * dper
    r = lambda *s: torch.randn(*s, generator=g)
    o = types.SimpleNamespace(regime=regime, nb=nb, k=k, dper=dper, n=n, l=l, dtype=dtype)
    o.u, o.delta = r(nb, kd, l).to(dtype), (0.5 * r(nb, kd, l)).to(dtype)
    o.B, o.C = r(nb, k, n, l).to(dtype), r(nb, k, n, l).to(dtype)
    o.D = 1 + 0.1 * r(kd)
    o.dout = r(nb, kd, l)
    if regime == "slow":
        o.delta_bias = 0.5 * r(kd) - 1.0
        o.A = torch.stack([_slow_a(g, k, dper, specials=True).reshape(kd) for _ in range(n)], 1).contiguous()
    elif regime == "undamped":
        o.delta_bias = 0.3 * r(kd) - 3.0
        o.A = torch.zeros(kd, n)
    else:
        raise ValueError(regime)
    return o


# ----------------------------------------------------------------------------- operands in sequence order, (L, S, N) layout
def _gather(c, i, dt):
    """image i of a fused-scan case -> u, gy (L, S), ranks (K, L, R), Bv, Cv (L, S, 1) views; S = K * D rows"""
    tbl, k, l, d, r, rg = c.table, c.k, c.l, c.d, c.r, c.rg
    u = c.x[i].to(dt)[tbl].permute(1, 0, 2).reshape(l, k * d)
    gy = c.gym[i].to(dt)[tbl].permute(1, 0, 2).reshape(l, k * d)
    rows = torch.stack([c.xdbl[i].view(l, k, rg)[tbl[j], j] for j in range(k)]).to(dt)         # (K, L, RG)
    spread = lambda v: v.t().reshape(l, k, 1).expand(l, k, d).reshape(l, k * d, 1)
    return u, gy, rows[..., :r], spread(rows[..., rg - 4]), spread(rows[..., rg - 3])


def _terms64(c, i):
    u, gy, ranks, bv, cv = _gather(c, i, torch.float64)
    raw = torch.einsum("klr,kdr->lkd", ranks, c.dt_w.double()).reshape(c.l, -1)
    A = (-torch.exp(c.A.double()) if c.a_log else c.A.double()).reshape(-1, 1)
    dt = F.softplus(raw + c.dt_b.double())[..., None]
    return dict(a=torch.exp(dt * A), bb=dt * bv * u[..., None], C=cv, Du=c.ds.double() * u, u=u, gy=gy, dt=dt, A=A, B=bv,
                D=c.ds.double())


def _hilo(t):
    hi = _bf16(t)
    return hi, _bf16(t - hi)


def _terms32(c, i, biased_exp=False):
    """the per-element terms as ScanWave::terms forms them, in fp32: x' = <ranks, dt_w log2e> + bias log2e on bf16 operands (hi
    + lo split without the lo * lo product for fp32 activations), t = log2(1 + exp2(x')) = dt log2e, a = exp2(t A),
    bb = t (B ln2 u).  biased_exp: the decay rounded toward zero instead of to nearest (within one ulp, all
    errors in one direction), to see which output an exp2 that is not correctly rounded moves most"""
    u, gy, ranks, bv, cv = _gather(c, i, torch.float32)
    w2 = c.dt_w * LOG2E_F
    mm = lambda p, q: torch.einsum("klr,kdr->lkd", p, q).reshape(c.l, -1)
    if c.dtype == torch.float32:
        (rh, rl), (wh, wl) = _hilo(ranks), _hilo(w2)
        x2 = mm(rh, wh) + mm(rh, wl) + mm(rl, wh)
    else:
        x2 = mm(_bf16(ranks), _bf16(w2))
    x2 = x2 + c.dt_b * LOG2E_F
    t = torch.log2(1.0 + torch.exp2(x2))
    t = torch.maximum(torch.minimum(t, x2), torch.minimum(torch.maximum(t, x2), torch.tensor(128.0)))[..., None]   # v_med3_f32
    A = (-torch.exp(c.A) if c.a_log else c.A).reshape(-1, 1)
    a = torch.exp2(t * A)
    if biased_exp:
        a64 = torch.exp2((t * A).double())
        a = a64.float()
        a = torch.where(a.double() > a64, torch.nextafter(a, torch.zeros_like(a)), a)
    return dict(a=a, bb=t * ((bv * LN2_F) * u[..., None]), C=cv, Du=c.ds * u, u=u, gy=gy, dt=t * LN2_F, A=A, B=bv,
                D=c.ds)


def _bterms(o, dt_):
    """boundary-op operands in the same layout; fp32: softplus as selective_scan.hip's softplus_lean"""
    l, kd, n, nb = o.l, o.k * o.dper, o.n, o.nb
    f = lambda t: t.to(dt_)
    u = f(o.u).permute(2, 0, 1).reshape(l, nb * kd)
    gy = f(o.dout).permute(2, 0, 1).reshape(l, nb * kd)
    x = (f(o.delta) + f(o.delta_bias)[None, :, None]).permute(2, 0, 1).reshape(l, nb * kd)
    if dt_ == torch.float64:
        dt = F.softplus(x)
    else:
        dt = torch.maximum(x, torch.log2(1.0 + torch.exp2(torch.clamp(x, max=60.0) * LOG2E_F)) * LN2_F)
    dt = dt[..., None]
    spread = lambda v: f(v).permute(3, 0, 1, 2).reshape(l, nb, o.k, 1, n).expand(l, nb, o.k, o.dper, n).reshape(l, nb * kd, n)
    A = f(o.A).repeat(nb, 1)
    D = f(o.D).repeat(nb)
    bv, cv = spread(o.B), spread(o.C)
    a = torch.exp(dt * A) if dt_ == torch.float64 else torch.exp2((dt * A) * LOG2E_F)
    return dict(a=a, bb=dt * bv * u[..., None], C=cv, Du=D * u, u=u, gy=gy, dt=dt, A=A, B=bv, D=D)


# ----------------------------------------------------------------------------- the recurrence, sequential and tile-wise
def _sequential(t, backward):
    """position by position in the dtype of the terms -> y (L, S), the state entering every tile (NT, S, N) and, with
    `backward`, the gradients"""
    a, bb = t["a"], t["bb"]
    l, s, n = a.shape
    h = torch.zeros(s, n, dtype=a.dtype)
    hs = torch.empty_like(a)
    entering = []
    for p in range(l):
        if p % TILE == 0:
            entering.append(h)
        h = a[p] * h + bb[p]
        hs[p] = h
    out = dict(y=(t["C"] * hs).sum(-1) + t["Du"], states=torch.stack(entering))
    if backward:
        gh = torch.empty_like(a)
        z = torch.zeros(s, n, dtype=a.dtype)
        cg = t["C"] * t["gy"][..., None]
        for p in range(l - 1, -1, -1):
            gh[p] = cg[p] + z
            z = a[p] * gh[p]
        hp = torch.cat([torch.zeros(1, s, n, dtype=a.dtype), hs[:-1]])
        out.update(_emit(t, hs, hp, gh, sequential=True))
    return out


def _emit(t, hs, hp, gh, sequential):
    """the per-position outputs and the parameter sums of the backward from h (after / before every position) and gh"""
    a, dt, u, gy = t["a"], t["dt"], t["u"], t["gy"]
    gdt = (gh * (a * t["A"] * hp + t["B"] * u[..., None])).sum(-1)
    graw = gdt * (1.0 - torch.exp(-dt[..., 0]))
    gu = t["D"] * gy + (gh * dt * t["B"]).sum(-1)
    tot = (lambda v: v.cumsum(0)[-1]) if sequential else (lambda v: v.sum(0))     # one accumulator / per-wave partial sums
    return dict(gu=gu, graw=graw, eb=gh * dt * u[..., None], ec=gy[..., None] * hs, gA=tot(gh * hp * a * dt), gD=tot(gy * u),
                gbias=tot(graw))


FAULTS = ("drop_old", "edge8", "edge16", "atile", "seg_skip", "state_shift", "adj_edge8", "adj_atile")


def _tiled(t, backward, nt_seg=None, fault=None):
    """tile-wise: 32-position tiles reduced to (A_tile, H_tile), folded tile by tile along the chain (the register-ring and
    LDS-DMA forms; W only decides which wave owns a tile) or, with nt_seg, segment by segment (two-pass wave-segment form), the
    positions of a tile replayed from the state entering it.  `fault` (CPU only) breaks one hand-over rule."""
    a, bb = t["a"], t["bb"]
    l, s, n = a.shape
    ntile = (l + TILE - 1) // TILE
    pad = ntile * TILE - l
    if pad:       # positions past the end are the identity, as in the kernels
        a = torch.cat([a, torch.ones(pad, s, n, dtype=a.dtype)])
        bb = torch.cat([bb, torch.zeros(pad, s, n, dtype=a.dtype)])
    a4, b4 = a.view(ntile, TILE, s, n), bb.view(ntile, TILE, s, n)
    pa, ph = torch.empty_like(a4), torch.empty_like(b4)          # inclusive prefixes from a zero state
    ca, ch = torch.ones_like(a4[:, 0]), torch.zeros_like(a4[:, 0])
    for j in range(TILE):
        ch = a4[:, j] * ch + b4[:, j]
        ca = ca * a4[:, j]
        pa[:, j], ph[:, j] = ca, ch
    ta, th = pa[:, -1].clone(), ph[:, -1]
    if fault == "atile":
        ta = pa[:, -2].clone()                                    # A_tile lacks its last factor
    hin = torch.zeros(ntile, s, n, dtype=a.dtype)
    if nt_seg is None:
        w_edge = {"edge8": 8, "edge16": 16}.get(fault)
        for i in range(1, ntile):
            prev = hin[i - 1] * (0.0 if fault == "drop_old" else 1.0)
            hin[i] = ta[i - 1] * prev + th[i - 1]
            if w_edge and i % w_edge == 0:
                hin[i] = 0.0                                      # the carry into a super-chunk is lost
    else:
        nseg = (ntile + nt_seg - 1) // nt_seg
        sa, sh = [], []
        for g in range(nseg):                                     # pass 0: a segment's aggregate
            ra, rh = torch.ones(s, n, dtype=a.dtype), torch.zeros(s, n, dtype=a.dtype)
            for i in range(g * nt_seg, min((g + 1) * nt_seg, ntile)):
                rh = ta[i] * rh + th[i]
                ra = ra * ta[i]
            sa.append(ra)
            sh.append(rh)
        for g in range(nseg):                                     # pass 1: fold the preceding segments, walk the tiles
            hcur = torch.zeros(s, n, dtype=a.dtype)
            for q in range(g):
                if fault == "seg_skip" and q == g - 1 and g >= 2:
                    continue                                      # the fold stops one segment short
                hcur = sa[q] * hcur + sh[q]
            for i in range(g * nt_seg, min((g + 1) * nt_seg, ntile)):
                hin[i] = hcur
                hcur = ta[i] * hcur + th[i]
    hs = (pa * hin[:, None] + ph).reshape(ntile * TILE, s, n)[:l]
    states = hin
    if fault == "state_shift":
        states = torch.cat([hin[1:], hin[-1:]])                   # every saved state is the next tile's
    out = dict(y=(t["C"] * hs).sum(-1) + t["Du"], states=states)
    if backward:
        hin_b = states                                            # the backward replays from the SAVED states
        hs_b = (pa * hin_b[:, None] + ph)
        hp_b = torch.cat([hin_b[:, None], hs_b[:, :-1]], 1).reshape(ntile * TILE, s, n)[:l]
        hs_b = hs_b.reshape(ntile * TILE, s, n)[:l]
        cg = t["C"] * t["gy"][..., None]
        if pad:
            cg = torch.cat([cg, torch.zeros(pad, s, n, dtype=a.dtype)])
        c4 = cg.view(ntile, TILE, s, n)
        qa, qz = torch.empty_like(a4), torch.empty_like(a4)       # suffix aggregates: z leaving position j leftwards
        ra, rz = torch.ones_like(a4[:, 0]), torch.zeros_like(a4[:, 0])
        for j in range(TILE - 1, -1, -1):
            qa[:, j], qz[:, j] = ra, rz                           # what enters position j from its right
            rz = a4[:, j] * (c4[:, j] + rz)
            if not (fault == "adj_atile" and j == 0):
                ra = ra * a4[:, j]
        zin = torch.zeros(ntile, s, n, dtype=a.dtype)
        for i in range(ntile - 2, -1, -1):
            zin[i] = ra[i + 1] * zin[i + 1] + rz[i + 1]
            if fault == "adj_edge8" and (i + 1) % 8 == 0:
                zin[i] = 0.0                                      # the adjoint entering a super-chunk from its right is lost
        gh = (c4 + qa * zin[:, None] + qz).reshape(ntile * TILE, s, n)[:l]
        out.update(_emit(t, hs_b, hp_b, gh, sequential=False))
    return out


# ----------------------------------------------------------------------------- results in the kernels' layouts
def _pack(c, outs, shuffle_seed=None):
    """per-image results of a fused-scan case -> ys (B, K, L, D), states (B, K, NT, D), gu, graw (B, K, L, D), gB, gC (B, K, L),
    gA, gD, gbias (B, K, D); shuffle_seed: sum gB / gC over the channels in a shuffled order with one fp32 accumulator"""
    k, l, d = c.k, c.l, c.d
    res = {}
    seq = lambda v: v.reshape(-1, k, d).permute(1, 0, 2)
    res["ys"] = torch.stack([seq(o["y"]) for o in outs])
    res["states"] = torch.stack([seq(o["states"][..., 0]) for o in outs])
    if "gu" in outs[0]:
        for name in ("gu", "graw"):
            res[name] = torch.stack([seq(o[name]) for o in outs])
        for name, key in (("gB", "eb"), ("gC", "ec")):
            per = []
            for o in outs:
                v = o[key][..., 0].reshape(l, k, d)
                if shuffle_seed is not None:
                    perm = torch.randperm(d, generator=torch.Generator().manual_seed(shuffle_seed))
                    v = v[..., perm].cumsum(-1)[..., -1]
                else:
                    v = v.sum(-1)
                per.append(v.t())
            res[name] = torch.stack(per)
        for name in ("gA", "gD", "gbias"):
            res[name] = torch.stack([(o[name][..., 0] if o[name].dim() == 2 else o[name]).reshape(k, d) for o in outs])
        if c.a_log:       # dL/dA_logs = dL/dA * A, as the kernel leaves it
            res["gA"] = res["gA"] * (-torch.exp(c.A.to(res["gA"].dtype))).reshape(k, d)
    return res


def reference(c):
    """fp64, position by position on the gathered operands: ys (B, K, L, D) and the state entering every tile (B, K, NT, D)"""
    return _pack(c, [_sequential(_terms64(c, i), False) for i in range(c.b)])


def reference_bwd(c):
    """fp64 gradients from the oracle of the op the fused kernels replace (oracle.selective_scan.selective_scan_bwd on the
    gathered operands, image by image): gu, graw (B, K, L, D), gB, gC (B, K, L), gA (dL/dA, or dL/dA_logs for a_log), gD, gbias
    (B, K, D) per image"""
    k, l, d, r, rg, tbl = c.k, c.l, c.d, c.r, c.rg, c.table
    a_neg = (-torch.exp(c.A.double()) if c.a_log else c.A.double()).reshape(k * d, 1)
    res = {n: [] for n in ("gu", "graw", "gB", "gC", "gA", "gD", "gbias")}
    for i in range(c.b):
        xi, ri = c.x[i].double(), c.xdbl[i].double().view(l, k, rg)
        u = torch.stack([xi[tbl[j]].t() for j in range(k)]).reshape(1, k * d, l)
        rows = torch.stack([ri[tbl[j], j] for j in range(k)])
        delta = torch.einsum("klr,kdr->kdl", rows[..., :r], c.dt_w.double()).reshape(1, k * d, l)
        Bm, Cm = rows[..., rg - 4].reshape(1, k, 1, l), rows[..., rg - 3].reshape(1, k, 1, l)
        dout = torch.stack([c.gym[i].double()[tbl[j]].t() for j in range(k)]).reshape(1, k * d, l)
        du, dd, dA, dB, dC, dD, dbias = oss.selective_scan_bwd(u.contiguous(), delta.contiguous(), a_neg, Bm.contiguous(),
                                                               Cm.contiguous(), c.ds.double(), c.dt_b.double(), dout.contiguous())
        res["gu"].append(du.reshape(k, d, l).permute(0, 2, 1))
        res["graw"].append(dd.reshape(k, d, l).permute(0, 2, 1))
        res["gB"].append(dB.reshape(k, l))
        res["gC"].append(dC.reshape(k, l))
        res["gA"].append((dA * a_neg if c.a_log else dA).reshape(k, d))
        res["gD"].append(dD.reshape(k, d))
        res["gbias"].append(dbias.reshape(k, d))
    return {n: torch.stack(v) for n, v in res.items()}


def emulate(c, tiled, backward=False, nt_seg=None, fault=None, shuffle_seed=None, biased_exp=False):
    """the fp32 evaluation of a fused-scan case, (a) position by position or (b) tile-wise, in the kernels' layouts"""
    outs = []
    for i in range(c.b):
        t = _terms32(c, i, biased_exp)
        outs.append(_tiled(t, backward, nt_seg, fault) if tiled else _sequential(t, backward))
    return _pack(c, outs, shuffle_seed)


def rel_errors(got, want):
    """(max |err| / max |want|, rms err / rms want), the two measures of test_ss2d_scan_backward_at_the_benchmarked_launches"""
    got, want = got.double().reshape(want.shape), want.double()
    e = got - want
    return (float(e.abs().max()) / (float(want.abs().max()) + 1e-300),
            float(e.pow(2).mean().sqrt()) / (float(want.pow(2).mean().sqrt()) + 1e-300))


FWD_OUTPUTS = ("ys", "states")
BWD_OUTPUTS = ("gu", "graw", "gB", "gC", "gA", "gD", "gbias")
_cache = {}


def e32(c, key, backward=False, nt_seg=None):
    """E32 of a case: per output the larger error, on each measure, of the two fp32 evaluations against fp64.  Cached under
    `key` (the arguments that built `c`) together with the fp64 reference: -> (reference dict, {output: (e_max, e_rms)})"""
    key = (key, backward, nt_seg)
    if key not in _cache:
        ref = reference(c)
        if backward:
            ref.update(reference_bwd(c))
        evals = [emulate(c, False, backward), emulate(c, True, backward, nt_seg, shuffle_seed=5)]
        names = FWD_OUTPUTS + (BWD_OUTPUTS if backward else ())
        _cache[key] = (ref, {n: tuple(max(rel_errors(ev[n], ref[n])[m] for ev in evals) for m in (0, 1)) for n in names})
    return _cache[key]


def bound(e, name=None):
    return FACTOR_FOR.get(name, FACTOR) * e


def check(got, want, e, name, out_dtype=torch.float32):
    """section-4 rule -> (ok, e_max, e_rms, bound_max, bound_rms).  fp32 output: both relative measures within FACTOR * E32.
    16-bit output: EVERY element within u |want| + (fp32 bound) max |want|, and rms err within (u + fp32 rms bound) rms want (the
    rounding of an element is at most u / 2 of it)."""
    got, want = got.double().reshape(want.shape), want.double()
    e_max, e_rms = rel_errors(got, want)
    b_max, b_rms = bound(e[0], name), bound(e[1], name)
    if out_dtype == torch.float32:
        return e_max <= b_max and e_rms <= b_rms, e_max, e_rms, b_max, b_rms
    u = U_ROUND[out_dtype]
    ok = bool(((got - want).abs() <= u * want.abs() + b_max * float(want.abs().max())).all()) and e_rms <= u + b_rms
    return ok, e_max, e_rms, b_max, b_rms


# ----------------------------------------------------------------------------- boundary op
def boundary_reference(o):
    """fp64 oracle of the boundary op: (out, (du, ddelta, dA, dB, dC, dD, dbias))"""
    f = lambda t: t.float()
    args = (f(o.u), f(o.delta), o.A, f(o.B), f(o.C), o.D, o.delta_bias)
    return oss.selective_scan_fwd(*args, True), oss.selective_scan_bwd(*args, o.dout, True)


def _bpack(o, r):
    l, nb, k, dper, n = o.l, o.nb, o.k, o.dper, o.n
    kd = k * dper
    rows = lambda v: v.reshape(l, nb, kd).permute(1, 2, 0)
    bc = lambda v: v.reshape(l, nb, k, dper, n).sum(3).permute(1, 2, 3, 0)
    out = dict(out=rows(r["y"]))
    if "gu" in r:
        out.update(du=rows(r["gu"]), ddelta=rows(r["graw"]), dB=bc(r["eb"]), dC=bc(r["ec"]), dA=r["gA"].reshape(nb, kd, n).sum(0),
                   dD=r["gD"].reshape(nb, kd).sum(0), dbias=r["gbias"].reshape(nb, kd).sum(0))
    return out


BOUNDARY_OUTPUTS = ("out", "du", "ddelta", "dA", "dB", "dC", "dD", "dbias")


def boundary_e32(o, key):
    """as e32() for the boundary op; the tile-wise evaluation stands for its 8-position lanes and 512-position chunks (the
    aggregates are folded in another order there, which FACTOR covers)"""
    if ("boundary", key) not in _cache:
        want, grads = boundary_reference(o)
        ref = dict(zip(BOUNDARY_OUTPUTS, (want,) + tuple(grads)))
        t = _bterms(o, torch.float32)
        evals = [_bpack(o, _sequential(t, True)), _bpack(o, _tiled(t, True))]
        _cache[("boundary", key)] = (ref, {n: tuple(max(rel_errors(ev[n], ref[n])[m] for ev in evals) for m in (0, 1))
                                           for n in BOUNDARY_OUTPUTS})
    return _cache[("boundary", key)]


# ----------------------------------------------------------------------------- the GPU cases (tests/test_gpu_scan_memory.py)
# name -> (family, h, d, r, b, input dtypes); the rows are those of the table in tests/test_gpu_scan_memory.py
FWD_CASES = {
    "raster37": ("raster", 37, 64, 4, 1, (torch.float32, torch.bfloat16)),        # rows 1, 2, 3, 7
    "helix37_wide": ("helix", 37, 2048, 64, 2, (torch.bfloat16,)),                # row 4
    "helix40_r8": ("helix", 40, 64, 8, 1, (torch.bfloat16, torch.float16)),       # rows 5, 7
    "helix40_r16": ("helix", 40, 64, 16, 1, (torch.bfloat16, torch.float16)),
    "helix40_r32": ("helix", 40, 64, 32, 1, (torch.bfloat16, torch.float16)),
    "helix37_d576": ("helix", 37, 576, 8, 2, (torch.bfloat16,)),                  # row 6
}
BWD_CASES = {
    "raster37": ("raster", 37, 64, 4, 1, (torch.float32, torch.bfloat16)),
    "helix40_d96": ("helix", 40, 96, 8, 2, (torch.bfloat16, torch.float16)),
    "helix37_d576": ("helix", 37, 576, 8, 2, (torch.bfloat16,)),
}


def seg_plan(l, rowtiles):
    """the wave-segment plan of tramba_ss2d_scan_cl (seg_plan in ss2d_fused.hip): -> (tiles per segment, segments)"""
    ntiles = (l + TILE - 1) // TILE
    want = max(1, 4096 // max(rowtiles, 1))
    nt = (ntiles + want - 1) // want
    nt = (nt + 2) // 3 * 3
    if ntiles <= 6:
        nt = (ntiles + 2) // 3 * 3
    return nt, (ntiles + nt - 1) // nt


@functools.lru_cache(maxsize=None)
def fused_case(table, name, regime, dtype, a_log=False):
    fam, h, d, r, b, _ = (FWD_CASES if table == "fwd" else BWD_CASES)[name]
    return make(regime, fam, h, b, d, r, dtype, seed=0, a_log=a_log)


def nt_seg_of(name):
    fam, h, d, r, b, _ = FWD_CASES[name]
    return seg_plan(h * h, b * (8 if fam == "helix" else 4) * ((d + 31) // 32))


def fwd_e32(name, regime, dtype, a_log=False, segment=False):
    """-> (case, fp64 reference, E32 per output) of a forward case; segment: the tile-wise evaluation folds by segments"""
    c = fused_case("fwd", name, regime, dtype, a_log)
    return (c,) + e32(c, ("fwd", name, regime, dtype, a_log), nt_seg=nt_seg_of(name)[0] if segment else None)


def bwd_e32(name, regime, dtype, a_log):
    c = fused_case("bwd", name, regime, dtype, a_log)
    return (c,) + e32(c, ("bwd", name, regime, dtype, a_log), backward=True)


# ----------------------------------------------------------------------------- device runs (H = tramba_amd.hip)
def record(label, name, got, want, e, out_dtype=torch.float32):
    ok, e_max, e_rms, b_max, b_rms = check(got.detach().cpu(), want, e, name, out_dtype)
    return dict(case=label, output=name, out_dtype=str(out_dtype)[6:], e32_max=e[0], e32_rms=e[1], bound_max=b_max, bound_rms=b_rms,
                err_max=e_max, err_rms=e_rms, ok=ok)


def _device(H, c, dev):
    if not hasattr(c, "dev"):
        order = H.scan_order(c.fam, c.h, c.h, dev)
        assert torch.equal(order.table.cpu().long(), c.table), "the library's scan table is not the oracle's"
        c.dev = (order, c.x.to(dev), c.xdbl.to(dev), c.gym.to(dev), (c.dt_w.to(dev), c.dt_b.to(dev), c.A.to(dev), c.ds.to(dev)))
    return c.dev


def run_scan(H, c, dev, form, ys_dtype, w=0, states=False):
    """one ss2d_scan_cl launch with the form (and the ring's W) forced; states: also the saved states as (B, K, NT, D) f32, from
    a buffer prefilled with NaN"""
    order, x, xdbl, _, par = _device(H, c, dev)
    st_buf = None
    if states:
        st_buf = H.ss2d_scan_states(x, order)
        st_buf.view(torch.float32).fill_(float("nan"))
    try:
        H.tune_set(H.TUNE_SCAN_FORM, form)
        H.tune_set(H.TUNE_SCAN_W, w)
        ys = H.ss2d_scan_cl(x, xdbl, order, *par, ys_dtype, states=st_buf, a_log=c.a_log)
    finally:
        H.tune_set(H.TUNE_SCAN_FORM, 0)
        H.tune_set(H.TUNE_SCAN_W, 0)
    torch.cuda.synchronize()
    H.device_error()
    if not states:
        return ys
    ntile = (c.l + TILE - 1) // TILE
    return ys, st_buf.view(torch.float32).view(c.b, c.k, ntile + 8, c.d)[:, :, :ntile]


def run_bwd(H, c, dev, with_states):
    """the training pair: forward launch (saving states or not), ss2d_scan_bwd_cl with bc_partials, the partials summed as
    ss2d_bwd_prep would -> outputs named as reference_bwd()"""
    order, x, xdbl, gym, par = _device(H, c, dev)
    st_buf = None
    if with_states:
        st_buf = H.ss2d_scan_states(x, order)
        st_buf.view(torch.float32).fill_(float("nan"))
        H.ss2d_scan_cl(x, xdbl, order, *par, c.dtype, states=st_buf, a_log=c.a_log)
    gu, graw, gB, gC, gpar = H.ss2d_scan_bwd_cl(x, xdbl, order, *par, gym, states=st_buf, a_log=c.a_log, bc_partials=True)
    torch.cuda.synchronize()
    H.device_error()
    gpar = gpar.view(c.b, 3, c.k, c.d)
    return dict(gu=gu, graw=graw, gB=gB.sum(dim=2), gC=gC.sum(dim=2), gA=gpar[:, 0], gD=gpar[:, 1], gbias=gpar[:, 2])


def bwd_records(H, dev, name, regime, dtype, a_log):
    c, ref, e = bwd_e32(name, regime, dtype, a_log)
    out = []
    for with_states in (True, False):
        got = run_bwd(H, c, dev, with_states)
        label = f"bwd {name} {regime} {str(dtype)[6:]} a_log={int(a_log)} {'states' if with_states else 'recompute'}"
        for n in BWD_OUTPUTS:
            assert bool(torch.isfinite(got[n].float()).all()), (label, n)
            out.append(record(label, n, got[n], ref[n], e[n], c.dtype if n in ("gu", "graw") else torch.float32))
    return out


BOUNDARY_L = {torch.float32: 1561, torch.bfloat16: 1600}     # 4 chunks of 512 positions, the last one ragged (25 / 64 positions)


def boundary_records(H, dev, regime, n, dtype):
    """selective_scan_fwd / _bwd on rows = 2 x 4 x 8: every output against the fp64 oracle, the forward also against the oracle's
    fp32-arithmetic form (within the bound plus that form's own error)"""
    l = BOUNDARY_L[dtype]
    o = make_boundary(regime, 2, 4, 8, n, l, dtype)
    ref, e = boundary_e32(o, (regime, n, l, dtype))
    g = [t.to(dev) for t in (o.u, o.delta, o.A, o.B, o.C, o.D, o.delta_bias)]
    assert H.selective_scan_nchunk(l, dtype) >= 4 and l % 512 != 0
    out, ckpt = H.selective_scan_fwd(*g, True, True)
    grads = H.selective_scan_bwd(*g, o.dout.to(dev), ckpt, True)
    torch.cuda.synchronize()
    H.device_error()
    label = f"boundary {regime} N={n} {str(dtype)[6:]} L={l}"
    recs = [record(label, "out", out, ref["out"], e["out"])]
    f = lambda t: t.float()
    f32 = oss.selective_scan_fwd_f32(f(o.u), f(o.delta), o.A, f(o.B), f(o.C), o.D, o.delta_bias, True)
    e_f32 = rel_errors(f32, ref["out"])[0]
    d_f32 = rel_errors(out.cpu(), f32.double())[0]
    recs.append(dict(case=label, output="out vs fp32 oracle", err_max=d_f32, bound_max=recs[0]["bound_max"] + e_f32,
                     ok=d_f32 <= recs[0]["bound_max"] + e_f32))
    for name, got in zip(BOUNDARY_OUTPUTS[1:], grads):
        recs.append(record(label, name, got, ref[name], e[name], dtype if name in ("du", "ddelta") else torch.float32))
    return recs
