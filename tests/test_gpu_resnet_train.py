"""GPU tests of the training-path entries of the ResNet-50 encoder: training-mode batch norm and the stem's max pool
(csrc/batchnorm.hip) and the backward of the bottleneck convolutions (csrc/resnet_conv.hip), then of the autograd Functions,
`Bottleneck.forward_cl` and `ResNet.features_cl` that reach them behind `encoders.set_library_training`.

References are fp64 on the same 16-bit inputs, every element is compared, outputs (and workspaces) are pre-filled with NaN and
inputs lie between NaN guard bands.  The bounds are derived, not measured.  With e = 2^-24, u the unit round-off of the output
format (2^-8 bf16, 2^-11 fp16), M rows per channel, and "n f32 additions in any order cost (n + 2) e times the sum of the
magnitudes":

bn_stats     mean:  bm = (M + 2) e sum|x| / M
             var (two passes; with d = mean error the exact second pass gives var + d^2):
                    bv = 1.01 [(M + 5) e (var + bm^2) + bm^2]       (subtraction, square, M additions, division; 1 % for the
                                                                     second-order terms)
             rstd = (var + eps)^-1/2:  r bv / (2 (var + eps - bv)) + 4 e r
             running: momentum x the bound of the new value + 5 e (|(1 - m) old| + |m new|)
bn_act       u |ref| + 4 e (|gamma xh| + |beta| + |res|),  xh = (x - mean) rstd  (subtraction, gamma rstd, fma, residual addition)
bn_act_bwd   dbeta: bb = (M + 2) e sum|dy'|;  dgamma: bg = (M + 4) e sum|dy' xh|  (xh costs two roundings per term)
             dx = k (dy' - m1 - xh m2), k = gamma rstd, m1 = dbeta / M, m2 = dgamma / M.  The cancellation is bounded through
             the magnitudes of the terms, not through |dx|:
                    u |ref| + |k| [bb / M + |xh| bg / M + 6 e (|dy'| + |m1| + |xh m2|)]
             dres is the masked dy itself: equal.
pool         a selection: equal to F.max_pool2d and to its autograd.
conv_dgrad   u |ref| + (K + 2) e A,  K = k k Cout products per element, A = sum |gy| |w|  (16-bit products are exact in f32)
conv_wgrad   (n + 2) e A,  n = M rounded up to the 32-token step plus the slab count, A = sum |gy| |x|  (f32 output)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF, HF = torch.bfloat16, torch.float16
E = 2.0 ** -24
NAN = float("nan")
GUARD = 4096
EPS, MOM = 1e-5, 0.1


def _name(dtype):
    return str(dtype)[6:]


def _guarded(t):
    """a copy of t inside one allocation with NaN guard bands before and after it (16-byte aligned)"""
    buf = torch.full((t.numel() + 2 * GUARD,), NAN, dtype=t.dtype, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


def _nan(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)


def _within(got, ref, bound, what):
    g = got.double()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output (an element not written, or a poisoned element read)"
    ratio = (g - ref).abs() / bound
    worst = float(ratio.max())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound, worst {worst:.3f}"
    return worst


def _ok(rc):
    from tramba_amd import hip
    assert rc == 0, hip.lib().tramba_last_error()


# ----------------------------------------------------------------------------- batch norm
# name: ((B, H, W, C), mean / std per channel)
BN_CASES = {
    "m35_5x7x64": ((1, 5, 7, 64), 0.0),                 # M = 35: one ragged row block
    "two_images_9x11x256": ((2, 9, 11, 256), 0.5),      # rows across two images, 4 channel blocks
    "c72_3x3": ((1, 3, 3, 72), 0.5),                    # C no multiple of 64: a channel block with one live lane
    "layer3_b4": ((4, 24, 24, 1024), 0.5),              # the workload's extremes: 18 row runs x 16 channel blocks
    "layer1": ((1, 96, 96, 64), 0.5),                   # 64 row runs x 1 channel block
    "offset50_9x11x64": ((2, 9, 11, 64), 50.0),         # |mean| = 50 std: E[x^2] - E[x]^2 loses 2500 x the digits
}
BN_DTYPES = [(n, BF) for n in BN_CASES] + [("m35_5x7x64", HF), ("layer1", HF)]
BN_IDS = [f"{n}-{_name(d)}" for n, d in BN_DTYPES]


def _bn_work(m, c):
    from tramba_amd import hip
    nbytes = hip.lib().tramba_bn_work(m, c)
    assert nbytes == 4 * hip.bn_work_floats(m, c) and hip.lib().tramba_bn_parts(m, c) == hip.bn_parts(m, c)
    return _nan((nbytes // 4,), torch.float32), nbytes


@functools.lru_cache(maxsize=None)
def _bn_inputs(name, dtype):
    """x, residual, dy in guard bands; gamma, beta, running buffers f32; the fp64 statistics of x"""
    shape, off = BN_CASES[name]
    c = shape[-1]
    std = synth.synth_tensor(f"rbn_{name}.std", (c,)).abs().mul(3).add(0.5)
    sign = torch.where(synth.synth_tensor(f"rbn_{name}.sign", (c,)) > 0, 1.0, -1.0)
    x = _guarded((synth.synth_input(f"rbn_x_{name}", shape) * std + off * std * sign).to(dtype).to(DEV))
    res = _guarded(synth.synth_input(f"rbn_res_{name}", shape).to(dtype).to(DEV))
    dy = _guarded(synth.synth_input(f"rbn_dy_{name}", shape).to(dtype).to(DEV))
    gamma = synth.synth_tensor(f"rbn_{name}.gamma", (c,)).mul(8).add(1).to(DEV)                # both signs
    beta = synth.synth_tensor(f"rbn_{name}.beta", (c,)).mul(5).to(DEV)
    rm = synth.synth_tensor(f"rbn_{name}.rm", (c,)).mul(20).to(DEV)
    rv = synth.synth_tensor(f"rbn_{name}.rv", (c,)).abs().mul(10).add(0.1).to(DEV)
    xd = x.double().view(-1, c)
    m = xd.shape[0]
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).sum(0) / m
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, m=m, c=c, mean=mean, var=var,
                absmean=xd.abs().sum(0) / m)


def _raw_stats(x, rm, rv, m, c, mom=MOM):
    from tramba_amd import hip
    mean, rstd = _nan((c,), torch.float32), _nan((c,), torch.float32)
    work, nbytes = _bn_work(m, c)
    p = lambda t: None if t is None else t.data_ptr()
    _ok(hip.lib().tramba_bn_stats_cl(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p(rm), p(rv), work.data_ptr(), nbytes, m, c,
                                     EPS, mom, hip.dt(x), hip._stream()))
    return mean, rstd


def _stats_bounds(d):
    m = d["m"]
    bm = (m + 2) * E * d["absmean"] + 1e-300
    bv = 1.01 * ((m + 5) * E * (d["var"] + bm ** 2) + bm ** 2) + 1e-300
    return bm, bv


@pytest.mark.parametrize("name,dtype", BN_DTYPES, ids=BN_IDS)
def test_bn_stats_and_running_update_match_fp64(name, dtype):
    from tramba_amd import hip
    d = _bn_inputs(name, dtype)
    m, c = d["m"], d["c"]
    assert hip.bn_supported(dtype, m, c)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    mean, rstd = _raw_stats(d["x"], rm, rv, m, c)
    bm, bv = _stats_bounds(d)
    what = f"bn_stats {name} {_name(dtype)}"
    _within(mean, d["mean"], bm, what + " mean")
    r = (d["var"] + EPS) ** -0.5
    _within(rstd, r, r * bv / (2 * (d["var"] + EPS - bv)) + 4 * E * r, what + " rstd")
    mom = float(torch.tensor(MOM, dtype=torch.float32))                # the momentum the kernel holds
    unb = m / (m - 1)
    old_m, old_v = (1 - mom) * d["rm"].double(), (1 - mom) * d["rv"].double()
    _within(rm, old_m + mom * d["mean"], mom * bm + 5 * E * (old_m.abs() + mom * d["mean"].abs()), what + " running_mean")
    _within(rv, old_v + mom * unb * d["var"], mom * unb * bv + 5 * E * (old_v.abs() + mom * unb * d["var"]),
            what + " running_var")
    # the binding: the same bits, the buffers updated in place; without buffers the same statistics
    rm2, rv2 = d["rm"].clone(), d["rv"].clone()
    got = hip.bn_stats_cl(d["x"], EPS, rm2, rv2, MOM)
    assert torch.equal(got[0], mean) and torch.equal(got[1], rstd) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
    got = hip.bn_stats_cl(d["x"], EPS)
    assert torch.equal(got[0], mean) and torch.equal(got[1], rstd)


def test_bn_running_update_agrees_with_the_framework():
    """F.batch_norm in training mode on the same 16-bit map updates its buffers to the same values within the two bounds"""
    d = _bn_inputs("two_images_9x11x256", BF)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    _raw_stats(d["x"], rm, rv, d["m"], d["c"])
    fm, fv = d["rm"].clone(), d["rv"].clone()
    F.batch_norm(d["x"].permute(0, 3, 1, 2).float(), fm, fv, None, None, True, MOM, EPS)
    bm, bv = _stats_bounds(d)
    unb = d["m"] / (d["m"] - 1)
    _within(rm, fm.double(), 2 * (MOM * bm + 5 * E * (d["rm"].double().abs() + d["mean"].abs())), "running_mean vs F.batch_norm")
    _within(rv, fv.double(), 2 * (MOM * unb * bv + 5 * E * (d["rv"].double().abs() + unb * d["var"])),
            "running_var vs F.batch_norm")


def _f32_stats(d):
    """the statistics as f32 inputs of the element-wise entries (what bn_stats_cl would hand over, to within its bound)"""
    return d["mean"].float().contiguous(), ((d["var"] + EPS) ** -0.5).float().contiguous()


def _raw_act(x, mean, rstd, gamma, beta, res, relu, m, c):
    from tramba_amd import hip
    y = _nan(x.shape, x.dtype)
    p = lambda t: None if t is None else t.data_ptr()
    _ok(hip.lib().tramba_bn_act_cl(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p(gamma), p(beta), p(res), y.data_ptr(), m, c,
                                   int(relu), hip.dt(x), hip._stream()))
    return y


@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, True)], ids=["plain", "relu", "res_relu"])
@pytest.mark.parametrize("name,dtype", BN_DTYPES, ids=BN_IDS)
def test_bn_act_matches_fp64(name, dtype, with_res, relu):
    from tramba_amd import hip
    d = _bn_inputs(name, dtype)
    mean, rstd = _f32_stats(d)
    res = d["res"] if with_res else None
    y = _raw_act(d["x"], mean, rstd, d["gamma"], d["beta"], res, relu, d["m"], d["c"])
    gx = d["gamma"].double() * (d["x"].double() - mean.double()) * rstd.double()
    resd = res.double() if with_res else torch.zeros_like(gx)
    pre = gx + d["beta"].double() + resd
    ref = pre.clamp_min(0) if relu else pre
    bound = U[dtype] * ref.abs() + 4 * E * (gx.abs() + d["beta"].double().abs() + resd.abs()) + 1e-30
    _within(y, ref, bound, f"bn_act {name} {_name(dtype)} res={with_res} relu={relu}")
    assert torch.equal(hip.bn_act_cl(d["x"], mean, rstd, d["gamma"], d["beta"], res, relu), y)
    if not with_res and not relu:                                      # NULL gamma / beta are 1 / 0, bitwise
        ones, zeros = torch.ones_like(d["gamma"]), torch.zeros_like(d["beta"])
        assert torch.equal(hip.bn_act_cl(d["x"], mean, rstd), hip.bn_act_cl(d["x"], mean, rstd, ones, zeros))


def _raw_bwd(dy, x, y, mean, rstd, gamma, relu, want_dres, want_affine, m, c):
    from tramba_amd import hip
    dx = _nan(x.shape, x.dtype)
    dres = _nan(x.shape, x.dtype) if want_dres else None
    dg = _nan((c,), torch.float32) if want_affine else None
    db = _nan((c,), torch.float32) if want_affine else None
    work, nbytes = _bn_work(m, c)
    p = lambda t: None if t is None else t.data_ptr()
    _ok(hip.lib().tramba_bn_act_bwd_cl(dy.data_ptr(), x.data_ptr(), p(y), mean.data_ptr(), rstd.data_ptr(), p(gamma),
                                       dx.data_ptr(), p(dres), p(dg), p(db), work.data_ptr(), nbytes, m, c, int(relu),
                                       hip.dt(x), hip._stream()))
    return dx, dres, dg, db


def _bwd_ref(d, mean, rstd, y, relu):
    """fp64 (dx, dres, dgamma, dbeta) and their bounds, from the f32 statistics and the 16-bit y the kernel reads"""
    m, c = d["m"], d["c"]
    dyp = d["dy"].double()
    if relu:
        dyp = torch.where(y > 0, dyp, torch.zeros_like(dyp))
    xh = (d["x"].double() - mean.double()) * rstd.double()
    flat = lambda t: t.reshape(-1, c)
    dbeta, dgamma = flat(dyp).sum(0), flat(dyp * xh).sum(0)
    bb = (m + 2) * E * flat(dyp).abs().sum(0) + 1e-30
    bg = (m + 4) * E * flat(dyp * xh).abs().sum(0) + 1e-30
    k = d["gamma"].double() * rstd.double()
    m1, m2 = dbeta / m, dgamma / m
    dx = k * (dyp - m1 - xh * m2)
    return dict(dx=dx, dres=dyp, dgamma=dgamma, dbeta=dbeta, bg=bg, bb=bb,
                bdx=lambda u: u * dx.abs() + k.abs() * (bb / m + xh.abs() * bg / m
                                                        + 6 * E * (dyp.abs() + m1.abs() + (xh * m2).abs())) + 1e-30)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name,dtype", BN_DTYPES, ids=BN_IDS)
def test_bn_act_bwd_matches_fp64_and_a_frozen_affine_keeps_dx(name, dtype, relu):
    from tramba_amd import hip
    d = _bn_inputs(name, dtype)
    m, c = d["m"], d["c"]
    mean, rstd = _f32_stats(d)
    y = _guarded(hip.bn_act_cl(d["x"], mean, rstd, d["gamma"], d["beta"], d["res"], True)) if relu else None
    dx, dres, dg, db = _raw_bwd(d["dy"], d["x"], y, mean, rstd, d["gamma"], relu, True, True, m, c)
    r = _bwd_ref(d, mean, rstd, y, relu)
    what = f"bn_act_bwd {name} {_name(dtype)} relu={relu}"
    _within(db, r["dbeta"], r["bb"], what + " dbeta")
    _within(dg, r["dgamma"], r["bg"], what + " dgamma")
    _within(dx, r["dx"], r["bdx"](U[dtype]), what + " dx")
    assert torch.equal(dres.double(), r["dres"]), what + " dres"
    if relu:
        assert 0.2 < float((y > 0).double().mean()) < 0.8              # the mask is a real one
    # frozen affine, no shortcut: dx bitwise the same, nothing else written
    fx, fres, fg, fb = _raw_bwd(d["dy"], d["x"], y, mean, rstd, d["gamma"], relu, False, False, m, c)
    assert torch.equal(fx, dx) and fres is None and fg is None and fb is None
    got = hip.bn_act_bwd_cl(d["dy"], d["x"], y, mean, rstd, d["gamma"], relu, want_dres=True)
    assert all(torch.equal(a, b) for a, b in zip(got, (dx, dres, dg, db)))
    got = hip.bn_act_bwd_cl(d["dy"], d["x"], y, mean, rstd, d["gamma"], relu, want_affine=False)
    assert torch.equal(got[0], dx) and got[1] is None and got[2] is None and got[3] is None


def test_backward_reference_formulas_equal_the_fp64_autograd_of_the_framework():
    """the closed forms the backward is compared with, against autograd through F.batch_norm + shortcut + ReLU in fp64"""
    d = _bn_inputs("two_images_9x11x256", BF)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    x64 = nchw(d["x"].double()).requires_grad_()
    r64 = nchw(d["res"].double()).requires_grad_()
    g64, b64 = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    out = F.relu(F.batch_norm(x64, None, None, g64, b64, True, MOM, EPS) + r64)
    out.backward(nchw(d["dy"].double()))
    r = _bwd_ref(d, d["mean"], (d["var"] + EPS) ** -0.5, out.detach().permute(0, 2, 3, 1), True)
    for got, ref in ((x64.grad.permute(0, 2, 3, 1), r["dx"]), (r64.grad.permute(0, 2, 3, 1), r["dres"]), (g64.grad, r["dgamma"]),
                     (b64.grad, r["dbeta"])):
        assert float((got - ref).abs().max()) <= 1e-9 * (1 + float(ref.abs().max()))


# ----------------------------------------------------------------------------- max pool
POOL_CASES = {"7x9": (2, 7, 9, 64), "8x8": (1, 8, 8, 72), "192x192x64": (1, 192, 192, 64)}


@functools.lru_cache(maxsize=None)
def _pool_inputs(name, dtype, quantised):
    b, h, w, c = POOL_CASES[name]
    x = synth.synth_input(f"rpool_x_{name}", (b, h, w, c))
    if quantised:
        x = (x * 1.5).round().clamp(-2, 1)                              # 4 distinct values: nearly every window ties
    else:
        x = x.clamp_min(0)                                              # a post-ReLU map: zeros tie
    x = _guarded(x.to(dtype).to(DEV))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gy = _guarded(synth.synth_input(f"rpool_gy_{name}", (b, ho, wo, c)).to(dtype).to(DEV))
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    yn = F.max_pool2d(xn, 3, 2, 1)
    yn.backward(gy.permute(0, 3, 1, 2).contiguous())
    return x, gy, yn.detach().permute(0, 2, 3, 1).contiguous(), xn.grad.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("quantised", [False, True], ids=["relu_map", "four_values"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=_name)
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool_equals_the_framework_forward_and_backward(name, dtype, quantised):
    from tramba_amd import hip
    x, gy, y_ref, gx_ref = _pool_inputs(name, dtype, quantised)
    b, h, w, c = x.shape
    assert hip.maxpool3s2_supported(dtype, h, w, c)
    if quantised:
        assert x.unique().numel() == 4
    y, gx = _nan(y_ref.shape, dtype), _nan(x.shape, dtype)
    lib = hip.lib()
    _ok(lib.tramba_maxpool3s2_cl(x.data_ptr(), y.data_ptr(), b, h, w, c, hip.dt(x), hip._stream()))
    assert torch.equal(y, y_ref)
    _ok(lib.tramba_maxpool3s2_bwd_cl(gy.data_ptr(), x.data_ptr(), gx.data_ptr(), b, h, w, c, hip.dt(x), hip._stream()))
    assert torch.isfinite(gx).all()
    diff = int((gx != gx_ref).sum())
    print(f"maxpool {name} {_name(dtype)} quantised={quantised}: {diff} of {gx.numel()} gradient elements differ")
    assert torch.equal(gx, gx_ref)
    assert torch.equal(hip.maxpool3s2_cl(x), y) and torch.equal(hip.maxpool3s2_bwd_cl(gy, x), gx)


def test_maxpool_padding_never_wins():
    """an all-negative map: zero padding would win every border window"""
    from tramba_amd import hip
    x = -(synth.synth_input("rpool_neg", (1, 7, 9, 64)).abs() + 1).to(BF).to(DEV)
    y = hip.maxpool3s2_cl(x)
    assert float(y.max()) < 0
    assert torch.equal(y, F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


# ----------------------------------------------------------------------------- backward of the bottleneck convolutions
# name: (B, H, W, Cin, Cout, k, s)
CONV_CASES = {
    "3x3_7x9": (1, 7, 9, 64, 64, 3, 1),
    "3x3s2_9x11_odd": (2, 9, 11, 128, 128, 3, 2),
    "3x3s2_8x12_even": (1, 8, 12, 128, 128, 3, 2),
    "down_7x9_s2": (2, 7, 9, 256, 512, 1, 2),
    "3x3_6x6_deep": (1, 6, 6, 256, 256, 3, 1),
    "1x1_5x5_cout72": (1, 5, 5, 64, 72, 1, 1),
    "1x1_5x5_cout8": (1, 5, 5, 64, 8, 1, 1),
    "layer1_conv2": (1, 96, 96, 64, 64, 3, 1),
    "layer3_conv1": (1, 24, 24, 1024, 256, 1, 1),
}
CONV_DTYPES = [(n, BF) for n in CONV_CASES] + [("3x3s2_9x11_odd", HF), ("down_7x9_s2", HF)]
CONV_IDS = [f"{n}-{_name(d)}" for n, d in CONV_DTYPES]


def _cols(xd, k, s, offset=0):
    """(B, Ho, Wo, Cin k k) fp64 patch rows of xd (B, Cin, H, W) for pad = k // 2 (F.unfold: a gather); offset: stride origin"""
    b, cin, h, w = xd.shape
    cols = F.unfold(xd, k, padding=k // 2, stride=1).transpose(1, 2).view(b, h, w, cin * k * k)
    return cols[:, offset::s, offset::s]


def _dgrad_ref(gyd, wd, x_shape, k, s, offset=0):
    """fp64 input gradient (B, H, W, Cin) of the unfold-and-matmul convolution, by its autograd (fold: a sum in fp64)"""
    b, h, w, cin = x_shape
    xz = torch.zeros((b, cin, h, w), dtype=torch.float64, device=DEV, requires_grad=True)
    y = _cols(xz, k, s, offset) @ wd.reshape(wd.shape[0], -1).t()
    hs, ws = y.shape[1], y.shape[2]
    (gx,) = torch.autograd.grad(y, xz, gyd[:, :hs, :ws])
    return gx.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _conv_inputs(name, dtype):
    from tramba_amd import hip
    b, h, w, cin, cout, k, s = CONV_CASES[name]
    ho, wo = hip.conv_out_size(h, k, s), hip.conv_out_size(w, k, s)
    x_clean = synth.synth_input(f"rct_x_{name}", (b, h, w, cin)).to(dtype).to(DEV)
    wt = synth.synth_tensor(f"rct_{name}.weight", (cout, cin, k, k)).to(dtype).to(DEV)           # reference layout
    gy = _guarded(synth.synth_input(f"rct_gy_{name}", (b, ho, wo, cout)).to(dtype).to(DEV))
    # pixels of x that no tap of any output reads (stride 2) are NaN in the copy the weight gradient is given
    ones = torch.ones((b, 1, h, w), dtype=torch.float64, device=DEV, requires_grad=True)
    (reach,) = torch.autograd.grad(_cols(ones, k, s).sum(), ones)
    x_nan = x_clean.clone()
    x_nan[(reach[:, 0] == 0)] = NAN
    return dict(x=_guarded(x_nan), x_clean=x_clean, wt=wt, wk=wt.permute(0, 2, 3, 1).contiguous(), gy=gy,
                unreachable=int((reach == 0).sum()))


@pytest.mark.parametrize("name,dtype", CONV_DTYPES, ids=CONV_IDS)
def test_conv_dgrad_matches_fp64_and_writes_every_element(name, dtype):
    from tramba_amd import hip
    b, h, w, cin, cout, k, s = CONV_CASES[name]
    d = _conv_inputs(name, dtype)
    assert hip.conv_train_supported(dtype, h, w, cin, cout, k, s)
    wtr = _guarded(hip.conv_transposed_weight(d["wk"]))
    assert wtr.shape == (cin, k, k, cout)
    gx = _nan((b, h, w, cin), dtype)
    _ok(hip.lib().tramba_conv_dgrad_cl(d["gy"].data_ptr(), wtr.data_ptr(), gx.data_ptr(), b, h, w, cin, cout, k, s, hip.dt(gx),
                                       hip._stream()))
    ref = _dgrad_ref(d["gy"].double(), d["wt"].double(), (b, h, w, cin), k, s)
    mag = _dgrad_ref(d["gy"].double().abs(), d["wt"].double().abs(), (b, h, w, cin), k, s)
    _within(gx, ref, U[dtype] * ref.abs() + (k * k * cout + 2) * E * mag + 1e-12, f"conv_dgrad {name} {_name(dtype)}")
    if s == 2 and k == 1:
        assert float(gx[:, 1::2].abs().max()) == 0 and float(gx[:, :, 1::2].abs().max()) == 0      # written, as zeros
    assert torch.equal(hip.conv_dgrad_cl(d["gy"], wtr, (b, h, w, cin), s), gx)


@pytest.mark.parametrize("name,dtype", CONV_DTYPES, ids=CONV_IDS)
def test_conv_wgrad_matches_fp64_and_reads_no_unreachable_pixel(name, dtype):
    from tramba_amd import hip
    b, h, w, cin, cout, k, s = CONV_CASES[name]
    d = _conv_inputs(name, dtype)
    lib = hip.lib()
    nsplit = lib.tramba_conv_wgrad_split(b, h, w, cin, cout, k, s)
    nbytes = lib.tramba_conv_wgrad_work(b, h, w, cin, cout, k, s)
    assert nsplit == hip.conv_wgrad_split(b, h, w, cin, cout, k, s) >= 1 and nbytes == nsplit * cout * k * k * cin * 4
    if k == 1 and s == 2:
        assert d["unreachable"] > 0
    work = _nan((nsplit, cout * k * k * cin), torch.float32)
    _ok(lib.tramba_conv_wgrad_cl(d["gy"].data_ptr(), d["x"].data_ptr(), work.data_ptr(), nbytes, b, h, w, cin, cout, k, s,
                                 hip.dt(d["gy"]), hip._stream()))
    assert torch.isfinite(work).all(), "a slab element not written, or an unreachable pixel read"
    gw = work.double().sum(0).view(cout, k, k, cin) if nsplit > 1 else work[0].double().view(cout, k, k, cin)
    cols = _cols(d["x_clean"].permute(0, 3, 1, 2).double(), k, s).reshape(-1, cin * k * k)
    gyd = d["gy"].double().view(-1, cout)
    to_k = lambda t: t.view(cout, cin, k, k).permute(0, 2, 3, 1)
    ref, mag = to_k(gyd.t() @ cols), to_k(gyd.abs().t() @ cols.abs())
    m = gyd.shape[0]
    n = hip.conv_wgrad_steps(m) * 32 + nsplit
    _within(gw, ref, (n + 2) * E * mag + 1e-12, f"conv_wgrad {name} {_name(dtype)} (slabs summed in fp64)")
    got = hip.conv_wgrad_cl(d["gy"], d["x"], k, s)
    assert got.dtype == torch.float32 and got.shape == (cout, k, k, cin)
    _within(got, ref, (n + 2) * E * mag + 1e-12, f"conv_wgrad {name} {_name(dtype)}")


def test_raw_convolution_of_the_training_forward_is_the_rounded_convolution():
    """conv_affine_cl with NULL scale / shift and no ReLU, the training path's forward, against fp64"""
    from tramba_amd import hip
    for name in ("3x3s2_9x11_odd", "down_7x9_s2"):
        b, h, w, cin, cout, k, s = CONV_CASES[name]
        d = _conv_inputs(name, BF)
        y = hip.conv_affine_cl(d["x_clean"], d["wk"], None, None, None, False, ksize=k, stride=s)
        cols = _cols(d["x_clean"].permute(0, 3, 1, 2).double(), k, s)
        wm = d["wt"].double().reshape(cout, -1)
        ref, mag = cols @ wm.t(), cols.abs() @ wm.abs().t()
        _within(y, ref, U[BF] * ref.abs() + (k * k * cin + 2) * E * mag + 1e-12, f"raw convolution {name}")


# ----------------------------------------------------------------------------- sharpness
def test_bounds_are_sharp_enough_to_see_a_wrong_kernel():
    """each wrong variant lies beyond its bound; the factor is printed"""
    from tramba_amd import hip
    seen = {}
    # a tap-mirrored weight and a stride origin one pixel off, against the input gradient's bound
    name = "3x3s2_9x11_odd"
    b, h, w, cin, cout, k, s = CONV_CASES[name]
    d = _conv_inputs(name, BF)
    gyd, wd = d["gy"].double(), d["wt"].double()
    ref = _dgrad_ref(gyd, wd, (b, h, w, cin), k, s)
    bound = U[BF] * ref.abs() + (k * k * cout + 2) * E * _dgrad_ref(gyd.abs(), wd.abs(), (b, h, w, cin), k, s) + 1e-12
    seen["tap-mirrored weight"] = ((_dgrad_ref(gyd, wd.flip(2, 3), (b, h, w, cin), k, s) - ref).abs() / bound).max()
    seen["stride origin off by one"] = ((_dgrad_ref(gyd, wd, (b, h, w, cin), k, s, offset=1) - ref).abs() / bound).max()
    # the unbiased variance in the normalisation, against the rstd bound
    d = _bn_inputs("m35_5x7x64", BF)
    bm, bv = _stats_bounds(d)
    r = (d["var"] + EPS) ** -0.5
    wrong = (d["var"] * d["m"] / (d["m"] - 1) + EPS) ** -0.5
    seen["unbiased variance in the normalisation"] = ((wrong - r).abs() / (r * bv / (2 * (d["var"] + EPS - bv)) + 4 * E * r)).max()
    # the naive variance E[x^2] - E[x]^2 in f32 on the offset map, against the variance bound
    d = _bn_inputs("offset50_9x11x64", BF)
    bm, bv = _stats_bounds(d)
    xf = d["x"].float().view(-1, d["c"])
    naive = (xf * xf).mean(0) - xf.mean(0) ** 2
    seen["naive f32 variance at |mean| = 50 std"] = ((naive.double() - d["var"]).abs() / bv).max()
    # momentum applied to the wrong side, against the running-mean bound
    mom = float(torch.tensor(MOM, dtype=torch.float32))
    right = (1 - mom) * d["rm"].double() + mom * d["mean"]
    wrong = mom * d["rm"].double() + (1 - mom) * d["mean"]
    seen["momentum on the wrong side"] = ((wrong - right).abs()
                                          / (mom * bm + 5 * E * ((1 - mom) * d["rm"].double().abs() + mom * d["mean"].abs()))).max()
    # a dropped ReLU mask, against the dbeta bound
    d = _bn_inputs("m35_5x7x64", BF)
    mean, rstd = _f32_stats(d)
    y = hip.bn_act_cl(d["x"], mean, rstd, d["gamma"], d["beta"], None, True)
    masked, plain = _bwd_ref(d, mean, rstd, y, True), _bwd_ref(d, mean, rstd, y, False)
    seen["dropped ReLU mask"] = ((plain["dbeta"] - masked["dbeta"]).abs() / masked["bb"]).median()   # (median: a channel that the
    # mask empties has a zero bound)
    for what, factor in seen.items():
        print(f"{what}: {float(factor):.3g} bounds away")
        assert float(factor) > 2, what
    # a tie that goes to the LAST maximum moves gradient elements (the pool is compared for equality)
    x, gy, _, gx_ref = _pool_inputs("7x9", BF, True)
    xn = x.permute(0, 3, 1, 2).flip(2, 3).contiguous().requires_grad_()                            # first of the flipped = last
    F.max_pool2d(xn, 3, 2, 1).backward(gy.permute(0, 3, 1, 2).flip(2, 3).contiguous())
    last = xn.grad.flip(2, 3).permute(0, 2, 3, 1)
    moved = int((last != gx_ref).sum())
    print(f"tie to the last maximum: {moved} of {gx_ref.numel()} gradient elements differ")
    assert moved > gx_ref.numel() // 10


# ----------------------------------------------------------------------------- reproducibility
def _entries(small):
    """every new entry as a closure over fixed inputs -> a tuple of output tensors"""
    from tramba_amd import hip
    bn = _bn_inputs("m35_5x7x64" if small else "layer3_b4", BF)
    cv = _conv_inputs("3x3s2_9x11_odd" if small else "layer1_conv2", BF)
    cname = "3x3s2_9x11_odd" if small else "layer1_conv2"
    b, h, w, cin, cout, k, s = CONV_CASES[cname]
    px, pgy, _, _ = _pool_inputs("7x9" if small else "192x192x64", BF, True)
    mean, rstd = _f32_stats(bn)
    y = hip.bn_act_cl(bn["x"], mean, rstd, bn["gamma"], bn["beta"], bn["res"], True)
    wtr = hip.conv_transposed_weight(cv["wk"])
    rm, rv = bn["rm"].clone(), bn["rv"].clone()

    def stats():
        rm.copy_(bn["rm"])
        rv.copy_(bn["rv"])
        return hip.bn_stats_cl(bn["x"], EPS, rm, rv, MOM) + (rm.clone(), rv.clone())
    return {
        "bn_stats": stats,
        "bn_act": lambda: (hip.bn_act_cl(bn["x"], mean, rstd, bn["gamma"], bn["beta"], bn["res"], True),),
        "bn_act_bwd": lambda: hip.bn_act_bwd_cl(bn["dy"], bn["x"], y, mean, rstd, bn["gamma"], True, want_dres=True),
        "maxpool": lambda: (hip.maxpool3s2_cl(px),),
        "maxpool_bwd": lambda: (hip.maxpool3s2_bwd_cl(pgy, px),),
        "conv_dgrad": lambda: (hip.conv_dgrad_cl(cv["gy"], wtr, (b, h, w, cin), s),),
        "conv_wgrad": lambda: (hip.conv_wgrad_cl(cv["gy"], cv["x"], k, s),),
    }


@pytest.mark.parametrize("small", [True, False], ids=["small", "workload"])
def test_two_runs_and_a_graph_replay_give_the_same_bits(small):
    for what, fn in _entries(small).items():
        first = [t.clone() for t in fn()]
        second = fn()
        assert all(torch.equal(a, b) for a, b in zip(first, second)), what
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                                       # warm up on the capture stream
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out = fn()
        torch.cuda.current_stream().wait_stream(side)
        for t in out:
            t.fill_(NAN) if t.is_floating_point() else None
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, out)), f"{what}: graph replay"


# ----------------------------------------------------------------------------- autograd Functions
def _counting(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapper)
    return calls


def test_functions_return_the_entries_results_in_the_parameters_layout():
    from tramba_amd import hip, resnet_train
    name = "3x3s2_9x11_odd"
    b, h, w, cin, cout, k, s = CONV_CASES[name]
    d = _conv_inputs(name, BF)
    x = d["x_clean"].clone().requires_grad_()
    weight = d["wt"].float().requires_grad_()                          # an fp32 master in the reference layout
    y = resnet_train._ConvCL.apply(x, weight, s)
    assert torch.equal(y, hip.conv_affine_cl(d["x_clean"], d["wk"], None, None, None, False, ksize=k, stride=s))
    y.backward(d["gy"])
    assert x.grad.dtype == BF and weight.grad.dtype == torch.float32 and weight.grad.shape == weight.shape
    assert torch.equal(x.grad, hip.conv_dgrad_cl(d["gy"], hip.conv_transposed_weight(d["wk"]), x.shape, s))
    assert torch.equal(weight.grad.permute(0, 2, 3, 1), hip.conv_wgrad_cl(d["gy"], d["x_clean"], k, s))
    x2 = d["x_clean"].clone().requires_grad_()                         # needs_input_grad skips the weight gradient
    resnet_train._ConvCL.apply(x2, weight.detach(), s).backward(d["gy"])
    assert torch.equal(x2.grad, x.grad)

    bn = _bn_inputs("two_images_9x11x256", BF)
    xb, res = bn["x"].clone().requires_grad_(), bn["res"].clone().requires_grad_()
    gamma, beta = bn["gamma"].clone().requires_grad_(), bn["beta"].clone().requires_grad_()
    rm, rv = bn["rm"].clone(), bn["rv"].clone()
    yb = resnet_train._BatchNormActCL.apply(xb, gamma, beta, res, rm, rv, EPS, MOM, True)
    rm2, rv2 = bn["rm"].clone(), bn["rv"].clone()
    mean, rstd = hip.bn_stats_cl(bn["x"], EPS, rm2, rv2, MOM)
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2) and not torch.equal(rm, bn["rm"])
    assert torch.equal(yb, hip.bn_act_cl(bn["x"], mean, rstd, bn["gamma"], bn["beta"], bn["res"], True))
    yb.backward(bn["dy"])
    want = hip.bn_act_bwd_cl(bn["dy"], bn["x"], yb.detach(), mean, rstd, bn["gamma"], True, want_dres=True)
    assert all(torch.equal(a, b) for a, b in zip((xb.grad, res.grad, gamma.grad, beta.grad), want))
    xf = bn["x"].clone().requires_grad_()                              # a frozen affine, no shortcut, no ReLU
    resnet_train._BatchNormActCL.apply(xf, bn["gamma"], bn["beta"], None, None, None, EPS, MOM, False).backward(bn["dy"])
    assert torch.equal(xf.grad, hip.bn_act_bwd_cl(bn["dy"], bn["x"], None, mean, rstd, bn["gamma"], False, want_affine=False)[0])

    px, pgy, y_ref, gx_ref = _pool_inputs("7x9", BF, True)
    xp = px.clone().requires_grad_()
    yp = resnet_train._MaxPoolCL.apply(xp)
    yp.backward(pgy)
    assert torch.equal(yp, y_ref) and torch.equal(xp.grad, gx_ref)


# ----------------------------------------------------------------------------- bottlenecks
import json  # noqa: E402
import os  # noqa: E402

import numpy as np  # noqa: E402

import resnet_train_blocks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parity(kind):
    """profiles/resnet_train_parity.json (scripts/measure_resnet_train_parity.py, 16 seeds on an MI355X, the blocks of
    tests/golden/resnet_train_blocks.py): per gradient tensor, m = (largest / smallest stock error) - 1 over the seeds -- the
    stock 16-bit path's own seed-to-seed spread is the yardstick, never the library path.  Tensors whose spread is not
    narrow (m >= 1) are listed there and left out: at most a quarter of them, and never a convolution weight."""
    with open(os.path.join(ROOT, "profiles", "resnet_train_parity.json")) as f:
        rec = json.load(f)[kind]
    m, left_out = rec["m"], set(rec["left_out"])
    assert left_out == {n for n, v in m.items() if not v < 1.0}
    assert len(left_out) <= len(m) // 4 and not any("conv" in n or n.endswith("downsample.0.weight") for n in left_out)
    return {n: v for n, v in m.items() if n not in left_out}, left_out


@pytest.mark.parametrize("kind", list(resnet_train_blocks.KINDS))
def test_block_gradients_keep_the_stock_error(kind):
    margins, left_out = _parity(kind)
    for seed in range(8):
        errors = resnet_train_blocks.block_errors(kind, seed)
        assert set(errors) == set(margins) | left_out
        for name, (lib, stock) in errors.items():
            print(f"{kind} seed {seed} {name}: library {lib:.3e} stock {stock:.3e}" + (" (left out)" if name in left_out else ""))
            if name not in left_out:
                assert lib <= stock * (1 + margins[name]), (kind, seed, name, lib, stock, margins[name])


class _NoStockOps:
    """torch.nn.functional with the three ops the training path replaces raising"""

    def __getattr__(self, name):
        if name in ("conv2d", "batch_norm", "max_pool2d"):
            raise AssertionError(f"F.{name} reached with the library training switch on")
        return getattr(F, name)


def _entry_counts(monkeypatch):
    from tramba_amd import hip
    return {n: _counting(monkeypatch, hip, n) for n in ("bn_stats_cl", "bn_act_cl", "bn_act_bwd_cl", "conv_affine_cl",
                                                        "conv_dgrad_cl", "conv_wgrad_cl", "maxpool3s2_cl", "maxpool3s2_bwd_cl")}


@pytest.mark.parametrize("kind", list(resnet_train_blocks.KINDS))
def test_block_with_the_switch_on_reaches_no_stock_op_and_repeats_bit_for_bit(monkeypatch, kind):
    from tramba_amd import models, resnet_train
    monkeypatch.setattr(resnet_train, "F", _NoStockOps())
    monkeypatch.setattr(models, "F", _NoStockOps())
    calls = _entry_counts(monkeypatch)
    one = resnet_train_blocks.block_grads(kind, 0, "library")
    assert [len(calls[n]) for n in ("bn_stats_cl", "bn_act_cl", "bn_act_bwd_cl", "conv_affine_cl", "conv_dgrad_cl",
                                    "conv_wgrad_cl")] == [4] * 6
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in one.values())
    two = resnet_train_blocks.block_grads(kind, 0, "library")
    assert all(torch.equal(one[k], two[k]) for k in one), [k for k in one if not torch.equal(one[k], two[k])]


_CONV_FORWARD = torch.nn.Conv2d.forward


def _pinned_conv(self, t):
    """nn.Conv2d.forward as a gather (F.unfold) and one matrix product, differentiable: the framework's own choice of
    convolution kernels splits reductions with atomics and does not repeat run to run (tests/test_gpu_resnet_conv.py)"""
    if self.groups != 1 or self.dilation != (1, 1) or self.bias is not None:
        return _CONV_FORWARD(self, t)
    b, _, h, w = t.shape
    ho = (h + 2 * self.padding[0] - self.kernel_size[0]) // self.stride[0] + 1
    wo = (w + 2 * self.padding[1] - self.kernel_size[1]) // self.stride[1] + 1
    cols = F.unfold(t, self.kernel_size, 1, self.padding, self.stride).transpose(1, 2)
    y = cols @ self.weight.reshape(self.out_channels, -1).t()
    return y.view(b, ho, wo, self.out_channels).permute(0, 3, 1, 2)


def test_switch_off_is_the_never_switched_block_and_fp32_and_eval_keep_the_stock_ops(monkeypatch):
    """(the framework's convolutions pinned to a deterministic GEMM form on both sides: its own choice does not repeat)"""
    from tramba_amd import encoders
    calls = _entry_counts(monkeypatch)
    monkeypatch.setattr(torch.nn.Conv2d, "forward", _pinned_conv)

    def on_then_off(blk):
        assert encoders.set_library_training(blk, True) == encoders.set_library_training(blk, False) == 1
    for mode in ("stock", "fp32"):
        never = resnet_train_blocks.block_grads("layer2", 0, mode, prepare=lambda blk: None)
        off = resnet_train_blocks.block_grads("layer2", 0, mode, prepare=on_then_off)
        assert all(torch.equal(never[k], off[k]) for k in never), [k for k in never if not torch.equal(never[k], off[k])]
    assert not any(calls.values())
    # the switch ON: fp32 activations, and eval mode with autograd, still reach no new entry
    blk, x = resnet_train_blocks.bottleneck("layer2", 0)
    assert encoders.set_library_training(blk, True) == 1
    from tramba_amd import resnet_train
    xf = x.float().requires_grad_()
    assert not resnet_train.train_path(blk, xf) and not resnet_train.train_path(blk.eval(), x.clone().requires_grad_())
    blk.train()
    blk(xf.permute(0, 3, 1, 2)).sum().backward()
    assert xf.grad is not None and not any(calls.values())
    with torch.no_grad():
        assert not resnet_train.train_path(blk, x)
    for bad in ("track", "momentum", "dilation"):
        blk, x = resnet_train_blocks.bottleneck("layer1", 0)
        encoders.set_library_training(blk, True)
        assert resnet_train.train_path(blk, x) and resnet_train.block_trainable(blk)
        if bad == "track":
            blk.bn2.track_running_stats = False
        elif bad == "momentum":
            blk.bn3.momentum = None
        else:
            blk.conv2.dilation = (2, 2)
        assert not resnet_train.block_trainable(blk), bad


# ----------------------------------------------------------------------------- whole model
def _train_model(library, frozen=False, dtype=torch.bfloat16, never=False):
    """never: the switch is not touched at all (library is then ignored); otherwise it is set on, then to `library`"""
    import tramba_amd as ta
    from tramba_amd import encoders
    m = ta.bulid_model_enc("Tramba-R-TSOD")
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        new.setdefault(k, sd[k])
    m.load_state_dict(new, strict=True)
    m = m.to(DEV).train()
    m.compute_dtype = dtype
    if frozen:
        m.freeze_encoder()
    for mod in m.modules():
        if isinstance(mod, ta.DropPath):
            mod.drop_prob = 0.0
    if not never:
        on, off = encoders.set_library_training(m, True), encoders.set_library_training(m, library)
        assert on == off == 17
    return m


def _batch():
    x = synth.synth_input("resnet_train_whole", (1, 3, 384, 384)).to(DEV)
    y = (synth.synth_input("resnet_train_whole_y", (1, 1, 384, 384)).to(DEV) > 0).float()
    return x, y


@functools.lru_cache(maxsize=None)
def _stock_step():
    """one fp32 stock step (16-bit activations with fp32 master weights do not run on the stock encoder): the names of the
    parameters that receive a gradient, and the encoder's buffers after it (for num_batches_tracked)"""
    from tramba_amd import train
    m = _train_model(library=False, dtype=None)
    train.train_step(m, train.get_opt(1e-4, m), *_batch())
    names = frozenset(k for k, p in m.named_parameters() if p.grad is not None)
    return names, {k: v.detach().clone() for k, v in m.encoder.named_buffers()}


def test_whole_model_train_step_on_the_library(monkeypatch):
    from tramba_amd import models, resnet_train, train
    x, y = _batch()
    have, stock_buffers = _stock_step()
    assert have and not any(k.startswith("encoder.layer4") for k in have)
    monkeypatch.setattr(resnet_train, "F", _NoStockOps())
    monkeypatch.setattr(models, "F", _NoStockOps())
    from tramba_amd import hip
    real_stats, updated, worst = hip.bn_stats_cl, {}, []

    def checked_stats(xm, eps, running_mean=None, running_var=None, momentum=0.1):
        old_m, old_v = running_mean.double(), running_var.double()
        out = real_stats(xm, eps, running_mean, running_var, momentum)
        xd = xm.double().view(-1, xm.shape[-1])
        n = xd.shape[0]
        mean = xd.mean(0)
        d = dict(m=n, mean=mean, var=((xd - mean) ** 2).sum(0) / n, absmean=xd.abs().sum(0) / n)
        bm, bv = _stats_bounds(d)
        mom, unb = float(torch.tensor(momentum, dtype=torch.float32)), n / (n - 1)
        for got, old, new, bnd in ((running_mean, old_m, d["mean"], bm), (running_var, old_v, unb * d["var"], unb * bv)):
            ref = (1 - mom) * old + mom * new
            ratio = (got.double() - ref).abs() / (mom * bnd + 5 * E * ((1 - mom) * old.abs() + mom * new.abs()))
            worst.append(float(ratio.max()))
            updated[got.data_ptr()] = updated.get(got.data_ptr(), 0) + 1
        return out
    monkeypatch.setattr(hip, "bn_stats_cl", checked_stats)
    calls = _entry_counts(monkeypatch)                                 # (counts the checked entry)
    m = _train_model(library=True)
    before = {k: v.detach().clone() for k, v in m.encoder.named_buffers()}
    loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
    print(f"running buffers of {len(worst) // 2} batch norms: worst |got - fp64 update| / bound = {max(worst):.4f}")
    assert len(worst) == 86 and max(worst) <= 1.0
    assert torch.isfinite(loss).all()
    assert {n: len(c) for n, c in calls.items()} == dict(bn_stats_cl=43, bn_act_cl=43, bn_act_bwd_cl=43, conv_affine_cl=42,
                                                         conv_dgrad_cl=42, conv_wgrad_cl=42, maxpool3s2_cl=1,
                                                         maxpool3s2_bwd_cl=1)
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert got == have, (sorted(got - have)[:5], sorted(have - got)[:5])
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    # running statistics: layer4's untouched; every other batch norm's buffers were handed to the statistics entry exactly
    # once, and (checked inside `checked_stats`, on each norm's own input) hold the fp64 update to the kernel-level bound
    after = dict(m.encoder.named_buffers())
    for k, v in after.items():
        if k.startswith("layer4"):
            assert torch.equal(v, before[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1 == int(stock_buffers[k]), k
        else:
            assert updated.pop(v.data_ptr()) == 1 and not torch.equal(v, before[k]), k
    assert not updated
    # a frozen encoder: the step runs, no weight gradient entry is reached
    del m
    for c in calls.values():
        del c[:]
    m = _train_model(library=True, frozen=True)
    loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
    assert torch.isfinite(loss).all() and not calls["conv_wgrad_cl"] and len(calls["bn_stats_cl"]) == 43
    assert all(p.grad is None for k, p in m.named_parameters() if not p.requires_grad)


def test_two_library_encoder_passes_from_the_same_state_give_the_same_bits():
    x, _ = _batch()
    runs = []
    for _ in range(2):
        m = _train_model(library=True)
        feats = m.encoder.features_cl(x.to(torch.bfloat16))
        dys = [synth.synth_input(f"resnet_train_repro_dy{i}", tuple(f.shape)).to(DEV).to(f.dtype) for i, f in enumerate(feats)]
        torch.autograd.backward(feats, dys)
        runs.append([f.detach() for f in feats] + [p.grad for k, p in m.encoder.named_parameters() if p.grad is not None]
                    + [b.detach().clone() for b in m.encoder.buffers()])
        del m
    assert len(runs[0]) == len(runs[1]) > 100
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _step_gradients(m):
    """one `train.train_step` -> ({parameter name: gradient}, {encoder buffer name: value})"""
    from tramba_amd import train
    loss = train.train_step(m, train.get_opt(1e-4, m), *_batch())
    assert torch.isfinite(loss).all()
    return ({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
            {k: v.detach().clone() for k, v in m.encoder.named_buffers()})


def _differing(one, two):
    assert set(one) == set(two)
    return [k for k in one if not torch.equal(one[k], two[k])]


def test_two_library_train_steps_from_the_same_state_give_the_same_gradients():
    """the whole step -- encoder, decoder, loss -- twice from the same state: every gradient and every encoder buffer bit for bit"""
    (g1, b1), (g2, b2) = (_step_gradients(_train_model(library=True)) for _ in range(2))
    assert len(g1) > 300
    diff = _differing(g1, g2) + _differing(b1, b2)
    print(f"{len(diff)} of {len(g1) + len(b1)} gradients / buffers differ between two library train steps: {diff[:8]}")
    assert not diff


def test_fp32_step_with_the_switch_on_or_on_then_off_is_the_never_switched_step(monkeypatch):
    """fp32 activations keep the stock path: an fp32 Tramba-R `train_step` through `BaseUMambaEnc.forward` with the switch
    ON, and one with it on then off, reach no new entry and give the gradients and buffers of the step of a model whose
    switch was never touched (the framework's convolutions pinned to a deterministic GEMM form on all three sides)"""
    calls = _entry_counts(monkeypatch)
    monkeypatch.setattr(torch.nn.Conv2d, "forward", _pinned_conv)
    m = _train_model(library=False, dtype=None, never=True)
    assert not any(hasattr(mod, "library_training") and "library_training" in mod.__dict__ for mod in m.modules())
    never = _step_gradients(m)
    del m
    m = _train_model(library=False, dtype=None)
    assert not m.encoder.library_training
    off = _step_gradients(m)
    del m
    m = _train_model(library=True, dtype=None)
    assert m.encoder.library_training and all(b.library_training for layer in (m.encoder.layer1, m.encoder.layer4) for b in layer)
    on = _step_gradients(m)
    for what, got in (("on then off", off), ("on", on)):
        diff = _differing(never[0], got[0]) + _differing(never[1], got[1])
        assert not diff, (what, diff[:8])
    assert not any(calls.values())
    assert any(k.startswith("layer4") and k.endswith("running_mean") for k in never[1])
    before = dict(_train_model(library=False, dtype=None, never=True).encoder.named_buffers())
    assert not torch.equal(on[1]["layer4.0.bn1.running_mean"], before["layer4.0.bn1.running_mean"].to(DEV))   # stock runs layer4


def test_eval_mode_with_autograd_and_fp32_keep_the_stock_forward_of_a_switched_encoder(monkeypatch):
    """`ResNet.features_cl` with the switch ON: in eval mode with autograd on (the encoder cast to bf16, so that the stock
    forward runs) and in train mode on fp32 activations it reaches no new entry, and returns what the unswitched encoder
    returns under the pinned convolution"""
    from tramba_amd import encoders, models
    calls = _entry_counts(monkeypatch)
    monkeypatch.setattr(torch.nn.Conv2d, "forward", _pinned_conv)
    torch.manual_seed(5)
    enc = models.ResNet().to(DEV)
    x = synth.synth_input("resnet_train_fallback", (2, 3, 64, 64)).to(DEV)

    def run(e, inp):
        inp = inp.detach().requires_grad_()
        feats = e.features_cl(inp)
        torch.autograd.backward(feats, [torch.ones_like(f) for f in feats])
        assert torch.isfinite(inp.grad).all() and float(inp.grad.abs().max()) > 0
        return [f.detach() for f in feats] + [inp.grad]
    for mode in ("bf16 eval", "fp32 train"):
        e = enc.to(BF).eval() if mode == "bf16 eval" else enc.float().train()
        inp = x.to(BF) if mode == "bf16 eval" else x
        state = {k: v.clone() for k, v in e.state_dict().items()}
        assert encoders.set_library_training(e, False) == 17
        want = run(e, inp)
        e.load_state_dict(state)                                       # (train mode moved the running statistics)
        assert encoders.set_library_training(e, True) == 17 and e.library_training
        got = run(e, inp)
        assert all(torch.equal(a, b) for a, b in zip(want, got)), mode
    assert not any(calls.values())


def test_graphed_train_step_follows_the_eager_step():
    """the yardsticks of tests/test_gpu_enc_train.py's test of the same name, on Tramba-R with the switch on; the replays
    advance num_batches_tracked and move the running mean"""
    import tramba_amd as ta
    from tramba_amd import train
    x, y = _batch()
    m = _train_model(library=True)
    opt = train.get_opt(1e-4, m)
    eager = [float(train.train_step(m, opt, x, y)) for _ in range(6)]
    del m, opt
    m = _train_model(library=True)
    step = ta.GraphedTrainStep(m, train.get_opt(1e-4, m, capturable=True))
    bn1 = m.encoder.bn1
    tracked = [int(bn1.num_batches_tracked)]
    got = [float(step(x, y))]                # eager warm-up steps (undone), capture, replay: exactly step 1
    tracked.append(int(bn1.num_batches_tracked))
    means = [bn1.running_mean.detach().clone()]
    for _ in range(5):
        got.append(float(step(x, y)))
        tracked.append(int(bn1.num_batches_tracked))
        means.append(bn1.running_mean.detach().clone())
    print(f"Tramba-R: graphed {got} eager {eager} num_batches_tracked {tracked}")
    assert got[0] == pytest.approx(eager[0], rel=1e-5)                 # same initial weights, same batch: same first loss
    assert np.allclose(got, eager, rtol=3e-2), (got, eager)
    assert len(step._graphs) == 1
    assert tracked == [tracked[0] + i for i in range(7)]
    assert all(not torch.equal(a, b) for a, b in zip(means, means[1:]))
