"""Every nonlinearity the kernels embed, probed at its tails and switch-over points (tests/golden/pointwise_cases.py): each probe
makes an output element equal ONE function value of a SWEEP argument (0, +-2^-30 .. +-1e4: where exp overflows, where 1 + exp(x)
rounds to 1, the softplus threshold 20 and clamp 60, the fp16 output limit), so that the check is on the function, not a sum.

Rule (tests/test_pointwise_host.py measures E32 per formula and shows that a tanh-GELU, an unguarded softplus, exp / (1 + exp), a
-log(sigmoid) BCE, a softmax without its row maximum and a clamping fp16 store all break it): with e = |got - want| / max(1,
|want|) against the fp64 reference, an fp32 output is within 8 x E32_F; a 16-bit output within u |want| + 8 E32_F max(1, |want|)
per element; every output is finite wherever the reference, rounded to the output dtype, is; the uint8 and range-limit cases
are bit-exact.  Every case appends a record (kernel, form, dtype, function, worst x, error, bound) to RECORDS; `form` names the
knob requested, and each test asserts or states that the library honours it at its shape.  RECORDS is what
scripts/measure_pointwise_parity.py dumps into profiles/pointwise_parity.json."""
import pytest
import torch

import pointwise_cases as pc

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF16, F16]
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
RECORDS = []


def hip():
    from tramba_amd import hip as h
    return h


def _dev():
    return torch.device("cuda")


def _sync(H):
    torch.cuda.synchronize()
    H.device_error()


def _hold(recs):
    RECORDS.extend(recs)
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    for r in recs:
        assert r["ok"], r


def _rec(kernel, form, dtype, function, got, want, xs, formula, out_dtype, variant=""):
    return pc.record(kernel, form, dtype, function, pc.check(got, want, xs, formula, out_dtype), variant)


# ----------------------------------------------------------------------------- boundary selective scan
def _scan_records(H, o, label):
    dev = _dev()
    g = [t.to(dev) for t in (o.u, o.delta, o.A, o.B, o.C, o.D, o.delta_bias)]
    out, ckpt = H.selective_scan_fwd(*g, o.softplus, True)
    grads = H.selective_scan_bwd(*g, o.dout.to(dev), ckpt, o.softplus)
    _sync(H)
    want_out, want_g = pc.scan_probe_oracle(o)
    ns = o.n if o.all_states else 1
    fwd, bwd_sp, bwd_d = ("softplus_lean", "softplus20", "dsoftplus_sigmoid") if o.softplus else ("identity",) * 3
    rows = torch.arange(o.kd)
    x_all = o.x_eff[None].double()
    own = o.xs[:, None].expand(o.kd, o.l)[None]                 # the argument behind out[r, t]: the row's own value
    recs = [_rec("selective_scan_fwd", f"N={o.n} L={o.l}", o.dtype, label, out / ns, want_out / ns, own, fwd, F32)]
    # the closed forms at the probed elements, independent of the oracle's recurrence
    ex = pc.scan_probe_expected(o)
    recs.append(_rec("selective_scan_fwd", f"N={o.n} L={o.l}", o.dtype, label + " closed form", out[0, rows, o.pos].cpu() / ns,
                     ex["out"] / ns, o.xs, fwd, F32))
    du, ddelta, dA, dB, dC, dD, dbias = grads
    wdu, wdd, wdA, wdB, wdC, wdD, wdbias = want_g
    xs_bc = torch.zeros(1, o.k, o.n, o.l)                        # the argument behind dB / dC [k, n, s]: the row of group k at s
    xs_bc[0, torch.arange(o.kd) // o.dper, :, o.pos] = o.xs[:, None].expand(o.kd, o.n)
    form = f"N={o.n} L={o.l}"
    recs += [
        _rec("selective_scan_bwd", form, o.dtype, label + " du", du.float() / ns, wdu / ns, x_all, bwd_sp, o.dtype),
        _rec("selective_scan_bwd", form, o.dtype, label + " ddelta", ddelta.float() / ns, wdd / ns, own, bwd_d, o.dtype),
        _rec("selective_scan_bwd", form, o.dtype, label + " ddelta closed form", ddelta[0, rows, o.pos].float().cpu() / ns,
             ex["ddelta"] / ns, o.xs, bwd_d, o.dtype),
        _rec("selective_scan_bwd", form, o.dtype, label + " dB", dB, wdB, xs_bc, bwd_sp, F32),
        _rec("selective_scan_bwd", form, o.dtype, label + " dC", dC, wdC, xs_bc, bwd_sp, F32),
        _rec("selective_scan_bwd", form, o.dtype, label + " dbias", dbias / ns, wdbias / ns, o.xs, bwd_d, F32),
        _rec("selective_scan_bwd", form, o.dtype, label + " dA", dA, wdA, torch.zeros(o.kd, o.n), "identity", F32),
        _rec("selective_scan_bwd", form, o.dtype, label + " dD", dD, wdD, o.xs, "identity", F32),
    ]
    return recs


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("l", pc.SCAN_LS)
@pytest.mark.parametrize("n", pc.SCAN_NS)
def test_selective_scan_softplus_and_its_derivative(n, l, dtype):
    """selective_scan_fwd / _bwd, 10 groups x 32 rows, d_state 1, 4 (fixed kernels) and 3, 16 (state-looped), L = 37 (scalar
    accesses) / 40 (16-byte accesses): A = 0, D = 0, u and dout one-hot per row, B = C = 1 in state 0, delta + delta_bias a sweep
    value at every position.  out[r, t >= s_r] = softplus(x_r) (softplus_lean: clamp 60), du = softplus (softplus20: threshold
    20), ddelta[r, s_r] = dbias = softplus' (sigmoid up to 20, 1 beyond), dB / dC in closed form -- all seven gradients against the
    fp64 oracle, the probed elements also against the closed form.  d_state 3 and 16 run a second time with B = C = 1 in EVERY
    state (every pass of the state loop), both sides divided by N."""
    H = hip()
    recs = _scan_records(H, pc.scan_probe(n, l, dtype), "softplus")
    if n in (3, 16):
        recs += _scan_records(H, pc.scan_probe(n, l, dtype, all_states=True), "softplus, all states")
    _hold(recs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 16])
def test_selective_scan_without_softplus(n, dtype):
    """delta_softplus = False on |x| <= 100: dt = x itself, out = x, ddelta = 1"""
    _hold(_scan_records(hip(), pc.scan_probe(n, 40 if dtype == BF16 else 37, dtype, softplus=False), "identity"))


# ----------------------------------------------------------------------------- GEMM epilogues
def _gemm_case(H, o, form, out_dtype, kernel="linear_cl"):
    dev = _dev()
    res = None if o.residual is None else o.residual.to(dev)
    y = H.linear_cl(o.x.to(dev), o.w.to(dev), o.bias.to(dev), res, o.act, out_dtype)
    _sync(H)
    want = act_want(o)
    return _rec(kernel, f"{pc.GEMM_FORM_NAME[form]} M={o.m} N={o.n} K={o.k}", o.dtype, pc.ACT_NAME[o.act], y, want, o.xs,
                pc.ACT_FORMULA[o.act], out_dtype)


def act_want(o):
    return pc.act_reference(o.act, o.xs)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("form", pc.GEMM_FORMS)
def test_gemm_epilogues_of_every_forced_form(form, dtype):
    """linear_cl with x = 0 and bias = SWEEP over the columns: y[m, n] = act(bias[n]) for SiLU, GELU, the sigmoid gate (residual
    = 1) and gelu'(residual) (bias = 1, residual = the sweep the dtype holds).  TUNE_GEMM_TILE 7 / 13 / 14 (LDS-DMA on 4 / 2 / 3
    stages), 16 / 17 (producer / consumer on 3 / 4 stages), 18 (the rule without them): fp32 output, fp32-level bound -- a
    tanh-GELU (4.7e-4 off) fails by 300 x.  M = 128, N = 512, K = 128 and the ragged M = 100, N = 520, K = 64 (scalar tail branch
    of tile_epilogue).  19 (weight-stationary: same-dtype output only, SiLU and GELU) is held to the 16-bit rule; every form
    also runs with a 16-bit output."""
    H = hip()
    recs = []
    try:
        H.tune_set(H.TUNE_GEMM_TILE, form)
        for name, (m, n, k) in pc.GEMM_SHAPES.items():
            if form == 19 and name != "whole":
                continue
            for act in pc.GEMM_ACTS:
                if form == 19 and act not in (pc.ACT_SILU, pc.ACT_GELU):
                    continue
                o = pc.gemm_probe(m, n, k, dtype, act)
                for out_dtype in ((dtype,) if form == 19 else (F32, dtype)):
                    recs.append(_gemm_case(H, o, form, out_dtype))
    finally:
        H.tune_set(H.TUNE_GEMM_TILE, 0)
    _hold(recs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_gemm_epilogues_of_the_other_kernels(dtype):
    """the kernels no knob selects: K = 72 (K % 64 != 0: linear_tiled_kernel), K = 50 (linear16_kernel), fp32 operands
    (linear32_kernel), at M = 100, N = 520"""
    H = hip()
    recs = []
    for k in ((50,) if dtype == F32 else (72, 50)):
        for act in pc.GEMM_ACTS:
            o = pc.gemm_probe(100, 520, k, dtype, act)
            for out_dtype in {F32, dtype}:
                recs.append(_gemm_case(H, o, 0, out_dtype))
    _hold(recs)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("form", [0, 13, 16, 19])
def test_dual_output_gemm_epilogue(form, dtype):
    """linear_dual_cl: (pre, act(pre)) = (bias, act(bias)), both in the input dtype, on the rule's form, LDS-DMA, producer /
    consumer and weight-stationary"""
    H = hip()
    dev = _dev()
    recs = []
    try:
        H.tune_set(H.TUNE_GEMM_TILE, form)
        for act in (pc.ACT_SILU, pc.ACT_GELU):
            o = pc.gemm_probe(128, 512, 128, dtype, act)
            pre, y = H.linear_dual_cl(o.x.to(dev), o.w.to(dev), o.bias.to(dev), act)
            _sync(H)
            label = f"{pc.GEMM_FORM_NAME[form]} M=128 N=512 K=128"
            recs.append(_rec("linear_dual_cl", label, dtype, "pre", pre, o.xs.double(), o.xs, "identity", dtype))
            recs.append(_rec("linear_dual_cl", label, dtype, pc.ACT_NAME[act], y, act_want(o), o.xs, pc.ACT_FORMULA[act], dtype))
    finally:
        H.tune_set(H.TUNE_GEMM_TILE, 0)
    _hold(recs)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("form", [0, 18])
def test_two_source_gemm_epilogue(form, dtype):
    """linear2_cl (K = 64 + 64): the producer / consumer kernel with the two-source loaders, and the register-staged lean kernel
    (knob 18)"""
    H = hip()
    dev = _dev()
    recs = []
    try:
        H.tune_set(H.TUNE_GEMM_TILE, form)
        for act in pc.GEMM_ACTS:
            o = pc.gemm_probe(100, 520, 128, dtype, act)
            res = None if o.residual is None else o.residual.to(dev)
            x = o.x.to(dev)
            y = H.linear2_cl(x[:, :64].contiguous(), x[:, 64:].contiguous(), o.w.to(dev), o.bias.to(dev), res, act, F32)
            _sync(H)
            recs.append(_rec("linear2_cl", f"{pc.GEMM_FORM_NAME[form]} M=100 N=520 K=64+64", dtype, pc.ACT_NAME[act], y, act_want(o),
                             o.xs, pc.ACT_FORMULA[act], F32))
    finally:
        H.tune_set(H.TUNE_GEMM_TILE, 0)
    _hold(recs)


# ----------------------------------------------------------------------------- norms and the depth-wise stencil
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", [64, 200])
def test_layernorm_gelu_epilogues(c, dtype):
    """layernorm_cl and add_layernorm_cl (dual: n and act(n)) with w = 0, b = a piece of SWEEP, act = GELU: the output is
    gelu(b) whatever x holds; 5 rows, C = 64 / 200, the sweep in pieces of C channels.  The dual output is the activation of n AS
    STORED in the activation dtype (train_fused.hip: the consumer's backward differentiates at the stored value, and so does the
    reference, whose GELU is a separate 16-bit op): pinned as gelu(round16(b))."""
    H = hip()
    dev = _dev()
    recs = []
    for b in pc.chunks(c):
        x, w, _ = pc.norm_probe(5, c, dtype, b)
        xs = b[None].expand(5, c)
        want = pc.ref_gelu(xs)
        y = H.layernorm_cl(x.to(dev), w.to(dev), b.to(dev), 1e-5, pc.ACT_GELU)
        xsum, n, na = H.add_layernorm_cl(x.view(1, 5, c).to(dev), torch.zeros(1, 5, c, dtype=dtype, device=dev), None, w.to(dev),
                                         b.to(dev), 1e-5, pc.ACT_GELU, dual=True)
        _sync(H)
        recs.append(_rec("layernorm_cl", f"C={c}", dtype, "gelu", y, want, xs, "gelu", dtype))
        stored = xs.to(dtype).float()        # dual: the activation is taken of n AS STORED (what the consumer's backward differentiates)
        recs.append(_rec("add_layernorm_cl", f"C={c}", dtype, "gelu(stored n)", na, pc.ref_gelu(stored), stored, "gelu", dtype))
        recs.append(_rec("add_layernorm_cl", f"C={c}", dtype, "none", n, xs.double(), xs, "identity", dtype))
    _hold(recs)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_merge_norm_epilogues(fam, out_dtype):
    """ss2d_merge_norm_cl on a 12 x 12 map, D = 64, ln_w = 0, ln_b = a piece of SWEEP, act = SiLU and GELU"""
    H = hip()
    dev = _dev()
    order = H.scan_order(fam, 12, 12, dev)
    g = torch.Generator().manual_seed(3)
    ys = torch.randn(1, order.k, 144, 64, generator=g).to(dev)
    recs = []
    for b in pc.chunks(64):
        xs = b[None].expand(144, 64)
        for act in (pc.ACT_SILU, pc.ACT_GELU):
            y = H.ss2d_merge_norm_cl(ys, order, torch.zeros(64, device=dev), b.to(dev), 1e-5, act, out_dtype)
            _sync(H)
            recs.append(_rec("ss2d_merge_norm_cl", fam, out_dtype, pc.ACT_NAME[act], y, pc.act_reference(act, xs), xs,
                             pc.ACT_FORMULA[act], out_dtype))
    _hold(recs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_merge_grad_silu_derivative(fam, dtype):
    """ss2d_merge_grad_cl = (merge(gu) + addend) * silu'(zpre) with gu = 0, addend = 1, zpre = the sweep the dtype holds, 12 x 12
    map, D = 64: the output is silu'(zpre) = s (1 + x (1 - s))"""
    H = hip()
    dev = _dev()
    order = H.scan_order(fam, 12, 12, dev)
    xs = pc.tiled(pc.sweep_for(dtype), 144 * 64).reshape(1, 144, 64)
    zpre = xs.to(dtype).to(dev)
    y = H.ss2d_merge_grad_cl(torch.zeros(1, order.k, 144, 64, dtype=dtype, device=dev), order, torch.ones_like(zpre), zpre)
    _sync(H)
    _hold([_rec("ss2d_merge_grad_cl", fam, dtype, "silu'", y, pc.ref_dsilu(xs), xs, "dsilu", dtype)])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("ks", [3, 7])
def test_depthwise_stencil_silu(ks, dtype):
    """dwconv_cl and dwconv_dual_cl, a centre tap of 1 and zeros elsewhere, x + bias = the sweep value of the channel (x its part
    in the dtype), 6 x 6 map, 320 channels: pre = the value, out = silu(value); the 7 x 7 stencil on the marching kernel (the
    library's choice) and on the row kernel (TUNE_DW_FORM 1).  dwconv_dual_cl takes the activation of the pre-activation AS STORED
    (norm_conv.hip, the reference's behaviour): pinned as silu(round16(value)); dwconv_cl activates the fp32 value."""
    H = hip()
    dev = _dev()
    o = pc.dw_probe(dtype, ks)
    recs = []
    try:
        for form in ((0, 1) if ks == 7 else (0,)):
            H.tune_set(H.TUNE_DW_FORM, form)
            x, wt, bt = o.x.to(dev), o.wt.to(dev), o.bt.to(dev)
            y = H.dwconv_cl(x, wt, bt, pc.ACT_SILU)
            pre, y2 = H.dwconv_dual_cl(x, wt, bt, pc.ACT_SILU)
            _sync(H)
            label = f"ks={ks} form={form}"
            recs.append(_rec("dwconv_cl", label, dtype, "silu", y, pc.ref_silu(o.xs), o.xs, "silu", dtype))
            stored = o.xs.to(dtype).float()  # dual: the activation is taken of the pre-activation AS STORED (norm_conv.hip)
            recs.append(_rec("dwconv_dual_cl", label, dtype, "silu(stored pre)", y2, pc.ref_silu(stored), stored, "silu", dtype))
            recs.append(_rec("dwconv_dual_cl", label, dtype, "pre", pre, o.xs.double(), o.xs, "identity", dtype))
    finally:
        H.tune_set(H.TUNE_DW_FORM, 0)
    _hold(recs)


# ----------------------------------------------------------------------------- loss
def _loss_rec(kernel, form, function, got, want, formula, variant=""):
    return _rec(kernel, form, F32, function, got, want, torch.zeros_like(want), formula, F32, variant)


@pytest.mark.parametrize("resized", [False, True], ids=["same", "resized"])
@pytest.mark.parametrize("label", ["zeros", "ones", "checker"])
def test_loss_on_saturated_logits(label, resized):
    """sod_loss / sod_loss_grad and sod_wloss / sod_wloss_grad (with and without IoU, eps 0 / 0.1, batch-mean and per-pixel BCE) on
    one 32 x 32 plane whose logits are SWEEP tiled (or a 16 x 16 map of it resized), labels all-0, all-1, checkerboard: the loss
    against fp64 max(z, 0) - z y + log1p(exp(-|z|)) (+ IoU), every gradient element against the closed form of loss_optim.hip's
    header (times the 1024 pixels, so that the measure e sees p - y), all finite, all within 8 x E32 (of the BCE term, of p - y)."""
    H = hip()
    dev = _dev()
    z, y = pc.loss_probe(label, resized)
    zd, yd = z.to(dev), y.to(dev)
    form = f"{label} {'16->32' if resized else '32'}"
    recs = []
    loss, coefs = H.sod_loss([zd], yd)
    grad = H.sod_loss_grad(zd, yd, coefs[0])
    _sync(H)
    want, wgrad = pc.loss_reference(z, y)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    recs.append(_loss_rec("sod_loss", form, "bce+iou", loss.reshape(1), want.reshape(1), "bce"))
    recs.append(_rec("sod_loss_grad", form, F32, "d(bce+iou)", grad * 1024, wgrad * 1024, z.expand_as(grad), "dbce", F32))
    wmap = H.loss_weight_map(yd, 15)
    wm = wmap.cpu()
    for eps in (0.0, 0.1):
        for with_iou in (True, False):
            for pixel in (False, True):
                loss, coefs = H.sod_wloss([zd], yd, wmap, None, eps, pixel, with_iou)
                grad = H.sod_wloss_grad(zd, yd, wmap, coefs[0], None, eps)
                _sync(H)
                assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
                want, wgrad = pc.loss_reference(z, y, wm, eps, with_iou, pixel)
                var = f"eps={eps} iou={int(with_iou)} pixel={int(pixel)}"
                recs.append(_loss_rec("sod_wloss", form, "wbce", loss.reshape(1), want.reshape(1), "bce", var))
                recs.append(_rec("sod_wloss_grad", form, F32, "d(wbce)", grad * 1024, wgrad * 1024, z.expand_as(grad), "dbce", F32,
                                 var))
    _hold(recs)


# ----------------------------------------------------------------------------- frames
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_logits_to_u8_is_bit_equal_on_the_sweep(dtype):
    """logits_to_u8 at the same size in and out on SWEEP-valued logits (the values the dtype holds): bit-equal to
    (torch.sigmoid(z) * 255).to(torch.uint8) computed on the CPU in fp32"""
    H = hip()
    z = pc.tiled(pc.sweep_for(dtype), 2 * 32 * 48).reshape(2, 1, 32, 48)
    got = H.logits_to_u8(z.to(dtype).to(_dev()), 32, 48)
    _sync(H)
    want = pc.ref_u8(z).reshape(2, 32, 48)
    diff = (got.cpu().int() - want.int()).abs()
    i = int(diff.reshape(-1).argmax())
    RECORDS.append(dict(kernel="logits_to_u8", form="32x48", dtype=IDS[dtype], function="uint8(sigmoid*255)",
                        worst_x=float(z.reshape(-1)[i]), error=float(diff.max()), bound=0.0, ok=bool(diff.max() == 0), out_dtype="uint8", variant=""))
    assert torch.equal(got.cpu(), want), (float(z.reshape(-1)[i]), int(got.cpu().reshape(-1)[i]), int(want.reshape(-1)[i]))


# ----------------------------------------------------------------------------- output range
def _bit_equal(kernel, form, got, want, xs):
    got = got.cpu()
    same = got.view(torch.int16) == want.view(torch.int16).expand_as(got)
    bad = (~same).reshape(-1).nonzero()
    i = int(bad[0]) if len(bad) else 0
    RECORDS.append(dict(kernel=kernel, form=form, dtype="float16", function="fp16 store", worst_x=float(xs.expand_as(got).reshape(-1)[i]),
                        error=float(len(bad)), bound=0.0, ok=len(bad) == 0, out_dtype="float16", variant=""))
    assert len(bad) == 0, (kernel, form, float(xs.expand_as(got).reshape(-1)[i]), float(got.reshape(-1)[i]))


def test_fp16_outputs_at_the_range_limit():
    """Sums of exactly 65503, 65504, 65519, 65520, 65536, 7e4 and their negatives stored as fp16: bit-equal to the IEEE
    conversion (65504 below 65520, inf from there on; no clamp, no garbage) out of linear_cl (identity weight, x + residual, on
    every forced form, the K = 72 and K = 60 kernels), layernorm_cl (w = 0, b = the sum) and the boundary scan's same-dtype
    output (the one-hot u scaled, softplus off, delta = 1)."""
    H = hip()
    dev = _dev()
    a, b, want = pc.range_probe()
    sums = a.double() + b.double()
    n = 128
    idx = torch.arange(n) % len(a)
    for k in (128, 72, 60):
        x = torch.zeros(64, k, dtype=F16)
        w = torch.zeros(n, k, dtype=F16)
        for j in range(n):                       # column j reads x[:, j % k]
            w[j, j % k] = 1.0
        cols = torch.arange(k) % len(a)
        x[:] = a[cols]
        res = torch.empty(64, n, dtype=F16)
        rest = sums[idx] - a[cols][torch.arange(n) % k].double()
        res[:] = rest.to(F16)
        assert torch.equal(res[0].double(), rest)
        assert torch.equal(x[0, torch.arange(n) % k].double() + res[0].double(), sums[idx])
        try:
            for form in ((0,) + pc.GEMM_FORMS if k == 128 else (0,)):
                H.tune_set(H.TUNE_GEMM_TILE, form)
                y = H.linear_cl(x.to(dev), w.to(dev), None, res.to(dev))
                _sync(H)
                _bit_equal("linear_cl", f"{pc.GEMM_FORM_NAME[form]} K={k}", y, want[idx][None], sums[idx][None])
        finally:
            H.tune_set(H.TUNE_GEMM_TILE, 0)
    bsum = pc.tiled(sums.float().numpy(), 64)
    g = torch.Generator().manual_seed(1)
    y = H.layernorm_cl(torch.randn(5, 64, generator=g).to(F16).to(dev), torch.zeros(64, device=dev), bsum.to(dev), 1e-5, pc.ACT_NONE)
    _sync(H)
    _bit_equal("layernorm_cl", "C=64", y, pc.f16_store(bsum)[None], bsum[None])
    # the scan: dt = 1 exactly (softplus off), u_r = 2^15 at s_r, D_r = sum / 2^15 - 1: out[r, s_r] = h + D u = the sum, exact in fp32
    o = pc.scan_probe(4, 40, F16, softplus=False, values=[1.0], u_scale=32768.0)
    tgt = pc.tiled(sums.float().numpy(), o.kd)
    o.D = (tgt.double() / 32768.0 - 1.0).float()
    assert torch.equal(32768.0 + o.D.double() * 32768.0, tgt.double())
    out, _ = H.selective_scan_fwd(*[t.to(dev) for t in (o.u, o.delta, o.A, o.B, o.C, o.D, o.delta_bias)], False, False, False)
    _sync(H)
    rows = torch.arange(o.kd)
    assert out.dtype == F16
    _bit_equal("selective_scan_fwd", "N=4 L=40 same-dtype output", out[0, rows, o.pos], pc.f16_store(tgt), tgt)


# ----------------------------------------------------------------------------- fused SS2D scan
RING, SEGMENT, LDS_DMA = 1, 2, 3        # TRAMBA_TUNE_SCAN_FORM


def _kd(t, c, shape):
    """the (K, D) arguments behind a (1, K, L, D) / (1, K, D) output"""
    return (t[None, :, None, :] if len(shape) == 4 else t[None]).expand(shape)


def _fused_forward(H, c, fam, mode, form, label, ys_dtypes):
    import scan_memory_cases as smc
    want = smc.reference(c)["ys"]
    assert float((want - pc.ss2d_expected(c)["ys"]).abs().max()) <= 1e-12 * float(want.abs().max())
    xs = _kd(c.xs, c, want.shape)
    return [_rec("ss2d_scan_cl", f"{fam} {label} {mode}", c.dtype, "softplus", smc.run_scan(H, c, _dev(), form, yd), want, xs,
                 "softplus_med3", yd) for yd in ys_dtypes]


@pytest.mark.parametrize("mode", ["bias", "mfma"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_fused_scan_softplus(fam, dtype, mode):
    """ss2d_scan_cl on a 12 x 12 map, D = 32, dt_rank 8, A = 0, Ds = 0, B = C = 1, x one-hot in position per channel: the
    per-direction ys holds softplus(x_kc) from the position that owns the impulse on (times the visits so far where a helix
    direction passes a position more than once) -- t = med3(log2(1 + 2^x'), x', 128).  x' from dt_bias alone (dt_w = 0, the whole
    sweep over the K * D channels, piece by piece) or out of the dt_proj MFMA (dt_bias = 0, a one-hot rank column times dt_w,
    |x'| <= 1e4).  The two forms this size can be forced into: register ring (knob 1) and wave-segment (knob 2: honoured whenever
    the workspace is passed), plus a launch without the segment workspace (the ring again at this size: 5 tiles).  Knob 3 is NOT
    honoured here (the LDS-DMA kernel wants L >= 1024): test_fused_scan_softplus_lds_dma.  ys in fp32 and in the input dtype,
    against the fp64 reference of scan_memory_cases and the closed form."""
    import scan_memory_cases as smc
    H = hip()
    kd = (4 if fam == "raster" else 8) * pc.SS2D_D
    assert not pc.ss2d_dma_runs(pc.SS2D_H ** 2, pc.SS2D_D, pc.SS2D_R, kd // pc.SS2D_D, BF16)
    recs = []
    for values in pc.ss2d_values(mode, kd):
        c = pc.ss2d_probe(fam, dtype, mode, values)
        recs += _fused_forward(H, c, fam, mode, RING, "ring (knob 1)", {F32, dtype})
        recs += _fused_forward(H, c, fam, mode, SEGMENT, "wave-segment (knob 2)", {F32, dtype})
        order, x, xdbl, _, par = smc._device(H, c, _dev())
        ys = H.ss2d_scan_cl(x, xdbl, order, *par, F32, segmented=False)
        _sync(H)
        want = smc.reference(c)["ys"]
        recs.append(_rec("ss2d_scan_cl", f"{fam} no workspace (knob 0: ring) {mode}", dtype, "softplus", ys, want, _kd(c.xs, c, want.shape),
                         "softplus_med3", F32))
    _hold(recs)


@pytest.mark.parametrize("mode", ["bias", "mfma"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_fused_scan_softplus_lds_dma(fam, dtype, mode):
    """The chained form on LDS-DMA staged operands (knob 3), which at padded rank 8 feeds bias * log2e to the dt_proj MFMA as a
    bf16 (hi, lo) pair: the probe above on a 32 x 32 map, the smallest square one on which the library honours the knob (16-bit
    map, L = 1024 = 2 super-chunks of 16 tiles, 4 / 8 sequences of 16 waves; asserted through ss2d_dma_runs, which restates
    `dma_ok`).  dt_bias is conditioned as scan_memory_cases does (the pair holds bias * log2e to an fp32 ulp), so the arguments
    are the sweep values to 2^-15."""
    H = hip()
    kd = (4 if fam == "raster" else 8) * pc.SS2D_D
    assert pc.ss2d_dma_runs(pc.SS2D_H_DMA ** 2, pc.SS2D_D, pc.SS2D_R, kd // pc.SS2D_D, dtype)
    recs = []
    for values in pc.ss2d_values(mode, kd):
        c = pc.ss2d_probe(fam, dtype, mode, values, form_dma=True, h=pc.SS2D_H_DMA)
        recs += _fused_forward(H, c, fam, mode, LDS_DMA, "LDS-DMA (knob 3) 32x32", (F32, dtype))
    _hold(recs)


@pytest.mark.parametrize("mode", ["bias", "mfma"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_fused_scan_backward_softplus_derivative(fam, dtype, mode):
    """ss2d_scan_bwd_cl on the probe above, the incoming gradient one-hot where x is: graw[k, p_kc, c] and the dt_bias gradient
    hold softplus'(x_kc) = 1 - exp2(-t) (times the visits ahead), gu / gB / gC hold softplus(x_kc), gD = the visits, gA = sums of
    products of two softplus values.  With the states the forward saved and with the sweep that recomputes them; all seven
    against the fp64 oracle, each within 8 x E32."""
    import scan_memory_cases as smc
    H = hip()
    dev = _dev()
    kd = (4 if fam == "raster" else 8) * pc.SS2D_D
    recs = []
    for values in pc.ss2d_values(mode, kd):
        c = pc.ss2d_probe(fam, dtype, mode, values)
        want = smc.reference_bwd(c)
        ex = pc.ss2d_expected(c)
        for n in ("graw", "gbias"):
            assert float((want[n] - ex[n]).abs().max()) <= 1e-12 * max(1.0, float(want[n].abs().max()))
        for with_states in (True, False):
            got = smc.run_bwd(H, c, dev, with_states)
            label, var = f"{fam} {mode}", "states" if with_states else "recompute"
            for n, formula, out_dtype in (("gu", "softplus_med3", dtype), ("graw", "dsoftplus_exp2", dtype), ("gB", "softplus_med3", F32),
                                          ("gC", "softplus_med3", F32), ("gA", "softplus_med3", F32), ("gD", "identity", F32),
                                          ("gbias", "dsoftplus_exp2", F32)):
                w = want[n]
                xs = _kd(c.xs, c, w.shape) if w.dim() == 4 or w.shape[-1] == c.d else torch.zeros_like(w)
                recs.append(_rec("ss2d_scan_bwd_cl", label, dtype, n, got[n], w, xs, formula, out_dtype, var))
    _hold(recs)


# ----------------------------------------------------------------------------- attention
def _attn_rec(kernel, form, dtype, function, got, want):
    return _rec(kernel, form, dtype, function, got, want, torch.zeros_like(want), "softmax", dtype)


def _attn_bwd_rec(kernel, form, dtype, function, got, want, amag):
    """the bound of tests/test_gpu_attn_train.py: 3 u A + 1e-6, A the same contraction over magnitudes (dS = P (dP - D) cancels
    under a peaked softmax: no bound relative to |want| can hold for a gradient)"""
    g, w = got.detach().double().cpu(), want.double().cpu()
    bound = 3.0 * pc.U_ROUND[dtype] * amag.double() + 1e-6
    err = (g - w).abs()
    ratio = err / bound
    i = int(ratio.reshape(-1).argmax())
    return dict(kernel=kernel, form=form, dtype=str(dtype)[6:], function=function, worst_x=0.0, error=float(err.reshape(-1)[i]),
                bound=float(bound.reshape(-1)[i]), ok=bool(torch.isfinite(g).all()) and bool((ratio <= 1.0).all()), out_dtype=str(dtype)[6:], variant="")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shift", [0, 6])
def test_window_attention_on_scores_spanning_hundreds(shift, dtype):
    """window_attention_cl and its backward at the Swin block of attn_blocks.py (24 x 24, 4 heads of 32, window 12), batch 1: q
    and k chosen so that the scaled scores of the fp64 reference span -724 .. +724 (asserted: beyond +-300): rows with ONE
    dominant key, rows whose scores are all equal, and with shift 6 the -100 mask on top (a dominant key of another region stays
    dominant at 624).  exp2 of everything below a row's maximum underflows, P is 0 / 1 exactly, so the forward is held to the
    16-bit rule u |want| + 8 E32(softmax) max(1, |want|) per element; dq / dk / dv to the bound of test_gpu_attn_train.py."""
    H = hip()
    dev = _dev()
    o = pc.window_attn_probe(dtype, shift)
    want, s = pc.window_attn_reference(o)
    lo, hi = pc.score_span(s)
    assert lo <= -pc.ATTN_SPAN and hi >= pc.ATTN_SPAN, (lo, hi)
    qkv, table, dy = o.qkv.to(dev), o.table.to(dev), o.dy.to(dev)
    got = H.window_attention_cl(qkv, table, o.ws, shift, o.heads)
    dqkv, _ = H.window_attention_bwd_cl(qkv, table, dy, o.ws, shift, o.heads)
    _sync(H)
    form = f"ws12 24x24 shift={shift}"
    recs = [_attn_rec("window_attention_cl", form, dtype, "softmax(qk)v", got, want)]
    wg = pc.attn_grads(pc.window_attn_reference, o, ("qkv",))["qkv"]
    amag = pc.window_attn_magnitudes(o)
    c = o.heads * o.hd
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * c, (i + 1) * c)
        recs.append(_attn_bwd_rec("window_attention_bwd_cl", form, dtype, part, dqkv[..., sl], wg[..., sl], amag[..., sl]))
    _hold(recs)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_kv_attention_on_scores_spanning_hundreds(dtype):
    """kv_attention_cl and its backward at the PVT block of attn_blocks.py (576 queries, 144 keys, 2 heads of 64), batch 1:
    scaled scores -512 .. +512 on the fp64 reference (asserted), one dominant key / all scores equal per row"""
    H = hip()
    dev = _dev()
    o = pc.kv_attn_probe(dtype)
    want, s = pc.kv_attn_reference(o)
    lo, hi = pc.score_span(s)
    assert lo <= -pc.ATTN_SPAN and hi >= pc.ATTN_SPAN, (lo, hi)
    q, kv, dy = o.q.to(dev), o.kv.to(dev), o.dy.to(dev)
    got = H.kv_attention_cl(q, kv, o.heads)
    dq, dkv = H.kv_attention_bwd_cl(q, kv, dy, o.heads)
    _sync(H)
    form = "n576 m144 hd64"
    recs = [_attn_rec("kv_attention_cl", form, dtype, "softmax(qk)v", got, want)]
    wg = pc.attn_grads(pc.kv_attn_reference, o, ("q", "kv"))
    aq, akv = pc.kv_attn_magnitudes(o)
    recs.append(_attn_bwd_rec("kv_attention_bwd_cl", form, dtype, "dq", dq, wg["q"], aq))
    recs.append(_attn_bwd_rec("kv_attention_bwd_cl", form, dtype, "dk, dv", dkv, wg["kv"], akv))
    _hold(recs)
