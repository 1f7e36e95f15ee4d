"""Backward kernels across fp16's range: a gradient-magnitude ladder, an overflow level and a poison level per case
(tests/test_fp16_range_host.py, tests/test_gpu_fp16_range.py).

Every backward entry is linear in its upstream gradient dy, so the fp64 reference R satisfies R(2^l dy) = 2^l R(dy)
exactly.  dy0 has a random sign and |dy0| log-uniform over 2^-8 .. 1, rounded to the 16-bit dtype of the case, its largest
element exactly 1; the kernel runs at dy = 2^l dy0 and got 2^-l is held against R(dy0), computed on the same rounded
inputs.  Level l = -6 is the working point of loss-scaled fp16 training (2^-22 per logit times the default scale 2^16): every
element of dy is then still a normal fp16 number (>= 2^-14), l = 0 is where the existing tests run, l = 6 is the upper side.

Per (case, output, level):
  bound      err <= T_unit + 4 e_store(l).  err in the metric of the kernel's existing 16-bit test, T_unit the tolerance
             that test uses at unit scale (imported where it is importable, quoted with its test otherwise), e_store(l) the
             error of the ideal kernel in the same metric: the fp64 reference at that level rounded once to the dtype the
             output is stored in (RNE, with subnormals) and scaled back.  Neither term comes from the code under test.
  overflow   the smallest integer l at which at least 1 % of the reference elements of a 16-bit output reach 2^17 (twice
             fp16's largest number); at most 50 % may.  Every such element must come back non-finite.
  poison     at l = 0 one element of dy is +Inf, in a second run NaN.  The fp64 reference run with NaN there gives the
             dependency set per output (its NaN mask without the products with a convolution's zero padding, never empty:
             Case.poison_masks); every element of it must come back non-finite.

A case knows its inputs, its reference and how to run the entry (`run(H, dy, dev)`, H = tramba_amd.hip); everything else
(ladder, e_store, bounds, overflow level, masks, the emulated ideal kernel and its mutants) is shared below."""
import functools
import types

import torch
import torch.nn.functional as F

import ss2d_dstate_cases as dc
import ss2d_dstate_train_cases as tc
from oracle import ops as oo

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
LEVELS = {F16: (-6, 0, 6), BF16: (-6, 0)}          # bf16 is the control: it has fp32's range, its error must be flat
OVERFLOW_AT = 2.0 ** 17
SHARE = (0.01, 0.50)
MARGIN = 4.0
FP16_MIN_NORMAL = 2.0 ** -14


def dy0(shape, seed, dtype):
    """sign random, |dy0| log-uniform over 2^-8 .. 1, rounded to `dtype`, max |dy0| = 1 exactly -> float64"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(-8.0 * torch.rand(shape, generator=g, dtype=F64))
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    v = (mag * sign).to(dtype).double()
    v.view(-1)[v.numel() // 7] = 1.0
    return v


def rnd(t, dtype):
    """float64 -> rounded once to `dtype` (RNE, subnormals kept, overflow to Inf) -> float64"""
    return t.to(dtype).double()


# ----------------------------------------------------------------------------- metrics of the existing tests
def metric_err(metric, got, want, o=None):
    """the smallest tolerance at which the existing test's comparison would pass:
    uA             max (|got - want| - 1e-6) / (u A), A = o.amag elementwise     (the attention backward tests: 3 u A + 1e-6)
    maxrel         max |got - want| / max |want|                             (the scan backward tests)
    allclose       np.testing.assert_allclose(rtol = atol = T)               (LayerNorm dx)
    allclose_max   assert_allclose(rtol = T, atol = T max |want|)            (parameter gradients)
    allclose_max1  assert_allclose(rtol = T, atol = T max(1, max |want|))    (the GELU-gradient GEMM)"""
    got, want = got.double().reshape(want.shape), want.double()
    d = torch.nan_to_num((got - want).abs(), nan=float("inf"))
    top = float(want.abs().max())
    if metric == "uA":
        return float(((d - 1e-6).clamp_min(0.0) / (o.u * o.amag + 1e-300)).max())
    if metric == "maxrel":
        return float(d.max()) / (top + 1e-300)
    if metric == "max_plus1":       # |got - want| <= T max |want| + T (test_ss2d_backward_small_contractions)
        return float(d.max()) / (top + 1.0)
    if metric == "rel_l2":          # tests/test_gpu_grad.py::test_dct_split_backward_against_the_oracle
        return float(torch.nan_to_num((got - want).norm(), nan=float("inf")) / want.norm())
    floor = {"allclose": 1.0, "allclose_max": top, "allclose_max1": max(1.0, top)}[metric]
    return float((d / (floor + want.abs())).max())


Out = types.SimpleNamespace


def out(store, metric, tol):
    """one output of an entry: the dtype it is stored in, the existing test's metric and its 16-bit tolerance"""
    return Out(store=store, metric=metric, tol=tol)


class Case:
    """name, dtype, outputs {name: out(...)}, up_dtype (dy's dtype on the device at the bound and poison levels),
    over_dtype (at the overflow level), dy0 (float64), reference(dy64) -> {name: float64}, run(H, dy, dev) -> {name: tensor}"""
    over_dtype = None
    overflow = True        # False: no dy that fits fp16 drives 1 % of a 16-bit output to 2^17 (the host test proves it per case)
    has_side = False       # a second upstream gradient rides dy's scale (gres, the dB / dC partials): reference(dy, side=False) omits it

    @functools.cached_property
    def ref0(self):
        return self.reference(self.dy0)

    @functools.cached_property
    def poison_at(self):
        """flat index of the poisoned element: near the middle, never the element that holds the maximum"""
        return (self.dy0.numel() // 2 + 3) % self.dy0.numel()

    def poisoned(self, value):
        dy = self.dy0.clone()
        dy.view(-1)[self.poison_at] = value
        return dy

    def poison_ref(self, value):
        """the fp64 reference with dy0's poisoned element set to `value` (cached per value)"""
        cache = self.__dict__.setdefault("_poison_refs", {})
        key = "nan" if value != value else value
        if key not in cache:
            cache[key] = self.reference(self.poisoned(value))
        return cache[key]

    @functools.cached_property
    def poison_masks(self):
        """per output, the elements that depend on the poisoned one: the NaN mask of the fp64 reference run with NaN there,
        less the elements whose coefficient is structurally zero -- the reference multiplies a convolution's zero padding
        into the sum (0 x NaN = NaN), a kernel that never reads the padding owes nothing there.  Those are the elements at
        which the reference's response to a one-hot dy (1 at the poisoned element, 0 elsewhere) is exactly zero."""
        hot = torch.zeros_like(self.dy0)
        hot.view(-1)[self.poison_at] = 1.0
        resp = self.reference(hot, side=False) if self.has_side else self.reference(hot)
        nan = {n: torch.isnan(v) for n, v in self.poison_ref(float("nan")).items()}
        assert all(bool((nan[n] | (resp[n] == 0)).all()) for n in nan), self.name          # support of the response within the NaN mask
        return {n: nan[n] & (resp[n] != 0) for n in nan}

    def dy_device(self, level, dev, poison=None, overflow=False):
        dy = (self.dy0 if poison is None else self.poisoned(poison)) * 2.0 ** level
        dtype = (self.over_dtype or self.up_dtype) if overflow else self.up_dtype
        sent = dy.to(dtype)
        assert torch.equal(torch.nan_to_num(sent.double(), nan=7.0), torch.nan_to_num(dy, nan=7.0)), (self.name, level)
        return sent.to(dev)


def e_store(case, name, level):
    o = case.outputs[name]
    ref = case.ref0[name]
    return metric_err(o.metric, rnd(ref * 2.0 ** level, o.store) * 2.0 ** -level, ref, o)


def bound(case, name, level):
    return case.outputs[name].tol + MARGIN * e_store(case, name, level)


def err_at(case, name, level, got):
    o = case.outputs[name]
    return metric_err(o.metric, got.double().cpu() * 2.0 ** -level, case.ref0[name], o)


def stored16(case):
    return [n for n, o in case.outputs.items() if o.store == F16]


def overflow_level(case):
    """-> (l, {16-bit output: share of elements with |R| 2^l >= 2^17}): the smallest integer l at which some 16-bit output
    has a share of at least 1 %"""
    names = stored16(case)
    assert names, case.name
    for level in range(-8, 60):
        shares = {n: float((case.ref0[n].abs() * 2.0 ** level >= OVERFLOW_AT).double().mean()) for n in names}
        if max(shares.values()) >= SHARE[0]:
            return level, shares
    raise AssertionError(case.name)


def overflow_masks(case, level):
    return {n: case.ref0[n].abs() * 2.0 ** level >= OVERFLOW_AT for n in stored16(case)}


# ----------------------------------------------------------------------------- the ideal kernel and its mutants (CPU)
def ideal(case, level=0, mutant=None, poison=None):
    """the ideal kernel: the fp64 reference of dy0 2^level (linear: R(dy0) 2^level; with `poison`, of the poisoned dy0) rounded
    once to each output's store dtype.  Mutants:
    "intermediate"  every output passes through a 16-bit value 2^-10 below it (x 2^-10, rounded to the 16-bit dtype, x 2^10):
                    what a kernel does that keeps a quantity smaller than its output in the activation dtype; a case that
                    has such a quantity restates it exactly instead (FunctionCase.intermediate: graw);
    "clamp"         16-bit outputs saturate at +-65504 instead of overflowing;
    "nan_to_num"    non-finite values are swallowed (as fmaxf-style clamps and masks do)"""
    ref = case.ref0 if poison is None else case.poison_ref(poison)
    exact = case.intermediate(level) if mutant == "intermediate" and hasattr(case, "intermediate") else None
    res = {}
    for n, o in case.outputs.items():
        v = ref[n] * 2.0 ** level if exact is None else exact[n]
        if mutant == "intermediate" and exact is None:
            v = rnd(v * 2.0 ** -10, case.dtype) * 2.0 ** 10
        if mutant == "clamp" and o.store == F16:
            v = v.clamp(-65504.0, 65504.0)
        v = rnd(v, o.store)
        if mutant == "nan_to_num":
            v = torch.nan_to_num(v, nan=0.0, posinf=65504.0, neginf=-65504.0)
        res[n] = v
    return res


# ----------------------------------------------------------------------------- SS2D scan backward, kernel level
# Two regimes of the same drawn tensors.  "unit": as ss2d_dstate_cases draws them (x ~ N(0, 1), B and C of order 1, dt_bias
# ~ N(-2, 0.5)): every output is of dy's magnitude or above.  "trained": x / 4, the x_proj weight / 16 (B, C and the rank rows of
# order 2^-4 .. 2^-6) and dt_bias - 3 (dt ~ 0.007, inside SS2D's dt_min .. dt_max = 0.001 .. 0.1): graw then lies 2^-13 .. 2^-15
# below gu, its bulk another 2^-5 lower -- the relation DESIGN section 29 measured in a block ("some 2^10 below the other
# activation gradients").  The scalings are powers of two: the rounded tensors stay exact.
REGIMES = {"unit": (1.0, 1.0, 0.0), "trained": (0.25, 0.0625, -3.0)}
SCAN_CFGS = {
    # N = 1: the shapes of tests/test_gpu_kernels.py::test_ss2d_core_training_gradients (b, h, D, R, family, N)
    "scan_n1_raster": ((2, 12, 64, 4, "raster", 1), "unit"),
    "scan_n1_window": ((1, 24, 40, 3, "window", 1), "unit"),
    "scan_n1_raster_trained": ((2, 12, 64, 4, "raster", 1), "trained"),
    # N > 1: cases of ss2d_dstate_train_cases
    "scan_single_launch": (tc.CORE_CASES["single_launch"], "unit"),
    "scan_segments_k8": (tc.CORE_CASES["segments_k8"], "unit"),
    "scan_ragged_r1": (tc.CORE_CASES["ragged_r1"], "unit"),
    "scan_segments_k8_trained": (tc.CORE_CASES["segments_k8"], "trained"),
}


def _core(cfg, regime, dtype):
    """(core case, scan case) of ss2d_dstate_cases in a regime"""
    cc0 = dc.core_case(cfg, dtype)
    sx, sw, db = REGIMES[regime]
    cc = types.SimpleNamespace(**vars(cc0))
    cc.x, cc.wx, cc.dtb = cc0.x * sx, cc0.wx * sw, cc0.dtb + db
    assert cc.x.dtype == cc.wx.dtype == dtype
    return cc, dc.core_as_scan_case(cc)


class ScanCase(Case):
    """hip.ss2d_scan_bwd_cl in the activation dtype: gu, graw stored in it; dB, dC, dA_logs, dD, dbias in fp32.  N = 1 as
    _SS2DCoreCL calls it (the forward launch saves the tile-entry states), N > 1 as _SS2DInnerCL does (bc_partials).  gym may
    arrive in fp32 or in the activation dtype; the bound and poison levels use the activation dtype, the overflow level
    fp32 (gu is of dy's magnitude, so 2^17 needs a dy beyond fp16).  Metric and tolerances: ss2d_dstate_train_cases.BASE_TOL."""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        self.cfg, self.regime = SCAN_CFGS[name]
        self.cc, self.c = _core(self.cfg, self.regime, dtype)
        c = self.c
        self.dy0 = dy0((c.b, c.l, c.d), 4000 + c.l + c.d + c.n, dtype)
        self.up_dtype, self.over_dtype = dtype, F32
        self.outputs = {n: out(dtype if n in ("gu", "graw") else F32, "maxrel", tc.base_tol(n, dtype)) for n in tc.OUTPUTS}

    def reference(self, dy):
        return tc.reference(self.c, dy)

    def leaves(self, res):
        """kernel-level gradients -> the leaves' (the linear maps around the kernel), for the host check against autograd"""
        return tc.compose(self.c, self.cc.wx, res)

    def oracle_leaves(self, dy):
        cc = self.cc
        lv = dict(x=cc.x.double(), wx=cc.wx.double(), dt_w=cc.wdt.double(), dt_b=cc.dtb.double(), a_logs=cc.a_logs.double(),
                  ds=cc.ds.double())
        lv = {k: v.clone().requires_grad_() for k, v in lv.items()}
        ys = oo.ss2d_core(lv["x"], lv["wx"], lv["dt_w"], lv["dt_b"], lv["a_logs"], lv["ds"], cc.fam, merge=False)
        y = oo.cross_merge(ys.permute(0, 1, 3, 2), cc.fam, cc.h, cc.h).permute(0, 2, 1)
        (y * dy).sum().backward()
        g = {k: v.grad for k, v in lv.items()}
        g["x"] = g["x"].permute(0, 2, 3, 1).reshape(cc.b, cc.l, cc.d)
        return g

    def run(self, H, dy, dev):
        c = self.c
        if c.n > 1:
            return tc.run_bwd(H, c, dy, dev)[0]
        x, xdbl, order, dt_w, dt_b, A, ds = dc.device_args(H, c, dev)
        a1 = A.reshape(-1)
        states = H.ss2d_scan_states(x, order)
        H.ss2d_scan_cl(x, xdbl, order, dt_w, dt_b, a1, ds, x.dtype, states=states)
        gu, graw, gb, gc, gpar = H.ss2d_scan_bwd_cl(x, xdbl, order, dt_w, dt_b, a1, ds, dy, states=states)
        gp = gpar.double().sum(0).cpu()                                            # (3, K, D): dA, dD, dbias
        return dict(gu=gu, graw=graw, gB=gb[:, :, None], gC=gc[:, :, None], gA=gp[0].reshape(-1, 1) * c.A.double(),
                    gD=gp[1].reshape(-1), gbias=gp[2].reshape(-1))


# ----------------------------------------------------------------------------- SS2D Functions (where fp16 is routed)
# (segments_k8 is not among them: each of its dt_w elements sums 8 x 576 graw terms and the fp16 rounding of graw averages out to
# 4e-2, under the bound -- it would not notice the 16-bit graw; ragged_r1 is the several-segment case here)
FN_CFGS = {"fn_core_raster": SCAN_CFGS["scan_n1_raster_trained"], "fn_inner_n_ragged_r1": (tc.CORE_CASES["ragged_r1"], "trained"),
           "fn_inner_n_single_launch": (tc.CORE_CASES["single_launch"], "trained")}


class FunctionCase(Case):
    """modules._SS2DCoreCL (N = 1) and modules._SS2DInnerCL (N > 1) under autograd: the gradient of dt_projs_weight is an fp32
    output computed from graw, which the kernels store in the activation dtype -- the 16-bit intermediate of DESIGN section 29.
    For fp16 the Functions therefore take the scan backward's fp32 form; each of these cases fails on dt_w at 2^-6 when they do
    not (the host test shows it on the exact restatement of the 16-bit graw: 4.2e-1, 2.0e-1, 3.5e-1 against 5e-2).
    Outputs: the leaves the scan backward feeds without another GEMM in between -- dt_w (from graw), dt_b, A, Ds (slab sums)
    -- max-relative, BASE_TOL as tests/test_gpu_kernels.py::test_ss2d_core_training_gradients holds them."""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        self.cfg, self.regime = FN_CFGS[name]
        self.cc, self.c = _core(self.cfg, self.regime, dtype)
        c = self.c
        self.dy0 = dy0((c.b, c.l, c.d), 5000 + c.l + c.d + c.n, dtype)
        self.up_dtype = dtype
        self.outputs = {n: out(F32, "maxrel", tc.base_tol(n, dtype)) for n in ("dt_w", "dt_b", "a", "ds")}

    def reference(self, dy, graw_dtype=None):
        res = tc.reference(self.c, dy)
        if graw_dtype is not None:
            res["graw"] = rnd(res["graw"], graw_dtype)
        lv = tc.compose(self.c, self.cc.wx, res)
        a = lv["a_logs"] if self.c.n > 1 else (lv["a_logs"] / self.c.A.double()).reshape(-1)       # N = 1: the leaf is A itself
        return dict(dt_w=lv["dt_w"], dt_b=lv["dt_b"], a=a, ds=lv["ds"])

    def intermediate(self, level):
        """the "intermediate" mutant, exactly: graw rounded to the activation dtype at that level, as the kernels store it"""
        return self.reference(self.dy0 * 2.0 ** level, graw_dtype=self.dtype)

    def run(self, H, dy, dev):
        from tramba_amd import modules as M
        c, cc = self.c, self.cc
        x, xdbl, order, dt_w, dt_b, A, ds = dc.device_args(H, c, dev)
        req = lambda t: t.detach().clone().requires_grad_()
        dtw, dtb, dsl = req(dt_w), req(dt_b), req(ds)
        if c.n == 1:
            a = req(A.reshape(-1))
            ym = M._SS2DCoreCL.apply(x, xdbl, dtw, dtb, a, dsl, order)
        else:
            a = req(cc.a_logs.to(dev))
            xw = cc.wx.float().to(dev)
            # z is unused without its gradient; xs = x: the Function's x_proj GEMM then reproduces the case's x_dbl rows
            ym = M._SS2DInnerCL.apply(x, x, xw, dtw, dtb.view(c.k, c.d), a, dsl, order)
        ym.backward(dy)
        return dict(dt_w=dtw.grad, dt_b=dtb.grad.reshape(c.k, c.d), a=a.grad, ds=dsl.grad)


# ----------------------------------------------------------------------------- norm family
def _ln_inputs(shape_x, c, seed, dtype):
    """x with a small spread (sigma 2^-3 around 0.3): rstd ~ 8, so that dx reaches 2^17 while dy still fits fp16"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape_x, generator=g) * 0.125 + 0.3).to(dtype)
    w, b = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    return x, w, b


LN_TOL = 3e-2     # tests/test_gpu_kernels.py::test_layernorm_training_path_matches_autograd and
                  # tests/test_gpu_stochastic_depth.py::test_layernorm_bwd_res_masked_against_fp64, 16-bit
LN_SHAPES = {"77x512": (77, 512), "50x40": (50, 40), "33x1024": (33, 1024)}     # rows, generic (C % 8 != 0 rows of 80 B) and wide forms


class LayerNormCase(Case):
    """hip.layernorm_bwd_cl and hip.layernorm_bwd_res_cl (with the skip connection's gradient gres, a second upstream
    gradient: scaled with dy): dx in the activation dtype, dw / db fp32 slab sums"""

    def __init__(self, name, dtype):
        entry, shape = name.split(":")
        self.name, self.dtype, self.entry = name, dtype, entry
        rows, c = LN_SHAPES[shape]
        self.x, self.w, self.b = _ln_inputs((rows, c), c, rows + c, dtype)
        self.dy0 = dy0((rows, c), 6000 + rows + c, dtype)
        self.gres0 = dy0((rows, c), 6500 + rows + c, dtype) if entry == "ln_res" else None
        self.has_side = self.gres0 is not None
        self.up_dtype = dtype
        self.outputs = dict(dx=out(dtype, "allclose", LN_TOL), dw=out(F32, "allclose_max", LN_TOL), db=out(F32, "allclose_max", LN_TOL))

    def _scale_of(self, dy):
        """the power of two by which this dy is the ladder's dy0 (gres rides the same scale); 1 for a poisoned dy"""
        top = float(torch.nan_to_num(dy, nan=0.0, posinf=0.0, neginf=0.0).abs().max())
        return top if top > 0 else 1.0

    def reference(self, dy, side=True):
        c = self.x.shape[-1]
        xr = self.x.double().requires_grad_()
        wr, br = self.w.double().requires_grad_(), self.b.double().requires_grad_()
        F.layer_norm(xr, (c,), wr, br, 1e-5).backward(dy)
        dx = xr.grad if self.gres0 is None or not side else xr.grad + self.gres0 * self._scale_of(dy)
        return dict(dx=dx, dw=wr.grad, db=br.grad)

    def run(self, H, dy, dev):
        x, w = self.x.to(dev), self.w.to(dev)
        if self.entry == "ln":
            dx, dw, db = H.layernorm_bwd_cl(x, dy, w)
        else:
            gres = (self.gres0 * self._scale_of(dy.double().cpu())).to(dy.dtype).to(dev)
            dx, _, dw, db = H.layernorm_bwd_res_cl(x, dy, w, 1e-5, gres=gres)
        return dict(dx=dx, dw=dw, db=db)


class ShuffleNormCase(Case):
    """hip.shuffle_norm_bwd_cl at (B, H, C, P) = (1, 5, 16, 4) (tests/test_gpu_kernels.py::test_shuffle_norm_cl's odd case);
    tolerances of tests/test_gpu_stochastic_depth.py::test_shuffle_norm_bwd_against_fp64"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        b, h, c, p = 1, 5, 16, 4
        self.p = p
        self.x, self.w, self.b = _ln_inputs((b, h, h, p * p * c), c, 31, dtype)
        self.dy0 = dy0((b, h * p, h * p, c), 6100, dtype)
        self.up_dtype = dtype
        self.outputs = dict(dx=out(dtype, "allclose", LN_TOL), dw=out(F32, "allclose_max", LN_TOL), db=out(F32, "allclose_max", LN_TOL))

    def reference(self, dy):
        xr = self.x.double().permute(0, 3, 1, 2).requires_grad_()
        wr, br = self.w.double().requires_grad_(), self.b.double().requires_grad_()
        oo.layernorm2d(oo.pixel_shuffle_groups(xr, self.p), wr, br).backward(dy.permute(0, 3, 1, 2))
        return dict(dx=xr.grad.permute(0, 2, 3, 1), dw=wr.grad, db=br.grad)

    def run(self, H, dy, dev):
        dx, dw, db = H.shuffle_norm_bwd_cl(self.x.to(dev), dy, self.w.to(dev), self.p)
        return dict(dx=dx, dw=dw, db=db)


class ShuffleNormHeadCase(Case):
    """hip.shuffle_norm_head_bwd_cl at (B, H, C, P) = (1, 5, 64, 2) (test_shuffle_norm_head_cl's odd case): the logit gradient
    arrives in fp32, dx leaves in the activation dtype, the row sums A_c = sum g xhat_c and G = sum g in fp32.  There is no
    16-bit kernel-level test of this entry; the LayerNorm backward's figures are used"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        b, h, c, p = 1, 5, 64, 2
        self.p, self.c = p, c
        self.x, self.w, self.b = _ln_inputs((b, h, h, p * p * c), c, 37, dtype)
        self.hw = torch.randn(c, generator=torch.Generator().manual_seed(38)) * 0.5
        self.dy0 = dy0((b, h * p, h * p), 6200, dtype)
        self.up_dtype = F32
        self.outputs = dict(dx=out(dtype, "allclose", LN_TOL), A=out(F32, "allclose_max", LN_TOL), G=out(F32, "allclose_max", LN_TOL))

    def reference(self, dy):
        xr = self.x.double().permute(0, 3, 1, 2).requires_grad_()
        xs = oo.pixel_shuffle_groups(xr, self.p)                                       # (B, C, HP, WP)
        mu, var = xs.mean(1, keepdim=True), xs.var(1, unbiased=False, keepdim=True)
        xhat = (xs - mu) / torch.sqrt(var + 1e-5)
        hw, w = self.hw.double(), self.w.double()
        logits = (xhat * (w * hw).view(1, -1, 1, 1)).sum(1)                            # the bias terms carry no x
        logits.backward(dy)
        a = (dy[:, None] * xhat.detach()).sum((0, 2, 3))
        return dict(dx=xr.grad.permute(0, 2, 3, 1), A=a, G=dy.sum().reshape(1))

    def run(self, H, dy, dev):
        dx, part = H.shuffle_norm_head_bwd_cl(self.x.to(dev), dy, self.w.to(dev), self.hw.to(dev), self.p)
        s = H.slab_sum(part)
        return dict(dx=dx, A=s[:self.c], G=s[self.c].reshape(1))


class RowDotCase(Case):
    """hip.rowdot_bwd_cl at rows x C = (77, 512): gy fp32 per row, gx in the activation dtype, gw / gb fp32.  No kernel-level
    test of this entry exists; the 16-bit figure of the LayerNorm backward is used"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        rows, c = 77, 512
        g = torch.Generator().manual_seed(71)
        self.x = torch.randn(rows, c, generator=g).to(dtype)
        self.w = torch.randn(c, generator=g) * 4.0                                     # |w| up to ~16: gx reaches 2^17 with gy in fp32
        self.dy0 = dy0((rows,), 6300, dtype)
        self.up_dtype = F32
        self.outputs = dict(gx=out(dtype, "allclose", LN_TOL), gw=out(F32, "allclose_max", LN_TOL), gb=out(F32, "allclose_max", LN_TOL))

    def reference(self, dy):
        return dict(gx=dy[:, None] * self.w.double(), gw=(dy[:, None] * self.x.double()).sum(0), gb=dy.sum().reshape(1))

    def run(self, H, dy, dev):
        gx, gw, gb = H.rowdot_bwd_cl(self.x.to(dev), dy, self.w.to(dev))
        return dict(gx=gx, gw=gw, gb=gb.reshape(1))


# ----------------------------------------------------------------------------- the GELU-gradient GEMM
GEMM_SHAPES = {"333x72x136": (333, 72, 136), "100x30x50": (100, 30, 50)}


class GeluGradGemmCase(Case):
    """hip.linear_cl(dy, w, None, h, ACT_GELU_GRAD_MUL) = (dy @ w^T) gelu'(h): the input gradient of Linear(GELU(h)), stored
    in the activation dtype; shapes and tolerance of tests/test_gpu_kernels.py::test_linear_gelu_grad_epilogue (2e-2).  w is
    drawn 8 times larger than there so that the output reaches 2^17 while dy still fits fp16"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        m, n, k = GEMM_SHAPES[name.split(":")[1]]
        g = torch.Generator().manual_seed(m + n)
        self.w = (torch.randn(n, k, generator=g) * 8.0 * k ** -0.5).to(dtype)
        self.h = (torch.randn(m, n, generator=g) * 1.5).to(dtype)
        self.dy0 = dy0((m, k), 7000 + m, dtype)
        self.up_dtype = dtype
        self.outputs = dict(y=out(dtype, "allclose_max1", 2e-2))

    def reference(self, dy):
        hd = self.h.double().requires_grad_()
        (dg,) = torch.autograd.grad(F.gelu(hd).sum(), hd)
        return dict(y=(dy @ self.w.double().t()) * dg)

    def run(self, H, dy, dev):
        return dict(y=H.linear_cl(dy, self.w.to(dev), None, self.h.to(dev), H.ACT_GELU_GRAD_MUL))



# ----------------------------------------------------------------------------- attention backward
U16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}        # tests/test_gpu_attn_train.py: |got - ref| <= 3 u A + 1e-6 per element
ATTN_TOL = 3.0


def _attn_out(dtype, store, amag):
    o = out(store, "uA", ATTN_TOL)
    o.u, o.amag = U16[dtype], amag
    return o


KV_SHAPES = {
    "kv_block_n576_m144": (2, 576, 144, 2, 64),       # the PVT block of attn_train_blocks.py: dim 128, 2 heads, sr 2 on 24 x 24
    "kv_cap_n100_m256": (2, 100, 256, 2, 64),         # the 256-key cap: rounds of 32 queries, the last holds 4
}
V_SCALE = 16.0     # v is drawn 16 times larger than tests/test_gpu_attn.py draws it: dP = dO v^T, and with it dq and dk, then reach
                   # 2^17 while dy still fits fp16 (dv = P^T dO is of dy's magnitude whatever the inputs)


class KvAttnCase(Case):
    """hip.kv_attention_bwd_cl: dq, dk, dv in the activation dtype.  Inputs as tests/test_gpu_attn.py draws them (q at 3 x, k at
    2 x unit scale: a peaked softmax), v at 16 x; metric, A and the bound 3 u A + 1e-6 of tests/test_gpu_attn_train.py"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        b, n, m, heads, hd = KV_SHAPES[name]
        self.heads = heads
        g = torch.Generator().manual_seed(8000 + n + m)
        c = heads * hd
        self.q = (torch.randn(b, n, c, generator=g) * 3.0).to(dtype)
        kv = torch.randn(b, m, 2, c, generator=g)
        kv[:, :, 0] *= 2.0
        kv[:, :, 1] *= V_SCALE
        self.kv = kv.view(b, m, 2 * c).to(dtype)
        self.dy0 = dy0((b, n, c), 8100 + n + m, dtype)
        self.up_dtype = dtype
        aq, ak, av = self._magnitudes(self.dy0)
        self.outputs = dict(dq=_attn_out(dtype, dtype, aq), dk=_attn_out(dtype, dtype, ak), dv=_attn_out(dtype, dtype, av))

    def _split(self):
        b, n, c = self.q.shape
        m, hd = self.kv.shape[1], c // self.heads
        return b, n, m, c, hd

    def reference(self, dy):
        b, n, m, c, hd = self._split()
        q, kv = self.q.double().requires_grad_(), self.kv.double().requires_grad_()
        qd = q.view(b, n, self.heads, hd).transpose(1, 2)
        k, v = kv.view(b, m, 2, self.heads, hd).permute(2, 0, 3, 1, 4)
        o = torch.softmax((qd @ k.transpose(-1, -2)) * hd ** -0.5, -1) @ v
        o.transpose(1, 2).reshape(b, n, c).backward(dy)
        return dict(dq=q.grad, dk=kv.grad[..., :c].clone(), dv=kv.grad[..., c:].clone())

    def _magnitudes(self, dy):
        b, n, m, c, hd = self._split()
        qd = self.q.double().view(b, n, self.heads, hd).transpose(1, 2)
        do = dy.view(b, n, self.heads, hd).transpose(1, 2)
        k, v = self.kv.double().view(b, m, 2, self.heads, hd).permute(2, 0, 3, 1, 4)
        p = torch.softmax((qd @ k.transpose(-1, -2)) * hd ** -0.5, -1)
        dpa = (do @ v.transpose(-1, -2)).abs()
        dsb = p * (dpa + (p * dpa).sum(-1, keepdim=True))
        aq = ((dsb @ k.abs()) * hd ** -0.5).transpose(1, 2).reshape(b, n, c)
        ak = ((dsb.transpose(-1, -2) @ qd.abs()) * hd ** -0.5).transpose(1, 2).reshape(b, m, c)
        av = (p.transpose(-1, -2) @ do.abs()).transpose(1, 2).reshape(b, m, c)
        return aq, ak, av

    def run(self, H, dy, dev):
        c = self.q.shape[-1]
        dq, dkv = H.kv_attention_bwd_cl(self.q.to(dev), self.kv.to(dev), dy, self.heads)
        return dict(dq=dq, dk=dkv[..., :c], dv=dkv[..., c:])


class WindowAttnCase(Case):
    """hip.window_attention_bwd_cl on the Swin block of attn_train_blocks.py (dim 128, 24 x 24, 4 heads, window 12, shift 6:
    all nine mask regions): dq, dk, dv in the activation dtype, the relative-position table's gradient in fp32 -- an fp32
    output computed from dS, which the kernel feeds to the matrix cores as a (hi, lo) pair in the activation dtype"""

    def __init__(self, name, dtype):
        from tramba_amd.encoders import SwinTransformerBlock
        self.name, self.dtype = name, dtype
        b, h, w, heads, hd, ws, shift = 2, 24, 24, 4, 32, 12, 6
        self.geo = (b, h, w, heads, hd, ws, shift)
        blk = SwinTransformerBlock(heads * hd, (h, w), heads, ws, shift, 1.0, 0.0)
        self.index, self.mask = blk.attn.relative_position_index, blk.attn_mask.double()
        g = torch.Generator().manual_seed(8200)
        c = heads * hd
        qkv = torch.randn(b, h, w, 3, c, generator=g)
        qkv[:, :, :, 0] *= 3.0
        qkv[:, :, :, 1] *= 2.0
        qkv[:, :, :, 2] *= V_SCALE
        self.qkv = qkv.view(b, h, w, 3 * c).to(dtype)
        self.table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.5
        self.dy0 = dy0((b, h, w, c), 8300, dtype)
        self.up_dtype = dtype
        a, at = self._magnitudes(self.dy0)
        self.outputs = dict(dq=_attn_out(dtype, dtype, a[..., :c]), dk=_attn_out(dtype, dtype, a[..., c:2 * c]),
                            dv=_attn_out(dtype, dtype, a[..., 2 * c:]), dtable=_attn_out(dtype, F32, at))

    def _scores(self, x, table):
        from tramba_amd.encoders import _windows
        b, h, w, heads, hd, ws, shift = self.geo
        n = ws * ws
        xw = _windows(torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)), ws)
        nw = xw.shape[1]
        q, k, v = xw.view(b, nw, n, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)             # (B, nW, nH, N, hd)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        s = s + table[self.index.view(-1)].view(n, n, heads).permute(2, 0, 1)[None, None] + self.mask[None, :, None]
        return q, k, v, torch.softmax(s, -1), nw

    def _win(self, t):
        from tramba_amd.encoders import _windows
        return _windows(torch.roll(t, shifts=(-self.geo[6],) * 2, dims=(1, 2)), self.geo[5])

    def _back(self, t):
        from tramba_amd.encoders import _unwindows
        b, h, w, heads, hd, ws, shift = self.geo
        return torch.roll(_unwindows(t, ws, h, w), shifts=(shift, shift), dims=(1, 2))

    def reference(self, dy):
        b, h, w, heads, hd, ws, shift = self.geo
        c, n = heads * hd, ws * ws
        x, t = self.qkv.double().requires_grad_(), self.table.double().requires_grad_()
        q, k, v, p, nw = self._scores(x, t)
        o = self._back((p @ v).transpose(2, 3).reshape(b, nw, n, c))
        o.backward(dy)
        return dict(dq=x.grad[..., :c].clone(), dk=x.grad[..., c:2 * c].clone(), dv=x.grad[..., 2 * c:].clone(), dtable=t.grad)

    def _magnitudes(self, dy):
        b, h, w, heads, hd, ws, shift = self.geo
        c, n = heads * hd, ws * ws
        q, k, v, p, nw = self._scores(self.qkv.double(), self.table.double())
        do = self._win(dy).view(b, nw, n, heads, hd).permute(0, 1, 3, 2, 4)
        dpa = (do @ v.transpose(-1, -2)).abs()
        dsb = p * (dpa + (p * dpa).sum(-1, keepdim=True))
        av = p.transpose(-1, -2) @ do.abs()
        aq = (dsb @ k.abs()) * hd ** -0.5
        ak = (dsb.transpose(-1, -2) @ q.abs()) * hd ** -0.5
        a = self._back(torch.stack([aq, ak, av]).permute(1, 2, 4, 0, 3, 5).reshape(b, nw, n, 3 * c))
        at = torch.zeros((2 * ws - 1) ** 2, heads, dtype=F64)
        at.index_add_(0, self.index.view(-1), dsb.sum((0, 1)).permute(1, 2, 0).reshape(n * n, heads))
        return a, at

    def run(self, H, dy, dev):
        b, h, w, heads, hd, ws, shift = self.geo
        c = heads * hd
        dqkv, dtable = H.window_attention_bwd_cl(self.qkv.to(dev), self.table.to(dev), dy, ws, shift, heads)
        return dict(dq=dqkv[..., :c], dk=dqkv[..., c:2 * c], dv=dqkv[..., 2 * c:], dtable=dtable)



# ----------------------------------------------------------------------------- depth-wise training pair
DW_SHAPES = {"2x9x32_k5": (2, 9, 32, 5), "1x24x130_k7": (1, 24, 130, 7)}       # tests/test_gpu_kernels.py::test_dwconv_training_path_...


class DwConvCase(Case):
    """modules._DwConvActCL (SS2D's depth-wise conv + SiLU on the training path) differentiated through z: the input gradient
    (the stencil with mirrored taps, activation dtype) and the weight / bias gradients (fp32 partial sums); the SiLU's own
    gradient belongs to the consumer.  Tolerances of test_dwconv_training_path_matches_autograd (3e-2).  The taps are drawn 8 x
    a unit-gain stencil so that the input gradient reaches 2^17 while dy still fits fp16"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        b, h, c, ks = DW_SHAPES[name.split(":")[1]]
        g = torch.Generator().manual_seed(h * c + ks)
        self.x = torch.randn(b, h, h, c, generator=g).to(dtype)
        self.w = torch.randn(c, 1, ks, ks, generator=g) * (8.0 / ks)
        self.b = 0.1 * torch.randn(c, generator=g)
        self.ks = ks
        self.dy0 = dy0((b, h, h, c), 9000 + h * c, dtype)
        self.up_dtype = dtype
        self.outputs = dict(gx=out(dtype, "allclose", 3e-2), gw=out(F32, "allclose_max", 3e-2), gb=out(F32, "allclose_max", 3e-2))

    def reference(self, dy):
        x = self.x.double().permute(0, 3, 1, 2).requires_grad_()
        w, b = self.w.double().requires_grad_(), self.b.double().requires_grad_()
        F.conv2d(x, w, b, padding=self.ks // 2, groups=x.shape[1]).backward(dy.permute(0, 3, 1, 2))
        return dict(gx=x.grad.permute(0, 2, 3, 1), gw=w.grad, gb=b.grad)

    def run(self, H, dy, dev):
        from tramba_amd import modules as M
        x = self.x.to(dev).requires_grad_()
        w, b = self.w.to(dev).requires_grad_(), self.b.to(dev).requires_grad_()
        z, _ = M._DwConvActCL.apply(x, w, b, H.ACT_SILU)
        z.backward(dy)
        return dict(gx=x.grad, gw=w.grad, gb=b.grad)


# ----------------------------------------------------------------------------- the tail of the SS2D backward
TAIL_CFGS = {"tail_n1_raster": (2, 12, 64, 4, "raster", 1), "tail_segments_k8": tc.CORE_CASES["segments_k8"]}


class TailCase(Case):
    """ss2d_bwd_prep -> rows_gemm_cl -> ss2d_bwd_assemble as one chain, as the 16-bit route of _SS2DInnerCL (N = 1 and N > 1)
    runs it: graw (activation dtype) is the upstream gradient, the dB / dC per-channel-tile partials (fp32) ride the same
    scale; the output is g_xd, the x_dbl-row gradients in spatial order, stored in the activation dtype.  Max-relative, the
    5e-2 at which test_ss2d_core_training_gradients holds the x_dbl gradient.  dt_w is drawn 8 x larger than the scan cases
    draw it so that the rank columns reach 2^17 while graw still fits fp16"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        b, h, d, r, fam, n = TAIL_CFGS[name]
        k, l = dc.k_of(fam), h * h
        self.geo = (b, h, d, r, fam, n, k, l)
        self.rg, self.r8, self.ct = dc.group_stride(r, n), dc.rank_pad(r), (d + 31) // 32
        self.table = dc.table_of(fam, h)
        g = torch.Generator().manual_seed(9500 + l + d + n)
        self.xdbl = torch.randn(b, l, k * self.rg, generator=g)
        self.dt_w = (torch.randn(k, d, r, generator=g) * 8.0 * r ** -0.5).to(dtype)
        self.dy0 = dy0((b, k, l, d), 9600 + l + d + n, dtype)
        self.part0 = [dy0((b, k, self.ct, n, l), 9700 + i + l + n, dtype) for i in range(2)]
        self.up_dtype = dtype
        self.outputs = dict(g_xd=out(dtype, "maxrel", tc.base_tol("gB", dtype)))

    def _scale_of(self, dy):
        top = float(torch.nan_to_num(dy, nan=0.0, posinf=0.0, neginf=0.0).abs().max())
        return top if top > 0 else 1.0

    has_side = True

    def reference(self, dy, side=True):
        b, h, d, r, fam, n, k, l = self.geo
        rg, r8 = self.rg, self.r8
        s = self._scale_of(dy) if side else 0.0
        gxd = torch.zeros(b, l, k, rg, dtype=F64)
        for i in range(b):
            for j in range(k):
                gs = torch.zeros(l, rg, dtype=F64)
                gs[:, :r] = dy[i, j] @ self.dt_w[j].double()
                gs[:, r8:r8 + n] = (self.part0[0][i, j].sum(0) * s).t()
                gs[:, r8 + n:r8 + 2 * n] = (self.part0[1][i, j].sum(0) * s).t()
                gxd[i, :, j].index_add_(0, self.table[j], gs)
        return dict(g_xd=gxd.view(b, l, k * rg))

    def run(self, H, dy, dev):
        b, h, d, r, fam, n, k, l = self.geo
        order = H.scan_order(fam, h, h, dev)
        assert torch.equal(order.table.cpu().long(), self.table)
        s = self._scale_of(dy.double().cpu())
        shape = (b, k, self.ct, l) if n == 1 else (b, k, self.ct, n, l)
        bpart, cpart = ((p * s).float().reshape(shape).contiguous().to(dev) for p in self.part0)
        ranks, gseq = H.ss2d_bwd_prep(self.xdbl.to(dev), order, bpart, cpart, r, self.dtype, n)
        dtw_t = self.dt_w.to(dev).transpose(1, 2).contiguous()                       # (K, R, D), activation dtype
        H.rows_gemm_cl(dy.view(b * k, l, d), dtw_t, gseq.view(b * k, l, self.rg), r)
        return dict(g_xd=H.ss2d_bwd_assemble(gseq, order, r, self.dtype, n))



class TailEntryCase(TailCase):
    """the three entries of the chain one by one, on TailCase's geometry and operands:
    prep      ss2d_bwd_prep: the dB / dC per-channel-tile partials (fp32, dy = the dB partials, the dC ones ride its scale)
              summed into columns R8 .. of g_seq (fp32); the existing test holds this sum bit for bit, the chain's 5e-2 is used
    rows      rows_gemm_cl: graw (activation dtype) @ dt_w into the first R fp32 columns; |err| <= 1e-5 max + 1e-5 as
              tests/test_gpu_kernels.py::test_ss2d_backward_small_contractions holds it
    assemble  ss2d_bwd_assemble: g_seq (fp32, = dy) through the inverse table into g_xd in the activation dtype; the padding
              columns of g_seq hold dy like the rest and must not reach the output"""

    def __init__(self, name, dtype):
        self.entry, cfg = name.split(":")
        super().__init__(cfg, dtype)
        self.name = name
        b, h, d, r, fam, n, k, l = self.geo
        if self.entry == "prep":
            self.dy0, self.up_dtype = self.part0[0], F32
            self.outputs = dict(bc=out(F32, "maxrel", tc.base_tol("gB", dtype)))
        elif self.entry == "rows":
            self.has_side = False
            self.outputs = dict(rows=out(F32, "max_plus1", 1e-5))
        else:
            self.has_side = False
            self.dy0, self.up_dtype = dy0((b, k, l, self.rg), 9800 + l + n, dtype), F32
            self.outputs = dict(g_xd=out(dtype, "maxrel", tc.base_tol("gB", dtype)))

    def reference(self, dy, side=True):
        b, h, d, r, fam, n, k, l = self.geo
        if self.entry == "prep":
            s = self._scale_of(dy) if side else 0.0
            return dict(bc=torch.cat([dy.sum(2), self.part0[1].sum(2) * s], 2).transpose(2, 3))     # (B, K, L, 2N)
        if self.entry == "rows":
            return dict(rows=torch.einsum("bkld,kdr->bklr", dy, self.dt_w.double()).reshape(b * k, l, r))
        gxd = torch.zeros(b, l, k, self.rg, dtype=F64)
        live = torch.zeros(self.rg, dtype=F64)              # the kernel's contract: the rank padding R .. R8 - 1 and the columns past
        live[:r] = 1.0                                      # R8 + 2N leave as zeros, whatever g_seq holds there (dy is non-zero there)
        live[self.r8:self.r8 + 2 * n] = 1.0
        for i in range(b):
            for j in range(k):
                gxd[i, :, j].index_add_(0, self.table[j], dy[i, j] * live)
        return dict(g_xd=gxd.view(b, l, k * self.rg))

    def run(self, H, dy, dev):
        b, h, d, r, fam, n, k, l = self.geo
        order = H.scan_order(fam, h, h, dev)
        assert torch.equal(order.table.cpu().long(), self.table)
        if self.entry == "prep":
            s = self._scale_of(dy.double().cpu())
            shape = (b, k, self.ct, l) if n == 1 else (b, k, self.ct, n, l)
            cpart = (self.part0[1] * s).float().reshape(shape).contiguous().to(dev)
            _, gseq = H.ss2d_bwd_prep(self.xdbl.to(dev), order, dy.reshape(shape).contiguous(), cpart, r, self.dtype, n)
            return dict(bc=gseq[..., self.r8:self.r8 + 2 * n])
        if self.entry == "rows":
            y = torch.zeros((b * k, l, self.rg), dtype=F32, device=dev)
            H.rows_gemm_cl(dy.view(b * k, l, d), self.dt_w.to(dev).transpose(1, 2).contiguous(), y, r)
            return dict(rows=y[..., :r])
        return dict(g_xd=H.ss2d_bwd_assemble(dy.contiguous(), order, r, self.dtype, n))


MERGE_CFGS = {"merge_grad_raster": ("raster", 12, 64, 2), "merge_grad_helix": ("helix", 12, 32, 1)}


class MergeGradCase(Case):
    """hip.ss2d_merge_grad_cl: gz = (merge(gu) + t) silu'(z), stored in the activation dtype -- the last launch of the SS2D
    Functions' backward.  gu (B, K, L, D) is dy, the x_proj branch's share t (B, L, D) rides its scale.  Max-relative, the 3e-2
    at which test_ss2d_core_training_gradients holds the input gradient.  Every input is 16-bit, |silu'| <= 1.1 and the merge
    adds K random-sign terms: no dy that fits fp16 takes 1 % of gz to 2^17 (overflow = False; proven in the host test)"""
    overflow, has_side = False, True

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        fam, h, d, b = MERGE_CFGS[name]
        k, l = dc.k_of(fam), h * h
        self.geo, self.table = (fam, h, d, b, k, l), dc.table_of(fam, h)
        g = torch.Generator().manual_seed(9900 + l + d)
        self.z = (torch.randn(b, l, d, generator=g) * 1.5).to(dtype)
        self.dy0 = dy0((b, k, l, d), 9910 + l + d, dtype)
        self.t0 = dy0((b, l, d), 9920 + l + d, dtype)
        self.up_dtype = dtype
        self.outputs = dict(gz=out(dtype, "maxrel", tc.base_tol("gu", dtype)))

    _scale_of = LayerNormCase._scale_of

    def reference(self, dy, side=True):
        fam, h, d, b, k, l = self.geo
        z = self.z.double()
        sg = torch.sigmoid(z)
        m = torch.zeros(b, l, d, dtype=F64)
        for i in range(b):
            for j in range(k):
                m[i].index_add_(0, self.table[j], dy[i, j])
        if side:
            m = m + self.t0 * self._scale_of(dy)
        return dict(gz=m * (sg * (1 + z * (1 - sg))))

    def run(self, H, dy, dev):
        fam, h, d, b, k, l = self.geo
        order = H.scan_order(fam, h, h, dev)
        assert torch.equal(order.table.cpu().long(), self.table)
        t = (self.t0 * self._scale_of(dy.double().cpu())).to(self.dtype).to(dev)
        return dict(gz=H.ss2d_merge_grad_cl(dy, order, t, self.z.to(dev)))


class DctCase(Case):
    """modules._DCTSplitCL's backward at n = 24, C = 32: gX = Wy^T [gLow 0; 0 gHigh] Wx, stored in the activation dtype; dy is the
    low quadrant's gradient, the high quadrant's rides its scale.  Relative L2 and the tolerances of
    tests/test_gpu_grad.py::test_dct_split_backward_against_the_oracle (fp16 2e-3, bf16 8e-3).  The transform is orthonormal: on
    a random-sign dy its gain is one, and no dy that fits fp16 takes 1 % of gX to 2^17 (overflow = False)"""
    overflow, has_side = False, True

    def __init__(self, name, dtype):
        from tramba_amd.modules import _dct_filter
        self.name, self.dtype = name, dtype
        b, n, c = 2, 24, 32
        self.w = _dct_filter(n)
        self.x = torch.randn(b, n, n, c, generator=torch.Generator().manual_seed(9950)).to(dtype)
        self.dy0 = dy0((b, n // 2, n // 2, c), 9951, dtype)
        self.gh0 = dy0((b, n // 2, n // 2, c), 9952, dtype)
        self.up_dtype = dtype
        self.outputs = dict(gx=out(dtype, "rel_l2", {F16: 2e-3, BF16: 8e-3}[dtype]))

    _scale_of = LayerNormCase._scale_of

    def reference(self, dy, side=True):
        x = self.x.double().permute(0, 3, 1, 2).requires_grad_()
        high, low = oo.dct2d_split(x, self.w.double(), self.w.double())
        loss = (low * dy.permute(0, 3, 1, 2)).sum()
        if side:
            loss = loss + (high * (self.gh0 * self._scale_of(dy)).permute(0, 3, 1, 2)).sum()
        loss.backward()
        return dict(gx=x.grad.permute(0, 2, 3, 1))

    def run(self, H, dy, dev):
        from tramba_amd import modules as M
        x = self.x.to(dev).requires_grad_()
        high, low = M._DCTSplitCL.apply(x, self.w.to(dev), self.w.to(dev))
        gh = (self.gh0 * self._scale_of(dy.double().cpu())).to(self.dtype).to(dev)
        torch.autograd.backward([high, low], [gh, dy])
        return dict(gx=x.grad)


# ----------------------------------------------------------------------------- the list
FACTORIES = {}
for _n in SCAN_CFGS:
    FACTORIES[_n] = ScanCase
for _n in FN_CFGS:
    FACTORIES[_n] = FunctionCase
for _s in LN_SHAPES:
    FACTORIES[f"ln:{_s}"] = LayerNormCase
    FACTORIES[f"ln_res:{_s}"] = LayerNormCase
FACTORIES["shuffle_norm"] = ShuffleNormCase
FACTORIES["shuffle_norm_head"] = ShuffleNormHeadCase
FACTORIES["rowdot"] = RowDotCase
for _s in GEMM_SHAPES:
    FACTORIES[f"gelu_grad_gemm:{_s}"] = GeluGradGemmCase
for _n in KV_SHAPES:
    FACTORIES[_n] = KvAttnCase
FACTORIES["window_ws12_24x24_s6"] = WindowAttnCase
for _s in DW_SHAPES:
    FACTORIES[f"dwconv:{_s}"] = DwConvCase
for _n in TAIL_CFGS:
    FACTORIES[_n] = TailCase
for _e in ("prep", "rows", "assemble"):
    for _n in TAIL_CFGS:
        FACTORIES[f"{_e}:{_n}"] = TailEntryCase
for _n in MERGE_CFGS:
    FACTORIES[_n] = MergeGradCase
FACTORIES["dct_split"] = DctCase
NAMES = tuple(FACTORIES)
# the cases with an overflow level: a 16-bit output (the Function cases and the tail's prep / rows entries have none) that a dy
# within fp16 can drive to 2^17 (tests/test_fp16_range_host.py holds this list against the cases themselves)
OVERFLOW_NAMES = [n for n in NAMES if FACTORIES[n].overflow and not n.startswith(("fn_", "prep:", "rows:"))]
PARAMS = [(n, d) for n in NAMES for d in (F16, BF16)]
IDS = [f"{n}-{str(d)[6:]}" for n, d in PARAMS]


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    return FACTORIES[name](name, dtype)
