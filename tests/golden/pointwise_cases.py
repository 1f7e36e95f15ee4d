"""The library's embedded nonlinearities at their tails and switch-over points: one SWEEP of finite fp32 arguments, fp64
references, numpy float32 emulations of the DOCUMENTED formulas (transcribed from the comments of csrc/common.h,
selective_scan.hip softplus_lean, ss2d_fused.hip ScanWave::terms and the fused backward, loss_optim.hip sig_terms) -- which exist
only to size the bounds and to show that the tests have teeth -- and probe builders that make ONE output element equal ONE
function value (tests/test_pointwise_host.py, tests/test_gpu_pointwise.py, scripts/measure_pointwise_parity.py).

Error measure: e = |got - want| / max(1, |want|).  E32_F = max(max over SWEEP of e(emulation_F, fp64), 2^-24).  An fp32 output
of a kernel must stay within FACTOR * E32_F of fp64, a 16-bit one within u |want| + FACTOR * E32_F max(1, |want|) per element."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import selective_scan as oss

F32 = np.float32
FACTOR = 8.0          # hardware exp2 / log2 / rcp are within an ulp but not correctly rounded (scan_memory_cases.FACTOR)
FLOOR = 2.0 ** -24
U_ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LOG2E, LN2 = F32(1.44269504088896), F32(0.693147180559945)
ACT_NONE, ACT_SILU, ACT_GELU, ACT_SIGMOID_GATE, ACT_GELU_GRAD_MUL = 0, 1, 2, 3, 4


# ----------------------------------------------------------------------------- the sweep
def _sweep():
    both = [2.0 ** -30, 1e-6, 1e-3, 0.5, 1, 2, 3, 5, 8, 10, 13.86, 15, 16.6, 17.4, 19.99, 25, 30, 41.6, 60, 87, 88.7, 88.8, 89, 100,
            103.9, 104, 200, 1e4]
    v = [0.0] + [s * a for a in both for s in (1.0, -1.0)]
    v = np.asarray(v, F32)
    v = np.concatenate([v, [F32(20), np.nextafter(F32(20), F32(np.inf)), np.nextafter(F32(60), F32(np.inf))]]).astype(F32)
    rnd = np.random.RandomState(20).uniform(-110.0, 110.0, 256).astype(F32)
    return np.concatenate([v, rnd])


SWEEP = _sweep()
assert SWEEP.dtype == F32 and len(SWEEP) == 316 and bool(np.isfinite(SWEEP).all())


def representable(dtype, values=SWEEP):
    """the subset of `values` that `dtype` holds exactly"""
    t = torch.from_numpy(np.asarray(values, F32))
    r = t.to(dtype).float()
    return t[(r == t) & torch.isfinite(r)].numpy()


SWEEP_BF16, SWEEP_F16 = representable(torch.bfloat16), representable(torch.float16)


def sweep_for(dtype):
    return {torch.float32: SWEEP, torch.bfloat16: SWEEP_BF16, torch.float16: SWEEP_F16}[dtype]


def tiled(values, n):
    """(n) f32 tensor: `values` repeated"""
    v = np.asarray(values, F32)
    return torch.from_numpy(np.resize(v, n).copy())


def split16(values, dtype):
    """values -> (part in `dtype`, fp32 remainder): float(part) + remainder == value exactly in fp32"""
    v = torch.as_tensor(np.asarray(values, F32))
    hi = v.to(dtype)
    lo = v - hi.float()
    assert torch.equal(hi.float() + lo, v)
    return hi, lo


# ----------------------------------------------------------------------------- fp64 references (torch)
def _t64(x):
    return torch.as_tensor(np.asarray(x, np.float64)) if not isinstance(x, torch.Tensor) else x.double()


def ref_softplus(x):
    return F.softplus(_t64(x))                      # threshold 20, as the reference


def ref_dsoftplus(x):
    x = _t64(x)
    return torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))


def ref_sigmoid(x):
    return torch.sigmoid(_t64(x))


def ref_silu(x):
    x = _t64(x)
    return x * torch.sigmoid(x)


def ref_dsilu(x):
    x = _t64(x)
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def ref_gelu(x):
    x = _t64(x)
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))       # erfc: full relative precision in the negative tail


def ref_dgelu(x):
    x = _t64(x)
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ref_bce(z, y):
    z, y = _t64(z), _t64(y)
    return torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))


def ref_dbce(z, y):
    return torch.sigmoid(_t64(z)) - _t64(y)


def ref_identity(x):
    return _t64(x)


def ref_attention(q, k, v, scale, bias=None):
    """softmax(q k^T scale + bias) v in fp64 on (..., n, hd) / (..., m, hd) operands -> (out, probabilities, scores)"""
    s = torch.einsum("...nd,...md->...nm", q.double(), k.double()) * scale
    if bias is not None:
        s = s + bias.double()
    p = torch.softmax(s, -1)
    return p @ v.double(), p, s


def ref_u8(z):
    """(torch.sigmoid(z) * 255).to(torch.uint8) in fp32 on the CPU"""
    z = torch.as_tensor(np.asarray(z, F32)) if not isinstance(z, torch.Tensor) else z.float()
    return (torch.sigmoid(z) * 255).to(torch.uint8)


# ----------------------------------------------------------------------------- fp32 emulations of the documented formulas (numpy)
def _f(x):
    return np.asarray(x, F32)


def _np(fn):
    @functools.wraps(fn)
    def wrapped(*a):
        with np.errstate(all="ignore"):
            out = fn(*[_f(t) for t in a])
        assert out.dtype == F32, fn.__name__
        return out
    return wrapped


@_np
def emu_softplus20(x):
    """common.h softplus20: log1p(exp(min(x, 20))) through w = 1 + z, select x beyond 20"""
    z = np.exp(np.minimum(x, F32(20)))
    w = F32(1) + z
    d = w - F32(1)
    sp = np.where(d == 0, z, np.log(w) * z / np.where(d == 0, F32(1), d))
    return np.where(x > 20, x, sp).astype(F32)


@_np
def emu_softplus_lean(x):
    """selective_scan.hip softplus_lean: max(x, ln2 * log2(1 + exp2(min(x, 60) * log2e)))"""
    z = np.exp2(np.minimum(x, F32(60)) * LOG2E)
    return np.maximum(x, np.log2(F32(1) + z) * LN2)


def _med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


@_np
def emu_t_med3(x):
    """ss2d_fused.hip: x' = x log2e, t = med3(log2(1 + exp2(x')), x', 128) = softplus(x) log2e"""
    x2 = x * LOG2E
    return _med3(np.log2(F32(1) + np.exp2(x2)), x2, F32(128)).astype(F32)


@_np
def emu_softplus_med3(x):
    return emu_t_med3(x) * LN2


@_np
def emu_dsoftplus_sigmoid(x):
    """selective-scan backward: sigmoid(raw) up to 20, 1 beyond"""
    return np.where(x <= 20, F32(1) / (F32(1) + np.exp(-x)), F32(1)).astype(F32)


@_np
def emu_dsoftplus_exp2(x):
    """fused backward: softplus' = 1 - exp(-dt) = 1 - exp2(-t)"""
    return F32(1) - np.exp2(-emu_t_med3(x))


@_np
def emu_sigmoid(x):
    return F32(1) / (F32(1) + np.exp(-x))


@_np
def emu_silu(x):
    return x * emu_sigmoid(x)


@_np
def emu_dsilu(x):
    s = emu_sigmoid(x)
    return s * (x * (F32(1) - s) + F32(1))


@_np
def emu_erf(x):
    """Abramowitz & Stegun 7.1.26"""
    ax = np.abs(x)
    t = F32(1) / (F32(0.3275911) * ax + F32(1))
    p = F32(1.061405429) * t + F32(-1.453152027)
    p = p * t + F32(1.421413741)
    p = p * t + F32(-0.284496736)
    p = p * t + F32(0.254829592)
    e = np.exp2(-ax * ax * LOG2E)
    return np.copysign(F32(1) - p * t * e, x)


RSQRT2 = F32(0.70710678118654752440)


@_np
def emu_gelu(x):
    return F32(0.5) * x * (F32(1) + emu_erf(x * RSQRT2))


@_np
def emu_dgelu(x):
    cdf = F32(0.5) * (F32(1) + emu_erf(x * RSQRT2))
    pdf = F32(0.39894228040143267794) * np.exp2(F32(-0.5) * x * x * LOG2E)
    return x * pdf + cdf


@_np
def emu_sig_terms_p(z):
    """loss_optim.hip sig_terms: sigmoid from exp(-|z|)"""
    e = np.exp(-np.abs(z))
    r = F32(1) / (F32(1) + e)
    return np.where(z >= 0, r, e * r).astype(F32)


@_np
def emu_bce(z, y):
    return np.maximum(z, F32(0)) - z * y + np.log1p(np.exp(-np.abs(z)))


@_np
def emu_dbce(z, y):
    return emu_sig_terms_p(z) - y


@_np
def emu_identity(x):
    return x


@_np
def emu_softmax_exp2(s):
    """attention.hip: p = exp2((s - rowmax) log2e) / sum, rows along the last axis"""
    e = np.exp2((s - s.max(-1, keepdims=True)) * LOG2E)
    return e / e.sum(-1, keepdims=True, dtype=F32)


def emu_u8(z):
    z = _f(z)
    with np.errstate(all="ignore"):
        sg = F32(1) / (F32(1) + np.exp(-z))
        return (sg * F32(255)).astype(np.int32).astype(np.uint8)


def f16_store(x):
    """the IEEE store of an fp32 value into fp16 (round to nearest even, inf from 65520)"""
    return torch.as_tensor(np.asarray(x, F32)).to(torch.float16)


# ----------------------------------------------------------------------------- injected faults (emulation only)
@_np
def fault_gelu_tanh(x):
    return F32(0.5) * x * (F32(1) + np.tanh(F32(0.7978845608) * (x + F32(0.044715) * x * x * x)))


@_np
def fault_softplus_unguarded(x):
    return np.log(F32(1) + np.exp(x))


@_np
def fault_sigmoid_exp_ratio(x):
    e = np.exp(x)
    return e / (F32(1) + e)


@_np
def fault_bce_log_sigmoid(z, y):
    p = F32(1) / (F32(1) + np.exp(-z))
    return -(y * np.log(p) + (F32(1) - y) * np.log(F32(1) - p))


@_np
def fault_softmax_no_max(s):
    e = np.exp2(s * LOG2E)
    return e / e.sum(-1, keepdims=True, dtype=F32)


def fault_f16_store_clamped(x):
    return torch.as_tensor(np.clip(np.asarray(x, F32), -65504, 65504)).to(torch.float16)


# ----------------------------------------------------------------------------- E32
BCE_LABELS = (0.0, 1.0, 0.5)
# name -> (emulation, fp64 reference, documented in)
FORMULAS = {
    "softplus20": (emu_softplus20, ref_softplus, "common.h"),
    "softplus_lean": (emu_softplus_lean, ref_softplus, "selective_scan.hip"),
    "softplus_med3": (emu_softplus_med3, ref_softplus, "ss2d_fused.hip"),
    "dsoftplus_sigmoid": (emu_dsoftplus_sigmoid, ref_dsoftplus, "selective_scan.hip"),
    "dsoftplus_exp2": (emu_dsoftplus_exp2, ref_dsoftplus, "ss2d_fused.hip"),
    "sigmoid": (emu_sigmoid, ref_sigmoid, "common.h"),
    "silu": (emu_silu, ref_silu, "common.h"),
    "dsilu": (emu_dsilu, ref_dsilu, "common.h"),
    "gelu": (emu_gelu, ref_gelu, "common.h"),
    "dgelu": (emu_dgelu, ref_dgelu, "common.h"),
    "identity": (emu_identity, ref_identity, "-"),
}
FORMULAS2 = {       # functions of (logit, label)
    "bce": (emu_bce, ref_bce, "loss_optim.hip"),
    "dbce": (emu_dbce, ref_dbce, "loss_optim.hip"),
}


def err(got, want):
    """e = |got - want| / max(1, |want|) elementwise (fp64 tensor; inf / nan where `got` is not finite)"""
    got, want = _t64(got), _t64(want)
    return (got - want).abs() / want.abs().clamp_min(1.0)


def softmax_rows():
    """score rows for the softmax formula: the sweep itself, one dominant key, all equal, a span of +-300"""
    s = SWEEP
    return np.stack([s, np.where(np.arange(len(s)) == 7, F32(300), F32(-300)), np.full(len(s), F32(88.8)),
                     np.linspace(-300, 300, len(s)).astype(F32)])


@functools.lru_cache(maxsize=None)
def e32_table():
    """{formula: (E32, worst x, finite everywhere)}"""
    out = {}
    for name, (emu, ref, _) in FORMULAS.items():
        got = emu(SWEEP)
        e = err(torch.from_numpy(got), ref(SWEEP))
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        i = int(e.argmax())
        out[name] = (max(float(e[i]), FLOOR), float(SWEEP[i]), bool(np.isfinite(got).all()))
    for name, (emu, ref, _) in FORMULAS2.items():
        worst, wx, fin = 0.0, 0.0, True
        for y in BCE_LABELS:
            got = emu(SWEEP, np.full_like(SWEEP, y))
            e = err(torch.from_numpy(got), ref(SWEEP, torch.full((len(SWEEP),), y, dtype=torch.float64)))
            e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
            i = int(e.argmax())
            if float(e[i]) >= worst:
                worst, wx = float(e[i]), float(SWEEP[i])
            fin = fin and bool(np.isfinite(got).all())
        out[name] = (max(worst, FLOOR), wx, fin)
    rows = softmax_rows()
    got = emu_softmax_exp2(rows)
    e = err(torch.from_numpy(got), torch.softmax(torch.from_numpy(rows).double(), -1))
    out["softmax"] = (max(float(e.max()), FLOOR), float(rows.reshape(-1)[int(e.argmax())]), bool(np.isfinite(got).all()))
    return out


def E32(name):
    return e32_table()[name][0]


# what a kernel's activation enum / output is held to: act -> (formula, reference)
ACT_FORMULA = {ACT_NONE: "identity", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_SIGMOID_GATE: "sigmoid", ACT_GELU_GRAD_MUL: "dgelu"}
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_SIGMOID_GATE: "sigmoid_gate", ACT_GELU_GRAD_MUL: "gelu_grad_mul"}


def check(got, want, xs, formula, out_dtype=torch.float32):
    """the rule of the module docstring -> dict(ok, error, bound, worst_x, finite).  got: any tensor, want: fp64 of the same shape, xs: the
    argument behind every element (same shape).  Elements whose reference, rounded to `out_dtype`, is not finite are skipped."""
    got, want = got.detach().double().cpu().reshape(-1), _t64(want).reshape(-1)
    xs = _t64(xs).reshape(-1)
    assert got.shape == want.shape == xs.shape, (got.shape, want.shape, xs.shape)
    live = torch.isfinite(want.float().to(out_dtype).float())
    finite = bool(torch.isfinite(got[live]).all())
    b32 = FACTOR * E32(formula)
    scale = want.abs().clamp_min(1.0)
    if out_dtype == torch.float32:
        bound = b32 * torch.ones_like(want)
        e = (got - want).abs() / scale
    else:
        bound = U_ROUND[out_dtype] * want.abs() + b32 * scale
        e = (got - want).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    ratio = torch.where(live, e / bound, torch.zeros_like(e))
    i = int(ratio.argmax())
    return dict(ok=finite and bool((ratio <= 1.0).all()), error=float(e[i]), bound=float(bound[i]), worst_x=float(xs[i]),
                finite=finite, out_dtype=str(out_dtype).replace("torch.", ""))


def record(kernel, form, dtype, function, res, variant=""):
    """variant: what tells apart cases that the profile keeps as one record (the worst of them)"""
    return dict(kernel=kernel, form=str(form), dtype=str(dtype).replace("torch.", ""), function=function, worst_x=res["worst_x"],
                error=res["error"], bound=res["bound"], ok=res["ok"], out_dtype=res["out_dtype"], variant=variant)


# ----------------------------------------------------------------------------- probe: boundary selective scan
SCAN_K, SCAN_DPER = 10, 32            # 320 rows >= len(SWEEP); the 32 rows of a group own 32 different positions
SCAN_NS = (1, 4, 3, 16)               # fixed kernels (1, 4), state-looped kernels (3, 16)
SCAN_LS = (37, 40)                    # scalar path / 16-byte path


def scan_probe(n, l, dtype, softplus=True, all_states=False, u_scale=1.0, values=None):
    """operands of selective_scan_fwd / _bwd with A = 0, D = 0, u and dout one-hot per row at s_r, B = C = 1 in state 0 (every
    state with all_states), delta + delta_bias = a sweep value at EVERY position (row r holds xs[r] at s_r):
    out[r, t >= s_r] = u_scale * softplus(xs[r]), ddelta[r, s_r] = u_scale * softplus'(xs[r])."""
    k, dper = SCAN_K, SCAN_DPER
    kd = k * dper
    vals = np.asarray(SWEEP if values is None else values, F32)
    if not softplus:
        vals = vals[np.abs(vals) <= 100]
    base = np.resize(vals, kd)
    pos = (np.arange(kd) % dper + 3) % l                       # s_r: distinct inside a group (dper <= l)
    x = np.empty((kd, l), F32)
    for t in range(l):                                         # row r: xs[r] at s_r, its neighbours in the sweep elsewhere
        x[:, t] = np.resize(vals, kd + l)[np.arange(kd) + (t - pos) % l]
    assert bool((x[np.arange(kd), pos] == base).all())
    o = types.SimpleNamespace(n=n, l=l, dtype=dtype, softplus=softplus, k=k, dper=dper, kd=kd, pos=torch.from_numpy(pos).long(),
                              xs=torch.from_numpy(base), all_states=all_states, u_scale=u_scale)
    if dtype == torch.float32:
        o.delta_bias = torch.from_numpy(base - F32(0.5) * base)         # an fp32 split that is exact as well: x = x/2 + x/2
        o.delta = (torch.from_numpy(x) - o.delta_bias[:, None])[None].contiguous()
        o.x_eff = (o.delta[0] + o.delta_bias[:, None])
    else:
        # the bias is one value per row, so the 16-bit part has to absorb the rest: delta = round16(x - bias), and the sweep
        # value is exact at s_r (bias = xs - round16(xs)); elsewhere delta + bias is a neighbour of a sweep value
        hi, lo = split16(base, dtype)
        o.delta_bias = lo
        d = (torch.from_numpy(x) - lo[:, None]).to(dtype)
        d[torch.arange(kd), o.pos] = hi
        o.delta = d[None].contiguous()
        o.x_eff = o.delta[0].float() + lo[:, None]
    assert torch.equal(o.x_eff[torch.arange(kd), o.pos], o.xs)
    onehot = torch.zeros(1, kd, l)
    onehot[0, torch.arange(kd), o.pos] = 1.0
    o.u = (onehot * u_scale).to(dtype)
    o.dout = onehot.clone()
    bc = torch.zeros(1, k, n, l)
    bc[:, :, (slice(None) if all_states else 0)] = 1.0
    o.B, o.C = bc.to(dtype), bc.clone().to(dtype)
    o.A = torch.zeros(kd, n)
    o.D = torch.zeros(kd)
    return o


def scan_probe_oracle(o):
    """fp64 oracle on the probe's operands: (out, (du, ddelta, dA, dB, dC, dD, dbias))"""
    f = lambda t: t.float()
    args = (f(o.u), f(o.delta), o.A, f(o.B), f(o.C), o.D, o.delta_bias)
    return oss.selective_scan_fwd(*args, o.softplus), oss.selective_scan_bwd(*args, o.dout, o.softplus)


def scan_probe_expected(o):
    """closed forms at the probed elements: out[r, s_r], du[r, s_r], ddelta[r, s_r] (kd) fp64"""
    ns = o.n if o.all_states else 1
    sp = ref_softplus(o.xs) if o.softplus else _t64(o.xs)
    dsp = ref_dsoftplus(o.xs) if o.softplus else torch.ones(o.kd, dtype=torch.float64)
    us = float(o.u.float().max())
    return dict(out=ns * us * sp, du=ns * sp, ddelta=ns * us * dsp)


# ----------------------------------------------------------------------------- probe: GEMM epilogues
GEMM_FORMS = (7, 13, 14, 16, 17, 18, 19)         # TUNE_GEMM_TILE values that force a form
GEMM_FORM_NAME = {0: "rule", 7: "DMA4", 13: "DMA2", 14: "DMA3", 16: "PC3", 17: "PC4", 18: "rule-no-PC/WS", 19: "WS"}
GEMM_SHAPES = {"whole": (128, 512, 128), "ragged": (100, 520, 64)}
GEMM_ACTS = (ACT_SILU, ACT_GELU, ACT_SIGMOID_GATE, ACT_GELU_GRAD_MUL)


def gemm_probe(m, n, k, dtype, act, seed=0):
    """x = 0, w random: y[i, j] = act(bias[j]) (residual = 1 for the gate); GELU_GRAD_MUL: bias = 1, residual = the sweep `dtype`
    holds -> y[i, j] = gelu'(residual[i, j]).  -> namespace x, w, bias, residual, xs (m, n) f32 the argument of every element"""
    g = torch.Generator().manual_seed(seed + n + k)
    o = types.SimpleNamespace(m=m, n=n, k=k, dtype=dtype, act=act)
    o.x = torch.zeros(m, k, dtype=dtype)
    o.w = torch.randn(n, k, generator=g).to(dtype)
    if act == ACT_GELU_GRAD_MUL:
        vals = sweep_for(dtype)
        o.bias = torch.ones(n)
        idx = (torch.arange(m)[:, None] * 7 + torch.arange(n)[None]) % len(vals)          # rows differ: every value in every tile
        o.xs = torch.from_numpy(vals)[idx]
        o.residual = o.xs.to(dtype)
        assert torch.equal(o.residual.float(), o.xs)
    else:
        o.bias = tiled(SWEEP, n)
        o.xs = o.bias[None].expand(m, n)
        o.residual = torch.ones(m, n, dtype=dtype) if act == ACT_SIGMOID_GATE else None
    return o


def act_reference(act, xs):
    return FORMULAS[ACT_FORMULA[act]][1](xs)


def gemm_probe_cpu(o):
    """the probe through a plain fp64 GEMM + epilogue: what the GPU test reads, from the operands alone"""
    acc = o.x.double() @ o.w.double().t() + o.bias.double()
    if o.act == ACT_GELU_GRAD_MUL:
        return acc * ref_dgelu(o.residual)
    y = act_reference(o.act, acc)
    return y * o.residual.double() if o.act == ACT_SIGMOID_GATE else y


# ----------------------------------------------------------------------------- probe: norms and the depth-wise stencil
def chunks(c, values=SWEEP):
    """the sweep cut into pieces of c channels (the last one wraps)"""
    v = np.asarray(values, F32)
    return [torch.from_numpy(np.resize(np.roll(v, -i), c).copy()) for i in range(0, len(v), c)]


def norm_probe(rows, c, dtype, b, seed=0):
    """LayerNorm operands with w = 0: the output is act(b) whatever x holds"""
    g = torch.Generator().manual_seed(seed + c)
    return torch.randn(rows, c, generator=g).mul(3).to(dtype), torch.zeros(c), b.clone()


DW_C = 320


def dw_probe(dtype, ks, hw=6):
    """x[., ., ., c] = the `dtype` part of sweep value c, bias[c] = the rest, a centre tap of 1: pre = the sweep value exactly"""
    vals = tiled(SWEEP, DW_C)
    hi, lo = split16(vals, dtype) if dtype != torch.float32 else (vals * 0.5, vals - vals * 0.5)
    x = hi.reshape(1, 1, 1, DW_C).expand(1, hw, hw, DW_C).contiguous()
    wt = torch.zeros(ks * ks, DW_C)
    wt[ks * ks // 2] = 1.0
    return types.SimpleNamespace(x=x, wt=wt, bt=lo.float().contiguous(), xs=vals[None, None, None].expand(1, hw, hw, DW_C))


# ----------------------------------------------------------------------------- probe: loss
LOSS_HW = 32


def loss_probe(label, resized):
    """one plane: logits = SWEEP tiled (32 x 32, or 16 x 16 resized to the 32 x 32 label), label all-0 / all-1 / checkerboard"""
    s = LOSS_HW // 2 if resized else LOSS_HW
    z = tiled(SWEEP, s * s).reshape(1, 1, s, s)
    if label == "checker":
        y = ((torch.arange(LOSS_HW)[:, None] + torch.arange(LOSS_HW)[None]) % 2).float().reshape(1, 1, LOSS_HW, LOSS_HW)
    else:
        y = torch.full((1, 1, LOSS_HW, LOSS_HW), float(label == "ones"))
    return z, y


def loss_reference(z, y, wmap=None, eps=0.0, with_iou=True, per_pixel=False):
    """fp64: mean BCE-with-logits in the form max(z, 0) - z y + log1p(exp(-|z|)) + IoU loss (train.py:76-85), or the weighted
    reading of utils/loss.py:14-42 -> (loss, d loss / d z) by the closed form of loss_optim.hip's header:
    d = a omega (p - yhat) + p (1 - p) W (cI y + cU)"""
    z0 = z.double()
    y = y.double()
    zz = F.interpolate(z0, y.shape[-2:], mode="bilinear") if z0.shape[-2:] != y.shape[-2:] else z0
    zz = zz.detach().requires_grad_()
    p = torch.sigmoid(zz)
    npix = y.shape[-1] * y.shape[-2]
    if wmap is None:
        bce = ref_bce(zz, y).mean()
        inter, union = (p * y).sum(), (p + y).sum()
        loss = bce + (1 - (inter + 1) / (union - inter + 1))
        w, omega, yhat, a = torch.ones_like(y), 1.0, y, 1.0 / npix
    else:
        w = wmap.double()
        yhat = (1 - eps) * y + eps / 2
        b = ref_bce(zz, yhat)
        b = b if per_pixel else b.mean()
        loss = (w * b).sum() / w.sum()
        omega, a = (w, 1.0 / float(w.sum())) if per_pixel else (1.0, 1.0 / npix)
        inter, union = (p * y * w).sum(), ((p + y) * w).sum()
        if with_iou:
            loss = loss + (1 - (inter + 1) / (union - inter + 1))
    # closed-form gradient on the label grid
    inter, union = inter.detach(), union.detach()
    den = union - inter + 1
    c_i, c_u = -(union + 2) / den ** 2, (inter + 1) / den ** 2          # d iou / d (p y W) collected on y, d iou / d (p W)
    if wmap is not None and not with_iou:
        c_i = c_u = torch.zeros(())
    pd = p.detach()
    grad = a * omega * (pd - yhat) + pd * (1 - pd) * w * (c_i * y + c_u)
    auto, = torch.autograd.grad(loss, zz)
    live = zz.detach() != 0          # (autograd takes a one-sided derivative of max(z, 0) and |z| at z = 0)
    assert float(((auto - grad) * live).abs().max()) <= 1e-12 * max(1.0, float(auto.abs().max())), "closed form != autograd"
    if z0.shape[-2:] != y.shape[-2:]:          # the resize is linear: its adjoint carries the gradient to the small map
        zs = z0.detach().requires_grad_()
        F.interpolate(zs, y.shape[-2:], mode="bilinear").backward(grad)
        grad = zs.grad
    return loss.detach(), grad.detach()


# ----------------------------------------------------------------------------- probe: output range (fp16)
RANGE_SUMS = (65503.0, 65504.0, 65519.0, 65520.0, 65536.0, 7e4)


def range_probe():
    """(a, b, want): fp16-representable a, b whose exact sums are RANGE_SUMS and their negatives; want = the IEEE fp16 store"""
    sums = torch.tensor([s * sg for s in RANGE_SUMS for sg in (1.0, -1.0)], dtype=torch.float64)
    a = torch.sign(sums) * torch.clamp((sums.abs() / 2048).floor() * 2048, max=63488.0)      # 31 * 2^11 at the most
    b = sums - a
    for t in (a, b):
        assert torch.equal(t.to(torch.float16).double(), t)
    return a.to(torch.float16), b.to(torch.float16), f16_store(sums.float())


# ----------------------------------------------------------------------------- probe: fused SS2D scan
SS2D_H, SS2D_D, SS2D_R = 12, 32, 8
SS2D_H_DMA = 32                        # the smallest square map on which TUNE_SCAN_FORM 3 is honoured (ss2d_dma_runs)
SS2D_MFMA_MAX = 1e4                    # |x'| = |x log2e| the dt_proj MFMA is asked to produce stays at or below this


def ss2d_dma_runs(l, d, r, seqs, dtype):
    """tramba_ss2d_scan_cl's `dma_ok`: does knob 3 reach the LDS-DMA kernel?  16-bit map, padded rank 8 / 16 / 32, whole 32-channel
    tiles, at least two super-chunks of wdma 32-position tiles, and the launch within 4096 waves"""
    wdma = 16 if seqs * 16 <= 4096 else 8
    return dtype != torch.float32 and (r + 7) // 8 * 8 in (8, 16, 32) and d % 32 == 0 and l >= 2 * wdma * 32 and seqs * wdma <= 4096


def ss2d_values(mode, kd):
    """the pieces of the sweep one launch holds (kd = K * D channels each); mfma: only what keeps |x'| <= 1e4"""
    vals = SWEEP if mode == "bias" else SWEEP[np.abs(SWEEP.astype(np.float64)) * 1.4426950408889634 <= SS2D_MFMA_MAX]
    return chunks(kd, vals)


def ss2d_probe(fam, dtype, mode, values, form_dma=False, h=SS2D_H):
    """a tests/golden/scan_memory_cases.py case (12 x 12 map, D = 32, dt_rank 8, batch 1) with A = 0, Ds = 0, the B and C columns
    of xdbl = 1, x and the incoming gradient one-hot in position per channel (channel c at spatial position 5 c + 1), and
      mode "bias": dt_w = 0, dt_bias = `values` over the K * D channels (form_dma: conditioned as scan_memory_cases does for the
                   LDS-DMA kernel, which feeds bias * log2e to the MFMA as a bf16 (hi, lo) pair);
      mode "mfma": dt_bias = 0, rank column 3 of xdbl = 1 at every position, dt_w[k, c, 3] = the value conditioned so that
                   fl32(w log2e) is a bf16 value (the operand the kernels round to): x' comes out of the MFMA.
    ys[0, k, p >= p_kc, c] = softplus(x_kc), graw[0, k, p_kc, c] = gbias[k, c] = softplus'(x_kc) where direction k passes the
    position once (ss2d_expected has the general form).  c.xs (K, D): the arguments."""
    import scan_memory_cases as smc
    c = smc.make("undamped", fam, h, 1, SS2D_D, SS2D_R, dtype)
    k, l, d, r, rg = c.k, c.l, c.d, c.r, c.rg
    v = torch.as_tensor(np.asarray(values, F32)).reshape(k, d)
    pos = (5 * torch.arange(d) + 1) % l
    assert len(set(pos.tolist())) == d
    x = torch.zeros(1, l, d)
    x[0, pos, torch.arange(d)] = 1.0
    c.x, c.gym = x.to(dtype), x.clone().to(dtype)
    xdbl = torch.zeros(1, l, k, rg)
    xdbl[..., rg - 4:rg - 2] = 1.0
    c.dt_w = torch.zeros(k, d, r)
    if mode == "bias":
        c.dt_b = (smc._prescaled_hilo(v) if form_dma else v.clone()).reshape(-1).contiguous()
        c.xs = c.dt_b.reshape(k, d).clone()
    else:
        xdbl[..., 3] = 1.0
        w = smc._prescaled_bf16(v)
        c.dt_w[:, :, 3] = w
        c.dt_b = torch.zeros(k * d)
        c.xs = w.clone()
    c.xdbl = xdbl.view(1, l, k * rg).contiguous()
    c.A, c.ds = torch.zeros(k * d), torch.zeros(k * d)
    c.pos = pos
    # a direction may pass a position once, several times or (helix 4 .. 7) not at all: visits[k, p, c] = 1 where direction k
    # reads channel c's impulse at sequence index p
    c.visits = (c.table[:, :, None] == pos[None, None, :]).double()
    if hasattr(c, "dev"):
        del c.dev
    return c


def ss2d_expected(c):
    """closed forms (fp64): ys (1, K, L, D) = softplus(x_kc) * (visits so far); graw (1, K, L, D) = softplus'(x_kc) at a visit
    * (visits from there on: A = 0 carries the adjoint back undamped); gbias (1, K, D) its sum over the sequence"""
    sp, dsp = ref_softplus(c.xs), ref_dsoftplus(c.xs)
    sofar = c.visits.cumsum(1)
    ahead = c.visits.flip(1).cumsum(1).flip(1)
    graw = dsp[:, None, :] * c.visits * ahead
    return dict(ys=(sp[:, None, :] * sofar)[None], graw=graw[None], gbias=graw.sum(1)[None])


# ----------------------------------------------------------------------------- probe: attention
ATTN_WINDOW = dict(b=1, h=24, w=24, heads=4, hd=32, ws=12)       # the Swin block of attn_blocks.py, batch 1
ATTN_KV = dict(b=1, n=576, m=144, heads=2, hd=64)                # the PVT block of attn_blocks.py (sr 2 on 24 x 24), batch 1
ATTN_TOP, ATTN_STEP = 64.0, 16.0


def _alpha_beta(nq, nk, heads, seed):
    """query amplitudes in {+64, -64, 0} (one dominant key at either end of the scale; every score equal) and key amplitudes:
    one key at +64, one at -64, the others on the levels -48 .. 48 in steps of 16 -- (nq, heads), (nk, heads)"""
    g = torch.Generator().manual_seed(seed)
    alpha = torch.tensor([ATTN_TOP, -ATTN_TOP, 0.0])[torch.randint(0, 3, (nq, heads), generator=g)]
    beta = (torch.randint(0, 7, (nk, heads), generator=g) - 3).float() * ATTN_STEP
    for hh in range(heads):
        j = torch.randperm(nk, generator=g)[:2]
        beta[j[0], hh], beta[j[1], hh] = ATTN_TOP, -ATTN_TOP
    return alpha, beta


def _to_windows(x, ws):
    b, h, w, c = x.shape
    return x.view(b, h // ws, ws, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, -1, ws * ws, c)


def _from_windows(xw, ws, h, w):
    b, c = xw.shape[0], xw.shape[-1]
    return xw.view(b, h // ws, w // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def window_attn_probe(dtype, shift, seed=0):
    """qkv (1, 24, 24, 3 C), table = 0, dy: q and k live in channel 0 of their head, amplitudes per _alpha_beta inside every
    (shifted) window, so that a row's scaled scores are +-724, +-543, ..., 0 (hd 32): exp2 of anything but the row maximum
    underflows, and P is 0 / 1 exactly"""
    a = ATTN_WINDOW
    b, h, w, heads, hd, ws = a["b"], a["h"], a["w"], a["heads"], a["hd"], a["ws"]
    c, n, nw = heads * hd, ws * ws, (h // ws) * (w // ws)
    g = torch.Generator().manual_seed(100 + seed)
    xw = torch.zeros(b, nw, n, 3, heads, hd)
    for i in range(nw):
        alpha, beta = _alpha_beta(n, n, heads, seed * 97 + i)
        xw[0, i, :, 0, :, 0], xw[0, i, :, 1, :, 0] = alpha, beta
    # channel 1: a random q against k = 1 shifts every score of a row by the same amount (the softmax does not move, equal
    # scores stay equal) and gives dk something to hold: dk[j, 1] = scale * sum_i dS_ij q_i1, while dq[i, 1] = scale * sum_j dS_ij = 0
    xw[:, :, :, 0, :, 1] = torch.randn(b, nw, n, heads, generator=g)
    xw[:, :, :, 1, :, 1] = 1.0
    xw[:, :, :, 2] = torch.randn(b, nw, n, heads, hd, generator=g)
    qkv = _from_windows(xw.reshape(b, nw, n, 3 * c), ws, h, w)
    if shift:
        qkv = torch.roll(qkv, shifts=(shift, shift), dims=(1, 2))
    dy = torch.randn(b, h, w, c, generator=g)
    return types.SimpleNamespace(qkv=qkv.to(dtype).contiguous(), table=torch.zeros((2 * ws - 1) ** 2, heads), dy=dy.to(dtype),
                                 ws=ws, shift=shift, heads=heads, hd=hd, dtype=dtype)


def shift_mask(h, w, ws, shift):
    """the -100 mask of the reference's SwinTransformerBlock: (nW, N, N), 0 where query and key share a region"""
    img = torch.zeros(1, h, w, 1)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = _to_windows(img, ws)[0, :, :, 0]
    diff = mw[:, None, :] - mw[:, :, None]
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff)).double()


def _window_split(o, x):
    """(B, H, W, n C) -> shifted windows (B, nW, N, n C), and the way back"""
    a = ATTN_WINDOW
    x = torch.roll(x, shifts=(-o.shift, -o.shift), dims=(1, 2)) if o.shift else x

    def back(t):
        t = _from_windows(t, o.ws, a["h"], a["w"])
        return torch.roll(t, shifts=(o.shift, o.shift), dims=(1, 2)) if o.shift else t
    return _to_windows(x, o.ws), back


def window_attn_reference(o, qkv=None):
    """fp64 on the rounded operands -> (out (B, H, W, C), scaled scores (B, nW, heads, N, N) with the mask added)"""
    a = ATTN_WINDOW
    xw, back = _window_split(o, (o.qkv if qkv is None else qkv).double())
    b, nw, n = xw.shape[:3]
    q, k, v = xw.view(b, nw, n, 3, o.heads, o.hd).permute(3, 0, 1, 4, 2, 5)
    bias = shift_mask(a["h"], a["w"], o.ws, o.shift)[None, :, None] if o.shift else None
    out, _, s = ref_attention(q, k, v, o.hd ** -0.5, bias)
    return back(out.transpose(2, 3).reshape(b, nw, n, o.heads * o.hd)), s


def _attn_magnitudes(q, k, v, do, s, scale):
    """the contractions of an attention backward taken over magnitudes, without cancellation (the A of the bound 3 u A + 1e-6,
    tests/test_gpu_attn_train.py): dV: P^T |dO|; dS~ = P (|dP| + sum_k P |dP|); dQ: scale dS~ |K|; dK: scale dS~^T |Q|"""
    p = torch.softmax(s, -1)
    dpa = (do @ v.transpose(-1, -2)).abs()
    dsb = p * (dpa + (p * dpa).sum(-1, keepdim=True))
    return (dsb @ k.abs()) * scale, (dsb.transpose(-1, -2) @ q.abs()) * scale, p.transpose(-1, -2) @ do.abs()


def window_attn_magnitudes(o):
    """A of dqkv, (B, H, W, 3 C)"""
    xw, back = _window_split(o, o.qkv.double())
    b, nw, n = xw.shape[:3]
    q, k, v = xw.view(b, nw, n, 3, o.heads, o.hd).permute(3, 0, 1, 4, 2, 5)
    do = _window_split(o, o.dy.double())[0].view(b, nw, n, o.heads, o.hd).permute(0, 1, 3, 2, 4)
    _, s = window_attn_reference(o)
    a = torch.stack(_attn_magnitudes(q, k, v, do, s, o.hd ** -0.5)).permute(1, 2, 4, 0, 3, 5).reshape(b, nw, n, -1)
    return back(a)


def kv_attn_probe(dtype, seed=0):
    a = ATTN_KV
    b, n, m, heads, hd = a["b"], a["n"], a["m"], a["heads"], a["hd"]
    g = torch.Generator().manual_seed(200 + seed)
    alpha, beta = _alpha_beta(n, m, heads, 7 + seed)
    q = torch.zeros(b, n, heads, hd)
    kv = torch.zeros(b, m, 2, heads, hd)
    q[0, :, :, 0], kv[0, :, 0, :, 0] = alpha, beta
    q[0, :, :, 1], kv[0, :, 0, :, 1] = torch.randn(n, heads, generator=g), 1.0          # (as window_attn_probe: dk != 0)
    kv[:, :, 1] = torch.randn(b, m, heads, hd, generator=g)
    dy = torch.randn(b, n, heads * hd, generator=g)
    return types.SimpleNamespace(q=q.view(b, n, -1).to(dtype), kv=kv.view(b, m, -1).to(dtype), dy=dy.to(dtype), heads=heads, hd=hd,
                                 dtype=dtype)


def kv_attn_reference(o, q=None, kv=None):
    q = (o.q if q is None else q).double()
    kv = (o.kv if kv is None else kv).double()
    b, n, c = q.shape
    m = kv.shape[1]
    qd = q.view(b, n, o.heads, o.hd).transpose(1, 2)
    k, v = kv.view(b, m, 2, o.heads, o.hd).permute(2, 0, 3, 1, 4)
    out, _, s = ref_attention(qd, k, v, o.hd ** -0.5)
    return out.transpose(1, 2).reshape(b, n, c), s


def kv_attn_magnitudes(o):
    """(A of dq (B, N, C), A of dkv (B, M, 2 C))"""
    b, n, c = o.q.shape
    m = o.kv.shape[1]
    qd = o.q.double().view(b, n, o.heads, o.hd).transpose(1, 2)
    do = o.dy.double().view(b, n, o.heads, o.hd).transpose(1, 2)
    k, v = o.kv.double().view(b, m, 2, o.heads, o.hd).permute(2, 0, 3, 1, 4)
    aq, ak, av = _attn_magnitudes(qd, k, v, do, kv_attn_reference(o)[1], o.hd ** -0.5)
    return aq.transpose(1, 2).reshape(b, n, c), torch.stack([ak, av]).permute(1, 3, 0, 2, 4).reshape(b, m, 2 * c)


def attn_grads(ref_fn, o, names):
    """fp64 autograd through the reference: {name: gradient} for the operand attributes `names`"""
    leaves = {nm: getattr(o, nm).double().requires_grad_() for nm in names}
    out, _ = ref_fn(o, **leaves)
    out.backward(o.dy.double())
    return {nm: t.grad for nm, t in leaves.items()}


ATTN_SPAN = 300.0


def score_span(s):
    return float(s.min()), float(s.max())


# ----------------------------------------------------------------------------- the host side of profiles/pointwise_parity.json
def _worst(e, xs):
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.reshape(-1).argmax())
    return float(e.reshape(-1)[i]), float(np.asarray(xs, np.float64).reshape(-1)[i])


def fault_table():
    """every injected fault (emulation only) -> dict(formula, e32, error, factor = error / (8 E32), worst_x, nonfinite); error and
    factor are None where the fault turns non-finite, the factor also for the bit-exact store (error = values that differ)"""
    out = {}

    def add(name, formula, got, want, xs):
        e, x = _worst(err(torch.from_numpy(got), want), xs)
        out[name] = dict(formula=formula, e32=E32(formula), error=e if math.isfinite(e) else None,
                         factor=e / (FACTOR * E32(formula)) if math.isfinite(e) else None, worst_x=x,
                         nonfinite=not bool(np.isfinite(got).all()))
    add("tanh-GELU for erf-GELU", "gelu", fault_gelu_tanh(SWEEP), ref_gelu(SWEEP), SWEEP)
    add("softplus = log(1 + exp(x)), no large-x guard", "softplus20", fault_softplus_unguarded(SWEEP), ref_softplus(SWEEP), SWEEP)
    add("sigmoid = exp(x) / (1 + exp(x))", "sigmoid", fault_sigmoid_exp_ratio(SWEEP), ref_sigmoid(SWEEP), SWEEP)
    ys = np.repeat(np.asarray(BCE_LABELS, F32), len(SWEEP))
    zs = np.tile(SWEEP, len(BCE_LABELS))
    add("BCE = -log(sigmoid)", "bce", fault_bce_log_sigmoid(zs, ys), ref_bce(zs, ys), zs)
    rows = softmax_rows()
    add("softmax without the row maximum", "softmax", fault_softmax_no_max(rows), torch.softmax(torch.from_numpy(rows).double(), -1), rows)
    _, _, want = range_probe()
    sums = torch.tensor([s * sg for s in RANGE_SUMS for sg in (1.0, -1.0)])
    got = fault_f16_store_clamped(sums.numpy())
    wrong = got.view(torch.int16) != want.view(torch.int16)
    out["fp16 store clamped to 65504"] = dict(formula="fp16 store", e32=0.0, error=float(wrong.sum()), factor=None,
                                              worst_x=float(sums[wrong][0]) if bool(wrong.any()) else 0.0, nonfinite=False)
    return out


def host_profile():
    t = e32_table()
    return dict(factor=FACTOR, sweep_points=len(SWEEP), sweep_bf16=len(SWEEP_BF16), sweep_f16=len(SWEEP_F16),
                e32={k: dict(e32=v[0], worst_x=v[1], finite=v[2], documented_in=(FORMULAS.get(k) or FORMULAS2.get(k) or
                                                                                 (0, 0, "attention.hip"))[2]) for k, v in t.items()},
                faults=fault_table())
