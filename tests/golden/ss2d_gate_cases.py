"""SS2D's z gate (vmamba.py:275-291 with disable_z=False) and the channels-last interface: the two-argument formulas of the
gate kernels with their fp64 references and numpy-float32 emulations, the pair sweep they are probed on, the operands of the
gated merge kernel in each of its three forms, and the oracle composition of the gated block (tests/test_ss2d_gate_host.py,
tests/test_gpu_ss2d_gate.py, scripts/bench_ss2d_gate.py).

Formulas (n = out_norm's output as stored, z = the gate's pre-activation as stored; documented in csrc/common.h):
    gate_fwd  p  = gelu(n) * silu(z)
    gate_gn   gn = silu(z) * gelu'(n)          (per unit of incoming gradient)
    gate_gz   gz = gelu(n) * silu'(z)
The rule is pointwise_cases': e = |got - want| / max(1, |want|); E32 = the worst e of the float32 emulation over the pair sweep
(floored at 2^-24); an fp32 output stays within FACTOR * E32, a 16-bit one within u |want| + FACTOR * E32 max(1, |want|);
elements whose reference is not finite in the output dtype are skipped."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import pointwise_cases as pc
from oracle import ops

F32 = np.float32
HELD = (-3.0, -0.5, 0.0, 0.5, 3.0, 30.0)      # the values one argument is held at while the other runs over the sweep
MAX_SKIPPED = 0.05

# name -> (emulation(n, z) float32, reference(n, z) fp64)
FORMULAS = {
    "gate_fwd": (lambda n, z: pc.emu_gelu(n) * pc.emu_silu(z), lambda n, z: pc.ref_gelu(n) * pc.ref_silu(z)),
    "gate_gn": (lambda n, z: pc.emu_silu(z) * pc.emu_dgelu(n), lambda n, z: pc.ref_silu(z) * pc.ref_dgelu(n)),
    "gate_gz": (lambda n, z: pc.emu_gelu(n) * pc.emu_dsilu(z), lambda n, z: pc.ref_gelu(n) * pc.ref_dsilu(z)),
}


def fault_sigmoid_gate(n, z):
    """the gate applied as sigmoid(z) instead of silu(z) (emulation only: shows that the rule has teeth)"""
    return pc.emu_gelu(n) * pc.emu_sigmoid(z)


def pairs(dtype, pad_to_odd=True):
    """(n, z) float32 arrays: n over sweep_for(dtype) with z held at each of HELD, then the roles swapped; every value is one
    `dtype` holds exactly (HELD is representable in all three).  pad_to_odd: the count is made no multiple of 8 (the scalar
    tail of the pointwise kernel) by repeating the first pairs."""
    sw = pc.sweep_for(dtype)
    held = np.asarray(HELD, F32)
    a = np.concatenate([np.tile(sw, len(held)), np.repeat(held, len(sw))])
    b = np.concatenate([np.repeat(held, len(sw)), np.tile(sw, len(held))])
    if pad_to_odd and len(a) % 8 == 0:
        a, b = np.concatenate([a, a[:3]]), np.concatenate([b, b[:3]])
    return a.astype(F32), b.astype(F32)


@functools.lru_cache(maxsize=None)
def e32(name):
    """E32 of a two-argument formula: the emulation against fp64 over the fp32 pair sweep (pointwise_cases' rule for `bce`)"""
    emu, ref = FORMULAS[name]
    n, z = pairs(torch.float32)
    with np.errstate(all="ignore"):
        got = np.asarray(emu(n, z), F32)
    e = pc.err(torch.from_numpy(got), ref(n, z))
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    return max(float(e.max()), pc.FLOOR)


def check(got, want, formula, out_dtype=torch.float32):
    """the rule of the module docstring -> dict(ok, error, bound, worst (index), skipped (share), finite)"""
    got, want = got.detach().double().cpu().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    live = torch.isfinite(want.float().to(out_dtype).float())
    finite = bool(torch.isfinite(got[live]).all())
    b32 = pc.FACTOR * e32(formula)
    scale = want.abs().clamp_min(1.0)
    if out_dtype == torch.float32:
        bound = b32 * torch.ones_like(want)
        e = (got - want).abs() / scale
    else:
        bound = pc.U_ROUND[out_dtype] * want.abs() + b32 * scale
        e = (got - want).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    ratio = torch.where(live, e / bound, torch.zeros_like(e))
    i = int(ratio.argmax())
    return dict(ok=finite and bool((ratio <= 1.0).all()), error=float(e[i]), bound=float(bound[i]), worst=i,
                skipped=1.0 - float(live.double().mean()), finite=finite)


def skipped_share(formula, dtype):
    """share of the pair sweep whose reference is not finite in `dtype` (from the reference alone)"""
    n, z = pairs(dtype)
    want = FORMULAS[formula][1](n, z)
    return 1.0 - float(torch.isfinite(want.float().to(dtype).float()).double().mean())


# ----------------------------------------------------------------------------- kernel 1a: the gated merge in its three forms
# name -> (form, family, K, B, H, D): the launcher's own selection rule (csrc/ss2d_fused.hip, merge_launch) puts each shape on
# the form it is named for whatever the dtype; tests/test_gpu_ss2d_gate.py reads the kernel's name back from the profiler.
MERGE_CASES = {
    "deep_d40": ("deep", "helix", 8, 2, 12, 40),          # 16-byte accesses on 2-byte rows
    "deep_d33": ("deep", "helix", 8, 2, 12, 33),          # vector width 1
    "stream_d64": ("stream", "raster", 4, 1, 96, 64),     # one wave iteration
    "stream_d384": ("stream", "raster", 4, 1, 96, 384),   # two
    "split_d1024": ("split", "raster", 4, 2, 12, 1024),
}


def merge_operands(name, dtype, seed=0):
    """(ys (B,K,L,D) f32 on multiples of 1/32 in [-4, 4] -- exact in bf16 and fp16, and any sum of K..200 of them is exact in
    fp32 in any order --, ln_w, ln_b f32, zpre (B,L,D) f32 = sweep_for(dtype) tiled)"""
    form, fam, k, b, h, d = MERGE_CASES[name]
    g = torch.Generator().manual_seed(seed + d)
    l = h * h
    ys = (torch.randn(b, k, l, d, generator=g) * 32).round().clamp_(-128, 128) / 32
    ln_w = 1.0 + 0.25 * torch.randn(d, generator=g)
    ln_b = 0.5 * torch.randn(d, generator=g)
    zpre = pc.tiled(pc.sweep_for(dtype), b * l * d).reshape(b, l, d)
    return ys, ln_w, ln_b, zpre


# ----------------------------------------------------------------------------- the gated block: modules and their oracle
D_MODEL, MAP, BATCH = 32, 12, 2


def make_ss2d(n, family, channel_first, gated, seed=11):
    """tramba_amd.SS2D(d_model=32, d_state=n) of a built-in family with every parameter moved off its initial value"""
    import tramba_amd as ta
    from tramba_amd import ops as tops
    torch.manual_seed(seed)
    kw = dict(scan=tops.CrossScan_Line, merge=tops.CrossMerge_Line, k_group=8) if family == "helix" else {}
    m = ta.SS2D(d_model=D_MODEL, d_state=n, channel_first=channel_first, disable_z=not gated, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    return m


def make_input(seed=12, batch=BATCH, h=MAP):
    """(B, C, H, W) float32"""
    return torch.randn(batch, D_MODEL, h, h, generator=torch.Generator().manual_seed(seed))


def oracle_ss2d(sd, x, family):
    """vmamba.py:275-291 composed from oracle.ops (as oracle/model.py ss2d does for the ungated block), NCHW in and out; the
    gate is present when in_proj is twice as wide as out_norm.  Any float dtype, autograd-capable."""
    di = sd["out_norm.weight"].shape[0]
    t = ops.linear2d(x, sd["in_proj.weight"], sd.get("in_proj.bias"))
    gated = t.shape[1] == 2 * di
    xh, z = t.chunk(2, dim=1) if gated else (t, None)
    wc = sd["conv2d.weight"]
    xh = F.silu(F.conv2d(xh, wc, sd.get("conv2d.bias"), padding=(wc.shape[-1] - 1) // 2, groups=wc.shape[0]))
    y = ops.ss2d_core(xh, sd["x_proj_weight"], sd["dt_projs_weight"], sd["dt_projs_bias"], sd["A_logs"], sd["Ds"], family)
    y = F.gelu(ops.layernorm2d(y, sd["out_norm.weight"], sd["out_norm.bias"]))
    if gated:
        y = y * F.silu(z)
    return ops.linear2d(y, sd["out_proj.weight"], sd.get("out_proj.bias"))


def oracle_with_grads(m, x, family, gy):
    """(output, {name: gradient} with "x" for the input) of the oracle composition on m's parameters, float32 on the CPU"""
    leaves = {k: v.detach().cpu().float().clone().requires_grad_() for k, v in m.state_dict().items()}
    xo = x.detach().cpu().float().clone().requires_grad_()
    want = oracle_ss2d(leaves, xo, family)
    (want * gy).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["x"] = xo.grad
    return want.detach(), grads


def split_in_proj(grads, di):
    """in_proj.weight's gradient as its two halves (the x half and the z half are checked separately)"""
    out = dict(grads)
    w = out.pop("in_proj.weight")
    out["in_proj.weight[x]"], out["in_proj.weight[z]"] = w[:di], w[di:]
    return out


# the reference's state_dict of an SS2D (names -> shapes), vmamba.py:56-112
def expected_state_dict(d_model, d_state, k_group, gated, ssm_ratio=2.0, d_conv=3, bias=False, conv_bias=False):
    di = int(ssm_ratio * d_model)
    r = -(-d_model // 16)
    out = {"in_proj.weight": (2 * di if gated else di, d_model), "conv2d.weight": (di, 1, d_conv, d_conv),
           "x_proj_weight": (k_group, r + 2 * d_state, di), "dt_projs_weight": (k_group, di, r), "dt_projs_bias": (k_group, di),
           "A_logs": (k_group * di, d_state), "Ds": (k_group * di,), "out_norm.weight": (di,), "out_norm.bias": (di,),
           "out_proj.weight": (d_model, di)}
    if bias:
        out["in_proj.bias"], out["out_proj.bias"] = (2 * di if gated else di,), (d_model,)
    if conv_bias:
        out["conv2d.bias"] = (di,)
    return out


# ----------------------------------------------------------------------------- launches of the fused training path
LAUNCH_CASES = {"bf16_n1": 1, "bf16_n16": 16}          # d_state; raster K = 4, d_model 32, 12 x 12, batch 2, bf16


def launch_class(name):
    """the framework's copy / cast kernels, its fills, everything else (the library's kernels among it) -- the classes of
    tests/test_gpu_ss2d_dstate_train.py"""
    return "copy" if "copy" in name.lower() else "fill" if "fill" in name.lower() else "other"


def module_launches(n, gated, dev="cuda"):
    """{kernel name: launches} of one forward + backward of SS2D(d_model=32, d_state=n, channel_first=True) in bf16 on the
    fused training path (the caller opts in for n > 1), counted with torch.profiler as
    tests/test_gpu_ss2d_dstate_train.py::inner_launches does, after one call that is not counted"""
    from torch.profiler import ProfilerActivity, profile
    m = make_ss2d(n, "raster", True, gated).to(dev)
    x = make_input().to(dev, torch.bfloat16)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(13)).to(dev, torch.bfloat16)

    def once():
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_()
        torch.cuda.synchronize()
        return lambda: m(xg).backward(gy)

    once()()
    run = once()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    counts = {}
    for ev in prof.key_averages():
        if not ev.key.startswith("hip"):
            counts[ev.key] = counts.get(ev.key, 0) + ev.count
    return counts
