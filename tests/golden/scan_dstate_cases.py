"""Cases of the d_state 3, 5..16 selective scan (the state-looped kernel pair), shared by tests/test_scan_dstate_host.py and
tests/test_gpu_scan_dstate.py: the shapes, the input builder of tests/test_gpu_kernels.py, the fp64 references (computed once
per case and left unchanged) and the `init16` case, the regime SS2D(d_state=16) is born in."""
import functools
import math
import types

import torch

import scan_memory_cases as smc
from oracle import selective_scan as oss

# (nb, k, dper, n, l)
SHAPES = [
    (2, 2, 3, 16, 37),      # LPR 16, scalar path; the four rows of a wave straddle a group and a batch
    (2, 2, 3, 8, 200),      # LPR 32
    (1, 2, 3, 16, 1000),    # LPR 64, two chunks, ragged
    (1, 4, 4, 16, 1153),    # three chunks, odd length
    (2, 1, 8, 8, 2304),     # 16-byte path, 4.5 chunks
    (1, 2, 5, 3, 520),      # odd N, 8 positions in the last chunk
    (1, 3, 5, 16, 1032),    # K = 3
    (2, 2, 6, 12, 72),      # N = 12
]
FWD_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
BWD_DTYPES = (torch.float32, torch.bfloat16)
GRADS = ("du", "ddelta", "dA", "dB", "dC", "dD", "dbias")


def scan_inputs(nb, k, dper, n, l, dtype, seed=0):
    """_scan_inputs of tests/test_gpu_kernels.py"""
    g = torch.Generator().manual_seed(seed)
    kd = k * dper
    r = lambda *s: torch.randn(*s, generator=g)
    a = dict(u=r(nb, kd, l), delta=0.5 * r(nb, kd, l) - 0.5, A=-(torch.rand(kd, n, generator=g) + 0.2),
             B=r(nb, k, n, l), C=r(nb, k, n, l), D=1 + 0.1 * r(kd), delta_bias=0.3 * r(kd))
    for key in ("u", "delta", "B", "C"):
        a[key] = a[key].to(dtype)
    return a


def _f(t):
    return t.float()


@functools.lru_cache(maxsize=None)
def fwd_case(shape, dtype):
    """-> (inputs, fp64 output, fp64 output of the no-softplus / no-D / no-bias call on |delta|)"""
    a = scan_inputs(*shape, dtype)
    want = oss.selective_scan_fwd(_f(a["u"]), _f(a["delta"]), a["A"], _f(a["B"]), _f(a["C"]), a["D"], a["delta_bias"], True)
    want2 = oss.selective_scan_fwd(_f(a["u"]), _f(a["delta"]).abs(), a["A"], _f(a["B"]), _f(a["C"]), None, None, False)
    return a, want, want2


@functools.lru_cache(maxsize=None)
def bwd_case(shape, dtype):
    """-> (inputs, dout, the seven fp64 gradients)"""
    nb, k, dper, n, l = shape
    a = scan_inputs(*shape, dtype, seed=3)
    dout = torch.randn(nb, k * dper, l, generator=torch.Generator().manual_seed(9))
    want = oss.selective_scan_bwd(_f(a["u"]), _f(a["delta"]), a["A"], _f(a["B"]), _f(a["C"]), a["D"], a["delta_bias"], dout, True)
    return a, dout, want


def as_boundary(shape, dtype, a, dout):
    """the inputs of a case as the namespace scan_memory_cases' evaluations take"""
    nb, k, dper, n, l = shape
    return types.SimpleNamespace(nb=nb, k=k, dper=dper, n=n, l=l, dtype=dtype, dout=dout, **a)


def grad_error(got, want):
    """the measure of test_selective_scan_bwd: max |err| / max(1, max |want|)"""
    want = want.double()
    return float((got.double().reshape(want.shape) - want).abs().max()) / max(1.0, float(want.abs().max()))


# ----------------------------------------------------------------------------- init16
INIT16_KEY = "init16"


@functools.lru_cache(maxsize=None)
def init16_case(dtype):
    """rows 2 x 4 x 8, d_state 16, four 512-position chunks with the last ragged, in the regime the constructor leaves:
    A[d, n] = -(n + 1) (A_log_init), delta_bias the inverse softplus of a dt log-uniform in [1e-3, 1e-1] per row (Dt_init), and
    a small delta (dt_projs_weight starts at +-dt_rank^-0.5 times an x_proj output)."""
    l = smc.BOUNDARY_L[dtype]
    o = smc.make_boundary("slow", 2, 4, 8, 16, l, dtype)
    kd = o.k * o.dper
    g = torch.Generator().manual_seed(1600 + l)
    o.A = -torch.arange(1, 17, dtype=torch.float32).repeat(kd, 1).contiguous()
    dt = torch.exp(torch.rand(kd, generator=g) * (math.log(1e-1) - math.log(1e-3)) + math.log(1e-3))
    o.delta_bias = dt + torch.log(-torch.expm1(-dt))
    o.delta = (0.1 * torch.randn(o.nb, kd, l, generator=g)).to(dtype)
    o.regime = INIT16_KEY
    return o


def init16_e32(dtype):
    o = init16_case(dtype)
    return (o,) + smc.boundary_e32(o, (INIT16_KEY, 16, o.l, dtype))
