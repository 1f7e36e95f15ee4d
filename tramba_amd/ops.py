"""Drop-in operator surface of the reference's L0/L1 layers, backed by libtramba_hip.

* ``selective_scan_cuda_oflex``-compatible ``fwd`` / ``bwd`` (call sites
  Models/SS2D/csms6s.py:910, :920-922) and the ``SelectiveScanOflex`` autograd.Function
  (csms6s.py:904-923) with the reference's exact argument list.
* ``CrossScan*/CrossMerge*`` autograd.Functions (csms6s.py:13-216): the scan-order *plugin API*
  ``SS2D(..., scan=Cls, merge=Cls, k_group=K)``; ``Cls.apply(x:(B,C,H,W)) -> (B,K,C,H*W)``,
  ``merge.apply(ys:(B,K,D,H,W)) -> (B,D,H*W)``, each the adjoint (= backward) of the other.

Unlike the reference nothing happens at import time: tables are generated on demand for ANY
square size (the reference ships 12/24/48/96 only, csms6s.py:58-61,107-110,157) and cached
per device.
"""
import contextlib

import torch

from . import hip


# ----------------------------------------------------------------------------- L0
_DET_MODES = (False, True, "torch")
_det_mode = False


def set_deterministic_scan(mode):
    """Select the backward of the reference-layout selective scan (SelectiveScanOflex, selective_scan_cuda_oflex.bwd and
    every module that runs through them): False (default) -- dB / dC, dA, dD and d delta_bias summed with fp32 atomics;
    True -- the atomic-free form, bitwise reproducible run to run; "torch" -- follow
    torch.are_deterministic_algorithms_enabled() at backward time.  Returns the previous mode."""
    global _det_mode
    if not any(mode is m or (isinstance(mode, str) and mode == m) for m in _DET_MODES):
        raise ValueError(f"set_deterministic_scan: mode must be False, True or 'torch', got {mode!r}")
    prev, _det_mode = _det_mode, mode
    return prev


def get_deterministic_scan():
    """the mode set by set_deterministic_scan"""
    return _det_mode


@contextlib.contextmanager
def deterministic_scan(mode=True):
    """with deterministic_scan(True): ... -- set_deterministic_scan for a block; the previous mode comes back on exit,
    whatever happens inside"""
    prev = set_deterministic_scan(mode)
    try:
        yield
    finally:
        set_deterministic_scan(prev)


_fused_dstate_training = False


def set_fused_dstate_training(on):
    """Opt in (True) or out (False, the default) of the fused channels-last TRAINING path of SS2D at d_state 2..16
    (modules._SS2DInnerCL on hip.ss2d_scan_n_cl and the state-looped scan backward).  Off, a module with
    d_state > 1 under autograd takes the reference graph with the scan plugins, as before.  Returns the previous value."""
    global _fused_dstate_training
    if on is not True and on is not False:
        raise ValueError(f"set_fused_dstate_training: the value must be True or False, got {on!r}")
    prev, _fused_dstate_training = _fused_dstate_training, on
    return prev


def get_fused_dstate_training():
    """the value set by set_fused_dstate_training"""
    return _fused_dstate_training


@contextlib.contextmanager
def fused_dstate_training(on=True):
    """with fused_dstate_training(True): ... -- set_fused_dstate_training for a block; the previous value comes back on
    exit, whatever happens inside"""
    prev = set_fused_dstate_training(on)
    try:
        yield
    finally:
        set_fused_dstate_training(prev)


def _scan_is_deterministic():
    if _det_mode == "torch":
        return torch.are_deterministic_algorithms_enabled()
    return _det_mode


class _OflexExtension:
    """Object with the two entry points of the absent CUDA extension."""

    @staticmethod
    def fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows, oflex):
        out, ckpt = hip.selective_scan_fwd(_c(u), _c(delta), A, _c(B), _c(C), D, delta_bias,
                                           bool(delta_softplus), bool(oflex), want_ckpt=True)
        return out, ckpt

    @staticmethod
    def bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows):
        du, ddelta, dA, dB, dC, dD, dbias = hip.selective_scan_bwd(
            _c(u), _c(delta), A, _c(B), _c(C), D, delta_bias, _c(dout), x, bool(delta_softplus),
            deterministic=_scan_is_deterministic())
        dA = dA.to(A.dtype)
        dB, dC = dB.to(B.dtype), dC.to(C.dtype)
        dD = None if dD is None else dD.to(D.dtype)
        dbias = None if dbias is None else dbias.to(delta_bias.dtype)
        return du, ddelta, dA, dB, dC, dD, dbias


selective_scan_cuda_oflex = _OflexExtension()


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


class SelectiveScanOflex(torch.autograd.Function):
    """Same call signature as csms6s.py:904-923."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=False, nrows=1, backnrows=1,
                oflex=True):
        ctx.delta_softplus = delta_softplus
        out, x = selective_scan_cuda_oflex.fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, 1, oflex)
        ctx.save_for_backward(u, delta, A, B, C, D, delta_bias, x)
        return out

    @staticmethod
    def backward(ctx, dout, *args):
        u, delta, A, B, C, D, delta_bias, x = ctx.saved_tensors
        du, ddelta, dA, dB, dC, dD, ddelta_bias = selective_scan_cuda_oflex.bwd(
            u, delta, A, B, C, D, delta_bias, dout, x, ctx.delta_softplus, 1)
        return du, ddelta, dA, dB, dC, dD, ddelta_bias, None, None, None, None


# ----------------------------------------------------------------------------- L1
def _make_scan_pair(family: str, k: int, doc_scan: str, doc_merge: str):
    class Scan(torch.autograd.Function):
        _tramba_family = family
        _tramba_k = k

        @staticmethod
        def forward(ctx, x):
            b, c, h, w = x.shape
            ctx.shape = (b, c, h, w)
            order = hip.scan_order(family, h, w, x.device)
            return hip.cross_scan(_c(x), order)

        @staticmethod
        def backward(ctx, ys):
            b, c, h, w = ctx.shape
            order = hip.scan_order(family, h, w, ys.device)
            return hip.cross_merge(_c(ys), order).view(b, c, h, w)

    class Merge(torch.autograd.Function):
        _tramba_family = family
        _tramba_k = k

        @staticmethod
        def forward(ctx, ys):
            b, kk, d, h, w = ys.shape
            ctx.shape = (h, w)
            order = hip.scan_order(family, h, w, ys.device)
            return hip.cross_merge(_c(ys).view(b, kk, d, h * w), order)

        @staticmethod
        def backward(ctx, x):
            h, w = ctx.shape
            b, c, l = x.shape
            order = hip.scan_order(family, h, w, x.device)
            return hip.cross_scan(_c(x), order).view(b, order.k, c, h, w)

    Scan.__doc__, Merge.__doc__ = doc_scan, doc_merge
    return Scan, Merge


CrossScan, CrossMerge = _make_scan_pair(
    "raster", 4, "csms6s.py:13-31 (row-major, column-major and their flips)", "csms6s.py:34-55")
CrossScan_Line, CrossMerge_Line = _make_scan_pair(
    "helix", 8, "csms6s.py:161-185 Helix: 4 raster + 4 Bresenham-line directions", "csms6s.py:188-216")
CrossScan_Window, CrossMerge_Window = _make_scan_pair(
    "window", 4, "csms6s.py:113-129 window-partition scan (Hi-Fi branch)", "csms6s.py:132-152")
CrossScan_Dilation, CrossMerge_Dilation = _make_scan_pair(
    "dilation", 4, "csms6s.py:64-80 dilated scan, rate 4 (Lo-Fi branch)", "csms6s.py:83-103")
for _cls, _name in ((CrossScan, "CrossScan"), (CrossMerge, "CrossMerge"),
                    (CrossScan_Line, "CrossScan_Line"), (CrossMerge_Line, "CrossMerge_Line"),
                    (CrossScan_Window, "CrossScan_Window"), (CrossMerge_Window, "CrossMerge_Window"),
                    (CrossScan_Dilation, "CrossScan_Dilation"), (CrossMerge_Dilation, "CrossMerge_Dilation")):
    _cls.__name__ = _cls.__qualname__ = _name


def flops_selective_scan_fn(B=1, L=256, D=768, N=16, with_D=True, with_Z=False, with_complex=False):
    """FLOP model of the scan, same formula as csms6s.py:772-793 (9*B*L*D*N + B*D*L)."""
    assert not with_complex
    flops = 9 * B * L * D * N
    if with_D:
        flops += B * D * L
    if with_Z:
        flops += B * D * L
    return flops
