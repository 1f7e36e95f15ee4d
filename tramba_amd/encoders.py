"""Swin-B and PVTv2-b4 encoders of Tramba-S / Tramba-P (Trambav6_enc.py:167-192), state_dict-compatible with the
reference's Models/encoder/{swin_encoder,pvtv2_encoder}.py (so `swin_base_patch4_window12_384_22k.pth` /
`pvt_v2_b4.pth` and Tramba-S / Tramba-P checkpoints load by name).

Token-major throughout: a (B, H*W, C) token tensor IS a channels-last (B, H, W, C) map, which is what the
decoder's HIP kernels take -- the reference's reshape/permute/contiguous hand-offs disappear.  In inference the
LayerNorms, every Linear (bias, GELU and the residual add fused in the GEMM epilogue) and PVT's depth-wise 3x3 run on
the library's HIP kernels, and so does attention in 16-bit inference: the qkv / q / kv GEMMs run on the token map as it
lies and `hip.window_attention_cl` (Swin: cyclic shift, window gather, relative-position bias and shift mask by index
arithmetic in the kernel) or `hip.kv_attention_cl` (PVT: heads by stride) reads and writes it in place, so a block is
LayerNorm, GEMM, attention, GEMM (+ residual), LayerNorm, GEMM, GEMM with no framework op between.  fp32 inference,
shapes the kernels do not take (more than 256 keys, head dims other than 32 / 64) and, by default, everything with
autograd on keep the stock `scaled_dot_product_attention` path (`_forward_stock`), with Swin's bias and mask folded into
one cached additive mask per block.

Training on the library's attention is opt-in: `set_fused_attention_training(model)` (or `build(name, args)` with
`args.fused_attention_training`) puts every Swin / PVT block whose activations are 16-bit and whose shape the kernels
take on `_WindowAttnFn` / `_KvAttnFn` whenever autograd is needed.  Their forward is the inference entry, they save
only their inputs, and their backward (`hip.window_attention_bwd_cl` / `hip.kv_attention_bwd_cl`) recomputes the softmax
rows: no roll, window partition, mask or bias tensor exists on that path, and the fp32 relative-position table receives
its f32 gradient from the kernel.  The Linears and LayerNorms around the attention stay on the stock autograd ops.

The dense convolutions (PVT's patch embeddings and spatial-reduction convs, Swin's patch embedding) run on `F.conv2d`
unless `set_library_convolutions(model)` (or `build(name, args)` with `args.library_convolutions`) puts them on the
library in 16-bit inference: `hip.patch_embed_ln` reads the NCHW image and writes LayerNorm-ed tokens,
`hip.conv3x3s2_cl` and `hip.patch_conv_cl` read the channels-last token map as it lies.  With the switch on, a Tramba-P
forward calls no framework convolution and is bitwise reproducible.

The whole training path moves onto the library with `set_library_training(model)` (or `build(name, args)` with
`args.library_training`; off by default, and with it off nothing changes).  With autograd on and 16-bit activations every
Linear runs on `_LinearTrainCL`, every LayerNorm on `_LayerNormCL`, PVT's depth-wise 3x3 on `_DwConvCL` on the token map as
it lies, its spatial-reduction convs on `_PatchConvFn` (`hip.patch_conv_cl` forward, `hip.patch_conv_dgrad_cl` /
`hip.patch_conv_wgrad_cl` backward, csrc/patch_conv_bwd.hip), its 3x3 / stride-2 patch embeddings on `_ConvIm2colCL`, and the
first-layer embeddings on `_LinearTrainCL` over patch rows made by a framework data-movement op (the image needs no
gradient).  The switch implies the fused attention backward; a block the attention kernels do not take keeps stock SDPA
for the attention alone.  A 16-bit Tramba-S / -P training step at 384 x 384 then reaches `F.linear`, `F.layer_norm`,
`F.conv2d` and `F.scaled_dot_product_attention` zero times from this file and captures as one `GraphedTrainStep`.  GELU,
residual adds, drop-path and the per-call 16-bit casts of the weights stay framework element-wise ops.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip
from .modules import (DropPath, _cache, _ConvIm2colCL, _dwconv_train_cl, _f32, _infer, _LayerNormCL, _LinearTrainCL)

_LOWP = (torch.bfloat16, torch.float16)


def _lib_train(m, x):
    """`m` was switched by set_library_training() and `x` is a 16-bit device tensor (the callers have established that
    autograd is needed): the op runs on the library's autograd Functions"""
    return getattr(m, "library_training", False) and x.is_cuda and x.dtype in _LOWP


def _lin(m: nn.Linear, x, act=hip.ACT_NONE, residual=None):
    if _infer(x, m.weight):
        w = m.weight if m.weight.dtype == x.dtype else _cache(m).get(("w", x.dtype), (m.weight,), lambda: m.weight.to(x.dtype))
        return hip.linear_cl(x.contiguous(), w, None if m.bias is None else _f32(m.bias), residual, act)
    if _lib_train(m, x) and m.in_features % 8 == 0 and m.out_features % 8 == 0:
        y = _LinearTrainCL.apply(x, m.weight, m.bias)
    else:
        y = F.linear(x, m.weight.to(x.dtype), None if m.bias is None else m.bias.to(x.dtype))
    if act == hip.ACT_GELU:
        y = F.gelu(y)
    return y if residual is None else y + residual


def _ln(m: nn.LayerNorm, x):
    if _infer(x, m.weight):
        return hip.layernorm_cl(x.contiguous(), _f32(m.weight), _f32(m.bias), m.eps)
    if _lib_train(m, x) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048:
        return _LayerNormCL.apply(x, m.weight, m.bias, m.eps)
    return F.layer_norm(x.float(), m.normalized_shape, m.weight.float(), m.bias.float(), m.eps).to(x.dtype)


class _PatchConvFn(torch.autograd.Function):
    """hip.patch_conv_cl (kernel = stride = r on the channels-last map) with its backward on the library: x (B, H, W, Cin),
    w (Cout, Cin, r, r) and b (Cout) as the module holds them -> (B, H // r, W // r, Cout).  Saves x and the K-major 16-bit
    weight the forward read; the f32 weight gradient returns to the parameter's layout with one permute (a copy, so its
    slab sum cannot be deferred)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        wk = w.detach().to(x.dtype).permute(0, 2, 3, 1).contiguous()
        ctx.save_for_backward(x, wk)
        ctx.has_bias, ctx.wdtype = b is not None, w.dtype
        return hip.patch_conv_cl(x, wk, None if b is None else b.detach().float().contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, wk = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = hip.patch_conv_dgrad_cl(gy, wk, x.shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = hip.patch_conv_wgrad_cl(gy, x, wk.shape[1], want_bias=ctx.has_bias)
            gw = gw.permute(0, 3, 1, 2).contiguous().to(ctx.wdtype)          # back to (Cout, Cin, r, r)
        return gx, gw, gb


def _embed_rows_train(proj: nn.Conv2d, x):
    """First-layer patch embedding on the training path: the image needs no gradient, so the patch rows are made by a
    framework data-movement op (a permute copy for kernel = stride, F.unfold otherwise) and the product and its weight
    gradient run on `_LinearTrainCL`, K padded to a multiple of 8.  x (B, 3, H, W) -> ((B, Ho * Wo, Cout), Ho, Wo)."""
    b, c, h, w = x.shape
    k, st, pd = proj.kernel_size[0], proj.stride[0], proj.padding[0]
    ho, wo = (h + 2 * pd - k) // st + 1, (w + 2 * pd - k) // st + 1
    if k == st and pd == 0:
        rows = x[:, :, :ho * k, :wo * k].reshape(b, c, ho, k, wo, k).permute(0, 2, 4, 1, 3, 5).reshape(b, ho * wo, c * k * k)
    else:
        rows = F.unfold(x, k, padding=pd, stride=st).transpose(1, 2)          # columns (c, ky, kx): the weight's own order
    # cast first: a 16-bit weight keeps _LinearTrainCL from deferring the slab sum of a gradient that the reshape / pad
    # backward below it reads; the gradient then returns to f32 through the cast's backward, as on the F.conv2d path
    w2 = proj.weight.to(x.dtype).reshape(proj.out_channels, -1)
    pad = -w2.shape[1] % 8
    if pad:
        rows, w2 = F.pad(rows, (0, pad)), F.pad(w2, (0, pad))
    return _LinearTrainCL.apply(rows.contiguous(), w2, proj.bias), ho, wo


def _embed_rows_ok(m, proj: nn.Conv2d, x):
    return (_lib_train(m, x) and not _infer(x, proj.weight) and not x.requires_grad and proj.groups == 1
            and proj.kernel_size[0] == proj.kernel_size[1] and proj.stride[0] == proj.stride[1]
            and proj.padding[0] == proj.padding[1] and proj.out_channels % 8 == 0)


class _WindowAttnFn(torch.autograd.Function):
    """hip.window_attention_cl with its backward on the library: saves (qkv, table), nothing of the softmax."""

    @staticmethod
    def forward(ctx, qkv, table, ws, shift, heads):
        qkv, table = qkv.contiguous(), table.contiguous()
        ctx.save_for_backward(qkv, table)
        ctx.geom = (ws, shift, heads)
        return hip.window_attention_cl(qkv, table, ws, shift, heads)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        qkv, table = ctx.saved_tensors
        ws, shift, heads = ctx.geom
        dqkv, dtable = hip.window_attention_bwd_cl(qkv, table, dy.contiguous(), ws, shift, heads,
                                                   need_table=ctx.needs_input_grad[1])
        return dqkv, dtable, None, None, None


class _KvAttnFn(torch.autograd.Function):
    """hip.kv_attention_cl with its backward on the library: saves (q, kv)."""

    @staticmethod
    def forward(ctx, q, kv, heads):
        q, kv = q.contiguous(), kv.contiguous()
        ctx.save_for_backward(q, kv)
        ctx.heads = heads
        return hip.kv_attention_cl(q, kv, heads)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        q, kv = ctx.saved_tensors
        dq, dkv = hip.kv_attention_bwd_cl(q, kv, dy.contiguous(), ctx.heads)
        return dq, dkv, None


def set_fused_attention_training(model, enabled=True):
    """Put the Swin / PVT blocks of `model` on the library's attention backward in 16-bit training (off by default).
    Returns the number of blocks switched.  A block still keeps the stock path for fp32 activations, for shapes the
    kernels do not take and when no autograd graph is needed."""
    count = 0
    for m in model.modules():
        if isinstance(m, (SwinTransformerBlock, _PvtAttention)):
            m.fused_attention_training = bool(enabled)
            count += 1
    return count


def set_library_training(model, enabled=True):
    """Put the training path of the Swin / PVT encoder of `model` on the library (off by default): with autograd on and
    16-bit activations every Linear and LayerNorm runs on `_LinearTrainCL` / `_LayerNormCL`, PVT's depth-wise 3x3 on
    `_DwConvCL`, its spatial-reduction convs on `_PatchConvFn`, its 3x3 / stride-2 patch embeddings on `_ConvIm2colCL`,
    the first-layer embeddings on `_LinearTrainCL` over framework-made patch rows, and attention on `_WindowAttnFn` /
    `_KvAttnFn` wherever the kernels take the shape (the switch implies `set_fused_attention_training`; a block they do
    not take keeps stock SDPA for the attention alone).  fp32 activations and inference are untouched.  Returns the
    number of modules switched.

    A Tramba-R model's `ResNet` encoder and each of its 16 `Bottleneck`s count as one module each (17).  In train mode, with
    16-bit activations and autograd on, `ResNet.features_cl` then runs conv1 as patch rows on `_LinearTrainCL`, every batch
    norm of the stem and layer1..3 on batch statistics (`hip.bn_stats_cl`, which updates the running buffers in place on the
    device, + `hip.bn_act_cl`), every bottleneck convolution as the raw `hip.conv_affine_cl` and the pool on
    `hip.maxpool3s2_cl`, each with its backward on the library (resnet_train).  `layer4`, which the decoder never
    reads, is not run: its parameters get no gradient on either path, but its running statistics and num_batches_tracked
    stay as they were, the one intended difference from the stock step.  fp32 activations, eval mode, a batch norm with
    track_running_stats=False or momentum=None and a dilated convolution keep the stock path."""
    from .models import Bottleneck, ResNet
    count, seen = 0, set()
    for m in model.modules():
        if isinstance(m, (ResNet, Bottleneck)):
            m.library_training = bool(enabled)
            count += 1
            continue
        if isinstance(m, _LIBRARY_TRAINING_KINDS):
            for sub in (m, *m.children()):
                if id(sub) not in seen and (sub is m or isinstance(sub, (nn.Linear, nn.LayerNorm, nn.Conv2d))):
                    seen.add(id(sub))
                    sub.library_training = bool(enabled)
                    count += 1
    return count


def set_library_convolutions(model, enabled=True):
    """Put the dense convolutions of the Swin / PVT encoder of `model` on the library in 16-bit inference (off by default):
    PVT's spatial-reduction convs (`hip.patch_conv_cl`), its patch embeddings (`hip.patch_embed_ln` on the image,
    `hip.conv3x3s2_cl` on the channels-last maps) and Swin's patch embedding (`hip.patch_embed_ln`).  Returns the number of
    modules switched.  A module still calls `_conv` for fp32 activations, with autograd on and for shapes the kernels do
    not take.  A Tramba-R model's `ResNet` encoder counts as one module: its stem runs on `hip.stem7_affine_relu_pool` and
    the bottlenecks of layer1..3 on `hip.conv_affine_cl` (models.ResNet.features_cl)."""
    from .models import ResNet
    count = 0
    for m in model.modules():
        if isinstance(m, (_OverlapPatchEmbed, _SwinPatchEmbed, ResNet)) or (isinstance(m, _PvtAttention) and m.sr_ratio > 1):
            m.library_convolutions = bool(enabled)
            count += 1
    return count


def _lowp_infer(x, *params):
    """16-bit activations and no autograd graph: what every library convolution needs"""
    return x.dtype in (torch.bfloat16, torch.float16) and _infer(x, *params)


def _conv_params(m: nn.Conv2d, dtype, kmajor):
    """(weight, bias) of a conv as the library reads them, derived from the module's own (after prepare_inference: rounded)
    tensors so that both paths multiply the same numbers: the weight K-major (Cout, kh, kw, Cin) in `dtype`, or in the
    reference layout in f32; the bias in f32."""
    def make():
        w = m.weight.detach()
        w = w.to(dtype).permute(0, 2, 3, 1).contiguous() if kmajor else w.float().contiguous()
        return w, None if m.bias is None else m.bias.detach().float().contiguous()
    return _cache(m).get(("libconv", dtype, kmajor), (m.weight, m.bias), make)


def _patch_embed_ln(proj: nn.Conv2d, norm: nn.LayerNorm, x):
    w, b = _conv_params(proj, x.dtype, kmajor=False)
    return hip.patch_embed_ln(x.contiguous(), w, b, _f32(norm.weight), _f32(norm.bias), norm.eps, proj.stride[0],
                              proj.padding[0], x.dtype)


def _patch_embed_ln_ok(proj: nn.Conv2d, norm: nn.LayerNorm, x):
    return (_lowp_infer(x, proj.weight, norm.weight) and proj.bias is not None and proj.in_channels == 3
            and proj.kernel_size[0] == proj.kernel_size[1] and proj.stride[0] == proj.stride[1]
            and proj.padding[0] == proj.padding[1] and tuple(norm.normalized_shape) == (proj.out_channels,)
            and hip.patch_embed_ln_supported(x.dtype, proj.kernel_size[0], proj.stride[0], proj.padding[0], proj.out_channels))


def _conv(m: nn.Conv2d, x):
    return F.conv2d(x, m.weight.to(x.dtype), None if m.bias is None else m.bias.to(x.dtype), m.stride, m.padding, 1, m.groups)


def _init_linear_ln(m):
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif isinstance(m, nn.LayerNorm):
        nn.init.ones_(m.weight)
        nn.init.zeros_(m.bias)


# ============================================================================= PVTv2 (pvtv2_encoder.py)
class _PvtDW(nn.Module):
    """pvtv2_encoder.py:373-384 (`mlp.dwconv.dwconv`): depth-wise 3x3 with bias on the token map."""

    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)


class _PvtMlp(nn.Module):
    """pvtv2_encoder.py:19-54: fc1 -> dw3x3 -> GELU -> fc2."""

    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.dwconv = _PvtDW(hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x, h, w, residual=None):
        b, n, _ = x.shape
        y = _lin(self.fc1, x)
        conv = self.dwconv.dwconv
        if _infer(y, conv.weight):
            taps = _cache(self).get("taps", (conv.weight,), lambda: conv.weight.detach().float().reshape(-1, 9).t().contiguous())
            y = hip.dwconv_cl(y.view(b, h, w, -1), taps, _f32(conv.bias), hip.ACT_GELU).view(b, n, -1)
        elif _lib_train(conv, y):
            y = F.gelu(_dwconv_train_cl(y.view(b, h, w, -1), conv).view(b, n, -1))     # on the token map as it lies
        else:
            y = _conv(conv, y.transpose(1, 2).reshape(b, -1, h, w)).flatten(2).transpose(1, 2)
            y = F.gelu(y)
        return _lin(self.fc2, y, residual=residual)


class _PvtAttention(nn.Module):
    """pvtv2_encoder.py:57-116: spatial-reduction attention (keys / values from an sr x sr strided conv of the map)."""

    fused_attention_training = False       # set_fused_attention_training(); no parameter, not in the state_dict
    library_convolutions = False           # set_library_convolutions(); likewise
    library_training = False               # set_library_training(); likewise (implies fused_attention_training)

    def __init__(self, dim, num_heads, qkv_bias, sr_ratio):
        super().__init__()
        assert dim % num_heads == 0
        self.dim, self.num_heads, self.sr_ratio = dim, num_heads, sr_ratio
        self.scale = (dim // num_heads) ** -0.5
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        if sr_ratio > 1:
            self.sr = nn.Conv2d(dim, dim, kernel_size=sr_ratio, stride=sr_ratio)
            self.norm = nn.LayerNorm(dim)

    def forward(self, x, h, w, residual=None):
        b, n, c = x.shape
        m = (h // self.sr_ratio) * (w // self.sr_ratio) if self.sr_ratio > 1 else n
        infer = _infer(x, self.q.weight)
        train = ((self.fused_attention_training or self.library_training) and not infer
                 and hip.kv_attention_train_supported(x.dtype, m, c, self.num_heads))
        if not train and not (infer and hip.kv_attention_supported(x.dtype, m, c, self.num_heads)):
            return self._forward_stock(x, h, w, residual)
        q = _lin(self.q, x)
        if self.sr_ratio > 1:
            xr = _ln(self.norm, self._reduce(x, h, w))
        else:
            xr = x
        if train:
            o = _KvAttnFn.apply(q, _lin(self.kv, xr), self.num_heads)
        else:
            o = hip.kv_attention_cl(q, _lin(self.kv, xr), self.num_heads)   # heads by stride: no view / permute copies
        return _lin(self.proj, o, residual=residual)

    def _reduce(self, x, h, w):
        """the sr x sr / stride sr conv of the token map -> (B, M, C) tokens"""
        b, n, c = x.shape
        if (self.library_convolutions and _lowp_infer(x, self.sr.weight)
                and hip.patch_conv_supported(x.dtype, c, c, self.sr_ratio)):
            wk, bias = _conv_params(self.sr, x.dtype, kmajor=True)    # kernel = stride: a patch GEMM on the map as it lies
            return hip.patch_conv_cl(x.contiguous().view(b, h, w, c), wk, bias).view(b, -1, c)
        if self._reduce_on_library(x):
            return _PatchConvFn.apply(x.contiguous().view(b, h, w, c), self.sr.weight, self.sr.bias).view(b, -1, c)
        return _conv(self.sr, x.transpose(1, 2).reshape(b, c, h, w)).flatten(2).transpose(1, 2)

    def _reduce_on_library(self, x):
        """training with the switch on: the sr conv and its backward run on the library"""
        return (_lib_train(self, x) and not _infer(x, self.sr.weight)
                and hip.patch_conv_train_supported(x.dtype, x.shape[-1], self.sr.out_channels, self.sr_ratio))

    def _forward_stock(self, x, h, w, residual=None):
        """stock torch attention: fp32, autograd on, or a key count the library does not take (e.g. 576 keys at 768x768)"""
        b, n, c = x.shape
        nh = self.num_heads
        q = _lin(self.q, x).view(b, n, nh, c // nh).transpose(1, 2)
        if self.sr_ratio > 1:
            if self._reduce_on_library(x):
                xr = self._reduce(x, h, w)
            else:
                xr = _conv(self.sr, x.transpose(1, 2).reshape(b, c, h, w)).flatten(2).transpose(1, 2)
            xr = _ln(self.norm, xr)
        else:
            xr = x
        kv = _lin(self.kv, xr).view(b, -1, 2, nh, c // nh).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, kv[0], kv[1], scale=self.scale)
        return _lin(self.proj, o.transpose(1, 2).reshape(b, n, c), residual=residual)


class _PvtBlock(nn.Module):
    """pvtv2_encoder.py:119-156."""

    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, drop_path, sr_ratio, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = _PvtAttention(dim, num_heads, qkv_bias, sr_ratio)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _PvtMlp(dim, int(dim * mlp_ratio))

    def forward(self, x, h, w):
        if not self.training:                      # drop_path is the identity: residual adds ride in the GEMM epilogues
            x = self.attn(_ln(self.norm1, x), h, w, residual=x)
            return self.mlp(_ln(self.norm2, x), h, w, residual=x)
        x = x + self.drop_path(self.attn(_ln(self.norm1, x), h, w))
        return x + self.drop_path(self.mlp(_ln(self.norm2, x), h, w))


class _OverlapPatchEmbed(nn.Module):
    """pvtv2_encoder.py:159-199: overlapping strided conv + LayerNorm -> tokens."""

    def __init__(self, patch, stride, cin, dim):
        super().__init__()
        self.proj = nn.Conv2d(cin, dim, kernel_size=patch, stride=stride, padding=patch // 2)
        self.norm = nn.LayerNorm(dim)

    library_convolutions = False           # set_library_convolutions(); no parameter, not in the state_dict
    library_training = False               # set_library_training(); likewise

    def forward(self, x, channels_last=False):
        """x: the NCHW image or map; channels_last: x is the previous stage's (B, H, W, C) map instead"""
        proj = self.proj
        if self.library_convolutions:
            if not channels_last and _patch_embed_ln_ok(proj, self.norm, x):
                y = _patch_embed_ln(proj, self.norm, x)                 # conv + bias + LayerNorm, one rounding
                b, h, w, c = y.shape
                return y.view(b, h * w, c), h, w
            if (channels_last and _lowp_infer(x, proj.weight) and proj.kernel_size == (3, 3) and proj.stride == (2, 2)
                    and proj.padding == (1, 1) and proj.in_channels % 64 == 0 and proj.out_channels % 8 == 0):
                wk, bias = _conv_params(proj, x.dtype, kmajor=True)
                y = hip.conv3x3s2_cl(x.contiguous(), wk.view(proj.out_channels, -1), bias)
                b, h, w, c = y.shape
                return _ln(self.norm, y.view(b, h * w, c)), h, w
        if not channels_last and _embed_rows_ok(self, proj, x):
            y, h, w = _embed_rows_train(proj, x)                        # patch rows by F.unfold, product on the library
            return _ln(self.norm, y), h, w
        if (channels_last and _lib_train(self, x) and not _infer(x, proj.weight) and proj.kernel_size == (3, 3)
                and proj.stride[0] == proj.stride[1] and proj.padding[0] == proj.padding[1] and proj.in_channels % 8 == 0
                and proj.out_channels % 8 == 0):
            y = _ConvIm2colCL.apply(x.contiguous(), proj.weight, proj.bias, proj.stride, proj.padding)
            b, h, w, c = y.shape
            return _ln(self.norm, y.view(b, h * w, c)), h, w
        if channels_last:
            x = x.permute(0, 3, 1, 2)                                   # the strided conv reads NCHW (a view)
        x = _conv(proj, x)
        h, w = x.shape[-2:]
        return _ln(self.norm, x.flatten(2).transpose(1, 2)), h, w


class PyramidVisionTransformerImpr(nn.Module):
    """pvtv2_encoder.py:202-366.  forward(x) -> [stage4, stage3, stage2, stage1] NCHW maps (deepest first, :358)."""

    def __init__(self, embed_dims=(64, 128, 256, 512), num_heads=(1, 2, 4, 8), mlp_ratios=(4, 4, 4, 4), qkv_bias=False,
                 drop_path_rate=0.0, depths=(3, 4, 6, 3), sr_ratios=(8, 4, 2, 1), eps=1e-5, in_chans=3):
        super().__init__()
        self.depths = list(depths)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for s in range(4):
            embed = _OverlapPatchEmbed(7 if s == 0 else 3, 4 if s == 0 else 2, in_chans if s == 0 else embed_dims[s - 1],
                                       embed_dims[s])
            blocks = nn.ModuleList([_PvtBlock(embed_dims[s], num_heads[s], mlp_ratios[s], qkv_bias, dpr[cur + i], sr_ratios[s],
                                              eps) for i in range(depths[s])])
            cur += depths[s]
            setattr(self, f"patch_embed{s + 1}", embed)
            setattr(self, f"block{s + 1}", blocks)
            setattr(self, f"norm{s + 1}", nn.LayerNorm(embed_dims[s], eps=eps))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        _init_linear_ln(m)
        if isinstance(m, nn.Conv2d):                                    # pvtv2_encoder.py:269-274
            fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
            m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
            if m.bias is not None:
                m.bias.data.zero_()

    def features_cl(self, x):
        """[(B, H, W, C) channels-last map per stage], shallow first."""
        outs = []
        b = x.shape[0]
        for s in range(1, 5):
            x, h, w = getattr(self, f"patch_embed{s}")(x, channels_last=s > 1)
            for blk in getattr(self, f"block{s}"):
                x = blk(x, h, w)
            x = _ln(getattr(self, f"norm{s}"), x)
            outs.append(x.view(b, h, w, -1))
            x = outs[-1]
        return outs

    def forward(self, x):
        return [o.permute(0, 3, 1, 2).contiguous() for o in self.features_cl(x)][::-1]


def pvt_v2_b4():
    """pvtv2_encoder.py:433-439."""
    return PyramidVisionTransformerImpr(embed_dims=(64, 128, 320, 512), num_heads=(1, 2, 5, 8), mlp_ratios=(8, 8, 4, 4),
                                        qkv_bias=True, eps=1e-6, depths=(3, 8, 27, 3), sr_ratios=(8, 4, 2, 1),
                                        drop_path_rate=0.1)


# ============================================================================= Swin (swin_encoder.py)
def _windows(x, ws):
    """(B, H, W, C) -> (B, nW, ws*ws, C)   (swin_encoder.py:36-48, batch kept as its own axis)"""
    b, h, w, c = x.shape
    return x.view(b, h // ws, ws, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, (h // ws) * (w // ws), ws * ws, c)


def _unwindows(xw, ws, h, w):
    """inverse of _windows (swin_encoder.py:51-65)"""
    b = xw.shape[0]
    return xw.view(b, h // ws, w // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, -1)


class _WindowAttention(nn.Module):
    """swin_encoder.py:68-147: window attention with a learned relative-position bias."""

    def __init__(self, dim, ws, num_heads, qkv_bias=True):
        super().__init__()
        self.dim, self.ws, self.num_heads = dim, ws, num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        ar = torch.arange(ws)
        coords = torch.stack(torch.meshgrid(ar, ar, indexing="ij")).flatten(1)             # (2, ws*ws)
        rel = coords[:, :, None] - coords[:, None, :] + (ws - 1)                           # (2, N, N), each in [0, 2ws-2]
        self.register_buffer("relative_position_index", rel[0] * (2 * ws - 1) + rel[1])
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def bias_mask(self, shift_mask, dtype):
        """(1, 1 or nW, nH, N, N) additive term: relative-position bias (+ the shifted-window mask)"""
        def build():
            n = self.ws * self.ws
            bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1)
            bias = bias.permute(2, 0, 1)[None, None].float()                                # (1, 1, nH, N, N)
            if shift_mask is not None:
                bias = bias + shift_mask[None, :, None].float()                            # (1, nW, nH, N, N)
            return bias.to(dtype).contiguous()
        if _infer(self.relative_position_bias_table):
            return _cache(self).get(("bias", dtype), (self.relative_position_bias_table,), build)
        return build()

    def forward(self, xw, shift_mask):
        b, nw, n, c = xw.shape
        nh = self.num_heads
        qkv = _lin(self.qkv, xw).view(b, nw, n, 3, nh, c // nh).permute(3, 0, 1, 4, 2, 5)   # (3, B, nW, nH, N, hd)
        o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=self.bias_mask(shift_mask, xw.dtype),
                                           scale=self.scale)
        return _lin(self.proj, o.transpose(2, 3).reshape(b, nw, n, c))


class _SwinMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x, residual=None):
        return _lin(self.fc2, _lin(self.fc1, x, act=hip.ACT_GELU), residual=residual)


class SwinTransformerBlock(nn.Module):
    """swin_encoder.py:166-273."""
    fused_attention_training = False       # set_fused_attention_training(); no parameter, not in the state_dict
    library_training = False               # set_library_training(); likewise (implies fused_attention_training)

    def __init__(self, dim, input_resolution, num_heads, window_size, shift_size, mlp_ratio, drop_path):
        super().__init__()
        self.input_resolution = input_resolution
        if min(input_resolution) <= window_size:          # one window covers the map: no partition, no shift (:197-200)
            shift_size, window_size = 0, min(input_resolution)
        self.window_size, self.shift_size = window_size, shift_size
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, window_size, num_heads)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _SwinMlp(dim, int(dim * mlp_ratio))
        mask = None
        if shift_size > 0:                                 # regions that wrap around under the cyclic shift (:213-232)
            h, w = input_resolution
            region = torch.zeros(1, h, w, 1)
            cuts = (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None))
            for i, hs in enumerate(cuts):
                for j, wsl in enumerate(cuts):
                    region[:, hs, wsl, :] = i * 3 + j
            ids = _windows(region, window_size)[0, :, :, 0]                                 # (nW, N)
            diff = ids[:, None, :] - ids[:, :, None]
            mask = torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))
        self.register_buffer("attn_mask", mask)

    def forward(self, x):
        h, w = self.input_resolution
        b, l, c = x.shape
        ws, sh, attn = self.window_size, self.shift_size, self.attn
        if ((self.fused_attention_training or self.library_training)
                and not _infer(x, attn.qkv.weight, attn.relative_position_bias_table)
                and hip.window_attention_train_supported(x.dtype, h, w, c, attn.num_heads, ws, sh)):
            return self._forward_fused_train(x)
        if self.training or not (_infer(x, attn.qkv.weight)
                                 and hip.window_attention_supported(x.dtype, h, w, c, attn.num_heads, ws, sh)):
            return self._forward_stock(x)
        # qkv and proj are per-token: they run on the map as it lies, and the kernel gathers its windows through the shift
        qkv = _lin(attn.qkv, _ln(self.norm1, x)).view(b, h, w, 3 * c)
        y = hip.window_attention_cl(qkv, _f32(attn.relative_position_bias_table), ws, sh, attn.num_heads)
        x = _lin(attn.proj, y.view(b, l, c), residual=x)
        return self.mlp(_ln(self.norm2, x), residual=x)

    def _forward_fused_train(self, x):
        """autograd on, 16-bit: the library's attention forward and backward on the unpermuted map (no roll, partition,
        mask or bias tensor); proj, drop_path and the residuals as in `_forward_stock`"""
        h, w = self.input_resolution
        b, l, c = x.shape
        attn = self.attn
        qkv = _lin(attn.qkv, _ln(self.norm1, x)).view(b, h, w, 3 * c)
        y = _WindowAttnFn.apply(qkv, attn.relative_position_bias_table.float(), self.window_size, self.shift_size,
                                attn.num_heads)
        y = _lin(attn.proj, y.view(b, l, c))
        if not self.training:
            x = x + y
            return self.mlp(_ln(self.norm2, x), residual=x)
        x = x + self.drop_path(y)
        return x + self.drop_path(self.mlp(_ln(self.norm2, x)))

    def _forward_stock(self, x):
        """stock torch attention on rolled / partitioned copies: training, fp32, or a shape the library does not take"""
        h, w = self.input_resolution
        b, l, c = x.shape
        ws, sh = self.window_size, self.shift_size
        y = _ln(self.norm1, x).view(b, h, w, c)
        if sh > 0:
            y = torch.roll(y, shifts=(-sh, -sh), dims=(1, 2))
        y = _unwindows(self.attn(_windows(y, ws), self.attn_mask), ws, h, w)
        if sh > 0:
            y = torch.roll(y, shifts=(sh, sh), dims=(1, 2))
        y = y.reshape(b, l, c)
        if not self.training:
            x = x + y
            return self.mlp(_ln(self.norm2, x), residual=x)
        x = x + self.drop_path(y)
        return x + self.drop_path(self.mlp(_ln(self.norm2, x)))


class PatchMerging(nn.Module):
    """swin_encoder.py:294-331: 2x2 neighbours -> 4C channels -> LayerNorm -> Linear(4C, 2C)."""

    def __init__(self, input_resolution, dim):
        super().__init__()
        self.input_resolution = input_resolution
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    def forward(self, x):
        h, w = self.input_resolution
        b, l, c = x.shape
        x = x.view(b, h // 2, 2, w // 2, 2, c)
        # channel order of the reference's cat([x0, x1, x2, x3]): (row parity, col parity) = (0,0), (1,0), (0,1), (1,1)
        x = x.permute(0, 1, 3, 4, 2, 5).reshape(b, (h // 2) * (w // 2), 4 * c)
        return _lin(self.reduction, _ln(self.norm, x))


class BasicLayer(nn.Module):
    """swin_encoder.py:343-399."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, drop_path, downsample):
        super().__init__()
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2,
                                 mlp_ratio, drop_path[i]) for i in range(depth)])
        self.downsample = PatchMerging(input_resolution, dim) if downsample else None

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return x if self.downsample is None else self.downsample(x)


class _SwinPatchEmbed(nn.Module):
    """swin_encoder.py:413-450."""

    def __init__(self, img_size, patch, cin, dim):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patches_resolution = [img_size // patch, img_size // patch]
        self.proj = nn.Conv2d(cin, dim, kernel_size=patch, stride=patch)
        self.norm = nn.LayerNorm(dim)

    library_convolutions = False           # set_library_convolutions(); no parameter, not in the state_dict
    library_training = False               # set_library_training(); likewise

    def forward(self, x):
        if tuple(x.shape[-2:]) != self.img_size:
            raise RuntimeError(f"Input image size {tuple(x.shape[-2:])} doesn't match model {self.img_size}")
        if self.library_convolutions and _patch_embed_ln_ok(self.proj, self.norm, x):
            return _patch_embed_ln(self.proj, self.norm, x).flatten(1, 2)
        if _embed_rows_ok(self, self.proj, x):
            return _ln(self.norm, _embed_rows_train(self.proj, x)[0])  # patch rows by a permute copy, product on the library
        return _ln(self.norm, _conv(self.proj, x).flatten(2).transpose(1, 2))


class SwinTransformer(nn.Module):
    """swin_encoder.py:461-594.  forward(x) -> [layer3 out, layer2 out, layer1 out, layer0 out, patch embedding] as NCHW
    maps (deepest first, :590-594); Tramba-S uses all but the first (Trambav6_enc.py:210-211), so `features_cl(x,
    last=False)` skips the last stage's blocks, whose output nothing reads."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 window_size=7, mlp_ratio=4.0, drop_path_rate=0.1):
        super().__init__()
        self.num_layers = len(depths)
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        self.patch_embed = _SwinPatchEmbed(img_size, patch_size, in_chans, embed_dim)
        res = self.patch_embed.patches_resolution
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([
            BasicLayer(int(embed_dim * 2 ** i), (res[0] // 2 ** i, res[1] // 2 ** i), depths[i], num_heads[i], window_size,
                       mlp_ratio, dpr[sum(depths[:i]):sum(depths[:i + 1])], downsample=i < self.num_layers - 1)
            for i in range(self.num_layers)])
        self.apply(_init_linear_ln)

    def features_cl(self, x, last=True):
        """[(B, H, W, C)] shallow first: patch embedding, then each layer's output (after its PatchMerging)."""
        b = x.shape[0]
        x = self.patch_embed(x)
        feats = []
        for i, layer in enumerate(self.layers):
            side = int(round(math.sqrt(x.shape[1])))
            feats.append(x.view(b, side, side, -1))
            if i == self.num_layers - 1 and not last:
                return feats
            x = layer(x)
        side = int(round(math.sqrt(x.shape[1])))
        feats.append(x.view(b, side, side, -1))
        return feats

    def forward(self, x):
        return [f.permute(0, 3, 1, 2).contiguous() for f in self.features_cl(x)][::-1]


# the module kinds set_library_training() flags, together with their direct Linear / LayerNorm / Conv2d children
_LIBRARY_TRAINING_KINDS = (_PvtDW, _PvtMlp, _PvtAttention, _PvtBlock, _OverlapPatchEmbed, PyramidVisionTransformerImpr,
                           _WindowAttention, _SwinMlp, SwinTransformerBlock, PatchMerging, _SwinPatchEmbed, SwinTransformer)
