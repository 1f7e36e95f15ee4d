"""Training path of the ResNet-50 encoder (Tramba-R) on the library: the autograd Functions behind
`encoders.set_library_training` and the bottleneck / stem built from them (resnet_encoder.py:62-110 under `model.train()`,
train.py:33,296: batch statistics, running buffers updated every step).

All maps are channels-last (B, H, W, C) in bf16 / fp16; parameters stay as the model holds them (fp32 masters), gradients
return in the parameter's layout and dtype.

    _ConvCL           raw convolution `hip.conv_affine_cl` (no scale / shift / ReLU: what the stock path hands its batch norm);
                      backward `hip.conv_dgrad_cl` / `hip.conv_wgrad_cl` (csrc/resnet_conv.hip)
    _BatchNormActCL   act(batch_norm(x) + residual) on batch statistics: `hip.bn_stats_cl` (which updates the running buffers
                      in place on the device) + `hip.bn_act_cl`; backward `hip.bn_act_bwd_cl` (csrc/batchnorm.hip)
    _MaxPoolCL        max_pool2d(3, 2, 1): `hip.maxpool3s2_cl` / `hip.maxpool3s2_bwd_cl`

Each op asks its predicate first; a refused shape runs the stock op on views for that op alone.  No atomics anywhere: a
training step on this path repeats bit for bit.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip
from .modules import from_cl, to_cl

_LOWP = (torch.bfloat16, torch.float16)


class _ConvCL(torch.autograd.Function):
    """x (B, H, W, Cin), w (Cout, Cin, k, k) as the module holds it -> the raw convolution (B, Ho, Wo, Cout), pad = k // 2.
    Saves x and the K-major 16-bit weight the forward read; the f32 weight gradient returns to the parameter's layout and
    dtype with one permute (a copy, so its slab sum cannot be deferred)."""

    @staticmethod
    def forward(ctx, x, w, stride):
        x = x.contiguous()
        wk = w.detach().to(x.dtype).permute(0, 2, 3, 1).contiguous()
        ctx.save_for_backward(x, wk)
        ctx.stride, ctx.wdtype = stride, w.dtype
        return hip.conv_affine_cl(x, wk, None, None, None, False, ksize=wk.shape[1], stride=stride)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, wk = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = hip.conv_dgrad_cl(gy, hip.conv_transposed_weight(wk), x.shape, ctx.stride)
        if ctx.needs_input_grad[1]:
            gw = hip.conv_wgrad_cl(gy, x, wk.shape[1], ctx.stride)
            gw = gw.permute(0, 3, 1, 2).contiguous().to(ctx.wdtype)          # back to (Cout, Cin, k, k)
        return gx, gw, None


class _BatchNormActCL(torch.autograd.Function):
    """act(gamma (x - mean) rstd + beta + residual) with the batch statistics of x.  running_mean / running_var are no
    autograd inputs: the statistics kernel updates them in place (None: no update).  They are not marked dirty: autograd
    wants a dirty tensor returned as an output, and these are module buffers outside the graph that nothing saves.  Saves x,
    the statistics and, for the ReLU mask alone, y."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, eps, momentum, relu):
        x = x.contiguous()
        residual = None if residual is None else residual.contiguous()
        mean, rstd = hip.bn_stats_cl(x, eps, running_mean, running_var, momentum)
        g32 = None if gamma is None else gamma.detach().float().contiguous()
        b32 = None if beta is None else beta.detach().float().contiguous()
        y = hip.bn_act_cl(x, mean, rstd, g32, b32, residual, relu)
        ctx.save_for_backward(x, y if relu else None, mean, rstd, g32)
        ctx.relu = bool(relu)
        ctx.dtypes = (None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, mean, rstd, g32 = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        need = ctx.needs_input_grad
        dx, dres, dgamma, dbeta = hip.bn_act_bwd_cl(dy, x, y, mean, rstd, g32, ctx.relu, want_dres=need[3],
                                                    want_affine=need[1] or need[2])
        dgamma = dgamma.to(ctx.dtypes[0]) if need[1] else None
        dbeta = dbeta.to(ctx.dtypes[1]) if need[2] else None
        return (dx if need[0] else None), dgamma, dbeta, dres, None, None, None, None, None


class _MaxPoolCL(torch.autograd.Function):
    """max_pool2d(3, 2, 1) on a channels-last map; saves the input, from which the backward recomputes the arg-max"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return hip.maxpool3s2_cl(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        return hip.maxpool3s2_bwd_cl(gy if gy.dtype == x.dtype else gy.to(x.dtype), x)


def conv_ok(conv: nn.Conv2d, x):
    """can _ConvCL take this convolution on this channels-last map?"""
    k, s = conv.kernel_size[0], conv.stride[0]
    return (conv.bias is None and conv.groups == 1 and conv.dilation == (1, 1) and conv.kernel_size == (k, k)
            and conv.stride == (s, s) and conv.padding == (k // 2, k // 2) and conv.padding_mode == "zeros"
            and x.shape[0] * x.shape[1] * x.shape[2] * max(conv.in_channels, conv.out_channels) * 2 < 2 ** 31
            and hip.conv_train_supported(x.dtype, x.shape[1], x.shape[2], conv.in_channels, conv.out_channels, k, s))


def bn_ok(bn: nn.BatchNorm2d, x):
    """can _BatchNormActCL take this batch norm on this channels-last map?  (A norm without running statistics or with a
    cumulative average never reaches this path: see `block_trainable`.)"""
    return hip.bn_supported(x.dtype, x.numel() // x.shape[-1], x.shape[-1])


def conv_cl(conv: nn.Conv2d, x):
    """the raw convolution of a channels-last map under autograd: one library launch, or F.conv2d on views"""
    if conv_ok(conv, x):
        return _ConvCL.apply(x, conv.weight, conv.stride[0])
    return to_cl(F.conv2d(from_cl(x), conv.weight.to(x.dtype), None, conv.stride, conv.padding, conv.dilation, conv.groups))


def bn_act_cl(bn: nn.BatchNorm2d, x, residual=None, relu=True):
    """act(bn(x) + residual) in training mode on a channels-last map: statistics (with the running-buffer update) and
    normalisation on the library, or F.batch_norm on views.  num_batches_tracked advances by a framework in-place add."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if bn_ok(bn, x):
        return _BatchNormActCL.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu)
    # (in the dtype of the running buffers -- f32 masters -- as the fp32 stock forward runs it: one dtype for every operand)
    cd = bn.running_mean.dtype
    y = F.batch_norm(from_cl(x).to(cd), bn.running_mean, bn.running_var, None if bn.weight is None else bn.weight.to(cd),
                     None if bn.bias is None else bn.bias.to(cd), True, bn.momentum, bn.eps)
    if residual is not None:
        y = y + from_cl(residual).to(cd)
    return to_cl(F.relu(y) if relu else y).to(x.dtype)


def maxpool_cl(x):
    """max_pool2d(3, 2, 1) of a channels-last map under autograd"""
    if hip.maxpool3s2_supported(x.dtype, x.shape[1], x.shape[2], x.shape[3]):
        return _MaxPoolCL.apply(x)
    return to_cl(F.max_pool2d(from_cl(x), kernel_size=3, stride=2, padding=1))


def _bn_trainable(bn):
    return isinstance(bn, nn.BatchNorm2d) and bn.track_running_stats and bn.running_mean is not None and bn.momentum is not None


def block_trainable(blk):
    """the layer forms that keep exactly the stock path: a batch norm without running statistics or with a cumulative
    average (momentum None), a dilated convolution"""
    norms = [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if blk.downsample is not None else [])
    convs = [blk.conv1, blk.conv2, blk.conv3] + ([blk.downsample[0]] if blk.downsample is not None else [])
    return all(_bn_trainable(n) for n in norms) and all(c.dilation == (1, 1) for c in convs)


def train_path(m, x):
    """`m` (a ResNet or a Bottleneck) was switched by set_library_training(), is in train mode, `x` is a 16-bit device tensor
    and autograd is on"""
    return (getattr(m, "library_training", False) and m.training and torch.is_grad_enabled() and x.is_cuda
            and x.dtype in _LOWP)


def bottleneck_train_cl(blk, x):
    """Bottleneck.forward (resnet_encoder.py:62-79) in training mode on a channels-last map: conv -> bn + relu -> conv ->
    bn + relu -> [downsample conv -> bn] -> conv -> bn + shortcut + relu"""
    out = bn_act_cl(blk.bn1, conv_cl(blk.conv1, x))
    out = bn_act_cl(blk.bn2, conv_cl(blk.conv2, out))
    out = conv_cl(blk.conv3, out)
    if blk.downsample is not None:
        x = bn_act_cl(blk.downsample[1], conv_cl(blk.downsample[0], x), relu=False)
    return bn_act_cl(blk.bn3, out, residual=x)


def stem_train_cl(enc, x):
    """conv1 + bn1 + ReLU + max pool of ResNet.forward (resnet_encoder.py:81-110) in training mode: x (B, 3, H, W) NCHW ->
    (B, Hp, Wp, 64) channels-last.  The image needs no gradient, so the 7x7 convolution is the first-layer-embedding route
    of the other encoders: patch rows from a framework data-movement op, product and weight gradient on `_LinearTrainCL`."""
    from .encoders import _embed_rows_train
    proj = enc.conv1
    # (the conditions of encoders._embed_rows_ok, but for a frozen weight too: the rows route needs no gradient to exist)
    if (not x.requires_grad and proj.bias is None and proj.groups == 1 and proj.dilation == (1, 1)
            and proj.kernel_size[0] == proj.kernel_size[1] and proj.stride[0] == proj.stride[1]
            and proj.padding[0] == proj.padding[1] and proj.out_channels % 8 == 0):
        rows, ho, wo = _embed_rows_train(proj, x)
        out = rows.view(x.shape[0], ho, wo, proj.out_channels)
    else:
        out = to_cl(F.conv2d(x, enc.conv1.weight.to(x.dtype), None, enc.conv1.stride, enc.conv1.padding))
    return maxpool_cl(bn_act_cl(enc.bn1, out))
