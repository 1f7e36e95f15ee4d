"""The two encoder blocks of the block-level attention parity check, with closed-form weights and inputs per seed: shared by
tests/test_gpu_attn.py (which asserts) and scripts/measure_attn_parity.py (which measures the margin the test allows), so
that both look at the same blocks, inputs and error."""
import torch

import synth

DEV = "cuda"


def seeded(module, seed):
    sd = module.state_dict()
    new = synth.synth_state_dict(((f"seed{seed}.{k}", v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    new = {k.split(".", 1)[1]: v for k, v in new.items()}
    for k in sd:
        new.setdefault(k, sd[k])
    module.load_state_dict(new, strict=True)
    return module.to(DEV).eval()


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def swin_block(seed):
    """(block, bf16 input): dim 128, 24 x 24, 4 heads, window 12, shift 6"""
    from tramba_amd.encoders import SwinTransformerBlock
    blk = seeded(SwinTransformerBlock(128, (24, 24), 4, 12, 6, 4.0, 0.0), seed)
    return blk, synth.synth_input(f"attn_swin_{seed}", (2, 576, 128)).to(DEV).bfloat16()


def pvt_block(seed):
    """(block, bf16 input): dim 128, 2 heads, sr 2, on 24 x 24"""
    from tramba_amd.encoders import _PvtBlock
    blk = seeded(_PvtBlock(128, 2, 4, True, 0.0, 2, 1e-6), seed)
    return blk, synth.synth_input(f"attn_pvt_{seed}", (2, 576, 128)).to(DEV).bfloat16()


def swin_block_outputs(seed):
    """(fused, stock, fp32 stock) outputs of the Swin block on the same rounded input"""
    blk, x = swin_block(seed)
    with torch.no_grad():
        return blk(x), blk._forward_stock(x), blk._forward_stock(x.float())


def pvt_block_outputs(seed):
    blk, x = pvt_block(seed)
    with torch.no_grad():
        fused = blk(x, 24, 24)
        blk.attn.forward = blk.attn._forward_stock
        try:
            return fused, blk(x, 24, 24), blk(x.float(), 24, 24)
        finally:
            del blk.attn.forward


def block_errors(kind, seed):
    """(fused, stock) relative L2 error of one bf16 block against its fp32 stock forward"""
    fused, stock, ref = (swin_block_outputs if kind == "swin" else pvt_block_outputs)(seed)
    return rel_l2(fused, ref), rel_l2(stock, ref)


def gemm_conv(m, x):
    """A stand-in for `encoders._conv` made of launches whose summation order is fixed: im2col (a gather) and the library's
    GEMM.  The framework's convolution may pick implicit-GEMM kernels that split the reduction over workgroups and add
    the parts with atomics (their names end in `gkgs`), so two runs of one convolution need not agree bitwise; a test that
    compares a graph replay with an eager forward bit for bit pins the convolutions with this."""
    import torch.nn.functional as F
    from tramba_amd import hip
    assert m.groups == 1 and m.dilation == (1, 1)
    b, _, h, w = x.shape
    kh, kw = m.kernel_size
    ho = (h + 2 * m.padding[0] - kh) // m.stride[0] + 1
    wo = (w + 2 * m.padding[1] - kw) // m.stride[1] + 1
    cols = F.unfold(x, m.kernel_size, 1, m.padding, m.stride).transpose(1, 2)           # (B, L, Cin kh kw)
    k = cols.shape[-1]
    kp = (k + 63) // 64 * 64
    cols = F.pad(cols, (0, kp - k)).contiguous()
    wt = F.pad(m.weight.detach().to(x.dtype).reshape(m.out_channels, k), (0, kp - k)).contiguous()
    y = hip.linear_cl(cols, wt, None if m.bias is None else m.bias.detach().float().contiguous())
    return y.view(b, ho, wo, m.out_channels).permute(0, 3, 1, 2)
