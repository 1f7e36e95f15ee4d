"""The two bottlenecks of the block-level Tramba-R TRAINING parity check, built from the project's own `Bottleneck`: a
layer1-type block (64 -> 256 with the downsample branch, 24 x 24, batch 2) and a layer2-type stride-2 block (256 -> 512,
24 x 24 -> 12 x 12, batch 2), in .train() with closed-form weights and inputs per seed, differentiated against a fixed
random dy.  Shared by tests/test_gpu_resnet_train.py (which asserts) and scripts/measure_resnet_train_parity.py (which
measures the margin the test allows), so that both look at the same blocks, inputs and errors."""
import torch
import torch.nn as nn

import synth
from attn_blocks import rel_l2, seeded  # noqa: F401

DEV = "cuda"
MODES = ("library", "stock", "fp32")
KINDS = {"layer1": (64, 64, 1), "layer2": (256, 128, 2)}          # inplanes, planes, stride


def bottleneck(kind, seed):
    """(fp32 block in .train() on the device, bf16 channels-last post-ReLU input (2, 24, 24, inplanes))"""
    from tramba_amd.models import Bottleneck
    inplanes, planes, stride = KINDS[kind]
    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    blk = seeded(Bottleneck(inplanes, planes, stride, down), seed).train()
    x = synth.synth_input(f"resnet_train_{kind}_{seed}", (2, 24, 24, inplanes)).clamp_min(0).to(DEV).bfloat16()
    return blk, x


def block_grads(kind, seed, mode, prepare=None):
    """{tensor name: gradient} of one block: "x" (channels-last) for the input and every block parameter by its state_dict
    name.  mode: "library" = fp32 master weights, bf16 activations, the library-training switch on (`forward_cl`);
    "stock" = the block cast to bf16 on the framework's ops; "fp32" = the fp32 block on the framework's ops.
    prepare(blk): called on the block before it runs (the tests flip switches with it)."""
    from tramba_amd.encoders import set_library_training
    blk, x = bottleneck(kind, seed)
    if mode == "library":
        assert set_library_training(blk, True) == 1
    elif mode == "stock":
        blk = blk.to(torch.bfloat16)
    if prepare is not None:
        prepare(blk)
    x = (x.float() if mode == "fp32" else x).detach().requires_grad_()
    y = blk.forward_cl(x) if mode == "library" else blk(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    dy = synth.synth_input(f"resnet_train_dy_{kind}_{seed}", tuple(y.shape)).to(DEV)
    y.backward(dy.to(y.dtype))
    grads = {"x": x.grad}
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        grads[name] = p.grad
    return grads


def block_errors(kind, seed):
    """{tensor name: (library, stock)} relative L2 errors of the 16-bit gradients against the fp32 stock gradients"""
    lib, stock, ref = (block_grads(kind, seed, m) for m in MODES)
    return {k: (rel_l2(lib[k], ref[k]), rel_l2(stock[k], ref[k])) for k in ref}
