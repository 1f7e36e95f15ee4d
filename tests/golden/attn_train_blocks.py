"""The two encoder blocks of the block-level attention TRAINING parity check: the blocks, weights and inputs of
attn_blocks.py, in .train() with drop_path 0, differentiated against a fixed random dy.  Shared by
tests/test_gpu_attn_train.py (which asserts) and scripts/measure_attn_train_parity.py (which measures the margin the test
allows), so that both look at the same blocks, inputs and errors."""
import torch

import synth
from attn_blocks import pvt_block, rel_l2, seeded, swin_block  # noqa: F401 (seeded: for the tests)

MODES = ("fused", "stock", "fp32")


def block_grads(kind, seed, mode):
    """{tensor name: gradient} of one block: "x" for the input and every block parameter by its state_dict name.
    mode: "fused" = bf16 with the fused-attention-training flag on, "stock" = bf16 with it off, "fp32" = fp32 stock."""
    from tramba_amd.encoders import set_fused_attention_training
    blk, x = (swin_block if kind == "swin" else pvt_block)(seed)
    blk.train()
    assert set_fused_attention_training(blk, mode == "fused") == 1
    dy = synth.synth_input(f"attn_train_dy_{kind}_{seed}", tuple(x.shape)).to(x.device)
    x = (x.float() if mode == "fp32" else x).detach().requires_grad_()
    y = blk(x) if kind == "swin" else blk(x, 24, 24)
    y.backward(dy.to(y.dtype))
    grads = {"x": x.grad}
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        grads[name] = p.grad
    return grads


def block_errors(kind, seed):
    """{tensor name: (fused, stock)} relative L2 errors of the bf16 gradients against the fp32 stock gradients"""
    fused, stock, ref = (block_grads(kind, seed, m) for m in MODES)
    return {k: (rel_l2(fused[k], ref[k]), rel_l2(stock[k], ref[k])) for k in ref}
