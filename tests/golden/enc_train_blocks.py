"""The two encoder blocks of the block-level encoder TRAINING parity check: the blocks, weights and inputs of
attn_blocks.py (one PVT block: dim 128, sr 2, 24 x 24; one Swin block: dim 128, window 12, shift 6), in .train() with
drop_path 0, differentiated against the fixed random dy of attn_train_blocks.py.  Shared by tests/test_gpu_enc_train.py
(which asserts) and scripts/measure_enc_train_parity.py (which measures the margin the test allows), so that both look at
the same blocks, inputs and errors."""
import synth
from attn_train_blocks import pvt_block, rel_l2, seeded, swin_block  # noqa: F401 (seeded: for the tests)

MODES = ("library", "stock", "fp32")


def block_grads(kind, seed, mode, prepare=None):
    """{tensor name: gradient} of one block: "x" for the input and every block parameter by its state_dict name.
    mode: "library" = bf16 with the library-training switch on, "stock" = bf16 with every switch off, "fp32" = fp32 stock.
    prepare(blk): called on the block before the switch is set (the tests build a never-switched block with it)."""
    from tramba_amd.encoders import set_library_training
    blk, x = (swin_block if kind == "swin" else pvt_block)(seed)
    blk.train()
    if prepare is not None:
        prepare(blk)
    else:
        assert set_library_training(blk, mode == "library") > 0
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
    """{tensor name: (library, stock)} relative L2 errors of the bf16 gradients against the fp32 stock gradients"""
    lib, stock, ref = (block_grads(kind, seed, m) for m in MODES)
    return {k: (rel_l2(lib[k], ref[k]), rel_l2(stock[k], ref[k])) for k in ref}
