"""The Tramba-R model of the whole-model accuracy check of tests/test_gpu_resnet_conv.py, with closed-form weights and inputs per
seed: shared by that test (which asserts) and scripts/measure_resnet_parity.py (which measures the margin the test allows), so
that both look at the same model, inputs and error."""
import copy

import torch

import synth

DEV = "cuda"
NAMES = ("feat2", "feat3", "feat4", "out0", "out1", "out2")     # the encoder's three features, the model's three outputs


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def models(img_size=384, dtype=torch.bfloat16):
    """(the 16-bit model as prepare_inference leaves it, an fp32 model holding the same -- rounded -- weights)"""
    import tramba_amd as ta
    m = ta.bulid_model_enc("Tramba-R-TSOD", img_size=img_size)
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        new.setdefault(k, sd[k])
    m.load_state_dict(new, strict=True)
    m = ta.prepare_inference(m.to(DEV).eval(), dtype)
    ref = copy.deepcopy(m).float()
    ref.compute_dtype = None
    return m, ref


def image(seed, img_size=384):
    return synth.synth_input(f"resnet_parity_seed{seed}", (1, 3, img_size, img_size)).to(DEV)


def quantities(m, x, library):
    """[feat2, feat3, feat4, out0, out1, out2] of one forward, the features channels-last"""
    from tramba_amd import encoders
    from tramba_amd.modules import to_cl
    encoders.set_library_convolutions(m, library)
    with torch.no_grad():
        xe = x if m.compute_dtype is None else x.to(m.compute_dtype)
        if library:
            feats = m.encoder.features_cl(xe)
        else:
            feats = [to_cl(o) for o in m.encoder(xe.contiguous(memory_format=torch.channels_last))[1:-1][::-1]]
        outs = m(x)
    encoders.set_library_convolutions(m, False)
    return [t.clone() for t in list(feats) + list(outs)]


def errors(m, ref, x):
    """{name: (library error, stock error)}: relative L2 of the 16-bit model's quantities to the fp32 model's"""
    want = quantities(ref, x, False)
    lib, stock = quantities(m, x, True), quantities(m, x, False)
    return {n: (rel_l2(a, w), rel_l2(b, w)) for n, a, b, w in zip(NAMES, lib, stock, want)}
