"""CPU tests of the host side of the Tramba-R training path (csrc/batchnorm.hip, the backward entries of
csrc/resnet_conv.hip, tramba_amd/resnet_train.py): the entries are declared, bound and exported; unsupported arguments are
refused with a message before any launch; the Python predicates and sizing helpers agree with the C side and accept every
layer of ResNet-50's layer1..3 at the workload sizes; the switch counts a Tramba-R model's encoder, flips back and leaves the
state_dict alone."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from test_attn_host import BF16, F16, F32, _TORCH, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tramba_bn_parts", "tramba_bn_work", "tramba_bn_stats_cl", "tramba_bn_act_cl", "tramba_bn_act_bwd_cl",
           "tramba_maxpool3s2_cl", "tramba_maxpool3s2_bwd_cl", "tramba_conv_dgrad_cl", "tramba_conv_wgrad_split",
           "tramba_conv_wgrad_work", "tramba_conv_wgrad_cl")


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip, resnet_train
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7                               # additions only
    for name in ENTRIES:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    assert hdr.count("resnet_encoder.py:62-110") >= 4
    for name in ("bn_stats_cl", "bn_act_cl", "bn_act_bwd_cl", "bn_supported", "maxpool3s2_cl", "maxpool3s2_bwd_cl",
                 "maxpool3s2_supported", "conv_dgrad_cl", "conv_wgrad_cl", "conv_train_supported"):
        assert callable(getattr(hip, name)), name
    for name in ("_ConvCL", "_BatchNormActCL", "_MaxPoolCL"):
        assert issubclass(getattr(resnet_train, name), torch.autograd.Function)


def _resnet50_layers(size):
    """(h, w, cin, cout, k, s) of every bottleneck convolution of layer1..3 and (m, c) of every batch norm, stem included, at
    a size x size image, batch 1"""
    convs, norms = [], []
    h = ((size - 1) // 2 + 1 - 1) // 2 + 1
    norms.append((((size - 1) // 2 + 1) ** 2, 64))
    inplanes = 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            ho = (h - 1) // s + 1
            convs += [(h, h, inplanes, planes, 1, 1), (h, h, planes, planes, 3, s), (ho, ho, planes, planes * 4, 1, 1)]
            norms += [(h * h, planes), (ho * ho, planes), (ho * ho, planes * 4)]
            if b == 0:
                convs.append((h, h, inplanes, planes * 4, 1, s))
                norms.append((ho * ho, planes * 4))
            inplanes, h = planes * 4, ho
    return convs, norms


def test_predicates_accept_every_layer_of_resnet50_and_refuse_fp32_and_dilation():
    from tramba_amd import hip, models, resnet_train
    for size in (384, 256):
        convs, norms = _resnet50_layers(size)
        assert len(convs) == 42 and len(norms) == 43
        for dtype in (torch.bfloat16, torch.float16):
            assert all(hip.conv_train_supported(dtype, *c) for c in convs)
            assert all(hip.bn_supported(dtype, 4 * m, c) and hip.bn_supported(dtype, m, c) for m, c in norms)
            hc = (size - 1) // 2 + 1
            assert hip.maxpool3s2_supported(dtype, hc, hc, 64)
        assert not any(hip.conv_train_supported(torch.float32, *c) for c in convs)
        assert not any(hip.bn_supported(torch.float32, m, c) for m, c in norms)
        assert not hip.maxpool3s2_supported(torch.float32, 192, 192, 64)
    assert not hip.bn_supported(torch.bfloat16, 1, 64) and not hip.bn_supported(torch.bfloat16, 35, 12)
    assert not hip.conv_train_supported(torch.bfloat16, 8, 8, 64, 72, 3, 1)          # the input gradient reduces over Cout
    assert hip.conv_train_supported(torch.bfloat16, 8, 8, 64, 72, 1, 1)              # ... except as a plain product
    # the module-level predicates, on meta-free CPU shapes: a dilated convolution and fp32 are refused
    blk = models.Bottleneck(64, 64, dilation=2)
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16)
    assert resnet_train.conv_ok(blk.conv1, x) and not resnet_train.conv_ok(blk.conv2, x)
    assert not resnet_train.block_trainable(blk) and resnet_train.block_trainable(models.Bottleneck(64, 64))
    assert not resnet_train.conv_ok(blk.conv1, x.float()) and not resnet_train.bn_ok(blk.bn1, x.float())
    blk = models.Bottleneck(64, 64)
    blk.bn2.momentum = None
    assert not resnet_train.block_trainable(blk)
    blk = models.Bottleneck(64, 64)
    blk.bn1.track_running_stats = False
    assert not resnet_train.block_trainable(blk)


def test_sizing_helpers_are_consistent_with_the_library():
    from tramba_amd import hip
    lib = hip.lib()
    for m, c in ((35, 64), (1, 64), (127, 8), (128, 72), (129, 72), (2304, 1024), (36864, 64), (147456, 256), (10 ** 7, 2048)):
        parts = lib.tramba_bn_parts(m, c)
        assert parts == hip.bn_parts(m, c) and 1 <= parts <= 64
        assert lib.tramba_bn_work(m, c) == 4 * hip.bn_work_floats(m, c) == 4 * (2 * parts + 2) * ((c + 63) // 64 * 64)
    assert lib.tramba_bn_parts(0, 64) == hip.bn_parts(0, 64) == 0 and lib.tramba_bn_work(0, 64) == 0
    for size in (384, 256):
        for batch in (1, 4):
            for h, w, cin, cout, k, s in _resnet50_layers(size)[0]:
                n = lib.tramba_conv_wgrad_split(batch, h, w, cin, cout, k, s)
                assert n == hip.conv_wgrad_split(batch, h, w, cin, cout, k, s) and 1 <= n <= 64
                assert lib.tramba_conv_wgrad_work(batch, h, w, cin, cout, k, s) == n * cout * k * k * cin * 4
    assert lib.tramba_conv_wgrad_split(1, 8, 8, 96, 64, 1, 1) == 0 == lib.tramba_conv_wgrad_work(1, 8, 8, 96, 64, 1, 1)
    assert lib.tramba_conv_wgrad_split(1, 8, 8, 64, 64, 5, 1) == 0


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg
    big = 1 << 30
    stats = lambda x=addr, m=64, c=64, dtype=BF16, work=addr, nbytes=big, eps=1e-5, mom=0.1: lib.tramba_bn_stats_cl(
        x, addr, addr, None, None, work, nbytes, m, c, eps, mom, dtype, None)
    rejected(stats(x=None), "null")
    rejected(stats(work=None), "null")
    rejected(stats(dtype=F32), "bf16/f16")
    rejected(stats(c=12), "C=12")
    rejected(stats(m=0), "empty")
    rejected(stats(m=1), "more than 1 value")
    rejected(stats(mom=1.5), "momentum")
    rejected(stats(nbytes=16), "workspace")
    rejected(stats(x=addr + 8), "aligned")
    act = lambda x=addr, m=64, c=64, dtype=BF16: lib.tramba_bn_act_cl(x, addr, addr, None, None, None, addr, m, c, 1, dtype, None)
    rejected(act(x=None), "null")
    rejected(act(dtype=F32), "bf16/f16")
    rejected(act(c=20), "C=20")
    rejected(act(x=addr + 8), "aligned")
    bwd = lambda dy=addr, y=addr, m=64, c=64, relu=1, dtype=BF16, nbytes=big: lib.tramba_bn_act_bwd_cl(
        dy, addr, y, addr, addr, None, addr, None, None, None, addr, nbytes, m, c, relu, dtype, None)
    rejected(bwd(dy=None), "null")
    rejected(bwd(y=None), "ReLU mask")
    rejected(bwd(dtype=7), "bf16/f16")
    rejected(bwd(nbytes=0), "workspace")
    rejected(bwd(dy=addr + 8), "aligned")
    rejected(bwd(y=None, relu=0, dy=addr + 8), "aligned")              # without relu y may be missing
    for entry in (lambda **k: lib.tramba_maxpool3s2_cl(k.get("x", addr), addr, k.get("b", 1), 8, 8, k.get("c", 64), k.get("dt", BF16), None),
                  lambda **k: lib.tramba_maxpool3s2_bwd_cl(addr, k.get("x", addr), addr, k.get("b", 1), 8, 8, k.get("c", 64),
                                                           k.get("dt", BF16), None)):
        rejected(entry(x=None), "null")
        rejected(entry(dt=F32), "bf16/f16")
        rejected(entry(c=4), "C=4")
        rejected(entry(b=0), "empty")
        rejected(entry(x=addr + 8), "aligned")
    dgrad = lambda gy=addr, cin=64, cout=64, k=3, s=1, dtype=BF16, h=8: lib.tramba_conv_dgrad_cl(gy, addr, addr, 1, h, 8, cin, cout,
                                                                                                 k, s, dtype, None)
    wgrad = lambda gy=addr, cin=64, cout=64, k=3, s=1, dtype=BF16, h=8, nbytes=big: lib.tramba_conv_wgrad_cl(
        gy, addr, addr, nbytes, 1, h, 8, cin, cout, k, s, dtype, None)
    for entry in (dgrad, wgrad):
        rejected(entry(gy=None), "null")
        rejected(entry(dtype=F32), "bf16/f16")
        rejected(entry(k=5), "ksize")
        rejected(entry(s=3), "stride")
        rejected(entry(h=0), "empty")
        rejected(entry(cout=12), "Cout=12")
        rejected(entry(gy=addr + 8), "aligned")
    rejected(dgrad(cout=72), "Cout=72")
    rejected(dgrad(cout=72, k=1, gy=addr + 8), "aligned")              # 1x1 / stride 1 takes Cout % 8
    rejected(wgrad(cin=96), "Cin=96")
    rejected(wgrad(nbytes=64), "workspace")
    del keep


def test_python_predicates_agree_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    # an accepted call would launch, so the C side is always asked with a misaligned tensor: alignment is its LAST check,
    # and reaching it means that it found nothing to object to in the shape
    for dtype in (BF16, F16, F32):
        for m, c in ((35, 64), (1, 64), (2, 8), (64, 12), (64, 0), (0, 64), (9216, 1024)):
            want = hip.bn_supported(_TORCH[dtype], m, c)
            rc = lib.tramba_bn_stats_cl(addr + 8, addr, addr, None, None, addr, 1 << 30, m, c, 1e-5, 0.1, dtype, None)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, m, c)
            seen.add(want)
        for h, w, c in ((192, 192, 64), (7, 9, 72), (1, 1, 8), (0, 4, 64), (4, 4, 12)):
            want = hip.maxpool3s2_supported(_TORCH[dtype], h, w, c)
            rc = lib.tramba_maxpool3s2_cl(addr + 8, addr, 1, h, w, c, dtype, None)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, h, w, c)
            seen.add(want)
        for h, w, cin, cout, k, s in ((96, 96, 64, 64, 3, 1), (24, 24, 1024, 256, 1, 1), (7, 9, 256, 512, 1, 2), (5, 5, 64, 72, 1, 1),
                                      (5, 5, 64, 72, 3, 1), (5, 5, 64, 72, 1, 2), (8, 8, 96, 64, 1, 1), (8, 8, 64, 64, 5, 1),
                                      (8, 8, 64, 64, 3, 3), (0, 8, 64, 64, 1, 1), (8, 8, 64, 12, 1, 1)):
            want = hip.conv_train_supported(_TORCH[dtype], h, w, cin, cout, k, s)
            bump = addr + 8
            rc_d = lib.tramba_conv_dgrad_cl(bump, addr, addr, 1, h, w, cin, cout, k, s, dtype, None)
            ok_d = "aligned" in lib.tramba_last_error().decode()
            rc_w = lib.tramba_conv_wgrad_cl(bump, addr, addr, 1 << 30, 1, h, w, cin, cout, k, s, dtype, None)
            ok_w = "aligned" in lib.tramba_last_error().decode()
            assert rc_d == rc_w == -1 and (ok_d and ok_w) == want, (dtype, h, w, cin, cout, k, s, ok_d, ok_w)
            seen.add(want)
    assert seen == {True, False}
    del keep


def test_bindings_refuse_cpu_tensors_and_mismatched_shapes(monkeypatch):
    from tramba_amd import hip
    bf = torch.bfloat16
    x, v = torch.zeros(1, 4, 4, 64, dtype=bf), torch.ones(64)
    for call in (lambda: hip.bn_stats_cl(x, 1e-5), lambda: hip.bn_act_cl(x, v, v), lambda: hip.bn_act_bwd_cl(x, x, x, v, v),
                 lambda: hip.maxpool3s2_cl(x), lambda: hip.maxpool3s2_bwd_cl(x, x),
                 lambda: hip.conv_dgrad_cl(x, torch.zeros(64, 1, 1, 64, dtype=bf), (1, 4, 4, 64)),
                 lambda: hip.conv_wgrad_cl(x, x, 1)):
        with pytest.raises(hip.TrambaHipError, match="HIP device"):
            call()
    monkeypatch.setattr(hip, "_dev", lambda *ts: None)                 # the shape checks come after the device check
    with pytest.raises(hip.TrambaHipError, match="bf16 / fp16"):
        hip.bn_stats_cl(x.float(), 1e-5)
    with pytest.raises(hip.TrambaHipError, match="running_mean"):
        hip.bn_stats_cl(x, 1e-5, torch.zeros(32), v)
    with pytest.raises(hip.TrambaHipError, match="more than 1 value"):
        hip.bn_stats_cl(torch.zeros(1, 1, 1, 64, dtype=bf), 1e-5)
    with pytest.raises(hip.TrambaHipError, match="residual"):
        hip.bn_act_cl(x, v, v, residual=torch.zeros(1, 4, 4, 32, dtype=bf))
    with pytest.raises(hip.TrambaHipError, match="gamma"):
        hip.bn_act_cl(x, v, v, gamma=v.double())
    with pytest.raises(hip.TrambaHipError, match="dy"):
        hip.bn_act_bwd_cl(x.half(), x, x, v, v)
    with pytest.raises(hip.TrambaHipError, match="required"):
        hip.bn_act_bwd_cl(x, x, None, v, v, relu=True)
    with pytest.raises(hip.TrambaHipError, match="does not belong"):
        hip.maxpool3s2_bwd_cl(x, x)
    with pytest.raises(hip.TrambaHipError, match="does not belong"):
        hip.conv_dgrad_cl(x, torch.zeros(64, 3, 3, 64, dtype=bf), (1, 4, 4, 64), stride=2)
    with pytest.raises(hip.TrambaHipError, match="wt must be"):
        hip.conv_dgrad_cl(x, torch.zeros(32, 3, 3, 64, dtype=bf), (1, 4, 4, 64))
    with pytest.raises(hip.TrambaHipError, match="ksize"):
        hip.conv_wgrad_cl(x, x, 5)
    assert hip.conv_transposed_weight(torch.zeros(8, 3, 3, 16)).shape == (16, 3, 3, 8)


def test_switch_counts_the_resnet_and_its_bottlenecks_flips_back_and_leaves_the_state_dict_alone():
    import tramba_amd as ta
    from tramba_amd import encoders, models
    model = ta.bulid_model_enc("Tramba-R-TSOD")
    keys = list(model.state_dict().keys())
    assert len(keys) == 507
    blocks = [m for m in model.modules() if isinstance(m, models.Bottleneck)]
    assert len(blocks) == 16 and not model.encoder.library_training and not any(b.library_training for b in blocks)
    assert encoders.set_library_training(model) == 17
    assert model.encoder.library_training and all(b.library_training for b in blocks)
    assert list(model.state_dict().keys()) == keys
    assert encoders.set_library_training(model, False) == 17
    assert not any(getattr(m, "library_training", False) for m in model.modules())
    assert list(model.state_dict().keys()) == keys
    assert encoders.set_library_training(models.Bottleneck(64, 64)) == 1
    on = ta.build("Tramba-R-SOD", SimpleNamespace(img_size=384, library_training=True))
    assert on.encoder.library_training and not on.encoder.library_convolutions
    off = ta.build("Tramba-R-SOD", SimpleNamespace(img_size=384))
    assert not off.encoder.library_training and list(on.state_dict().keys()) == list(off.state_dict().keys())


def test_training_path_needs_the_flag_train_mode_16_bit_and_autograd():
    """(a CPU tensor is never on the path: the device is part of the condition)"""
    from tramba_amd import models, resnet_train

    class OnDevice(torch.Tensor):
        is_cuda = True
    enc = models.ResNet().train()
    x16 = torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16).as_subclass(OnDevice)
    assert not resnet_train.train_path(enc, x16)                       # flag off
    enc.library_training = True
    assert resnet_train.train_path(enc, x16)
    assert not resnet_train.train_path(enc, torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16))      # a CPU tensor
    assert not resnet_train.train_path(enc, torch.zeros(1, 3, 32, 32).as_subclass(OnDevice))      # fp32 activations
    assert not resnet_train.train_path(enc.eval(), x16)                # eval mode with autograd
    with torch.no_grad():
        assert not resnet_train.train_path(enc.train(), x16)           # no autograd
    assert not enc._train_path(x16)                                    # its bottlenecks were not switched
    for m in enc.modules():
        if isinstance(m, models.Bottleneck):
            m.library_training = True
    assert enc._train_path(x16)
    enc.layer2[1].bn2.momentum = None
    assert not enc._train_path(x16)
