"""CPU tests of the ResNet-50 encoder entries' host side (csrc/resnet_conv.hip): declared, bound and exported; unsupported
arguments are refused with a message before any launch; the Python predicates agree with the C checks; the folded batch norm
and the output-size helpers reproduce the framework's; the switch counts a Tramba-R model's encoder, flips back and leaves
the state_dict alone."""
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_attn_host import BF16, F16, F32, _TORCH, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv_affine(lib, addr, x=True, w=True, scale=True, shift=True, residual=True, y=True, batch=1, h=24, wd=24, cin=128,
                 cout=128, ksize=3, stride=1, relu=1, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_conv_affine_cl(p(x), p(w), p(scale), p(shift), p(residual), p(y), batch, h, wd, cin, cout, ksize, stride,
                                     relu, dtype, None)


def _stem(lib, addr, img=True, w=True, scale=True, shift=True, y=True, batch=1, h=64, wd=64, img_dtype=F32, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_stem7_affine_relu_pool(p(img), p(w), p(scale), p(shift), p(y), batch, h, wd, img_dtype, dtype, None)


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_conv_affine_cl", "tramba_stem7_affine_relu_pool"):
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "resnet_encoder.py:62-110" in hdr
    for name in ("conv_affine_cl", "conv_affine_supported", "stem7_affine_relu_pool", "stem7_pool_supported"):
        assert callable(getattr(hip, name)), name


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg

    for missing in ("x", "w", "y"):
        rejected(_conv_affine(lib, addr, **{missing: False}), "null")
    for dtype in (F32, 7):
        rejected(_conv_affine(lib, addr, dtype=dtype), "bf16/f16")
    for ksize in (0, 2, 5, 7):
        rejected(_conv_affine(lib, addr, ksize=ksize), "ksize")
    for stride in (0, 3, 4):
        rejected(_conv_affine(lib, addr, stride=stride), "stride")
    rejected(_conv_affine(lib, addr, cin=96), "Cin=96")
    rejected(_conv_affine(lib, addr, cin=32), "Cin=32")
    rejected(_conv_affine(lib, addr, cout=12), "Cout=12")
    rejected(_conv_affine(lib, addr, batch=0), "empty")
    rejected(_conv_affine(lib, addr, h=0), "empty")
    rejected(_conv_affine(lib, addr, batch=64, h=1024, wd=1024, cin=64, cout=64), "32-bit")      # 2^33 bytes of input
    rejected(_conv_affine(lib, addr + 8), "aligned")
    # alignment is the last check: with the optional tensors missing (allowed) the call gets that far
    rejected(_conv_affine(lib, addr + 8, scale=False, shift=False, residual=False), "aligned")

    for missing in ("img", "w", "scale", "shift", "y"):
        rejected(_stem(lib, addr, **{missing: False}), "null")
    rejected(_stem(lib, addr, dtype=F32), "output")
    rejected(_stem(lib, addr, img_dtype=F16, dtype=BF16), "image")
    rejected(_stem(lib, addr, batch=0), "empty")
    rejected(_stem(lib, addr, wd=0), "empty")
    rejected(_stem(lib, addr, batch=70000), "too many")                        # the batch is a grid dimension
    rejected(_stem(lib, addr + 8), "aligned")
    del keep


def test_python_predicates_agree_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    # an accepted call would launch, so the C side is asked with a misaligned tensor: alignment is its LAST check, and
    # reaching it means that it found nothing to object to in the shape
    for dtype in (BF16, F16, F32):
        for h, w, cin, cout, k, s in ((96, 96, 64, 64, 1, 1), (96, 96, 64, 64, 3, 1), (96, 96, 256, 128, 3, 2),
                                      (24, 24, 1024, 256, 1, 1), (7, 9, 256, 512, 1, 2), (4, 4, 64, 72, 1, 1),
                                      (8, 8, 96, 64, 1, 1), (8, 8, 64, 12, 3, 1), (8, 8, 64, 64, 5, 1), (8, 8, 64, 64, 2, 2),
                                      (8, 8, 64, 64, 3, 3), (8, 8, 0, 64, 1, 1), (0, 8, 64, 64, 1, 1), (8, 8, 32, 64, 3, 1),
                                      (20000, 20000, 64, 64, 1, 1)):
            want = hip.conv_affine_supported(_TORCH[dtype], h, w, cin, cout, k, s)
            rc = _conv_affine(lib, addr + (8 if want else 0), h=h, wd=w, cin=cin, cout=cout, ksize=k, stride=s, dtype=dtype)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, h, w, cin, cout, k, s)
            seen.add(want)
        for h, w in ((384, 384), (18, 22), (1, 1), (0, 5), (5, 0)):
            want = hip.stem7_pool_supported(_TORCH[dtype], h, w)
            rc = _stem(lib, addr + (8 if want else 0), h=h, wd=w, dtype=dtype)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, h, w)
            seen.add(want)
    assert seen == {True, False}
    del keep


def test_bindings_refuse_cpu_tensors_and_mismatched_shapes(monkeypatch):
    from tramba_amd import hip
    bf = torch.bfloat16
    x, w = torch.zeros(1, 8, 8, 64, dtype=bf), torch.zeros(64, 3, 3, 64, dtype=bf)
    sc = torch.ones(64)
    with pytest.raises(hip.TrambaHipError, match="HIP device"):
        hip.conv_affine_cl(x, w, sc, sc)
    with pytest.raises(hip.TrambaHipError, match="HIP device"):
        hip.stem7_affine_relu_pool(torch.zeros(1, 3, 16, 16), torch.zeros(64, 3, 7, 7), sc, sc, bf)
    # the shape checks come after the device check: ask them without it
    monkeypatch.setattr(hip, "_dev", lambda *ts: None)
    for bad_w in (torch.zeros(64, 3, 3, 128, dtype=bf), torch.zeros(64, 3, 1, 64, dtype=bf), torch.zeros(64, 9 * 64, dtype=bf),
                  torch.zeros(64, 3, 3, 64, dtype=torch.float16)):
        with pytest.raises(hip.TrambaHipError, match="need x"):
            hip.conv_affine_cl(x, bad_w, sc, sc)
    with pytest.raises(hip.TrambaHipError, match="k = 1"):
        hip.conv_affine_cl(x, w, sc, sc, ksize=1)
    with pytest.raises(hip.TrambaHipError, match="scale"):
        hip.conv_affine_cl(x, w, torch.ones(32), sc)
    with pytest.raises(hip.TrambaHipError, match="shift"):
        hip.conv_affine_cl(x, w, sc, sc.double())
    for bad_res in (torch.zeros(1, 8, 8, 32, dtype=bf), torch.zeros(1, 4, 4, 64, dtype=bf), torch.zeros(1, 8, 8, 64)):
        with pytest.raises(hip.TrambaHipError, match="residual"):
            hip.conv_affine_cl(x, w, sc, sc, residual=bad_res)
    with pytest.raises(hip.TrambaHipError, match="residual"):      # the stride-2 map is 4 x 4
        hip.conv_affine_cl(x, w, sc, sc, residual=torch.zeros(1, 8, 8, 64, dtype=bf), stride=2)
    with pytest.raises(hip.TrambaHipError, match="ksize"):
        hip.conv_affine_cl(x, torch.zeros(64, 5, 5, 64, dtype=bf), sc, sc)
    with pytest.raises(hip.TrambaHipError, match="need img"):
        hip.stem7_affine_relu_pool(torch.zeros(1, 3, 16, 16), torch.zeros(64, 3, 3, 3), sc, sc, bf)
    with pytest.raises(hip.TrambaHipError, match="need img"):
        hip.stem7_affine_relu_pool(torch.zeros(1, 4, 16, 16), torch.zeros(64, 3, 7, 7), sc, sc, bf)
    with pytest.raises(hip.TrambaHipError, match="scale"):
        hip.stem7_affine_relu_pool(torch.zeros(1, 3, 16, 16), torch.zeros(64, 3, 7, 7), torch.ones(32), sc, bf)


def test_folded_batch_norm_reproduces_eval_mode_batch_norm_in_fp64():
    from tramba_amd import models
    g = torch.Generator().manual_seed(5)
    bn = nn.BatchNorm2d(24).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(24, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(24, generator=g, dtype=torch.float64) * 3)
        bn.running_mean.copy_(torch.randn(24, generator=g, dtype=torch.float64) * 2)
        bn.running_var.copy_(torch.rand(24, generator=g, dtype=torch.float64) * 4 + 1e-3)
    bn.eval()
    x = torch.randn(2, 24, 5, 7, generator=g, dtype=torch.float64) * 5
    scale, shift = models._bn_affine(bn, torch.float64)
    assert scale.dtype == torch.float64 and scale.shape == shift.shape == (24,)
    want = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    got = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    assert float((got - want).detach().abs().max()) <= 1e-12
    assert torch.equal(want, bn(x))
    # the copies the library reads are f32
    s32, h32 = models._bn_affine(bn)
    assert s32.dtype == h32.dtype == torch.float32 and float((s32.double() - scale).abs().max()) < 1e-5


def test_output_size_helpers_equal_the_framework_shapes():
    from tramba_amd import hip
    for n in range(7, 41):
        x = torch.zeros(1, 1, n, 47 - n)
        for k in (1, 3):
            for s in (1, 2):
                y = F.conv2d(x, torch.zeros(1, 1, k, k), None, s, k // 2)
                assert tuple(y.shape[2:]) == (hip.conv_out_size(n, k, s), hip.conv_out_size(47 - n, k, s)), (n, k, s)
        y = F.max_pool2d(F.conv2d(x, torch.zeros(1, 1, 7, 7), None, 2, 3), 3, 2, 1)
        assert tuple(y.shape[2:]) == (hip.stem7_pool_out_size(n), hip.stem7_pool_out_size(47 - n)), n
        assert hip.conv_out_size(n, 7, 2) == (n - 1) // 2 + 1


def test_switch_counts_the_resnet_flips_back_and_leaves_the_state_dict_alone():
    import tramba_amd as ta
    from tramba_amd import encoders, models
    model = ta.bulid_model_enc("Tramba-R-TSOD")
    keys = list(model.state_dict().keys())
    assert len(keys) == 507
    assert isinstance(model.encoder, models.ResNet) and model.encoder.library_convolutions is False      # off by default
    assert encoders.set_library_convolutions(model) == 1
    assert model.encoder.library_convolutions is True
    assert list(model.state_dict().keys()) == keys
    assert encoders.set_library_convolutions(model, enabled=False) == 1
    assert model.encoder.library_convolutions is False
    assert list(model.state_dict().keys()) == keys
    assert "library_convolutions" not in model.encoder.__dict__.get("_parameters", {})
    assert encoders.set_library_convolutions(torch.nn.Linear(4, 4)) == 0
    assert encoders.set_library_convolutions(models.ResNet()) == 1


def test_build_sets_the_flag_only_when_asked():
    import tramba_amd as ta
    on = ta.build("Tramba-R-SOD", SimpleNamespace(img_size=384, library_convolutions=True))
    assert on.encoder.library_convolutions is True
    off = ta.build("Tramba-R-SOD", SimpleNamespace(img_size=384))
    assert off.encoder.library_convolutions is False
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off = ta.build("Tramba-R-SOD", SimpleNamespace(img_size=384, library_convolutions=False))
    assert off.encoder.library_convolutions is False


def test_library_path_needs_the_flag_eval_mode_16_bit_and_no_autograd():
    from tramba_amd import models
    enc = models.ResNet()
    x16, x32 = torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16), torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        assert not enc.eval()._library_path(x16)                      # flag off
        enc.library_convolutions = True
        assert enc._library_path(x16)
        assert not enc._library_path(x32)                             # fp32 activations
        assert not enc.train()._library_path(x16)                     # batch statistics
    assert not enc.eval()._library_path(x16)                          # autograd on, parameters require grad
