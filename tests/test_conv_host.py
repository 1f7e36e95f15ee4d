"""CPU tests of the encoder-convolution entries' host side (csrc/patch_conv.hip): declared, bound and exported; every
unsupported argument is refused with a message before any launch; the Python predicates the encoder modules ask agree with the
C checks; the switch counts the modules it flips, flips them back and leaves the state_dict alone."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from test_attn_host import BF16, F16, F32, _TORCH, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _patch_conv(lib, addr, x=True, w=True, bias=True, y=True, batch=1, h=24, wd=24, cin=128, cout=128, r=4, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_patch_conv_cl(p(x), p(w), p(bias), p(y), batch, h, wd, cin, cout, r, dtype, None)


def _patch_embed(lib, addr, img=True, w=True, bias=True, ln_w=True, ln_b=True, y=True, batch=1, h=64, wd=64, k=7, stride=4,
                 pad=3, cout=64, img_dtype=F32, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_patch_embed_ln(p(img), p(w), p(bias), p(ln_w), p(ln_b), p(y), batch, h, wd, k, stride, pad, cout, 1e-5,
                                     img_dtype, dtype, None)


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_patch_conv_cl", "tramba_patch_embed_ln"):
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    for name in ("patch_conv_cl", "patch_conv_supported", "patch_embed_ln", "patch_embed_ln_supported"):
        assert callable(getattr(hip, name)), name


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg

    for missing in ("x", "w", "y"):
        rejected(_patch_conv(lib, addr, **{missing: False}), "null")
    rejected(_patch_conv(lib, addr, cin=96, cout=96), "Cin=96")
    for r in (1, 9, 0, -2):
        rejected(_patch_conv(lib, addr, r=r), "2..8")
    rejected(_patch_conv(lib, addr, cout=12), "Cout=12")
    for dtype in (F32, 7):
        rejected(_patch_conv(lib, addr, dtype=dtype), "bf16/f16")
    rejected(_patch_conv(lib, addr, h=3), "empty")                    # no output row
    rejected(_patch_conv(lib, addr, batch=0), "empty")
    rejected(_patch_conv(lib, addr, batch=64, h=1024, wd=1024, cin=64, cout=64), "32-bit")       # 2^33 bytes of input
    rejected(_patch_conv(lib, addr + 8), "aligned")
    # alignment is the last check: with a missing bias (allowed) the call gets that far
    rejected(_patch_conv(lib, addr + 8, bias=False), "aligned")

    for missing in ("img", "w", "bias", "ln_w", "ln_b", "y"):
        rejected(_patch_embed(lib, addr, **{missing: False}), "null")
    for form in ((3, 2, 1, 64), (7, 4, 3, 128), (4, 4, 0, 64), (7, 4, 2, 64), (7, 2, 3, 64), (4, 4, 0, 96), (16, 16, 0, 128)):
        k, stride, pad, cout = form
        rejected(_patch_embed(lib, addr, k=k, stride=stride, pad=pad, cout=cout), "neither")
    rejected(_patch_embed(lib, addr, dtype=F32), "output")
    rejected(_patch_embed(lib, addr, img_dtype=F16, dtype=BF16), "image")
    rejected(_patch_embed(lib, addr, k=4, stride=4, pad=0, cout=128, h=3), "empty")
    rejected(_patch_embed(lib, addr, batch=0), "empty")
    rejected(_patch_embed(lib, addr + 8), "aligned")
    del keep


def test_python_predicates_agree_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    # an accepted call would launch, so the C side is asked with a misaligned tensor: alignment is its LAST check, and
    # reaching it means that it found nothing to object to in the shape
    for dtype in (BF16, F16, F32):
        for cin, cout, r in ((64, 64, 8), (128, 128, 4), (320, 320, 2), (64, 8, 2), (96, 96, 2), (64, 12, 2), (64, 64, 1),
                             (64, 64, 9), (512, 512, 3), (32, 64, 2), (0, 64, 2)):
            want = hip.patch_conv_supported(_TORCH[dtype], cin, cout, r)
            rc = _patch_conv(lib, addr + (8 if want else 0), h=24, wd=24, cin=cin, cout=cout, r=r, dtype=dtype)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, cin, cout, r)
            seen.add(want)
        for form in ((7, 4, 3, 64), (4, 4, 0, 128), (3, 2, 1, 64), (7, 4, 3, 128), (4, 4, 0, 64), (4, 4, 1, 128), (7, 2, 3, 64)):
            want = hip.patch_embed_ln_supported(_TORCH[dtype], *form)
            k, stride, pad, cout = form
            rc = _patch_embed(lib, addr + (8 if want else 0), k=k, stride=stride, pad=pad, cout=cout, dtype=dtype)
            assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, form)
            seen.add(want)
    assert seen == {True, False}
    del keep


def test_bindings_refuse_cpu_tensors_and_mismatched_weights():
    from tramba_amd import hip
    bf = torch.bfloat16
    with pytest.raises(hip.TrambaHipError):
        hip.patch_conv_cl(torch.zeros(1, 8, 8, 64, dtype=bf), torch.zeros(64, 2, 2, 64, dtype=bf), torch.zeros(64))
    with pytest.raises(hip.TrambaHipError):
        hip.patch_embed_ln(torch.zeros(1, 3, 16, 16), torch.zeros(64, 3, 7, 7), torch.zeros(64), torch.ones(64), torch.zeros(64),
                           1e-5, 4, 3, bf)


def _switched(model):
    from tramba_amd import encoders
    return [m for m in model.modules()
            if isinstance(m, (encoders._OverlapPatchEmbed, encoders._SwinPatchEmbed))
            or (isinstance(m, encoders._PvtAttention) and m.sr_ratio > 1)]


@pytest.mark.parametrize("name,count", [("Tramba-P-TSOD", 42), ("Tramba-S-TSOD", 1)])
def test_switch_counts_modules_flips_back_and_leaves_the_state_dict_alone(name, count):
    import tramba_amd as ta
    from tramba_amd import encoders
    model = ta.bulid_model_enc(name)
    keys = list(model.state_dict().keys())
    mods = _switched(model)
    assert len(mods) == count and not any(m.library_convolutions for m in mods)                  # off by default
    assert encoders.set_library_convolutions(model) == count
    assert all(m.library_convolutions for m in mods)
    assert list(model.state_dict().keys()) == keys
    # PVT's last stage has sr_ratio 1: no convolution there, nothing to switch
    assert not any(m.library_convolutions for m in model.modules()
                   if isinstance(m, encoders._PvtAttention) and m.sr_ratio == 1)
    assert encoders.set_library_convolutions(model, enabled=False) == count
    assert not any(m.library_convolutions for m in mods)
    assert list(model.state_dict().keys()) == keys
    assert encoders.set_library_convolutions(torch.nn.Linear(4, 4)) == 0


@pytest.mark.parametrize("name,count", [("Tramba-P-TSOD", 42), ("Tramba-S-TSOD", 1)])
def test_build_sets_the_flags_only_when_asked(name, count):
    import tramba_amd as ta
    on = ta.build(name, SimpleNamespace(img_size=384, library_convolutions=True))
    assert sum(m.library_convolutions for m in _switched(on)) == count
    off = ta.build(name, SimpleNamespace(img_size=384))
    assert len(_switched(off)) == count and not any(m.library_convolutions for m in _switched(off))
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off = ta.build(name, SimpleNamespace(img_size=384, library_convolutions=False))
    assert not any(m.library_convolutions for m in _switched(off))
