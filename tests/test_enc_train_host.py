"""CPU tests of the host side of the patch-convolution backward entries and of the encoder training switch: the entries are
declared, bound and exported; every unsupported argument, a missing and a one-byte-short workspace included, is refused
with a message before any launch; the workspace size is a pure function of the shape; the Python predicate the encoder asks
agrees with the C checks; `set_library_training` counts the modules it flips and leaves the state_dict alone."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from test_attn_host import BF16, F16, F32, _TORCH, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tramba_patch_conv_dgrad_cl", "tramba_patch_conv_wgrad_cl", "tramba_patch_conv_wgrad_work",
         "tramba_patch_conv_wgrad_split")
BIG = 1 << 40          # a workspace size no shape here needs: the check it satisfies is the entry's last


def _dgrad(lib, addr, gy=True, w=True, gx=True, off=0, batch=2, h=24, wd=24, cin=128, cout=128, r=4, dtype=BF16):
    p = lambda on: addr + off if on else None
    return lib.tramba_patch_conv_dgrad_cl(p(gy), p(w), p(gx), batch, h, wd, cin, cout, r, dtype, None)


def _wgrad(lib, addr, gy=True, x=True, work=True, work_bytes=BIG, off=0, batch=2, h=24, wd=24, cin=128, cout=128, r=4,
           dtype=BF16, want_bias=1):
    p = lambda on: addr + off if on else None
    return lib.tramba_patch_conv_wgrad_cl(p(gy), p(x), addr if work else None, work_bytes, batch, h, wd, cin, cout, r,
                                          want_bias, dtype, None)


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import encoders, hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in NAMES:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    for name in ("patch_conv_train_supported", "patch_conv_dgrad_cl", "patch_conv_wgrad_cl"):
        assert callable(getattr(hip, name)), name
    assert issubclass(encoders._PatchConvFn, torch.autograd.Function) and callable(encoders.set_library_training)
    # each new entry cites the reference lines it serves
    for name in NAMES[:2]:
        at = hdr.index("int " + name + "(")
        assert "pvtv2_encoder.py" in hdr[at - 2500:at], name


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg

    for call, tensors in ((_dgrad, ("gy", "w", "gx")), (_wgrad, ("gy", "x"))):
        for missing in tensors:
            rejected(call(lib, addr, **{missing: False}), "null")
        for dtype in (F32, 7, -1):
            rejected(call(lib, addr, dtype=dtype), "dtype")
        for r in (1, 9, 0, -2):
            rejected(call(lib, addr, r=r), "stride")
        for cin in (32, 96, 65, 0):
            rejected(call(lib, addr, cin=cin), "Cin" if cin else "empty")
        for cout in (4, 12, 127, 0):
            rejected(call(lib, addr, cout=cout), "Cout" if cout else "empty")
        rejected(call(lib, addr, h=3), "empty")                       # a map smaller than one patch
        rejected(call(lib, addr, batch=0), "empty")
        rejected(call(lib, addr, batch=4096, h=512, wd=512), "32-bit")
        for off in (8, 4, 2):
            rejected(call(lib, addr, off=off), "aligned")
    need = lib.tramba_patch_conv_wgrad_work(2, 24, 24, 128, 128, 4)
    nsplit = lib.tramba_patch_conv_wgrad_split(2, 24, 24, 128, 128, 4)
    assert nsplit >= 1 and need == nsplit * (128 * 16 * 128 + 128) * 4
    rejected(_wgrad(lib, addr, work=False), "workspace")
    rejected(_wgrad(lib, addr, work_bytes=need - 1), "workspace")
    rejected(_wgrad(lib, addr, work_bytes=0), "workspace")
    del keep


def test_workspace_size_is_pure_and_the_split_depends_on_the_shape_alone():
    lib = _lib()
    for cin, cout, r in ((64, 64, 8), (128, 128, 4), (320, 320, 2), (64, 8, 2), (512, 512, 2)):
        for h, wd in ((96, 96), (20, 28), (26, 22), (8, 8)):
            sizes = [lib.tramba_patch_conv_wgrad_work(b, h, wd, cin, cout, r) for b in (1, 2, 3, 4, 8)]
            splits = [lib.tramba_patch_conv_wgrad_split(b, h, wd, cin, cout, r) for b in (1, 2, 3, 4, 8)]
            assert sizes == [lib.tramba_patch_conv_wgrad_work(b, h, wd, cin, cout, r) for b in (1, 2, 3, 4, 8)]
            slab = (cout * r * r * cin + cout) * 4
            assert all(s >= 1 for s in splits) and sizes == [s * slab for s in splits], (cin, cout, r, h, wd)
            # a run is a whole number of 32-token steps and no run is empty
            for b, s in zip((1, 2, 3, 4, 8), splits):
                steps = (b * (h // r) * (wd // r) + 31) // 32
                assert s <= steps and s <= 16
    # shapes the entries refuse need nothing
    assert lib.tramba_patch_conv_wgrad_work(1, 24, 24, 96, 128, 4) == 0 and lib.tramba_patch_conv_wgrad_split(1, 24, 24, 128, 12, 4) == 0
    assert lib.tramba_patch_conv_wgrad_work(1, 24, 24, 128, 128, 9) == 0 and lib.tramba_patch_conv_wgrad_work(0, 24, 24, 128, 128, 4) == 0


def test_python_predicate_agrees_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    for dtype in (BF16, F16, F32):
        for r in (1, 2, 3, 4, 8, 9):
            for cin in (32, 64, 96, 128, 320):
                for cout in (4, 8, 60, 64, 320):
                    want = hip.patch_conv_train_supported(_TORCH[dtype], cin, cout, r)
                    # an accepted call would launch, so the C side is asked with a misaligned tensor: alignment is the last
                    # check of the shape (only the workspace follows), and reaching it means nothing else was objected to
                    for call in (_dgrad, _wgrad):
                        rc = call(lib, addr, off=8 if want else 0, h=8 * r, wd=8 * r, cin=cin, cout=cout, r=r, dtype=dtype)
                        assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (dtype, r, cin, cout)
                    # the workspace query knows no dtype: it follows the shape checks alone
                    assert (lib.tramba_patch_conv_wgrad_work(1, 8 * r, 8 * r, cin, cout, r) > 0) == \
                        hip.patch_conv_train_supported(torch.bfloat16, cin, cout, r)
                    seen.add(want)
    assert seen == {True, False}
    # the f32 weight gradient of a layer must stay below 2^31 bytes: the forward's domain is wider there
    assert hip.patch_conv_supported(torch.bfloat16, 4096, 4096, 8) and not hip.patch_conv_train_supported(torch.bfloat16, 4096, 4096, 8)
    rc = _dgrad(lib, addr, off=8, h=8, wd=8, cin=4096, cout=4096, r=8)
    assert rc == -1 and "32-bit" in lib.tramba_last_error().decode()
    del keep


def test_bindings_refuse_cpu_tensors_and_mismatched_shapes():
    from tramba_amd import hip
    bf = torch.bfloat16
    with pytest.raises(hip.TrambaHipError):
        hip.patch_conv_dgrad_cl(torch.zeros(1, 4, 4, 8, dtype=bf), torch.zeros(8, 2, 2, 64, dtype=bf), (1, 8, 8, 64))
    with pytest.raises(hip.TrambaHipError):
        hip.patch_conv_wgrad_cl(torch.zeros(1, 4, 4, 8, dtype=bf), torch.zeros(1, 8, 8, 64, dtype=bf), 2)


def test_switch_counts_modules_flips_back_and_leaves_the_state_dict_alone():
    import tramba_amd as ta
    from tramba_amd import encoders
    swin = encoders.SwinTransformer(img_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)
    pvt = encoders.pvt_v2_b4()
    for model in (swin, pvt):
        keys = list(model.state_dict().keys())
        nparams = len(list(model.parameters()))
        leaves = [m for m in model.modules() if isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm, torch.nn.Conv2d))]
        assert not any(getattr(m, "library_training", False) for m in model.modules())              # off by default
        count = encoders.set_library_training(model)
        assert count > len(leaves) and all(m.library_training for m in leaves)                       # every op, and the blocks
        assert list(model.state_dict().keys()) == keys and len(list(model.parameters())) == nparams
        assert encoders.set_library_training(model, False) == count
        assert not any(getattr(m, "library_training", False) for m in model.modules())
        assert list(model.state_dict().keys()) == keys
    assert encoders.set_library_training(torch.nn.Linear(4, 4)) == 0
    # build(): args.library_training, off unless asked for
    for name in ("Tramba-P-TSOD", "Tramba-S-TSOD"):
        on = ta.build(name, SimpleNamespace(img_size=384, library_training=True))
        flagged = [m for m in on.modules() if getattr(m, "library_training", False)]
        assert flagged and all(any(m is e for e in on.encoder.modules()) for m in flagged)          # the encoder only
        off = ta.build(name, SimpleNamespace(img_size=384))
        assert not any(getattr(m, "library_training", False) for m in off.modules())
        assert list(on.state_dict().keys()) == list(off.state_dict().keys())
