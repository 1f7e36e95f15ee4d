"""CPU tests of the fused attention entries' host side: declared, bound and exported; every unsupported argument is refused
with a message before any launch; the Python predicates the encoder modules ask agree with the C checks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tramba_window_attn_cl", "tramba_kv_attn_cl")
F32, F16, BF16 = 0, 1, 2


def _lib():
    from tramba_amd import hip
    return hip.lib()


def _addr():
    # plausible non-null 16-byte aligned addresses: a rejected call never touches them
    buf = (ctypes.c_char * 256)()
    a = ctypes.addressof(buf)
    return buf, (a + 15) // 16 * 16


def _window(lib, addr, qkv=True, table=True, y=True, batch=2, h=24, w=24, heads=4, hd=32, ws=12, shift=6, dtype=BF16):
    return lib.tramba_window_attn_cl(addr if qkv else None, addr if table else None, addr if y else None, batch, h, w, heads,
                                     hd, ws, shift, dtype, None)


def _kv(lib, addr, q=True, kv=True, y=True, batch=2, n=144, m=144, heads=8, hd=64, dtype=BF16):
    return lib.tramba_kv_attn_cl(addr if q else None, addr if kv else None, addr if y else None, batch, n, m, heads, hd,
                                 dtype, None)


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in NAMES:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    for name in ("window_attention_cl", "kv_attention_cl", "window_attention_supported", "kv_attention_supported"):
        assert callable(getattr(hip, name)), name


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg

    for missing in ("qkv", "table", "y"):
        rejected(_window(lib, addr, **{missing: False}), "null")
    for dtype in (F32, 7):
        rejected(_window(lib, addr, dtype=dtype), "dtype")
    for hd in (16, 48, 128, 0):
        rejected(_window(lib, addr, hd=hd), "hd")
    for ws in (0, -3, 17):
        rejected(_window(lib, addr, ws=ws, h=17 * 4, w=17 * 4, shift=0), "ws")
    rejected(_window(lib, addr, h=25), "multiple of ws")            # H % ws != 0
    rejected(_window(lib, addr, w=30), "multiple of ws")
    for shift in (-1, 12, 40):
        rejected(_window(lib, addr, shift=shift), "shift")
    rejected(_window(lib, addr + 8), "aligned")

    for missing in ("q", "kv", "y"):
        rejected(_kv(lib, addr, **{missing: False}), "null")
    for dtype in (F32, -1):
        rejected(_kv(lib, addr, dtype=dtype), "dtype")
    for hd in (16, 96):
        rejected(_kv(lib, addr, hd=hd), "hd")
    for m in (0, -5, 257, 576):
        rejected(_kv(lib, addr, m=m), "M")
    rejected(_kv(lib, addr, n=0), "N")
    rejected(_kv(lib, addr + 4), "aligned")
    del keep


# (dtype, h, w, heads, hd, ws, shift)
WINDOW_SHAPES = [
    (BF16, 24, 24, 4, 32, 12, 6), (F16, 24, 36, 2, 32, 12, 6), (BF16, 12, 12, 2, 32, 12, 0), (BF16, 14, 14, 3, 32, 7, 3),
    (F16, 16, 16, 1, 64, 8, 4), (BF16, 16, 16, 2, 32, 16, 0), (BF16, 96, 96, 4, 32, 12, 6), (BF16, 16, 16, 2, 32, 16, 15),
    (F32, 24, 24, 4, 32, 12, 6), (BF16, 24, 24, 4, 16, 12, 6), (BF16, 24, 24, 4, 128, 12, 6), (BF16, 34, 34, 4, 32, 17, 0),
    (BF16, 25, 24, 4, 32, 12, 6), (BF16, 24, 30, 4, 32, 12, 0), (BF16, 24, 24, 4, 32, 12, 12), (BF16, 24, 24, 4, 32, 12, -1),
    (BF16, 24, 24, 4, 48, 12, 0),
]
# (dtype, m, heads, hd)
KV_SHAPES = [
    (BF16, 144, 8, 64), (F16, 36, 5, 64), (BF16, 1, 2, 32), (BF16, 17, 2, 32), (F16, 256, 1, 64),
    (F32, 144, 8, 64), (BF16, 257, 8, 64), (BF16, 576, 8, 64), (BF16, 0, 8, 64), (BF16, 144, 8, 16), (BF16, 144, 4, 128),
]
_TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


def test_python_predicates_agree_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    for dtype, h, w, heads, hd, ws, shift in WINDOW_SHAPES:
        want = hip.window_attention_supported(_TORCH[dtype], h, w, heads * hd, heads, ws, shift)
        if want:
            # an accepted call would launch, so the C side is asked with a misaligned tensor: alignment is its LAST check,
            # and reaching it means that it found nothing to object to in the shape
            rc = _window(lib, addr + 8, h=h, w=w, heads=heads, hd=hd, ws=ws, shift=shift, dtype=dtype)
            assert rc == -1 and "aligned" in lib.tramba_last_error().decode(), (h, w, heads, hd, ws, shift)
        else:
            rc = _window(lib, addr, h=h, w=w, heads=heads, hd=hd, ws=ws, shift=shift, dtype=dtype)
            assert rc == -1 and "aligned" not in lib.tramba_last_error().decode(), (h, w, heads, hd, ws, shift)
        seen.add(want)
    assert seen == {True, False}
    assert not hip.window_attention_supported(torch.bfloat16, 24, 24, 100, 3, 12, 0)        # C is no multiple of heads
    seen = set()
    for dtype, m, heads, hd in KV_SHAPES:
        want = hip.kv_attention_supported(_TORCH[dtype], m, heads * hd, heads)
        rc = _kv(lib, addr + (8 if want else 0), m=m, heads=heads, hd=hd, dtype=dtype)
        assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (m, heads, hd)
        seen.add(want)
    assert seen == {True, False}
    del keep


def test_binding_refuses_cpu_tensors():
    from tramba_amd import hip
    with pytest.raises(hip.TrambaHipError):
        hip.window_attention_cl(torch.zeros(1, 12, 12, 96, dtype=torch.bfloat16), torch.zeros(23 * 23, 1), 12, 0, 1)
    with pytest.raises(hip.TrambaHipError):
        hip.kv_attention_cl(torch.zeros(1, 16, 32, dtype=torch.bfloat16), torch.zeros(1, 4, 64, dtype=torch.bfloat16), 1)


def test_binding_refuses_no_heads_with_its_own_error():
    from tramba_amd import hip

    class OnDevice:                       # what _dev() looks at: the shape check comes before any pointer is taken
        is_cuda = True

        def __init__(self, t):
            self.t = t

        def is_contiguous(self):
            return True

        def __getattr__(self, name):
            return getattr(self.t, name)

    q = OnDevice(torch.zeros(1, 16, 32, dtype=torch.bfloat16))
    with pytest.raises(hip.TrambaHipError, match="kv_attention_cl"):
        hip.kv_attention_cl(q, OnDevice(torch.zeros(1, 4, 64, dtype=torch.bfloat16)), 0)
    with pytest.raises(hip.TrambaHipError, match="window_attention_cl"):
        hip.window_attention_cl(OnDevice(torch.zeros(1, 12, 12, 96, dtype=torch.bfloat16)), OnDevice(torch.zeros(529, 1)), 12, 0, 0)
    assert not hip.window_attention_supported(torch.bfloat16, 12, 12, 32, 0, 12, 0)
    assert not hip.kv_attention_supported(torch.bfloat16, 144, 64, 0)
