"""CPU tests of the frame pipeline's host side (csrc/frames.hip): the coefficient and normalisation tables the library
generates reproduce the loader's test transform exactly -- PIL's Image.resize(BILINEAR) through a numpy restatement of the
kernel's two integer passes, and to_tensors for all 256 byte values -- and bad sizes are rejected before any launch.
The GPU side: tests/test_gpu_frames.py."""
import numpy as np
import pytest
import torch
from PIL import Image

from tramba_amd import data

SIZES = [(384, 384), (384, 500), (500, 384), (200, 600), (600, 200), (1, 1), (2, 3000), (5, 7), (375, 500), (383, 385),
         (1080, 1920), (3000, 4000)]
TARGETS = [256, 384, 768]


def _table(h, w, oh, ow):
    from tramba_amd import hip
    return hip.resize_table_host(h, w, oh, ow, data.IMAGENET_MEAN, data.IMAGENET_STD)


def _split(table, h, w, oh, ow):
    """the table's sections (layout: csrc/frames.hip)"""
    kx = 1 if w == ow else int(np.ceil(max(w / ow, 1.0))) * 2 + 1
    ky = 1 if h == oh else int(np.ceil(max(h / oh, 1.0))) * 2 + 1
    o = 0
    xb = table[o:o + 2 * ow].reshape(ow, 2); o += 2 * ow
    xk = table[o:o + ow * kx].reshape(ow, kx); o += ow * kx
    yb = table[o:o + 2 * oh].reshape(oh, 2); o += 2 * oh
    yk = table[o:o + oh * ky].reshape(oh, ky); o += oh * ky
    lut = table[o:o + 768].view(np.float32).reshape(3, 256)
    assert o + 768 == table.size
    return xb, xk, yb, yk, lut


def _pass(img, bounds, coef, axis):
    """one integer pass along `axis` of an (H, W, 3) u8 image: 2^21 + sum px k, >> 22, clamped"""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for i, (lo, n) in enumerate(bounds):
        out[i] = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), src[lo:lo + n], axes=1)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), 0, axis)


def _frame(h, w, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[: h // 2, : w // 2] = 255                       # saturated and flat regions exercise the clamp
    img[h // 2:, w // 2:] = 0
    return img


@pytest.mark.parametrize("s", TARGETS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_resize_tables_reproduce_pil_bilinear(hw, s):
    h, w = hw
    img = _frame(h, w, h * 7919 + w)
    table = _table(h, w, s, s)
    xb, xk, yb, yk, _ = _split(table, h, w, s, s)
    assert (xb[:, 1] >= 1).all() and (xb[:, 0] + xb[:, 1] <= w).all() and (yb[:, 0] + yb[:, 1] <= h).all()
    # the horizontal pass only for the rows the vertical pass reads, as the kernel does
    lo, hi = yb[0, 0], yb[-1, 0] + yb[-1, 1]
    mid = np.zeros((h, s, 3), np.uint8)
    mid[lo:hi] = _pass(img[lo:hi], xb, xk, axis=1)
    got = _pass(mid, yb, yk, axis=0)
    want = np.asarray(Image.fromarray(img).resize((s, s), Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


def test_unchanged_axis_is_a_copy():
    table = _table(384, 500, 384, 384)
    xb, xk, yb, yk, _ = _split(table, 384, 500, 384, 384)
    assert yk.shape == (384, 1) and (yk[:, 0] == 1 << 22).all() and (yb[:, 0] == np.arange(384)).all()
    assert (yb[:, 1] == 1).all()


def test_normalisation_table_equals_to_tensors_for_every_byte():
    _, _, _, _, lut = _split(_table(4, 4, 4, 4), 4, 4, 4, 4)
    img = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, axis=-1)
    want = data.to_tensors({"image": Image.fromarray(img)})["image"].numpy().reshape(3, 256)
    assert lut.dtype == np.float32 and np.array_equal(lut.view(np.int32), want.view(np.int32))
    # the all-fp32 restatement is NOT the loader's rule: the fp64 operands matter
    f = np.arange(256, dtype=np.float32) / np.float32(255)
    fp32 = (f[None] - np.asarray(data.IMAGENET_MEAN, np.float32)[:, None]) / np.asarray(data.IMAGENET_STD, np.float32)[:, None]
    assert not np.array_equal(fp32.astype(np.float32), want)


def test_frame_entries_are_exported_and_bound():
    from tramba_amd import hip
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_resize_table_words", "tramba_resize_table", "tramba_frames_to_input", "tramba_logits_to_u8"):
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.tramba_resize_table_words(1080, 1920, 384, 384) > 768


def test_bad_sizes_are_rejected_not_fatal():
    from tramba_amd import hip
    lib = hip.lib()
    m = np.asarray(data.IMAGENET_MEAN, np.float64)
    sd = np.asarray(data.IMAGENET_STD, np.float64)
    buf = np.zeros(1 << 16, np.int32)
    p = buf.ctypes.data          # never dereferenced by a kernel: every call below is rejected before a launch
    big, out_big = hip.FRAME_MAX_DIM + 1, hip.FRAME_MAX_OUT + 1
    for hw in ((0, 8), (8, 0), (big, 8), (8, big), (-1, 8)):
        assert lib.tramba_resize_table_words(hw[0], hw[1], 384, 384) == 0
        assert lib.tramba_resize_table(hw[0], hw[1], 384, 384, m.ctypes.data, sd.ctypes.data, p, buf.size) < 0
        assert lib.tramba_frames_to_input(p, p, p, 1, hw[0], hw[1], 384, 384, 0, None) < 0
    assert lib.tramba_resize_table_words(8, 8, out_big, 8) == 0 and lib.tramba_resize_table_words(8, 8, 8, 0) == 0
    assert lib.tramba_resize_table(8, 8, 4, 4, m.ctypes.data, sd.ctypes.data, p, 10) < 0
    assert b"words" in lib.tramba_last_error()
    assert lib.tramba_resize_table(8, 8, 4, 4, None, sd.ctypes.data, p, buf.size) < 0
    assert lib.tramba_frames_to_input(None, p, p, 1, 8, 8, 4, 4, 0, None) < 0 and b"null" in lib.tramba_last_error()
    assert lib.tramba_frames_to_input(p, p, p, 0, 8, 8, 4, 4, 0, None) < 0
    assert lib.tramba_frames_to_input(p, p, p, 1, 8, 8, out_big, 4, 0, None) < 0
    assert lib.tramba_logits_to_u8(None, p, 1, 8, 8, 16, 16, hip.F32, None) < 0
    assert lib.tramba_logits_to_u8(p, p, 1, 8, 8, big, 16, hip.F32, None) < 0
    assert lib.tramba_logits_to_u8(p, p, 1, out_big, 8, 16, 16, hip.F32, None) < 0
    assert lib.tramba_logits_to_u8(p, p, 1, 8, 8, 16, 16, 7, None) < 0 and b"dtype" in lib.tramba_last_error()
    with pytest.raises(hip.TrambaHipError):
        hip.resize_table_host(big, 8, 384, 384, data.IMAGENET_MEAN, data.IMAGENET_STD)


def test_wrappers_refuse_host_tensors_and_bad_frames():
    from tramba_amd import hip, infer
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(hip.TrambaHipError):
        hip.frames_to_input(frames, torch.zeros(4096, dtype=torch.int32), 4, 4)     # host tensors: no CPU path
    with pytest.raises(hip.TrambaHipError):
        hip.logits_to_u8(torch.zeros(1, 1, 8, 8), 16, 16)
    for bad in (np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8), np.uint8),
                np.zeros((1, 1, 8, 8, 3), np.uint8)):
        with pytest.raises((TypeError, ValueError)):
            infer.check_frames(bad)
    with pytest.raises(ValueError):
        infer.check_frames(np.zeros((1, hip.FRAME_MAX_DIM + 1, 1, 3), np.uint8))
