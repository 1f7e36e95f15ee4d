"""CPU tests of the device train transform's host side (tramba_amd/augment.py, csrc/augment.hip): the tables the library
builds, run through numpy restatements of the kernels' integer and fp32 passes, give Pillow's bytes (bicubic and nearest
resize, rotate + centre crop, the three enhancers); the draw recorder consumes numpy's stream exactly as data.Augment; bad
sizes are rejected before any launch.  The GPU side: tests/test_gpu_augment.py."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from tramba_amd import augment, data, hip

SIZES = [(384, 384), (384, 500), (500, 384), (200, 600), (600, 200), (1, 1), (2, 3000), (5, 7), (375, 500), (383, 385),
         (1080, 1920), (3000, 4000)]
TARGETS = [256, 384, 768]
LO, HI = 1040, 1042


def _image(h, w, seed, channels=3):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, channels)).astype(np.uint8)
    img[: h // 3, : w // 3] = 255                       # flat and saturated regions exercise the clamps
    img[2 * h // 3:, 2 * w // 3:] = 0
    return img if channels == 3 else img[..., 0]


def _pass(img, bounds, coef, axis):
    """one integer pass along `axis`: 2^21 + sum px k, floor(/ 2^22), clamped at both ends (the kernels' clip)"""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    taps = coef.shape[1]
    idx = np.minimum(bounds[:, :1] + np.arange(taps)[None], src.shape[0] - 1)
    k = np.where(np.arange(taps)[None] < bounds[:, 1:2], coef, 0).astype(np.int64)
    acc = (1 << 21) + np.einsum("ot,ot...->o...", k, src[idx])
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def _scale_axis(host, size, r):
    off = int(host[HI + r - int(host[LO])])
    taps = hip.augment_scale_taps(size, r)
    bounds = host[off:off + 2 * r].reshape(r, 2)
    coef = host[off + 2 * r:off + 2 * r + r * taps].reshape(r, taps)
    return bounds, coef


def _bicubic(img, host, size, r):
    bounds, coef = _scale_axis(host, size, r)
    return _pass(_pass(img, bounds, coef, 1), bounds, coef, 0)


def _reachable(size):
    return sorted({int(np.round(size * f)) for f in np.linspace(0.75, 1.25, 4001)[:-1]} - {size})


@pytest.mark.parametrize("size", [32, 256, 384])
def test_bicubic_tables_reproduce_pil_resize(size):
    host = hip.augment_size_table_host(size, data.IMAGENET_MEAN, data.IMAGENET_STD)
    assert host[LO] <= min(_reachable(size)) and max(_reachable(size)) <= host[LO + 1]
    rgb = _image(size, size, size)
    gray = _image(size, size, size + 1, channels=1)
    for r in _reachable(size):
        for img in (rgb, gray):
            want = np.asarray(Image.fromarray(img).resize((r, r)))        # PIL's default filter: bicubic
            assert np.array_equal(_bicubic(img, host, size, r), want), (size, r, img.ndim)


def _source(h, w, size):
    t = hip.augment_source_table_host(h, w, size)
    rw = hip.lib().tramba_resize_table_words(h, w, size, size)
    return t[4 + rw:4 + rw + size], t[4 + rw + size:4 + rw + 2 * size], t


@pytest.mark.parametrize("size", TARGETS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_nearest_tables_reproduce_pil_resize(hw, size):
    h, w = hw
    mask = _image(h, w, h * 31 + w, channels=1)
    nx, ny, t = _source(h, w, size)
    got = np.where((ny[:, None] >= 0) & (nx[None] >= 0), mask[np.maximum(ny, 0)[:, None], np.maximum(nx, 0)[None]], 0)
    want = np.asarray(Image.fromarray(mask).resize((size, size), Image.NEAREST))
    assert np.array_equal(got, want)
    # the bilinear words in front are tramba_resize_table's, unchanged
    rw = hip.lib().tramba_resize_table_words(h, w, size, size)
    bil = hip.resize_table_host(h, w, size, size, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(t[4:4 + rw], bil)


def _rotate(img, coef):
    s = img.shape[0]
    y, x = np.mgrid[0:s, 0:s].astype(np.int64)
    sx = (coef[2] + x * coef[0] + y * coef[1]) >> 16
    sy = (coef[5] + x * coef[3] + y * coef[4]) >> 16
    ok = (sx >= 0) & (sx < s) & (sy >= 0) & (sy < s)
    out = img[np.clip(sy, 0, s - 1), np.clip(sx, 0, s - 1)]
    out[~ok] = 0
    return out


@pytest.mark.parametrize("size", [32, 256, 384])
def test_rotation_words_reproduce_pil_rotate_and_crop(size):
    img = _image(size, size, 5 + size)
    for deg in range(-10, 10):
        deg = deg + 360 if deg < 0 else deg
        turned = Image.fromarray(img).rotate(deg, expand=True)
        want = np.asarray(turned.crop(data._centre_box(turned.size, (size, size))))
        if deg == 0:
            assert np.array_equal(want, img)                 # a copy: the kernels skip it
            with pytest.raises(hip.TrambaHipError):
                hip.augment_rotation(size, 0)
            continue
        assert np.array_equal(_rotate(img, hip.augment_rotation(size, deg)), want), deg


# ----------------------------------------------------------------------------- enhancers (the kernel's arithmetic)
def _blend(deg, px, factor):
    a = np.float32(factor)
    t = deg.astype(np.float32) + a * (px.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def _contrast(img, factor):
    l = (img[..., 0].astype(np.int64) * 19595 + img[..., 1].astype(np.int64) * 38470 + img[..., 2].astype(np.int64) * 7471
         + 0x8000) >> 16
    mean = int(float(l.sum()) / l.size + 0.5)
    return _blend(np.full_like(img, mean), img, factor)


def _smooth(img, kern):
    h, w, _ = img.shape
    f = img.astype(np.float32)
    out = img.copy()
    ss = np.zeros((h - 2, w - 2, 3), np.float32)
    for r, dy in enumerate((1, 0, -1)):                # Pillow's order: the row below, the row, the row above
        row = f[1 + dy:h - 1 + dy]
        ss += row[:, :-2] * kern[3 * r] + row[:, 1:-1] * kern[3 * r + 1] + row[:, 2:] * kern[3 * r + 2]
    inner = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.floor(ss.astype(np.float64) + 0.5)))
    out[1:-1, 1:-1] = inner.astype(np.uint8)
    return out


def _sharpness(img, factor, kern):
    return _blend(_smooth(img, kern), img, factor)


@pytest.mark.parametrize("size", [32, 256, 384])
def test_enhancer_arithmetic_reproduces_pil(size):
    kern = hip.augment_size_table_host(size, data.IMAGENET_MEAN, data.IMAGENET_STD)[1024:1033].view(np.float32)
    rs = np.random.RandomState(size)
    img = _image(size, size, 77 + size)
    mine = {hip.AUG_CONTRAST: _contrast, hip.AUG_BRIGHTNESS: lambda i, f: _blend(np.zeros_like(i), i, f),
            hip.AUG_SHARPNESS: lambda i, f: _sharpness(i, f, kern)}
    pil = {hip.AUG_CONTRAST: ImageEnhance.Contrast, hip.AUG_BRIGHTNESS: ImageEnhance.Brightness,
           hip.AUG_SHARPNESS: ImageEnhance.Sharpness}
    for trial in range(12):                            # every enhancer on the outputs of the others
        order = rs.permutation(3)
        cur = img
        for code in order:
            factor = float(1 + rs.random_sample() / 10)
            want = np.asarray(pil[code](Image.fromarray(cur)).enhance(factor))
            got = mine[code](cur, factor)
            assert np.array_equal(got, want), (trial, code)
            cur = want


# ----------------------------------------------------------------------------- the draws
class _Log:
    """numpy's legacy generator, logging every call"""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        fn = getattr(self.rs, name)

        def call(*a):
            r = fn(*a)
            self.calls.append((name, a, None if r is None else float(r)))
            return r
        return call


@pytest.mark.parametrize("seed", [1026, 7, 123457])
def test_recorder_makes_augments_draws(seed):
    size = 32
    ref, rec = _Log(seed), _Log(seed)
    aug, recorder = data.Augment(ref), augment.DrawRecorder(rec)
    img = Image.fromarray(_image(size, size, 3))
    gt = Image.fromarray(_image(size, size, 4, channels=1))
    seen = set()
    for i in range(200):
        before = len(ref.calls)
        aug({"image": img, "gt": gt})
        r = recorder(size)
        calls = ref.calls[before:]
        assert calls == rec.calls[before:], i
        # the decisions, read back from Augment's own draws
        f = calls[0][2] * 0.5 + 0.75
        assert r["scale"] == (int(np.round(size * f)) if calls[1][2] < 0.5 else 0)
        assert r["mirror"] == (calls[2][2] < 0.5)
        deg = int(calls[4][2]) % 360
        assert r["degrees"] == (deg if calls[5][2] < 0.5 else None)
        assert [augment._ENH_CODE[m] for m in aug.enhancers] == [augment._ENH_CODE[m] for m in recorder.enhancers]
        seen.add(len(r["enhance"]))
    assert ref.rs.random_sample() == rec.rs.random_sample()      # same stream position
    assert seen == {0, 1, 2, 3}


def test_pack_layout():
    size = 32
    pairs = [(_image(h, w, h + w), _image(h, w, h * w, channels=1), {"scale": r, "mirror": m, "degrees": d, "enhance": e})
             for (h, w), r, m, d, e in [((5, 7), 40, True, 3, [(2, 1.05)]), ((33, 20), 32, False, 0, []),
                                         ((1, 1), 0, False, None, [(0, 1.0), (1, 1.09), (2, 1.01)])]]
    batch = augment.pack(pairs, size)
    desc = augment.descriptors(batch)
    flat = batch["packed"].numpy()
    for d, (img, gt, rec) in zip(desc, pairs):
        h, w = gt.shape
        assert (d[augment._D_H], d[augment._D_W]) == (h, w)
        assert np.array_equal(flat[d[augment._D_IMG]:d[augment._D_IMG] + h * w * 3], img.reshape(-1))
        assert np.array_equal(flat[d[augment._D_MASK]:d[augment._D_MASK] + h * w], gt.reshape(-1))
    assert desc[0, augment._D_R] == 40 and desc[0, augment._D_OFF] == 4 and desc[0, augment._D_ROT] == 1
    assert desc[1, augment._D_R] == 0 and desc[1, augment._D_ROT] == 0          # R == S and 0 degrees are copies
    assert desc[2, augment._D_ENH] == 3 and list(desc[2, augment._D_OP:augment._D_OP + 3]) == [0, 1, 2]


def test_bad_sizes_are_rejected():
    with pytest.raises(hip.TrambaHipError):
        hip.augment_source_table_host(hip.FRAME_MAX_DIM + 1, 10, 32)
    with pytest.raises(hip.TrambaHipError):
        hip.augment_source_table_host(10, 10, hip.FRAME_MAX_OUT + 1)
    with pytest.raises(hip.TrambaHipError):
        hip.augment_source_table_host(0, 10, 32)
    with pytest.raises(hip.TrambaHipError):
        hip.augment_size_table_host(2, data.IMAGENET_MEAN, data.IMAGENET_STD)
    with pytest.raises(hip.TrambaHipError):
        hip.augment_size_table_host(hip.FRAME_MAX_OUT + 1, data.IMAGENET_MEAN, data.IMAGENET_STD)
    with pytest.raises(hip.TrambaHipError):
        hip.augment_scale_taps(32, 32)                     # R == S is a copy, not a table
    with pytest.raises(hip.TrambaHipError):
        hip.augment_scale_taps(32, 41)
    assert hip.lib().tramba_augment_workspace(0, 32) == 0 and hip.lib().tramba_augment_workspace(1, 2) == 0
    # the C entry point checks the host descriptors before any launch (no device needed to be refused)
    pairs = [(_image(4, 4, 1), _image(4, 4, 2, channels=1), {"scale": 0, "mirror": False, "degrees": None, "enhance": []})]
    batch = augment.pack(pairs, 32)
    desc = augment.descriptors(batch).copy()
    desc[0, augment._D_SRC] = 1
    dummy = 1                                               # never dereferenced: refused before any launch
    for word, value in ((augment._D_H, hip.FRAME_MAX_DIM + 1), (augment._D_W, 0), (augment._D_R, 41),
                        (augment._D_IMG, 1 << 40), (augment._D_ENH, 4)):
        bad = desc.copy()
        bad[0, word] = value
        rc = hip.lib().tramba_augment_batch(dummy, bad.ctypes.data, batch["packed"].numel(), dummy, dummy, dummy, dummy,
                                            1 << 30, 1, 32, None)
        assert rc < 0, word
    rc = hip.lib().tramba_augment_batch(dummy, desc.ctypes.data, batch["packed"].numel(), dummy, dummy, dummy, dummy,
                                        1 << 30, 1, hip.FRAME_MAX_OUT + 1, None)
    assert rc < 0
    with pytest.raises(hip.TrambaHipError):
        hip.augment_batch(torch.zeros(8, dtype=torch.uint8), desc, torch.zeros(1, dtype=torch.int32), 32,
                          torch.zeros(1, dtype=torch.uint8))
