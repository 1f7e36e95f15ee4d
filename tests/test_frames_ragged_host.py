"""CPU tests of the mixed-size frame path's host side (tramba_amd/infer.py pack_frames, csrc/frames.hip
tramba_frames_ragged_check): the packed layout and its descriptors, every refusal of the descriptor check (an error code
and a message, never an abort, never a launch), the capacity buckets and the folder grouping of predict_folder(batch=N).
The GPU side: tests/test_gpu_frames_ragged.py."""
import os
import re

import numpy as np
import pytest
import torch

from tramba_amd import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 7), (2, 3000), (1080, 1920), (3000, 4000)]
S = 384
# descriptor words (include/tramba_hip.h)
FRAME, H, W, TABLE, KX, KY, OUT, RH, RW = range(9)


def _frame(h, w, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[: h // 2, : w // 2] = 255
    img[h // 2:, w // 2:] = 0
    return img


def _taps(n, s):
    return 1 if n == s else int(np.ceil(max(n / s, 1.0))) * 2 + 1


@pytest.fixture(scope="module")
def packed():
    from tramba_amd import infer
    frames = [_frame(h, w, 11 + k) for k, (h, w) in enumerate(SIZES)]
    frames[1] = torch.from_numpy(frames[1])                  # numpy and torch frames mix
    batch = infer.pack_frames(frames, S)
    return frames, batch, infer.descriptors(batch)


def test_pack_frames_layout_and_round_trip(packed):
    from tramba_amd import hip, infer
    frames, batch, desc = packed
    buf = batch["packed"]
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and batch["batch"] == len(SIZES) and batch["img_size"] == S
    assert desc.shape == (len(SIZES), hip.FRAMES_DESC_WORDS) and desc.dtype == np.int64
    head = len(SIZES) * hip.FRAMES_DESC_WORDS * 8
    flat = buf.numpy()
    assert np.array_equal(flat[:head].view(np.int64).reshape(desc.shape), desc)        # the descriptors lead the buffer
    end = 0
    for d, f, (h, w) in zip(desc, frames, SIZES):
        assert (d[H], d[W]) == (h, w) and (d[KX], d[KY]) == (_taps(w, S), _taps(h, S))
        assert d[FRAME] >= head and d[FRAME] % 16 == 0 and d[FRAME] + h * w * 3 <= buf.numel()
        assert np.array_equal(flat[d[FRAME]:d[FRAME] + h * w * 3].reshape(h, w, 3), np.asarray(f))
        table = hip.resize_table_host(h, w, S, S, data.IMAGENET_MEAN, data.IMAGENET_STD)
        assert d[TABLE] >= head and d[TABLE] % 16 == 0
        assert np.array_equal(flat[d[TABLE]:d[TABLE] + table.nbytes].view(np.int32), table)
        assert d[OUT] % 16 == 0 and d[OUT] >= end                   # maps aligned, increasing, disjoint
        end = d[OUT] + h * w
        assert np.array([d[RH], d[RW]]).astype(np.uint32).view(np.float32).tolist() == \
            [np.float32(S) / np.float32(h), np.float32(S) / np.float32(w)]
        assert (d[RW + 1:] == 0).all()
    assert infer.output_bytes(desc) == -(-end // 16) * 16
    assert infer.frame_sizes(desc) == SIZES


def test_equal_sizes_share_one_table():
    from tramba_amd import infer
    batch = infer.pack_frames([_frame(40, 60, 1), _frame(30, 30, 2), _frame(40, 60, 3)], S)
    desc = infer.descriptors(batch)
    assert desc[0, TABLE] == desc[2, TABLE] != desc[1, TABLE] and desc[0, FRAME] != desc[2, FRAME]


def test_pack_frames_is_a_collate_function():
    from torch.utils.data import DataLoader
    from tramba_amd import infer
    frames = [_frame(8 + k, 9 + 2 * k, k) for k in range(5)]
    batches = list(DataLoader(frames, batch_size=2, collate_fn=infer.PackFrames(S)))
    assert [b["batch"] for b in batches] == [2, 2, 1]
    assert infer.frame_sizes(infer.descriptors(batches[1])) == [(10, 13), (11, 15)]


def _check(desc, size=S, packed_bytes=None, capacity=None, batch=None, parts=3):
    from tramba_amd import hip
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    rc = hip.lib().tramba_frames_ragged_check(desc.ctypes.data, desc.shape[0] if batch is None else batch, size,
                                              packed_bytes, capacity, parts)
    return rc, hip.lib().tramba_last_error()


def test_check_accepts_what_pack_frames_makes(packed):
    from tramba_amd import hip, infer
    _, batch, desc = packed
    n, cap = batch["packed"].numel(), infer.output_bytes(desc)
    assert _check(desc, S, n, cap)[0] == 0
    assert _check(desc, S, n + 5, 2 * cap)[0] == 0
    hip.frames_ragged_check(desc, S, n, cap)                       # the wrapper: no exception
    assert _check(desc, S, n, 0, parts=hip.RAGGED_IN)[0] == 0        # the input half does not look at the outputs
    assert _check(desc, S, 0, cap, parts=hip.RAGGED_OUT)[0] == 0     # nor the output half at the inputs


def test_check_refuses_bad_descriptors(packed):
    from tramba_amd import hip
    _, batch, good = packed
    n, cap = batch["packed"].numel(), int(good[-1, OUT] + good[-1, H] * good[-1, W])
    head = good.shape[0] * hip.FRAMES_DESC_WORDS * 8

    def refused(word_edits, needle, **kw):
        d = good.copy()
        for (i, word), v in word_edits.items():
            d[i, word] = v
        args = dict(size=S, packed_bytes=n, capacity=cap)
        args.update(kw)
        rc, msg = _check(d, **args)
        assert rc < 0 and needle in msg, (word_edits, kw, rc, msg)

    refused({(1, H): 0}, b"side")
    refused({(1, W): -3}, b"side")
    refused({(2, W): hip.FRAME_MAX_DIM + 1}, b"side")
    refused({(3, FRAME): n - 10}, b"outside")                       # the frame runs past the buffer
    refused({(3, FRAME): n + 16}, b"outside")
    refused({(0, FRAME): 1 << 62}, b"outside")
    refused({(0, FRAME): head - 16}, b"descriptor")                 # inside the descriptor area
    refused({(0, FRAME): -16}, b"descriptor")
    refused({(2, TABLE): 0}, b"descriptor")
    refused({(2, TABLE): n - 64}, b"outside")
    refused({(2, TABLE): int(good[2, TABLE]) + 2}, b"align")
    refused({(1, KX): int(good[1, KX]) + 2}, b"taps")
    refused({(4, KY): 1}, b"taps")
    refused({(1, OUT): int(good[1, OUT]) + 8}, b"align")
    refused({(2, OUT): int(good[1, OUT])}, b"increas")               # equal: not increasing
    refused({(2, OUT): 0, (1, OUT): 16, (0, OUT): 32}, b"increas")   # decreasing
    refused({(4, OUT): int(good[3, OUT]) + 16}, b"overlap")          # starts inside map 3 (1080x1920)
    refused({(0, OUT): -16}, b"increas")
    refused({}, b"capacity", capacity=cap - 1)
    refused({}, b"capacity", capacity=0)
    refused({(3, RH): int(good[3, RH]) + 1}, b"scale")
    refused({(3, RW): 0}, b"scale")
    refused({}, b"batch", batch=0)
    refused({}, b"batch", batch=65536)
    refused({}, b"batch", batch=-1)
    refused({}, b"size", size=2)
    refused({}, b"size", size=hip.FRAME_MAX_OUT + 1)
    refused({}, b"outside", packed_bytes=n - 1)
    refused({}, b"descriptor", packed_bytes=head - 8)
    refused({}, b"parts", parts=0)
    assert hip.lib().tramba_frames_ragged_check(None, 1, S, 1024, 1024, 3) < 0 and b"null" in hip.lib().tramba_last_error()
    bad = good.copy()
    bad[1, H] = 0
    with pytest.raises(hip.TrambaHipError):
        hip.frames_ragged_check(bad, S, n, cap)


def test_launching_entries_check_before_any_launch(packed):
    """a bad host copy is refused by both launching entries; the device pointers are never dereferenced"""
    from tramba_amd import hip
    _, batch, good = packed
    lib = hip.lib()
    n, cap = batch["packed"].numel(), int(good[-1, OUT] + good[-1, H] * good[-1, W])
    buf = np.zeros(64, np.uint8)
    p = (buf.ctypes.data + 15) & ~15          # 16-byte aligned, as the entries demand of device buffers
    bad = good.copy()
    bad[0, H] = hip.FRAME_MAX_DIM + 1
    b = good.shape[0]
    assert lib.tramba_frames_to_input_ragged(p, bad.ctypes.data, n, p, b, S, 0, None) < 0
    assert b"side" in lib.tramba_last_error()
    assert lib.tramba_logits_to_u8_ragged(p, p, bad.ctypes.data, p, cap, b, S, hip.F32, None) < 0
    assert b"side" in lib.tramba_last_error()
    assert lib.tramba_frames_to_input_ragged(None, good.ctypes.data, n, p, b, S, 0, None) < 0
    assert b"null" in lib.tramba_last_error()
    assert lib.tramba_frames_to_input_ragged(p + 8, good.ctypes.data, n, p, b, S, 0, None) < 0
    assert b"align" in lib.tramba_last_error()
    assert lib.tramba_frames_to_input_ragged(p, good.ctypes.data, n, p, 0, S, 0, None) < 0
    assert lib.tramba_frames_to_input_ragged(p, good.ctypes.data, n - 1, p, b, S, 0, None) < 0
    assert lib.tramba_logits_to_u8_ragged(p, p, good.ctypes.data, p, cap - 1, b, S, hip.F32, None) < 0
    assert b"capacity" in lib.tramba_last_error()
    assert lib.tramba_logits_to_u8_ragged(p, p, good.ctypes.data, p, cap, b, S, 7, None) < 0
    assert b"dtype" in lib.tramba_last_error()
    with pytest.raises(hip.TrambaHipError):                         # host tensors: no CPU path
        hip.frames_to_input_ragged(batch["packed"], good, S)
    with pytest.raises(hip.TrambaHipError):
        hip.logits_to_u8_ragged(torch.zeros(b, 1, S, S), batch["packed"], good, torch.zeros(cap, dtype=torch.uint8))


def test_pack_frames_refusals():
    from tramba_amd import hip, infer
    ok = _frame(8, 8, 0)
    with pytest.raises(ValueError):
        infer.pack_frames([], S)
    with pytest.raises(TypeError):
        infer.pack_frames([ok, np.zeros((8, 8, 3), np.float32)], S)
    with pytest.raises(TypeError):
        infer.pack_frames([ok, [[1, 2, 3]]], S)
    with pytest.raises(TypeError):
        infer.pack_frames(np.stack([ok, ok]), S)                    # a uniform batch is not a list
    with pytest.raises(ValueError):
        infer.pack_frames([np.zeros((8, 8, 4), np.uint8)], S)
    with pytest.raises(ValueError):
        infer.pack_frames([np.zeros((2, 8, 8, 3), np.uint8)], S)
    with pytest.raises(ValueError):
        infer.pack_frames([np.zeros((hip.FRAME_MAX_DIM + 1, 1, 3), np.uint8)], S)
    with pytest.raises(hip.TrambaHipError):
        infer.pack_frames([ok], hip.FRAME_MAX_OUT + 1)
    with pytest.raises(TypeError):
        infer.preprocess([ok, np.zeros((8, 8, 3), np.float32)])     # refused before any device is touched
    with pytest.raises(ValueError):
        infer.preprocess([])


def test_host_table_cache_is_bounded():
    from tramba_amd import infer
    for k in range(infer.MAX_HOST_TABLES + 8):
        infer.pack_frames([np.zeros((3 + k, 4, 3), np.uint8)], 8)
    assert len(infer._host_tables) == infer.MAX_HOST_TABLES


def test_capacity_bucket():
    from tramba_amd import infer
    last = 0
    for need in list(range(1, 70)) + [4095, 4096, 4097, 65536, 65537, 6220800, (1 << 24) - 1, 1 << 24, (1 << 24) + 1,
                                      3 * 10 ** 9]:
        c = infer.capacity_bucket(need)
        assert c >= need and c & (c - 1) == 0 and c >= last and c >= infer.MIN_BUCKET
        assert c == infer.MIN_BUCKET or c < 2 * need                # the smallest power of two that holds the need
        last = c
    with pytest.raises(ValueError):
        infer.capacity_bucket(0)


def test_folder_groups_keep_loader_order_and_a_short_last_group(tmp_path):
    from tramba_amd import infer
    names = ["img10.png", "img2.png", "img1.jpg", "b.jpeg", "a.png", "img3.png", "note.txt"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    paths = data._listing(str(tmp_path), (".jpg", ".png", ".jpeg"))
    order = [os.path.basename(p) for p in paths]
    assert order == ["a.png", "b.jpeg", "img1.jpg", "img2.png", "img3.png", "img10.png"]      # the loader's natural order
    groups = infer.folder_groups(paths, 4)
    assert [len(g) for g in groups] == [4, 2] and [p for g in groups for p in g] == paths
    assert [len(g) for g in infer.folder_groups(paths, 3)] == [3, 3]
    assert [len(g) for g in infer.folder_groups(paths, 1)] == [1] * 6
    assert infer.folder_groups([], 3) == []
    for bad in (0, -1, 2.5, 65536, True):
        with pytest.raises(ValueError):
            infer.folder_groups(paths, bad)


def test_ragged_entries_are_declared_exported_and_bound():
    from tramba_amd import hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_frames_ragged_check", "tramba_frames_to_input_ragged", "tramba_logits_to_u8_ragged"):
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    assert f"#define TRAMBA_FRAMES_DESC_WORDS {hip.FRAMES_DESC_WORDS}\n" in hdr
