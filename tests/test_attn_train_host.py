"""CPU tests of the attention backward entries' host side: declared, bound and exported; every unsupported argument, a
missing and a one-byte-short workspace included, is refused with a message before any launch; the workspace sizes are pure
functions of the shape; the Python predicates the encoder modules ask agree with the C checks; the training switch counts
the blocks it flips and leaves the state_dict alone."""
import os
import re

import pytest
import torch

from test_attn_host import BF16, F32, KV_SHAPES, WINDOW_SHAPES, _TORCH, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tramba_window_attn_bwd_cl", "tramba_window_attn_bwd_work", "tramba_kv_attn_bwd_cl", "tramba_kv_attn_bwd_work")
BIG = 1 << 40          # a workspace size no shape here needs: the check it satisfies is the entries' last


def _window(lib, addr, qkv=True, table=True, dy=True, dqkv=True, dtable=True, work=True, work_bytes=BIG, batch=2, h=24, w=24,
            heads=4, hd=32, ws=12, shift=6, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_window_attn_bwd_cl(p(qkv), p(table), p(dy), p(dqkv), p(dtable), p(work), work_bytes, batch, h, w, heads,
                                         hd, ws, shift, dtype, None)


def _kv(lib, addr, q=True, kv=True, dy=True, dq=True, dkv=True, work=True, work_bytes=BIG, batch=2, n=144, m=144, heads=8,
        hd=64, dtype=BF16):
    p = lambda on: addr if on else None
    return lib.tramba_kv_attn_bwd_cl(p(q), p(kv), p(dy), p(dq), p(dkv), p(work), work_bytes, batch, n, m, heads, hd, dtype,
                                     None)


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in NAMES:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    for name in ("window_attention_bwd_cl", "kv_attention_bwd_cl", "window_attention_train_supported",
                 "kv_attention_train_supported"):
        assert callable(getattr(hip, name)), name


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()

    def rejected(rc, word):
        assert rc == -1, rc                                           # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg

    for missing in ("qkv", "table", "dy", "dqkv"):
        rejected(_window(lib, addr, **{missing: False}), "null")
    for dtype in (F32, 7):
        rejected(_window(lib, addr, dtype=dtype), "dtype")
    for hd in (16, 48, 128, 0):
        rejected(_window(lib, addr, hd=hd), "hd")
    for ws in (0, -3, 17):
        rejected(_window(lib, addr, ws=ws, h=17 * 4, w=17 * 4, shift=0), "ws")
    rejected(_window(lib, addr, h=25), "multiple of ws")
    rejected(_window(lib, addr, w=30), "multiple of ws")
    for shift in (-1, 12, 40):
        rejected(_window(lib, addr, shift=shift), "shift")
    rejected(_window(lib, addr + 8), "aligned")
    need = lib.tramba_window_attn_bwd_work(2, 24, 24, 4, 32, 12)
    assert need == 2 * 4 * 4 * 23 * 23 * 4
    rejected(_window(lib, addr, work=False), "workspace")
    rejected(_window(lib, addr, work_bytes=need - 1), "workspace")
    rejected(_window(lib, addr, work_bytes=0), "workspace")

    for missing in ("q", "kv", "dy", "dq", "dkv"):
        rejected(_kv(lib, addr, **{missing: False}), "null")
    for dtype in (F32, -1):
        rejected(_kv(lib, addr, dtype=dtype), "dtype")
    for hd in (16, 96):
        rejected(_kv(lib, addr, hd=hd), "hd")
    for m in (0, -5, 257, 576):
        rejected(_kv(lib, addr, m=m), "M")
    rejected(_kv(lib, addr, n=0), "N")
    rejected(_kv(lib, addr + 4), "aligned")
    need = lib.tramba_kv_attn_bwd_work(2, 144, 144, 8, 64)
    assert need > 0 and need % (2 * 8 * 2 * 144 * 64 * 4) == 0          # whole f32 dK / dV partials per (batch, head)
    rejected(_kv(lib, addr, work=False), "workspace")
    rejected(_kv(lib, addr, work_bytes=need - 1), "workspace")
    del keep


def test_workspace_sizes_are_pure_and_monotone_in_batch():
    lib = _lib()
    for args in ((24, 24, 4, 32, 12), (96, 96, 4, 32, 12), (16, 16, 1, 64, 16), (14, 14, 3, 32, 7)):
        sizes = [lib.tramba_window_attn_bwd_work(b, *args) for b in (1, 2, 3, 4, 8, 64)]
        assert sizes == [lib.tramba_window_attn_bwd_work(b, *args) for b in (1, 2, 3, 4, 8, 64)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (args, sizes)
    for args in ((144, 144, 8, 64), (9216, 144, 1, 64), (2304, 144, 2, 64), (576, 144, 5, 64), (100, 256, 2, 64), (20, 40, 2, 32),
                 (12726, 40, 2, 32)):
        sizes = [lib.tramba_kv_attn_bwd_work(b, *args) for b in (1, 2, 3, 4, 8, 64, 300)]
        assert sizes == [lib.tramba_kv_attn_bwd_work(b, *args) for b in (1, 2, 3, 4, 8, 64, 300)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (args, sizes)
    # shapes the entries refuse need nothing
    assert lib.tramba_window_attn_bwd_work(1, 25, 24, 4, 32, 12) == 0 and lib.tramba_window_attn_bwd_work(1, 24, 24, 4, 48, 12) == 0
    assert lib.tramba_kv_attn_bwd_work(1, 144, 257, 8, 64) == 0 and lib.tramba_kv_attn_bwd_work(1, 0, 144, 8, 64) == 0


def test_python_predicates_agree_with_the_c_checks():
    from tramba_amd import hip
    lib = _lib()
    keep, addr = _addr()
    seen = set()
    for dtype, h, w, heads, hd, ws, shift in WINDOW_SHAPES:
        want = hip.window_attention_train_supported(_TORCH[dtype], h, w, heads * hd, heads, ws, shift)
        assert want == hip.window_attention_supported(_TORCH[dtype], h, w, heads * hd, heads, ws, shift)
        # an accepted call would launch, so the C side is asked with a misaligned tensor: alignment is its last check of the
        # shape (only the workspace follows), and reaching it means that it found nothing to object to
        rc = _window(lib, addr + (8 if want else 0), h=h, w=w, heads=heads, hd=hd, ws=ws, shift=shift, dtype=dtype)
        assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (h, w, heads, hd, ws, shift)
        seen.add(want)
    assert seen == {True, False}
    seen = set()
    for dtype, m, heads, hd in KV_SHAPES:
        want = hip.kv_attention_train_supported(_TORCH[dtype], m, heads * hd, heads)
        assert want == hip.kv_attention_supported(_TORCH[dtype], m, heads * hd, heads)
        rc = _kv(lib, addr + (8 if want else 0), m=m, heads=heads, hd=hd, dtype=dtype)
        assert rc == -1 and (("aligned" in lib.tramba_last_error().decode()) == want), (m, heads, hd)
        seen.add(want)
    assert seen == {True, False}
    del keep


def test_bindings_refuse_cpu_tensors():
    from tramba_amd import hip
    bf = torch.bfloat16
    with pytest.raises(hip.TrambaHipError):
        hip.window_attention_bwd_cl(torch.zeros(1, 12, 12, 96, dtype=bf), torch.zeros(23 * 23, 1),
                                    torch.zeros(1, 12, 12, 32, dtype=bf), 12, 0, 1)
    with pytest.raises(hip.TrambaHipError):
        hip.kv_attention_bwd_cl(torch.zeros(1, 16, 32, dtype=bf), torch.zeros(1, 4, 64, dtype=bf), torch.zeros(1, 16, 32, dtype=bf), 1)


def test_switch_counts_blocks_flips_back_and_leaves_the_state_dict_alone():
    from tramba_amd import encoders
    swin = encoders.SwinTransformer(img_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)
    pvt = encoders.pvt_v2_b4()
    for model, count, kinds in ((swin, 24, (encoders.SwinTransformerBlock,)), (pvt, 41, (encoders._PvtAttention,))):
        keys = list(model.state_dict().keys())
        blocks = [m for m in model.modules() if isinstance(m, kinds)]
        assert len(blocks) == count and not any(m.fused_attention_training for m in blocks)     # off by default
        assert encoders.set_fused_attention_training(model) == count
        assert all(m.fused_attention_training for m in blocks)
        assert list(model.state_dict().keys()) == keys
        assert encoders.set_fused_attention_training(model, False) == count
        assert not any(m.fused_attention_training for m in blocks)
        assert list(model.state_dict().keys()) == keys
    assert encoders.set_fused_attention_training(torch.nn.Linear(4, 4)) == 0
