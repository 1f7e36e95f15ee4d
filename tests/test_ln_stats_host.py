"""CPU tests of the row-statistics entries' host side (csrc/linear.hip: tramba_linear_rowstat_cl, tramba_linear2_rowstat_cl,
tramba_linear_ln_rowstat_cl): declared, bound and exported; bad arguments are refused with a message before any launch; the
Python side carves y and its slab out of one allocation and hands a slab on only where it still describes the tensor."""
import ctypes
import os
import re

import torch

from test_attn_host import BF16, F32, _addr, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tramba_linear_rowstat_cl", "tramba_linear2_rowstat_cl", "tramba_linear_ln_rowstat_cl")


def test_entries_are_declared_bound_and_exported():
    from tramba_amd import hip, modules
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7                               # additions only
    for name in NAMES:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    assert modules.ROW_STATS is True and modules.FOLD_LAYERNORM is True


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib()
    keep, addr = _addr()
    emitted = ctypes.c_int(7)

    def rejected(rc, word):
        assert rc == -1, rc                                            # TRAMBA_ERR_ARG
        msg = lib.tramba_last_error().decode()
        assert word in msg, msg
    # a slab without the flag that says whether it was written; a misaligned slab
    rejected(lib.tramba_linear_rowstat_cl(addr, addr, None, None, addr, 64, 64, 64, 0, BF16, BF16, addr, None, None), "emitted")
    rejected(lib.tramba_linear_rowstat_cl(addr, addr, None, None, addr, 64, 64, 64, 0, BF16, BF16, addr + 4,
                                          ctypes.byref(emitted), None), "8-byte")
    assert emitted.value == 0                                          # cleared before anything else
    rejected(lib.tramba_linear2_rowstat_cl(addr, addr, 64, addr, None, None, addr, 64, 64, 128, 0, BF16, BF16, addr, None, None),
             "emitted")
    # the argument checks of the plain entries still come first
    rejected(lib.tramba_linear_rowstat_cl(None, addr, None, None, addr, 64, 64, 64, 0, BF16, BF16, addr, ctypes.byref(emitted),
                                          None), "null")
    # the consumer: the partial count must be K / 64
    for p in (0, 1, 3):
        rejected(lib.tramba_linear_ln_rowstat_cl(addr, addr, addr, None, None, addr, 64, 64, 128, 1e-5, 0, BF16, BF16, addr, p,
                                                 None), "partials")
    rejected(lib.tramba_linear_ln_rowstat_cl(addr, addr, addr, None, None, addr, 64, 64, 128, 1e-5, 0, F32, F32, addr, 2, None),
             "16-bit")


def test_one_allocation_holds_the_output_and_its_slab():
    from tramba_amd import hip
    for m, n in ((1, 64), (65, 200), (130, 100), (3, 3)):
        for dtype in (torch.bfloat16, torch.float16):
            extra = hip._rowstat_extra(True, dtype, dtype, m, n)
            buf = torch.zeros(m * n + extra, dtype=dtype)
            y, slab = hip._rowstat_split(buf, (m, n), m, n)
            assert tuple(y.shape) == (m, n) and tuple(slab.shape) == (m, (n + 63) // 64, 2) and slab.dtype == torch.float32
            assert y.data_ptr() == buf.data_ptr() and slab.is_contiguous() and y.is_contiguous()
            assert slab.data_ptr() % 16 == 0 or buf.data_ptr() % 16                       # 16 bytes behind an aligned base
            assert slab.data_ptr() >= y.data_ptr() + m * n * 2                             # behind y, not over it
            assert slab.data_ptr() + slab.numel() * 4 == buf.data_ptr() + buf.numel() * 2  # and inside the allocation
    for args in ((False, torch.bfloat16, torch.bfloat16), (True, torch.float32, torch.float32),
                 (True, torch.bfloat16, torch.float32)):
        assert hip._rowstat_extra(*args, 64, 64) == 0


def test_a_slab_is_handed_on_only_where_it_describes_the_tensor():
    from tramba_amd import hip
    x = torch.zeros(4, 6, 128, dtype=torch.bfloat16)
    slab = torch.zeros(24, 2, 2)
    assert hip.rowstat_for(x, 128) is None                              # none attached
    x._tramba_rowstat = (slab, x._version)
    assert hip.rowstat_for(x, 128) is slab
    assert hip.rowstat_for(x, 64) is None and hip.rowstat_for(x, 96) is None          # another K: another partial count
    assert hip.rowstat_for(x.view(24, 128), 128) is None                # another tensor object
    x.add_(1)
    assert hip.rowstat_for(x, 128) is None                              # written to since
