"""The stochastic-depth mask table (modules._MaskPool) and DropPath's use of it, on the CPU with stand-in modules: one draw
per step, one row per (DropPath, use), values 0 or 1 / keep, and the dtype and fp32 rows of one draw."""
import pytest
import torch
from torch import nn

from tramba_amd import modules as M

CPU = torch.device("cpu")


def _pool():
    return M._MaskPool()


def _warm(pool, uses, keep=0.5, batch=512):
    """a first step that creates the slots of `uses` ((module, count) pairs): a step after begin_step() finds them all and
    draws its table once, at its first take"""
    for mod, k in uses:
        for _ in range(k):
            pool.take(mod, keep, batch, torch.float32, CPU)
    pool.begin_step()


def test_values_are_zero_or_inverse_keep():
    torch.manual_seed(0)
    pool, mod = _pool(), nn.Identity()
    for keep in (0.4, 0.6, 0.8):
        pool.begin_step()
        row = pool.take(mod, keep, 256, torch.float32, CPU, want_f32=True)
        inv = float(torch.tensor(1.0) / torch.tensor(keep, dtype=torch.float32))
        assert row.shape == (256,) and row.dtype == torch.float32
        assert bool(((row == 0) | (row == inv)).all()) and bool((row == 0).any()) and bool((row != 0).any())


def test_dtype_row_and_f32_row_come_from_one_draw():
    torch.manual_seed(1)
    pool, mod = _pool(), nn.Identity()
    _warm(pool, [(mod, 2)], 0.6, 64)
    r0 = pool.take(mod, 0.6, 64, torch.bfloat16, CPU)
    r1 = pool.take(mod, 0.6, 64, torch.bfloat16, CPU, want_f32=True)
    assert r0.dtype == torch.bfloat16 and r1.dtype == torch.float32
    i0, i1 = pool.slots[(id(mod), 0)][0], pool.slots[(id(mod), 1)][0]
    assert torch.equal(pool.buf, pool.buf32.to(torch.bfloat16))
    assert torch.equal(r0, pool.buf32[i0].to(torch.bfloat16)) and torch.equal(r1, pool.buf32[i1])


def test_uses_and_modules_get_their_own_rows():
    torch.manual_seed(2)
    pool, a, b = _pool(), nn.Identity(), nn.Identity()
    _warm(pool, [(a, 2), (b, 2)])
    rows = [pool.take(a, 0.5, 512, torch.float32, CPU), pool.take(a, 0.5, 512, torch.float32, CPU),
            pool.take(b, 0.5, 512, torch.float32, CPU), pool.take(b, 0.5, 512, torch.float32, CPU)]
    idx = [pool.slots[k][0] for k in ((id(a), 0), (id(a), 1), (id(b), 0), (id(b), 1))]
    assert len(set(idx)) == 4
    for i in range(4):
        for j in range(i):
            assert not torch.equal(rows[i], rows[j]), (i, j)


def test_begin_step_draws_a_new_table_and_keeps_the_old_rows():
    torch.manual_seed(3)
    pool, mod = _pool(), nn.Identity()
    _warm(pool, [(mod, 2)])
    r = pool.take(mod, 0.5, 512, torch.float32, CPU)
    saved, table = r.clone(), pool.buf
    r_again = pool.take(mod, 0.5, 512, torch.float32, CPU)      # same step: same table, next row
    assert pool.buf is table and not torch.equal(r_again, r)
    pool.begin_step()
    r2 = pool.take(mod, 0.5, 512, torch.float32, CPU)
    assert pool.buf is not table
    assert pool.slots[(id(mod), 0)][0] == 0 and not torch.equal(r2, saved)
    assert torch.equal(r, saved)                                    # what autograd saved keeps its values


def test_new_keep_gets_a_new_slot_and_new_batch_a_redraw():
    torch.manual_seed(4)
    pool, mod = _pool(), nn.Identity()
    pool.take(mod, 0.6, 32, torch.float32, CPU)
    slot = pool.slots[(id(mod), 0)][0]
    pool.begin_step()
    row = pool.take(mod, 0.8, 32, torch.float32, CPU, want_f32=True)
    assert pool.slots[(id(mod), 0)][0] != slot and pool.keep[pool.slots[(id(mod), 0)][0]] == 0.8
    inv = float(torch.tensor(1.0) / torch.tensor(0.8, dtype=torch.float32))
    assert bool(((row == 0) | (row == inv)).all())
    table = pool.buf
    other = pool.take(nn.Identity(), 0.8, 48, torch.float32, CPU)   # same step, another batch size
    assert other.shape == (48,) and pool.buf is not table and pool.buf.shape[1] == 48


def test_the_17th_use_without_begin_step_starts_a_new_table():
    torch.manual_seed(5)
    pool, mod = _pool(), nn.Identity()
    _warm(pool, [(mod, 16)], batch=8)
    first = pool.take(mod, 0.5, 8, torch.float32, CPU)
    table = pool.buf
    for _ in range(15):
        pool.take(mod, 0.5, 8, torch.float32, CPU)
        assert pool.buf is table
    assert len(pool.keep) == 16
    pool.take(mod, 0.5, 8, torch.float32, CPU)
    assert pool.buf is not table and len(pool.keep) == 16 and pool.count[id(mod)] == 1
    assert first.shape == (8,)


def test_model_mask_pool_gives_each_model_its_pool():
    m1 = nn.Sequential(M.DropPath(0.3), M.DropPath(0.5))
    m2 = nn.Sequential(M.DropPath(0.3))
    p1, p2 = M.model_mask_pool(m1), M.model_mask_pool(m2)
    assert p1 is not p2 and p1 is not M._mask_pool
    assert M.model_mask_pool(m1) is p1
    assert all(d.__dict__["_pool"] is p1 for d in m1) and m2[0].__dict__["_pool"] is p2


def test_mask_f32_is_none_in_eval_mode_and_at_zero_drop():
    x = torch.zeros(4, 3, 2, 2)
    dp = M.DropPath(0.3)
    dp.__dict__["_pool"] = _pool()
    assert dp.mask_f32(x) is not None and dp.mask_f32(x).shape == (4,)
    dp.eval()
    assert dp.mask_f32(x) is None
    assert M.DropPath(0.0).mask_f32(x) is None


@pytest.mark.parametrize("keep", [0.4, 0.8])
def test_keep_rate_of_a_large_draw(keep):
    torch.manual_seed(6)
    pool = _pool()
    n = 200_000
    row = pool.take(nn.Identity(), keep, n, torch.float32, CPU, want_f32=True)
    rate = float((row != 0).double().mean())
    assert abs(rate - keep) <= 5 * (keep * (1 - keep) / n) ** 0.5, rate
