"""GPU tests of the LayerNorm family's rows form (csrc/norm.h: LPR lanes per row, 64 / LPR rows per wave, one 16-byte pack of
VM elements per lane; VM = 4 for fp32, 8 for 16-bit) through every public entry that dispatches on it:

  layernorm_cl, shuffle_norm_cl, shuffle_norm_head_cl, add_layernorm_cl (with and without y, mask, dual, gate), the three
  LayerNorm backwards, shuffle_norm_head_bwd_cl, rowdot_cl, rowdot_bwd_cl.

C = VM * {1, 2, 4, 8, 16, 32, 64} reaches every LPR of the one dispatcher (with_lpr); VM * 3 and VM * 25 leave lanes of a row
without a pack (`cok` false).  Row-dot forward needs LPR * VM to divide C, so there its LPR falls to 1 (row_form_dividing).
37 rows leave the last wave ragged for every LPR; 4609 rows (4612 through the pixel shuffle) give several partial rows.

Every result is compared with fp64 torch on the same inputs under the tolerance the entry's existing test uses
(test_gpu_kernels.py, test_gpu_stochastic_depth.py, test_gpu_grad.py; row-dot backward has no kernel-level test of its own and
takes the LayerNorm backward's figures, as tests/golden/fp16_range_cases.py does).  The partial tables are sized by the
library's `_parts` queries and checked against what the launch writes."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MULTS = (1, 2, 4, 8, 16, 32, 64, 3, 25)
FORMS = [pytest.param(t, m, id=f"{n}-{m}vm") for t, n in ((F32, "f32"), (BF16, "bf16")) for m in MULTS]
SHUFFLES = ((2, 1, 3, 3), (4, 1, 1, 2))                       # (p, B, H, W): 36 and 32 rows
SHUFFLE_BIG = (2, 1, 1, 1153)                                 # 4612 rows: several partial rows
SENTINEL = 12345.0


def hip():
    from tramba_amd import hip as h
    return h


def _vm(dtype):
    return 4 if dtype == F32 else 8


def _rel_l2(got, want):
    want = want.double()
    return float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-30))


def _close(got, want, tol, atol=None, what=""):
    np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=tol, atol=tol if atol is None else atol,
                               err_msg=str(what))


@functools.lru_cache(maxsize=None)
def _rows_case(dtype, c, rows):
    """inputs of a (rows, C) map (on the host, rounded to dtype) and the fp64 LayerNorm forward / backward of them"""
    g = torch.Generator().manual_seed(rows * 131 + c)
    b = 1 if rows == 37 else 11                               # 4609 = 11 * 419
    x = (torch.randn(b, rows // b, c, generator=g) * 1.5 + 0.3).to(dtype)
    y, dy, gres, gate = (torch.randn(b, rows // b, c, generator=g).to(dtype) for _ in range(4))
    w, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    hw = torch.randn(c, generator=g) * c ** -0.5
    gy = torch.randn(b, rows // b, generator=g)
    mask = torch.tensor(([2.0, 0.0, 1.25, 0.5] * b)[:b])
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    n = F.layer_norm(xr, (c,), wr, br, 1e-5)
    n.backward(dy.double())
    return dict(x=x, y=y, dy=dy, gres=gres, gate=gate, w=w, b=bias, hw=hw, gy=gy, mask=mask, n=n.detach(), dx=xr.grad,
                dw=wr.grad, db=br.grad)


@functools.lru_cache(maxsize=None)
def _shuffle_case(dtype, c, cfg):
    """inputs of a (B, H, W, P*P*C) map; the fp64 pixel shuffle + LayerNorm (+ head), forward and backward"""
    p, b, h, w_ = cfg
    g = torch.Generator().manual_seed(h * w_ * 17 + c + p)
    x = (torch.randn(b, h, w_, p * p * c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(b, h * p, w_ * p, c, generator=g).to(dtype)
    gl = torch.randn(b, h * p, w_ * p, generator=g)
    w, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    hw = torch.randn(c, generator=g) * c ** -0.5

    def shuffled(t):
        return t.view(b, h, w_, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h * p, w_ * p, c)
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    n = F.layer_norm(shuffled(xr), (c,), wr, br, 1e-5)
    n.backward(dy.double())
    out = dict(x=x, dy=dy, gl=gl, w=w, b=bias, hw=hw, n=n.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)
    # the head: logits = n . hw + hb; its backward in the kernel's terms, A_c = sum g xhat_c and G = sum g
    x2 = x.double().requires_grad_()
    xs = shuffled(x2)
    xhat = (xs - xs.mean(-1, keepdim=True)) / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + 1e-5)
    ((xhat * (w.double() * hw.double())).sum(-1) * gl.double()).sum().backward()
    out.update(logits=out["n"] @ hw.double() - 0.21, hdx=x2.grad, A=(gl.double()[..., None] * xhat.detach()).sum((0, 1, 2)),
               G=gl.double().sum())
    return out


def _dev(case, *names):
    return [case[k].to(DEV) for k in names]


# ------------------------------------------------------------------------------------------------ forward entries
@pytest.mark.parametrize("dtype,m", FORMS)
def test_forward_entries_against_fp64(dtype, m):
    h = hip()
    c, tol = _vm(dtype) * m, 1e-5 if dtype == F32 else 2e-2
    k = _rows_case(dtype, c, 37)
    x, y, gate, w, b, hw, mask = _dev(k, "x", "y", "gate", "w", "b", "hw", "mask")
    for act, fn in ((h.ACT_NONE, lambda t: t), (h.ACT_GELU, F.gelu)):             # test_layernorm_cl
        _close(h.layernorm_cl(x, w, b, 1e-5, act), fn(k["n"]), tol, what=("layernorm_cl", c, act))
    got = h.rowdot_cl(x, hw, 0.37)                                                 # test_rowdot_cl
    _close(got, k["x"].double() @ k["hw"].double() + 0.37, 1e-5, 1e-5 if dtype == F32 else 1e-4, what=("rowdot_cl", c))
    # add_layernorm_cl (test_add_layernorm_masked_against_fp64): the sum within one ulp, n and act(n) of the values AS STORED
    for with_y, with_m, act, with_gate in ((False, False, h.ACT_NONE, False), (True, False, h.ACT_NONE, False),
                                           (True, True, h.ACT_NONE, False), (True, True, h.ACT_GELU, False),
                                           (False, False, h.ACT_GELU, True), (True, True, h.ACT_GELU, True)):
        dual = act != h.ACT_NONE
        xs, n, na = h.add_layernorm_cl(x, y if with_y else None, mask if with_m else None, w, b, 1e-5, act, dual=dual,
                                       gate=gate if with_gate else None)
        what = ("add_layernorm_cl", c, with_y, with_m, act, with_gate)
        base = k["x"]
        if with_y:
            ref = k["x"].double() + k["y"].double() * (k["mask"].double().view(-1, 1, 1) if with_m else 1.0)
            fi = torch.finfo(dtype)
            ulp = fi.eps * torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(fi.tiny))))
            assert bool(((xs.cpu().double() - ref).abs() <= ulp).all()), what
            base = xs.cpu()
        else:
            assert xs is None
        _close(n, F.layer_norm(base.double(), (c,), k["w"].double(), k["b"].double(), 1e-5), tol, what=what)
        if dual:
            want = F.gelu(n.cpu().double()) * (F.silu(k["gate"].double()) if with_gate else 1.0)
            _close(na, want, tol, what=what)
        else:
            assert na is None
    for cfg in SHUFFLES:                                                           # test_shuffle_norm_cl, test_shuffle_norm_head_cl
        s = _shuffle_case(dtype, c, cfg)
        x, w, b, hw = _dev(s, "x", "w", "b", "hw")
        _close(h.shuffle_norm_cl(x, w, b, cfg[0]), s["n"], tol, what=("shuffle_norm_cl", c, cfg))
        htol = 1e-4 if dtype == F32 else 2e-2
        _close(h.shuffle_norm_head_cl(x, w, b, hw, -0.21, cfg[0]), s["logits"], htol, what=("shuffle_norm_head_cl", c, cfg))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_unaligned_parameters_take_the_wave_form(dtype):
    """w and b 4 bytes past a 16-byte boundary: layernorm_cl, shuffle_norm_cl and add_layernorm_cl fall back to the one-row-
    per-wave form and still give the aligned launch's result (the same fp64 tolerance; the two forms sum in another order).
    shuffle_norm_head_cl and rowdot_cl have no such form: they require aligned parameters"""
    h = hip()
    c, tol = _vm(dtype) * 16, 1e-5 if dtype == F32 else 2e-2
    k, s = _rows_case(dtype, c, 37), _shuffle_case(dtype, c, SHUFFLES[0])
    x, y, w, b, mask = _dev(k, "x", "y", "w", "b", "mask")
    xs = s["x"].to(DEV)

    def off4(t):
        v = torch.zeros(c + 1, device=DEV)[1:]
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
        return v
    wu, bu = off4(w), off4(b)
    runs = {"layernorm_cl": lambda w_, b_: [h.layernorm_cl(x, w_, b_)],
            "shuffle_norm_cl": lambda w_, b_: [h.shuffle_norm_cl(xs, w_, b_, SHUFFLES[0][0])],
            "add_layernorm_cl": lambda w_, b_: list(h.add_layernorm_cl(x, y, mask, w_, b_, 1e-5, h.ACT_GELU, dual=True))}
    for name, run in runs.items():
        for a, u in zip(run(w, b), run(wu, bu)):
            _close(u, a.cpu().double(), tol, what=(name, "unaligned against aligned"))
    _close(h.layernorm_cl(x, wu, bu), k["n"], tol, what="layernorm_cl, unaligned against fp64")
    _close(h.shuffle_norm_cl(xs, off4(s["w"].to(DEV)), off4(s["b"].to(DEV)), SHUFFLES[0][0]), s["n"], tol,
           what="shuffle_norm_cl, unaligned against fp64")


# ------------------------------------------------------------------------------------------------ backward entries
def _check_ln_bwd(got, k, dtype, what, gres=None):
    tol, ptol = (2e-5, 1e-4) if dtype == F32 else (3e-2, 3e-2)                    # test_layernorm_training_path_matches_autograd
    dx, dw, db = got
    _close(dx, k["dx"] if gres is None else k["dx"] + gres.double(), tol, what=what)
    _close(dw, k["dw"], ptol, ptol * float(k["dw"].abs().max()), what=what)
    _close(db, k["db"], ptol, ptol * float(k["db"].abs().max()), what=what)


@pytest.mark.parametrize("rows", [37, 4609])
@pytest.mark.parametrize("dtype,m", FORMS)
def test_backward_entries_against_fp64(dtype, m, rows):
    h = hip()
    c = _vm(dtype) * m
    k = _rows_case(dtype, c, rows)
    x, dy, gres, w, hw, gy, mask = _dev(k, "x", "dy", "gres", "w", "hw", "gy", "mask")
    assert rows == 37 or h.lib().tramba_layernorm_bwd_parts(rows, c, h.dt(x)) > 1
    _check_ln_bwd(h.layernorm_bwd_cl(x, dy, w), k, dtype, ("layernorm_bwd_cl", c, rows))
    dx, dxm, dw, db = h.layernorm_bwd_res_cl(x, dy, w, gres=gres, mask=mask, want_masked=True)
    _check_ln_bwd((dx, dw, db), k, dtype, ("layernorm_bwd_res_cl", c, rows), gres=k["gres"])
    # dxm = dx (as stored) * mask[sample], rounded once (test_layernorm_bwd_res_masked_against_fp64)
    want_m = (dx.cpu().double() * k["mask"].double().view(-1, 1, 1)).to(dtype)
    assert torch.equal(dxm.cpu(), want_m), ("dxm", c, rows)
    # row-dot backward: gx = gy w (dtype), gw = sum gy x, gb = sum gy
    assert rows == 37 or h.lib().tramba_rowdot_bwd_parts(rows, c, h.dt(x)) > 1
    gx, gw, gb = h.rowdot_bwd_cl(x, gy, hw)
    tol, ptol = (2e-5, 1e-4) if dtype == F32 else (3e-2, 3e-2)
    gy64 = k["gy"].double()
    _close(gx, gy64[..., None] * k["hw"].double(), tol, what=("rowdot_bwd_cl gx", c, rows))
    gw_ref = (gy64[..., None] * k["x"].double()).sum((0, 1))
    _close(gw, gw_ref, ptol, ptol * float(gw_ref.abs().max()), what=("rowdot_bwd_cl gw", c, rows))
    _close(gb.reshape(1), gy64.sum().reshape(1), ptol, ptol * float(gy64.sum().abs()), what=("rowdot_bwd_cl gb", c, rows))
    # through the pixel shuffle: shuffle_norm_bwd_cl and the fused norm + head backward
    for cfg in (SHUFFLES if rows == 37 else (SHUFFLE_BIG,)):
        s = _shuffle_case(dtype, c, cfg)
        x, dy, gl, w, hw = _dev(s, "x", "dy", "gl", "w", "hw")
        _check_ln_bwd(h.shuffle_norm_bwd_cl(x, dy, w, cfg[0]), s, dtype, ("shuffle_norm_bwd_cl", c, cfg))
        dx, part = h.shuffle_norm_head_bwd_cl(x, gl, w, hw, cfg[0])
        assert rows == 37 or part.shape[0] > 1
        sums = part.double().sum(0)
        htol = 2e-5 if dtype == F32 else 1.5e-2                                   # test_shuffle_norm_head_training_pair
        assert _rel_l2(dx, s["hdx"]) < htol, ("shuffle_norm_head_bwd_cl dx", c, cfg, _rel_l2(dx, s["hdx"]))
        assert _rel_l2(sums[:c], s["A"]) < max(htol, 1e-4), ("shuffle_norm_head_bwd_cl A", c, cfg, _rel_l2(sums[:c], s["A"]))
        assert _rel_l2(sums[c], s["G"]) < max(htol, 1e-4), ("shuffle_norm_head_bwd_cl G", c, cfg, _rel_l2(sums[c], s["G"]))


# ------------------------------------------------------------------------------------------------ sizing against launch
def _guarded(parts, width):
    """a partial table of `parts` rows of NaN and one guard row of a finite sentinel behind them"""
    t = torch.full((parts + 1, width), float("nan"), device=DEV)
    t[parts] = SENTINEL
    return t


def _check_guarded(t, parts, payload, what):
    assert bool((t[parts] == SENTINEL).all()), (what, "the launch wrote past the rows its sizing query returned")
    assert not bool(torch.isnan(t[:parts, :payload]).any()), (what, "a partial row the query counted was not written")


@pytest.mark.parametrize("rows", [37, 4609])
@pytest.mark.parametrize("dtype,m", FORMS)
def test_parts_queries_size_what_the_launches_write(dtype, m, rows):
    """the raw library entries with a table of exactly the queried rows plus a guard row: the guard stays, every payload slot
    below it is written.  The head backward pads its rows to C + 4 with three slots nothing reads (test_head_backwards):
    slots 0 .. C are asserted there and in the row-dot backward"""
    h = hip()
    lib = h.lib()
    c = _vm(dtype) * m
    k = _rows_case(dtype, c, rows)
    x, dy, w, hw, gy = _dev(k, "x", "dy", "w", "hw", "gy")
    d, st = h.dt(x), h._stream()
    parts = lib.tramba_layernorm_bwd_parts(rows, c, d)
    assert parts >= 1 and (rows == 37 or parts > 1)
    t, t2, dx = _guarded(parts, 2 * c), _guarded(parts, 2 * c), torch.empty_like(x)
    # (through the thin C entries, which hip.py no longer calls: they are ABI and stay covered here)
    h._check(lib.tramba_layernorm_bwd_cl(h._ptr(x), h._ptr(dy), h._ptr(w), h._ptr(dx), h._ptr(t), rows, c, 1e-5, d, st),
             "layernorm_bwd_cl")
    h._check(lib.tramba_layernorm_bwd_res_cl(h._ptr(x), h._ptr(dy), h._ptr(w), h._ptr(dx), h._ptr(t2), None, None, 0, None, rows,
                                             c, 1e-5, d, st), "layernorm_bwd_res_cl")
    _check_guarded(t, parts, 2 * c, ("layernorm_bwd", c, rows))
    assert torch.equal(t, t2), ("layernorm_bwd_res_cl without a residual against layernorm_bwd_cl", c, rows)
    parts = lib.tramba_rowdot_bwd_parts(rows, c, d)
    assert parts >= 1 and (rows == 37 or parts > 1)
    t = _guarded(parts, c + 4)
    h._check(lib.tramba_rowdot_bwd_cl(h._ptr(x), h._ptr(gy), h._ptr(hw), h._ptr(dx), h._ptr(t), rows, c, d, st), "rowdot_bwd_cl")
    _check_guarded(t, parts, c + 1, ("rowdot_bwd", c, rows))
    for cfg in (SHUFFLES if rows == 37 else (SHUFFLE_BIG,)):
        p, b, hh, ww = cfg
        s = _shuffle_case(dtype, c, cfg)
        x, dy, gl, w, hw = _dev(s, "x", "dy", "gl", "w", "hw")
        srows, dx = b * hh * ww * p * p, torch.empty_like(x)
        parts = lib.tramba_layernorm_bwd_parts(srows, c, d)
        t = _guarded(parts, 2 * c)
        h._check(lib.tramba_shuffle_norm_bwd_cl(h._ptr(x), h._ptr(dy), h._ptr(w), h._ptr(dx), h._ptr(t), b, hh, ww, c, p, 1e-5, d,
                                                st), "shuffle_norm_bwd_cl")
        _check_guarded(t, parts, 2 * c, ("shuffle_norm_bwd", c, cfg))
        parts = lib.tramba_shuffle_norm_head_bwd_parts(b, hh, ww, c, p, d)
        assert parts >= 1 and (rows == 37 or parts > 1)
        t = _guarded(parts, c + 4)
        h._check(lib.tramba_shuffle_norm_head_bwd_cl(h._ptr(x), h._ptr(gl), h._ptr(w), h._ptr(hw), h._ptr(dx), h._ptr(t), b, hh,
                                                     ww, c, p, 1e-5, d, st), "shuffle_norm_head_bwd_cl")
        _check_guarded(t, parts, c + 1, ("shuffle_norm_head_bwd", c, cfg))
    torch.cuda.synchronize()
