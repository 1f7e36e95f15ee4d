"""GPU tests of the attention backward kernels (csrc/attention_bwd.hip), of the autograd Functions over them and of the
opt-in switch that puts the Swin / PVT blocks on them in 16-bit training.

Kernel level.  The reference gradients are fp64 autograd through the forward tests' references (`_window_ref` / `_kv_ref` of
test_gpu_attn.py: roll, window partition, `relative_position_index` and `attn_mask` of modules built at that resolution),
on the same 16-bit q / k / v / dy and the f32 table.  Bound per gradient element:

    |got - ref| <= 3 u A + 1e-6,   u = 2^-8 (bf16) / 2^-11 (fp16), the unit round-off,

with A the same contraction taken over magnitudes, without cancellation:
    dV: P^T |dO|;   dS~ = P o (|dP| + sum_k P |dP|);   dQ: hd^-0.5 dS~ |K|;   dK: hd^-0.5 dS~^T |Q|;   dtable: dS~ binned.
A faithful kernel commits two 16-bit roundings per element (one operand, one store): 2 u A to first order; the third u
leaves room for one more.  dS~ and not |dS|, because dS = P (dP - D) cancels under a peaked softmax and what is left there
is f32 round-off of order 2^-24 dS~.  Every element is compared and the worst ratio of each case is printed.

Measured on an MI355X, worst |got - ref| / (u A) over all cases: dq 0.92, dk 0.96, dv 0.995, dtable 0.005 -- the kernel feeds P
and dS to the MFMAs as hi + lo operand pairs, so the store rounding (at most u / 2 of the value, and the value is at most A)
is all that is left (with single rounded operands the same cases gave 1.40 / 1.79 / 1.93).

Module level.  A block's gradients with the flag on must be as close to the fp32 stock gradients as the stock bf16 path's,
within the stock path's own seed-to-seed spread per tensor (profiles/attn_train_parity.json).
"""
import json
import os

import pytest
import torch

import attn_train_blocks
import synth
import test_gpu_attn as fwd
from test_gpu_attn import BF, HF

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _dy(tag, dtype, shape):
    return torch.randn(*shape, generator=fwd._gen("dy", tag, dtype, *shape)).to(dtype).to(DEV)


def _poison(*shapes_dtypes):
    return tuple(torch.full(s, float("nan"), dtype=d, device=DEV) for s, d in shapes_dtypes)


def _check(got, ref, amag, dtype, what):
    assert got.shape == ref.shape, what
    g = got.double()
    assert torch.isfinite(g).all(), what
    err = (g - ref).abs()
    worst = float((err / (U[dtype] * amag + 1e-30))[err > 1e-6].max()) if bool((err > 1e-6).any()) else 0.0
    print(f"{what}: worst |got - ref| = {worst:.3f} u A")
    excess = err - (3.0 * U[dtype] * amag + 1e-6)
    assert float(excess.max()) <= 0.0, f"{what}: {int((excess > 0).sum())} elements beyond 3 u A, worst {worst:.2f}"
    return worst


# ----------------------------------------------------------------------------- window form
def _window_grads_ref(qkv, table, dy, ws, shift, heads):
    """fp64 autograd through the forward reference: (dqkv (B, H, W, 3C), dtable)"""
    x = qkv.double().requires_grad_()
    t = table.double().requires_grad_()
    out, _ = fwd._window_ref(x, t, ws, shift, heads)
    out.backward(dy.double())
    return x.grad, t.grad


def _window_magnitudes(qkv, table, dy, ws, shift, heads):
    """(A of dqkv (B, H, W, 3C), A of dtable): the contractions over magnitudes, fp64, the long way round"""
    from tramba_amd.encoders import _unwindows, _windows
    b, h, w, c3 = qkv.shape
    c, n = c3 // 3, ws * ws
    hd = c // heads
    index, mask = fwd._swin_buffers(h, w, heads, hd, ws, shift)

    def win(t):
        t = t.double()
        return _windows(torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t, ws)
    xw = win(qkv)
    nw = xw.shape[1]
    q, k, v = xw.view(b, nw, n, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)             # (B, nW, nH, N, hd)
    do = win(dy).view(b, nw, n, heads, hd).permute(0, 1, 3, 2, 4)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    s = s + table.double()[index.view(-1)].view(n, n, heads).permute(2, 0, 1)[None, None]
    if shift:
        s = s + mask[None, :, None]
    p = torch.softmax(s, -1)
    dpa = (do @ v.transpose(-1, -2)).abs()
    dsb = p * (dpa + (p * dpa).sum(-1, keepdim=True))
    av = p.transpose(-1, -2) @ do.abs()
    aq = (dsb @ k.abs()) * hd ** -0.5
    ak = (dsb.transpose(-1, -2) @ q.abs()) * hd ** -0.5
    a = torch.stack([aq, ak, av]).permute(1, 2, 4, 0, 3, 5).reshape(b, nw, n, 3 * c)   # (B, nW, N, [3][heads][hd])
    a = _unwindows(a, ws, h, w)
    if shift:
        a = torch.roll(a, shifts=(shift, shift), dims=(1, 2))
    at = torch.zeros((2 * ws - 1) ** 2, heads, dtype=torch.float64, device=qkv.device)
    at.index_add_(0, index.view(-1), dsb.sum((0, 1)).permute(1, 2, 0).reshape(n * n, heads))
    return a, at


# The forward's cases (name: (dtypes, B, H, W, heads, hd, ws, shift, table scale)).  The window form has no host-side launch
# split -- one workgroup per (window, head) whatever the batch -- and one kernel per key count: ws 7 / 8 take the 64-key
# kernel, ws 12 the 160-key kernel (3 rounds of 64 queries, the last ragged), ws 16 the 256-key kernel (8 rounds of 32).
WINDOW_CASES = {k: fwd.WINDOW_CASES[k] for k in (
    "ws12_24x24_s6", "ws12_12x12_s0", "ws12_24x36_s6", "ws7_14x14_s3", "ws8_16x16_s4_hd64", "ws16_16x16_s0",
    "ws16_32x32_s8_hd64", "ws12_24x24_s6_big_table")}
WINDOW_PARAMS = [(name, dt) for name, case in WINDOW_CASES.items() for dt in case[0]]


def _window_case(name, dtype):
    _, b, h, w, heads, hd, ws, shift, tscale = WINDOW_CASES[name]
    qkv, table = fwd._window_inputs(name, dtype, b, h, w, heads, hd, ws, tscale)
    if tscale > 1:
        table = table.clamp(-30, 30)
        assert float(table.abs().max()) > 20
    return qkv, table, _dy(name, dtype, (b, h, w, heads * hd)), ws, shift, heads


@pytest.mark.parametrize("name,dtype", WINDOW_PARAMS, ids=[f"{n}-{str(d)[6:]}" for n, d in WINDOW_PARAMS])
def test_window_backward_matches_fp64(name, dtype):
    from tramba_amd import hip
    qkv, table, dy, ws, shift, heads = _window_case(name, dtype)
    out = _poison((qkv.shape, dtype), (table.shape, torch.float32))
    dqkv, dtable = hip.window_attention_bwd_cl(qkv, table, dy, ws, shift, heads, out=out)
    assert dqkv is out[0] and dtable is out[1] and dqkv.dtype == dtype and dtable.dtype == torch.float32
    rq, rt = _window_grads_ref(qkv, table, dy, ws, shift, heads)
    a, at = _window_magnitudes(qkv, table, dy, ws, shift, heads)
    c = qkv.shape[-1] // 3
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * c, (i + 1) * c)
        _check(dqkv[..., sl], rq[..., sl], a[..., sl], dtype, f"{name} {part}")
    _check(dtable, rt, at, dtype, f"{name} dtable")


# ----------------------------------------------------------------------------- kv form
def _kv_grads_ref(q, kv, dy, heads):
    x = q.double().requires_grad_()
    y = kv.double().requires_grad_()
    out, _ = fwd._kv_ref(x, y, heads)
    out.backward(dy.double())
    return x.grad, y.grad


def _kv_magnitudes(q, kv, dy, heads):
    b, n, c = q.shape
    m, hd = kv.shape[1], c // heads
    qd = q.double().view(b, n, heads, hd).transpose(1, 2)
    do = dy.double().view(b, n, heads, hd).transpose(1, 2)
    k, v = kv.double().view(b, m, 2, heads, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax((qd @ k.transpose(-1, -2)) * hd ** -0.5, -1)
    dpa = (do @ v.transpose(-1, -2)).abs()
    dsb = p * (dpa + (p * dpa).sum(-1, keepdim=True))
    aq = ((dsb @ k.abs()) * hd ** -0.5).transpose(1, 2).reshape(b, n, c)
    ak = (dsb.transpose(-1, -2) @ qd.abs()) * hd ** -0.5                            # (B, nH, M, hd)
    av = p.transpose(-1, -2) @ do.abs()
    return aq, torch.stack([ak, av]).permute(1, 3, 0, 2, 4).reshape(b, m, 2 * c)


# The forward's cases (name: (dtypes, B, N, M, heads, hd)), hd 32 in bf16 only, stage 1 at batch 1.  The host deals the
# rounds of 64 queries (32 above 160 keys) of one (batch, head) to about 256 / heads workgroups: rounds-per-workgroup =
# ceil(rounds / min(rounds, 256 / heads)); the branch is named per case.
KV_CASES = {
    "n144_m144_h8": ((BF, HF), 2, 144, 144, 8, 64),     # PVT stage 4: 3 rounds -> one round per workgroup, 3 partials
    "n576_m36_h5": ((BF,), 1, 576, 36, 5, 64),          # C = 320; one round per workgroup, 9 partials per head
    "n100_m1": ((BF,), 2, 100, 1, 2, 64),               # one key: P = 1, dS = 0, dq = dk = 0, dv = sum of dy
    "n100_m17": ((BF,), 2, 100, 17, 2, 64),
    "n100_m256": ((BF,), 2, 100, 256, 2, 64),           # the cap: rounds of 32 queries, the last holds 4
    "n100_m160_hd32": ((BF,), 1, 100, 160, 2, 32),
    "n9216_m144_h1": ((BF,), 1, 9216, 144, 1, 64),      # PVT stage 1: 144 rounds, one per workgroup: 144 partials
    "n20_m40_b300": ((BF,), 300, 20, 40, 2, 32),        # one round: the whole problem in one workgroup, one partial
    # 199 rounds against 128 workgroups -> 2 rounds per workgroup, 100 workgroups per (batch, head), the last with one
    # round, and that round with 54 queries
    "n12726_m40_rpw2": ((BF,), 2, 12726, 40, 2, 32),
}
KV_PARAMS = [(name, dt) for name, case in KV_CASES.items() for dt in case[0]]


def _kv_case(name, dtype):
    _, b, n, m, heads, hd = KV_CASES[name]
    q, kv = fwd._kv_inputs(name, dtype, b, n, m, heads, hd)
    return q, kv, _dy(name, dtype, (b, n, heads * hd)), heads


def _check_kv(name, dtype, q, kv, dy, heads, dq, dkv):
    rq, rkv = _kv_grads_ref(q, kv, dy, heads)
    aq, akv = _kv_magnitudes(q, kv, dy, heads)
    c = q.shape[-1]
    _check(dq, rq, aq, dtype, f"{name} dq")
    _check(dkv[..., :c], rkv[..., :c], akv[..., :c], dtype, f"{name} dk")
    _check(dkv[..., c:], rkv[..., c:], akv[..., c:], dtype, f"{name} dv")


@pytest.mark.parametrize("name,dtype", KV_PARAMS, ids=[f"{n}-{str(d)[6:]}" for n, d in KV_PARAMS])
def test_kv_backward_matches_fp64(name, dtype):
    from tramba_amd import hip
    q, kv, dy, heads = _kv_case(name, dtype)
    out = _poison((q.shape, dtype), (kv.shape, dtype))
    dq, dkv = hip.kv_attention_bwd_cl(q, kv, dy, heads, out=out)
    assert dq is out[0] and dkv is out[1]
    _check_kv(name, dtype, q, kv, dy, heads, dq, dkv)


def test_kv_backward_ignores_what_lies_beyond_m():
    """17 keys at the head of a larger allocation whose remaining rows are NaN, and a dkv whose allocation continues past M
    with a sentinel: pad keys are read from nowhere and written nowhere"""
    from tramba_amd import hip
    heads, hd, n, m = 2, 64, 100, 17
    q, kv = fwd._kv_inputs("nan", BF, 1, n, m, heads, hd)
    dy = _dy("nan", BF, (1, n, heads * hd))
    big = torch.full((1, 64, 2 * heads * hd), float("nan"), dtype=BF, device=DEV)
    big[:, :m] = kv
    sl = big[:, :m]
    assert sl.is_contiguous() and sl.data_ptr() == big.data_ptr() and torch.isnan(big[:, m:]).all()
    dbig = torch.full((1, 64, 2 * heads * hd), 7.0, dtype=BF, device=DEV)
    dq, dkv = hip.kv_attention_bwd_cl(q, sl, dy, heads, out=(torch.empty_like(q), dbig[:, :m]))
    assert dkv.data_ptr() == dbig.data_ptr()
    assert torch.isfinite(dq).all() and torch.isfinite(dkv).all()
    assert bool((dbig[:, m:] == 7.0).all())
    tq, tkv = hip.kv_attention_bwd_cl(q, kv, dy, heads)
    assert torch.equal(dq, tq) and torch.equal(dkv, tkv)
    _check_kv("nan beyond M", BF, q, kv, dy, heads, dq, dkv)


def test_window_backward_without_the_table_gradient():
    from tramba_amd import hip
    qkv, table, dy, ws, shift, heads = _window_case("ws12_24x24_s6", BF)
    full, dtable = hip.window_attention_bwd_cl(qkv, table, dy, ws, shift, heads)
    out = _poison((qkv.shape, BF))
    dqkv, none = hip.window_attention_bwd_cl(qkv, table, dy, ws, shift, heads, need_table=False, out=(out[0], None))
    assert none is None and dtable is not None
    assert torch.equal(dqkv, full)


# ----------------------------------------------------------------------------- properties, both forms
def _ops():
    """forward + backward of both forms on the forward tests' property inputs"""
    from tramba_amd import hip
    qkv, table = fwd._window_inputs("prop", BF, 2, 24, 24, 4, 32, 12)
    q, kv = fwd._kv_inputs("prop", BF, 2, 144, 144, 8, 64)
    dyw, dyk = _dy("propw", BF, (2, 24, 24, 128)), _dy("propk", BF, (2, 144, 512))
    return {"window": lambda: (hip.window_attention_cl(qkv, table, 12, 6, 4),
                               *hip.window_attention_bwd_cl(qkv, table, dyw, 12, 6, 4)),
            "kv": lambda: (hip.kv_attention_cl(q, kv, 8), *hip.kv_attention_bwd_cl(q, kv, dyk, 8))}


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_two_runs_and_a_graph_replay_are_bitwise_equal():
    for name, op in _ops().items():
        eager = op()
        assert _same(eager, op()), name
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                got = op()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            for t in got:
                t.zero_()
            g.replay()
        torch.cuda.synchronize()
        assert _same(got, eager), name


def test_two_streams_at_once_give_the_same_bits():
    ops = _ops()
    side = torch.cuda.Stream()
    for name, op in ops.items():
        ref = [t.clone() for t in op()]
        torch.cuda.synchronize()
        for sname, sop in ops.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                keep = [sop() for _ in range(12)]
            outs = [op() for _ in range(6)]
            torch.cuda.synchronize()
            assert all(_same(o, ref) for o in outs), (name, sname)
            del keep


def test_backward_is_exactly_linear_in_dy():
    """bwd(2 dy) = 2 bwd(dy) bit for bit: a power-of-two scale commutes with every rounding of the kernel as long as no
    value overflows or falls into the denormals, which is asserted on the inputs and on the fp64 dS first (no shift mask
    here: a masked P of e^-100 is an f32 denormal)."""
    from tramba_amd import hip
    b, h, w, heads, hd, ws = 2, 24, 24, 4, 32, 12
    qkv, table = fwd._window_inputs("lin", BF, b, h, w, heads, hd, ws)
    dy = _dy("lin", BF, (b, h, w, heads * hd))
    q, kv = fwd._kv_inputs("lin", BF, 2, 144, 144, 8, 64)
    dyk = _dy("link", BF, (2, 144, 512))
    for t in (dy, dyk):
        assert torch.isfinite(t * 2).all() and float(t.abs().max()) < 1e3
        assert float(t.abs()[t != 0].min()) > 1e-30
    x = qkv.double().requires_grad_()
    out, _ = fwd._window_ref(x, table.double(), ws, 0, heads)
    out.backward(dy.double())
    g = x.grad.abs()
    assert float(g.max()) < 1e6 and float(g[g > 0].min()) > 1e-30        # far from bf16 / f32 overflow and denormals
    one, t1 = hip.window_attention_bwd_cl(qkv, table, dy, ws, 0, heads)
    two, t2 = hip.window_attention_bwd_cl(qkv, table, dy * 2, ws, 0, heads)
    assert torch.equal(one * 2, two) and torch.equal(t1 * 2, t2)
    assert float(one.abs().max()) > 0 and float(t1.abs().max()) > 0
    oq, okv = hip.kv_attention_bwd_cl(q, kv, dyk, 8)
    tq, tkv = hip.kv_attention_bwd_cl(q, kv, dyk * 2, 8)
    assert torch.equal(oq * 2, tq) and torch.equal(okv * 2, tkv)
    assert float(oq.abs().max()) > 0 and float(okv.abs().max()) > 0


# ----------------------------------------------------------------------------- module level
def _counting(monkeypatch, owner, name, record=None):
    calls = []
    real = getattr(owner, name)

    def wrapper(*a, **k):
        calls.append(record(*a, **k) if record else 1)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapper)
    return calls


def _parity_margins(kind):
    """profiles/attn_train_parity.json (scripts/measure_attn_train_parity.py, 16 seeds on an MI355X, the blocks of
    tests/golden/attn_train_blocks.py): per gradient tensor, m = (largest / smallest stock error) - 1 over the seeds -- the
    stock 16-bit path's own seed-to-seed spread is the yardstick, never the fused path."""
    with open(os.path.join(ROOT, "profiles", "attn_train_parity.json")) as f:
        m = json.load(f)[kind]["m"]
    for name, v in m.items():
        assert 0.0 < v < 1.0, (name, v)
    return m


@pytest.mark.parametrize("kind", ["swin", "pvt"])
def test_block_gradients_keep_the_stock_error(monkeypatch, kind):
    from tramba_amd import hip
    calls = _counting(monkeypatch, hip, "window_attention_bwd_cl" if kind == "swin" else "kv_attention_bwd_cl")
    margins = _parity_margins(kind)
    for seed in range(8):
        before = len(calls)
        errors = attn_train_blocks.block_errors(kind, seed)
        assert len(calls) - before == 1                                # the fused run, once; not the two stock runs
        assert set(errors) == set(margins)
        for name, (fused, stock) in errors.items():
            print(f"{kind} seed {seed} {name}: fused {fused:.3e} stock {stock:.3e}")
            assert fused <= stock * (1 + margins[name]), (kind, seed, name, fused, stock, margins[name])


@pytest.mark.parametrize("kind", ["swin", "pvt"])
def test_flag_on_reaches_the_backward_once_and_no_stock_attention_op(monkeypatch, kind):
    import torch.nn.functional as F
    from tramba_amd import encoders, hip
    bwd = _counting(monkeypatch, hip, "window_attention_bwd_cl" if kind == "swin" else "kv_attention_bwd_cl")
    sdpa = _counting(monkeypatch, F, "scaled_dot_product_attention")
    roll = _counting(monkeypatch, torch, "roll")
    mask = _counting(monkeypatch, encoders._WindowAttention, "bias_mask")
    grads = attn_train_blocks.block_grads(kind, 0, "fused")
    assert len(bwd) == 1 and not sdpa and not roll and not mask
    assert all(torch.isfinite(g).all() for g in grads.values())
    if kind == "swin":
        assert grads["attn.relative_position_bias_table"].dtype == torch.float32
        assert float(grads["attn.relative_position_bias_table"].abs().max()) > 0


def test_flag_off_fp32_and_576_keys_keep_the_parent_path(monkeypatch):
    from tramba_amd import hip
    from tramba_amd.encoders import SwinTransformerBlock, _PvtBlock, set_fused_attention_training
    wcalls = _counting(monkeypatch, hip, "window_attention_bwd_cl")
    kcalls = _counting(monkeypatch, hip, "kv_attention_bwd_cl")
    fw = _counting(monkeypatch, hip, "window_attention_cl")
    fk = _counting(monkeypatch, hip, "kv_attention_cl")
    x = synth.synth_input("attn_train_stock", (1, 576, 128)).to(DEV)
    dy = synth.synth_input("attn_train_stock_dy", (1, 576, 128)).to(DEV)

    def grads(blk, inp, *extra):
        blk.zero_grad(set_to_none=True)
        inp = inp.detach().requires_grad_()
        blk(inp, *extra).backward(dy.to(inp.dtype))
        return [inp.grad] + [p.grad for p in blk.parameters()]
    swin = attn_train_blocks.seeded(SwinTransformerBlock(128, (24, 24), 4, 12, 6, 4.0, 0.0), 0).train()
    pvt = attn_train_blocks.seeded(_PvtBlock(128, 2, 4, True, 0.0, 1, 1e-6), 0).train()      # sr 1 on 24 x 24: 576 keys
    cases = [(swin, x.bfloat16(), (), False), (swin, x, (), True), (pvt, x.bfloat16(), (24, 24), True)]
    for blk, inp, extra, flag in cases:
        set_fused_attention_training(blk, False)
        stock = grads(blk, inp, *extra)
        set_fused_attention_training(blk, flag)
        again = grads(blk, inp, *extra)
        assert all(torch.equal(a, b) for a, b in zip(stock, again))
    assert not wcalls and not kcalls and not fw and not fk


# ----------------------------------------------------------------------------- whole model
def _train_model(name, fused, frozen=False):
    import tramba_amd as ta
    from tramba_amd import encoders
    m = ta.bulid_model_enc(name)
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        new.setdefault(k, sd[k])
    m.load_state_dict(new, strict=True)
    m = m.to(DEV).train()
    m.compute_dtype = torch.bfloat16
    if frozen:
        m.freeze_encoder()
    assert encoders.set_fused_attention_training(m, fused) == (24 if "-S-" in name else 41)
    return m


@pytest.mark.parametrize("name,entry,count", [("Tramba-S-TSOD", "window_attention_bwd_cl", 22),
                                              ("Tramba-P-TSOD", "kv_attention_bwd_cl", 41)])
def test_whole_model_train_step_on_the_fused_attention(monkeypatch, name, entry, count):
    from tramba_amd import hip, train
    x = synth.synth_input("attn_train_whole", (1, 3, 384, 384)).to(DEV)
    y = (synth.synth_input("attn_train_whole_y", (1, 1, 384, 384)).to(DEV) > 0).float()
    calls = _counting(monkeypatch, hip, entry, record=lambda *a, **k: k.get("need_table", True))
    m = _train_model(name, fused=False)
    train.train_step(m, train.get_opt(1e-4, m), x, y)
    assert not calls
    have = {k for k, p in m.named_parameters() if p.grad is not None}
    assert have
    del m
    m = _train_model(name, fused=True)
    loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
    assert torch.isfinite(loss).all()
    assert len(calls) == count and all(calls)
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert have <= got
    assert all(torch.isfinite(p.grad).all() for k, p in m.named_parameters() if k in have)
    if "-S-" in name:
        del m, calls[:]
        m = _train_model(name, fused=True, frozen=True)
        loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
        assert torch.isfinite(loss).all()
        assert len(calls) == count and not any(calls)                  # need_table=False in every block
        assert all(p.grad is None for k, p in m.named_parameters() if "relative_position_bias_table" in k)
