"""GPU tests of the fused attention kernels (csrc/attention.hip) and of the encoder blocks that reach them.

The reference is fp64 torch on the same 16-bit-rounded inputs.  The window form is rebuilt the long way -- torch.roll,
window partition, scores, `relative_position_index` of a `_WindowAttention` and `attn_mask` of a `SwinTransformerBlock`
constructed at that resolution (the buffers the oracle tests pin to the reference) -- so the kernel's index and region
arithmetic is checked against them, not against a restatement of itself.

Bound per output element: |got - ref| <= 3 u vmax + 1e-6, u = 2^-9 (bf16) / 2^-11 (fp16), vmax = the largest |v| over that
problem's keys in that channel.  The output is a convex combination of v: rounding P costs <= u vmax, rounding relative to
the f32 row sum of the unrounded P at most one more, rounding the output <= u vmax; the f32 terms stay below 1e-6.
Every element is compared.
"""
import functools
import json
import os
import zlib

import pytest
import torch

import attn_blocks
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
BF, HF = torch.bfloat16, torch.float16


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def _check(got, ref, vmax, dtype, what):
    assert got.dtype == dtype and got.shape == ref.shape, what
    g = got.double()
    assert torch.isfinite(g).all(), what
    excess = (g - ref).abs() - (3.0 * U[dtype] * vmax + 1e-6)
    worst = float(((g - ref).abs() / (U[dtype] * vmax + 1e-30)).max())
    print(f"{what}: worst |got - ref| = {worst:.3f} u vmax")
    assert float(excess.max()) <= 0.0, f"{what}: {int((excess > 0).sum())} elements beyond 3 u vmax, worst {worst:.2f}"


# ----------------------------------------------------------------------------- window form
@functools.lru_cache(maxsize=None)
def _swin_buffers(h, w, heads, hd, ws, shift):
    from tramba_amd.encoders import SwinTransformerBlock
    blk = SwinTransformerBlock(heads * hd, (h, w), heads, ws, shift, 1.0, 0.0)
    assert (blk.window_size, blk.shift_size) == (ws, shift)
    mask = None if blk.attn_mask is None else blk.attn_mask.to(DEV).double()
    return blk.attn.relative_position_index.to(DEV), mask


def _window_ref(qkv, table, ws, shift, heads):
    """(ref, vmax), both (B, H, W, C) fp64, the long way round"""
    from tramba_amd.encoders import _unwindows, _windows
    b, h, w, c3 = qkv.shape
    c, n = c3 // 3, ws * ws
    hd = c // heads
    index, mask = _swin_buffers(h, w, heads, hd, ws, shift)
    x = qkv.double()
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = _windows(x, ws)                                                            # (B, nW, N, 3C)
    nw = xw.shape[1]
    q, k, v = xw.view(b, nw, n, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)             # (B, nW, nH, N, hd)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    s = s + table.double()[index.view(-1)].view(n, n, heads).permute(2, 0, 1)[None, None]
    if shift:
        s = s + mask[None, :, None]
    o = torch.softmax(s, -1) @ v
    vmax = v.abs().amax(-2, keepdim=True).expand_as(o)

    def back(t):
        t = _unwindows(t.transpose(2, 3).reshape(b, nw, n, c), ws, h, w)
        return torch.roll(t, shifts=(shift, shift), dims=(1, 2)) if shift else t
    return back(o), back(vmax)


def _window_inputs(tag, dtype, b, h, w, heads, hd, ws, table_scale=0.5, q_scale=3.0):
    g = _gen("win", tag, dtype, b, h, w, heads, hd, ws)
    c = heads * hd
    qkv = torch.randn(b, h, w, 3, c, generator=g)
    qkv[:, :, :, 0] *= q_scale                       # q and k at 2-4x unit scale: a peaked softmax
    qkv[:, :, :, 1] *= 2.0
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * table_scale
    return qkv.view(b, h, w, 3 * c).to(dtype).to(DEV), table.to(DEV)


# name: (dtypes, B, H, W, heads, hd, ws, shift, table scale).  The host deals 16-query tiles to workgroups by
# tiles-per-workgroup = clamp(problems * tiles / 512, 1, tiles), problems = B * windows * heads; the branch is named per case.
WINDOW_CASES = {
    # N = 144 of the model, 2 x 2 windows: all nine mask regions.  32 problems x 9 tiles: one tile per workgroup
    "ws12_24x24_s6": ((BF, HF), 2, 24, 24, 4, 32, 12, 6, 0.5),
    # the single window of the res <= ws case.  2 problems: one tile per workgroup
    "ws12_12x12_s0": ((BF,), 1, 12, 12, 2, 32, 12, 0, 0.5),
    # H != W: an H / W swap shows.  one tile per workgroup
    "ws12_24x36_s6": ((BF,), 1, 24, 36, 2, 32, 12, 6, 0.5),
    # N = 49, ragged against 16 and 32; C = 96.  one tile per workgroup
    "ws7_14x14_s3": ((BF,), 1, 14, 14, 3, 32, 7, 3, 0.5),
    "ws8_16x16_s4_hd64": ((BF,), 1, 16, 16, 1, 64, 8, 4, 0.5),
    # N = 256, the cap (the 8-step kernel)
    "ws16_16x16_s0": ((BF,), 1, 16, 16, 2, 32, 16, 0, 0.5),
    "ws16_32x32_s8_hd64": ((HF,), 1, 32, 32, 1, 64, 16, 8, 0.5),
    # table entries up to +-30
    "ws12_24x24_s6_big_table": ((BF,), 1, 24, 24, 2, 32, 12, 6, 10.0),
    # Swin stage 0 at batch 1: 256 problems x 9 tiles -> 4 tiles per workgroup, 3 workgroups per problem (4 + 4 + 1 tiles)
    "ws12_96x96_s6_b1": ((BF,), 1, 96, 96, 4, 32, 12, 6, 0.5),
    # 528 problems x 4 tiles -> the whole problem in one workgroup (tiles-per-workgroup = tiles)
    "ws7_28x28_s3_b11": ((BF,), 11, 28, 28, 3, 32, 7, 3, 0.5),
}
WINDOW_PARAMS = [(name, dt) for name, case in WINDOW_CASES.items() for dt in case[0]]


@pytest.mark.parametrize("name,dtype", WINDOW_PARAMS, ids=[f"{n}-{str(d)[6:]}" for n, d in WINDOW_PARAMS])
def test_window_attention_matches_fp64(name, dtype):
    from tramba_amd import hip
    _, b, h, w, heads, hd, ws, shift, tscale = WINDOW_CASES[name]
    qkv, table = _window_inputs(name, dtype, b, h, w, heads, hd, ws, tscale)
    if tscale > 1:
        table = table.clamp(-30, 30)
        assert float(table.abs().max()) > 20
    got = hip.window_attention_cl(qkv, table, ws, shift, heads)
    ref, vmax = _window_ref(qkv, table, ws, shift, heads)
    _check(got, ref, vmax, dtype, name)


@pytest.mark.parametrize("shift", [6, 0])
def test_window_mask_and_bias_in_isolation(shift):
    """q = 0 and table = 0: every key of the query's own region weighs the same -> the mean of v over that region (the
    -100 of the other regions is exp(-100) ~ 4e-44 of a weight).  q = 0 with a random table: the bias-only softmax."""
    from tramba_amd import hip
    from tramba_amd.encoders import _unwindows, _windows
    b, h, w, heads, hd, ws = 1, 24, 36, 2, 32, 12
    c, n = heads * hd, ws * ws
    qkv, table = _window_inputs("iso", BF, b, h, w, heads, hd, ws)
    qkv.view(b, h, w, 3, c)[:, :, :, 0] = 0
    got = hip.window_attention_cl(qkv, torch.zeros_like(table), ws, shift, heads)
    _, mask = _swin_buffers(h, w, heads, hd, ws, shift)
    v = qkv.view(b, h, w, 3, c)[:, :, :, 2].double()
    if shift:
        v = torch.roll(v, shifts=(-shift, -shift), dims=(1, 2))
    vw = _windows(v, ws)                                                            # (B, nW, N, C)
    same = torch.ones(vw.shape[1], n, n, dtype=torch.float64, device=DEV) if mask is None else (mask == 0).double()
    if shift:
        assert len({int(x) for x in same.sum(-1).flatten().tolist()}) > 2          # regions of several sizes occur
    mean = (same / same.sum(-1, keepdim=True))[None] @ vw
    vmax = vw.abs().amax(-2, keepdim=True).expand_as(mean)
    mean, vmax = _unwindows(mean, ws, h, w), _unwindows(vmax, ws, h, w)
    if shift:
        mean, vmax = (torch.roll(t, shifts=(shift, shift), dims=(1, 2)) for t in (mean, vmax))
    _check(got, mean, vmax, BF, f"region mean, shift {shift}")
    got = hip.window_attention_cl(qkv, table * 4, ws, shift, heads)
    ref, vmax = _window_ref(qkv, table * 4, ws, shift, heads)
    _check(got, ref, vmax, BF, f"bias only, shift {shift}")


# ----------------------------------------------------------------------------- kv form
def _kv_ref(q, kv, heads):
    b, n, c = q.shape
    m, hd = kv.shape[1], c // heads
    qd = q.double().view(b, n, heads, hd).transpose(1, 2)
    k, v = kv.double().view(b, m, 2, heads, hd).permute(2, 0, 3, 1, 4)
    o = torch.softmax((qd @ k.transpose(-1, -2)) * hd ** -0.5, -1) @ v              # (B, nH, N, hd)
    vmax = v.abs().amax(-2, keepdim=True).expand_as(o)
    return o.transpose(1, 2).reshape(b, n, c), vmax.transpose(1, 2).reshape(b, n, c)


def _kv_inputs(tag, dtype, b, n, m, heads, hd):
    g = _gen("kv", tag, dtype, b, n, m, heads, hd)
    c = heads * hd
    q = torch.randn(b, n, c, generator=g) * 3.0
    kv = torch.randn(b, m, 2, c, generator=g)
    kv[:, :, 0] *= 2.0
    return q.to(dtype).to(DEV), kv.view(b, m, 2 * c).to(dtype).to(DEV)


# name: (dtypes, B, N, M, heads, hd); tiles-per-workgroup rule as above with problems = B * heads
KV_CASES = {
    "n144_m144_h8": ((BF, HF), 2, 144, 144, 8, 64),     # PVT stage 4: 16 problems x 9 tiles, one tile per workgroup
    "n576_m36_h5": ((BF,), 1, 576, 36, 5, 64),          # C = 320; M ragged against 16
    "n100_m1": ((BF,), 2, 100, 1, 2, 64),               # N ragged against 16: the last tile stores 4 rows
    "n100_m17": ((BF,), 2, 100, 17, 2, 64),
    "n100_m256": ((BF,), 2, 100, 256, 2, 64),           # the cap
    "n100_m160_hd32": ((BF, HF), 1, 100, 160, 2, 32),
    "n9216_m144_h1": ((BF,), 2, 9216, 144, 1, 64),      # PVT stage 1: 2 problems x 576 tiles -> 2 tiles per workgroup
    "n20_m40_b300": ((BF,), 300, 20, 40, 2, 32),        # 600 problems x 2 tiles -> the whole problem in one workgroup
}
KV_PARAMS = [(name, dt) for name, case in KV_CASES.items() for dt in case[0]]


@pytest.mark.parametrize("name,dtype", KV_PARAMS, ids=[f"{n}-{str(d)[6:]}" for n, d in KV_PARAMS])
def test_kv_attention_matches_fp64(name, dtype):
    from tramba_amd import hip
    _, b, n, m, heads, hd = KV_CASES[name]
    q, kv = _kv_inputs(name, dtype, b, n, m, heads, hd)
    got = hip.kv_attention_cl(q, kv, heads)
    ref, vmax = _kv_ref(q, kv, heads)
    _check(got, ref, vmax, dtype, name)


def test_kv_attention_ignores_what_lies_beyond_m():
    """17 keys at the head of a larger allocation whose remaining rows are NaN: pad keys are read from nowhere"""
    from tramba_amd import hip
    heads, hd, n, m = 2, 64, 100, 17
    q, kv = _kv_inputs("nan", BF, 1, n, m, heads, hd)
    big = torch.full((1, 64, 2 * heads * hd), float("nan"), dtype=BF, device=DEV)
    big[:, :m] = kv
    sl = big[:, :m]
    assert sl.is_contiguous() and sl.data_ptr() == big.data_ptr() and torch.isnan(big[:, m:]).all()
    got = hip.kv_attention_cl(q, sl, heads)
    assert torch.isfinite(got).all()
    ref, vmax = _kv_ref(q, kv, heads)
    _check(got, ref, vmax, BF, "nan beyond M")
    assert torch.equal(got, hip.kv_attention_cl(q, kv, heads))


# ----------------------------------------------------------------------------- properties, both forms
def _ops():
    from tramba_amd import hip
    qkv, table = _window_inputs("prop", BF, 2, 24, 24, 4, 32, 12)
    q, kv = _kv_inputs("prop", BF, 2, 144, 144, 8, 64)
    return {"window": lambda: hip.window_attention_cl(qkv, table, 12, 6, 4), "kv": lambda: hip.kv_attention_cl(q, kv, 8)}


def test_two_runs_and_a_graph_replay_are_bitwise_equal():
    for name, op in _ops().items():
        eager = op()
        assert torch.equal(eager, op()), name
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                got = op()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            got.zero_()
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, eager), name


def test_two_streams_at_once_give_the_same_bits():
    ops = _ops()
    side = torch.cuda.Stream()
    for name, op in ops.items():
        ref = op().clone()
        torch.cuda.synchronize()
        for sname, sop in ops.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                keep = [sop() for _ in range(30)]
            outs = [op() for _ in range(10)]
            torch.cuda.synchronize()
            assert all(torch.equal(o, ref) for o in outs), (name, sname)
            del keep


# ----------------------------------------------------------------------------- module level
def _counting(monkeypatch, name):
    from tramba_amd import hip
    calls = []
    real = getattr(hip, name)

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(hip, name, wrapper)
    return calls


def _parity_margin(kind):
    """profiles/attn_parity.json (scripts/measure_attn_parity.py, 16 seeds on an MI355X, the blocks of tests/golden/
    attn_blocks.py): both paths are 16-bit roundings of the same math and differ only in where P is rounded, so the stock
    path's own seed-to-seed spread is the yardstick: m = (largest stock error / smallest stock error) - 1 over the seeds
    (0.027 for the Swin block, 0.041 for the PVT block).  Read from the file, so the test and the measurement cannot drift."""
    with open(os.path.join(ROOT, "profiles", "attn_parity.json")) as f:
        m = json.load(f)[kind]["m"]
    assert 0.0 < m < 0.1, m            # a seed-to-seed spread of one block's rounding error; anything else is not that number
    return m


SEEDS = range(8)


@pytest.mark.parametrize("kind", ["swin", "pvt"])
def test_block_reaches_the_kernel_once_and_keeps_the_stock_error(monkeypatch, kind):
    calls = _counting(monkeypatch, "window_attention_cl" if kind == "swin" else "kv_attention_cl")
    m = _parity_margin(kind)
    for seed in SEEDS:
        before = len(calls)
        fused, stock = attn_blocks.block_errors(kind, seed)          # one fused forward, one stock 16-bit, one stock fp32
        assert len(calls) - before == 1
        print(f"{kind} seed {seed}: fused {fused:.3e} stock {stock:.3e}")
        assert fused <= stock * (1 + m), (kind, seed, fused, stock, m)


def test_fused_swin_block_builds_no_bias_mask_tensor():
    blk, x = attn_blocks.swin_block(0)
    with torch.no_grad():
        blk(x)
        assert "_tramba_cache" not in blk.attn.__dict__               # no expanded bias + mask tensor on this path
        blk._forward_stock(x)
    assert ("bias", torch.bfloat16) in blk.attn._tramba_cache._store   # the stock path's, as before


def test_block_keeps_the_stock_path_where_the_kernel_does_not_apply(monkeypatch):
    from tramba_amd.encoders import SwinTransformerBlock, _PvtBlock
    wcalls = _counting(monkeypatch, "window_attention_cl")
    kcalls = _counting(monkeypatch, "kv_attention_cl")
    swin = attn_blocks.seeded(SwinTransformerBlock(128, (24, 24), 4, 12, 6, 4.0, 0.0), 0)
    pvt = attn_blocks.seeded(_PvtBlock(128, 2, 4, True, 0.0, 1, 1e-6), 0)                 # sr 1 on 24 x 24: 576 keys
    x = synth.synth_input("attn_stock", (1, 576, 128)).to(DEV)
    with torch.no_grad():
        swin(x)                                                                 # fp32
        pvt(x.bfloat16(), 24, 24)                                               # 576 keys > 256
    swin(x.bfloat16().requires_grad_())                                         # autograd on
    swin.train()
    with torch.no_grad():
        swin(x.bfloat16())                                                      # training mode
    assert not wcalls and not kcalls


# ----------------------------------------------------------------------------- whole model
@pytest.mark.parametrize("name,entry,count", [("Tramba-S-TSOD", "window_attention_cl", 22),
                                              ("Tramba-P-TSOD", "kv_attention_cl", 41)])
def test_whole_model_reaches_the_kernels_and_replays_bitwise(monkeypatch, name, entry, count):
    """The library attention is reached once per block, builds no bias + mask tensor, and a `GraphedForward` replay is
    bit-identical to the eager forward.

    The bitwise half runs with the encoders' framework convolutions (patch embeddings, PVT's `sr`) pinned to
    `attn_blocks.gemm_conv`, in the eager forward and in the capture alike.  The framework's own choice is not
    reproducible run to run: PVT's third patch embedding at batch 4 gave different bits on 60 of 60 repeats of the same
    call (an implicit-GEMM kernel that splits the reduction and adds the parts with atomics), and the same kernel family
    serves batch 1 -- there an unpinned form of this test failed once in a full-suite run with nothing of this project in
    the difference.  Everything else in the forward is the library's, so with the convolutions pinned any difference is
    the library's own (pinned: 0 of 10 eager forwards and 0 of 10 replays differ, at batch 1 and at batch 4)."""
    import tramba_amd as ta
    from tramba_amd import encoders
    m = ta.bulid_model_enc(name)
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        new.setdefault(k, sd[k])
    m.load_state_dict(new, strict=True)
    m = ta.prepare_inference(m.to(DEV).eval(), torch.bfloat16)
    x = synth.synth_input("attn_whole", (1, 3, 384, 384)).to(DEV)
    calls = _counting(monkeypatch, entry)
    with torch.no_grad():
        plain = [o.clone() for o in m(x)]       # the model as it ships, framework convolutions included
    assert len(calls) == count                  # Swin: features_cl(last=False) skips the last stage's two blocks
    assert all(torch.isfinite(o).all() for o in plain)
    for mod in m.modules():
        cache = mod.__dict__.get("_tramba_cache")
        assert cache is None or not any(isinstance(k, tuple) and k[0] == "bias" for k in cache._store), type(mod)
    monkeypatch.setattr(encoders, "_conv", attn_blocks.gemm_conv)
    with torch.no_grad():
        eager = [o.clone() for o in m(x)]
        again = m(x)
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    assert len(calls) == 3 * count
    assert all(torch.isfinite(o).all() for o in eager)
    graphed = ta.GraphedForward(m, strict=True)
    for _ in range(2):
        replay = graphed(x)
        torch.cuda.synchronize()
        for a, b in zip(eager, replay):
            assert torch.equal(a, b)
