"""GPU tests of the encoder convolutions on the library (csrc/patch_conv.hip) and of the modules that reach them behind
`encoders.set_library_convolutions`.

References are fp64 on the same 16-bit-rounded inputs, built from `F.unfold` (a gather) and an fp64 matmul, never from an
fp64 `conv2d`.  Every element is compared against a bound that is derived, not measured:

patch_conv_cl      |y - ref| <= u |ref| + (K + 2) 2^-24 A + 1e-6,  A = sum_k |x_k| |w_k| + |bias|
                   (products of 16-bit numbers are exact in f32; K f32 additions in any order, the partial sums and the
                   bias cost at most (K + 2) 2^-24 A to first order; one rounding to the 16-bit output costs u |ref|)
patch_embed_ln     |y - ref| <= u |ref| + 2^-24 (K + 16)(2 + |z|) |ln_w| max_c(A_c) / sigma + 1e-6
                   (an f32 convolution error e_c <= (K + 1) 2^-24 A_c per channel moves the normalised value z by at most
                   (max_c e_c)(2 + |z|) / sigma to first order -- itself, the mean and the deviation; the remaining
                   operations of the LayerNorm are a handful of f32 roundings, covered by the + 15)

u is the unit round-off of the output format: 2^-8 for bf16, 2^-11 for fp16.  The worst ratio to the bound is printed per case.
"""
import functools
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attn_blocks
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF, HF = torch.bfloat16, torch.float16
NAN = float("nan")


def _name(dtype):
    return str(dtype)[6:]


# ----------------------------------------------------------------------------- patch_conv_cl
# name: (B, H, W, Cin, Cout, r)
PATCH_CASES = {
    "r8_ragged_20x28": (2, 20, 28, 64, 64, 8),      # 2 x 3 tokens per image: M = 12 < one tile; K = 4096, the deepest
    "r4_24x24": (1, 24, 24, 128, 128, 4),           # M = 36: a ragged last tile
    "r2_26x22_c320": (2, 26, 22, 320, 320, 2),      # M = 286, a tile straddles the two images; Cout = 5 x 64
    "r2_8x8_cout8": (3, 8, 8, 64, 8, 2),            # the narrowest column block
    "r8_96x96_stage1": (1, 96, 96, 64, 64, 8),      # the workload's own stage-1 call
}


@functools.lru_cache(maxsize=None)
def _patch_inputs(name, dtype):
    """(x with NaN in the trailing rows / columns, K-major weight, f32 bias, fp64 ref, fp64 bound), all on the device"""
    b, h, w, cin, cout, r = PATCH_CASES[name]
    ho, wo = h // r, w // r
    k = r * r * cin
    x = synth.synth_input(f"pconv_x_{name}", (b, h, w, cin)).to(dtype).to(DEV)
    wt = synth.synth_tensor(f"pconv_{name}.weight", (cout, cin, r, r)).to(dtype).to(DEV)        # reference layout
    bias = synth.synth_tensor(f"pconv_{name}.bias", (cout,)).mul(10).to(DEV)
    xd = x[:, :r * ho, :r * wo].permute(0, 3, 1, 2).double()
    cols = F.unfold(xd, r, stride=r).transpose(1, 2)                                            # (B, L, Cin r r)
    wd = wt.double().reshape(cout, k)
    ref = (cols @ wd.t() + bias.double()).view(b, ho, wo, cout)
    mag = (cols.abs() @ wd.abs().t() + bias.double().abs()).view(b, ho, wo, cout)
    bound = U[dtype] * ref.abs() + (k + 2) * 2.0 ** -24 * mag + 1e-6
    x[:, r * ho:] = NAN                                                # what the kernel must never read
    x[:, :, r * wo:] = NAN
    return x, wt.permute(0, 2, 3, 1).contiguous(), bias, ref, bound


def _raw_patch_conv(x, wk, bias, y):
    from tramba_amd import hip
    b, h, w, cin = x.shape
    rc = hip.lib().tramba_patch_conv_cl(x.data_ptr(), wk.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(), b,
                                        h, w, cin, wk.shape[0], wk.shape[1], hip.dt(x), hip._stream())
    assert rc == 0, hip.lib().tramba_last_error()


def _within(got, ref, bound, what):
    g = got.double()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output (an element not written, or a poisoned element read)"
    ratio = (g - ref).abs() / bound
    worst = float(ratio.max())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound, worst {worst:.3f}"


@pytest.mark.parametrize("dtype", [BF, HF], ids=_name)
@pytest.mark.parametrize("name", list(PATCH_CASES))
def test_patch_conv_matches_fp64(name, dtype):
    from tramba_amd import hip
    x, wk, bias, ref, bound = _patch_inputs(name, dtype)
    b, h, w, cin, cout, r = PATCH_CASES[name]
    assert hip.patch_conv_supported(dtype, cin, cout, r)
    y = torch.full(ref.shape, NAN, dtype=dtype, device=DEV)            # poisoned: every output must be written
    _raw_patch_conv(x, wk, bias, y)
    _within(y, ref, bound, f"patch_conv {name} {_name(dtype)}")
    got = hip.patch_conv_cl(x, wk, bias)
    assert got.dtype == dtype and torch.equal(got, y)
    # no bias == a zero bias, bitwise
    assert torch.equal(hip.patch_conv_cl(x, wk, None), hip.patch_conv_cl(x, wk, torch.zeros_like(bias)))


def test_patch_conv_bound_is_sharp_enough_to_see_a_wrong_kernel():
    """what a dropped kernel row or a mis-strided weight would give lies orders of magnitude beyond the bound"""
    x, wk, bias, ref, bound = _patch_inputs("r4_24x24", BF)
    b, h, w, cin, cout, r = PATCH_CASES["r4_24x24"]
    xd = x.double().view(b, h // r, r, w // r, r, cin).permute(0, 1, 3, 2, 4, 5)                 # (B, Ho, Wo, di, dj, c)
    wd = wk.double()
    dropped = torch.einsum("bijyxc,oyxc->bijo", xd[:, :, :, :r - 1], wd[:, :r - 1]) + bias.double()
    swapped = torch.einsum("bijyxc,oxyc->bijo", xd, wd) + bias.double()
    full = torch.einsum("bijyxc,oyxc->bijo", xd, wd) + bias.double()
    assert float(((full - ref).abs() / bound).max()) < 1e-3           # the same contraction, written another way
    for wrong in (dropped, swapped):
        assert float(((wrong - ref).abs() / bound).max()) > 30


# ----------------------------------------------------------------------------- patch_embed_ln
# name: (form, B, H, W); form = (k, stride, pad, Cout)
PVT_FORM, SWIN_FORM = (7, 4, 3, 64), (4, 4, 0, 128)
EMBED_CASES = {
    "pvt_21x30": (PVT_FORM, 2, 21, 30),             # 6 x 8 tokens: padding on all four sides, odd sizes
    "pvt_64x64": (PVT_FORM, 1, 64, 64),
    "swin_24x24": (SWIN_FORM, 2, 24, 24),
}


@functools.lru_cache(maxsize=None)
def _embed_inputs(name, dtype):
    """image values exactly representable in `dtype` (so the f32 and the 16-bit image hold the same numbers), conv weights
    and bias rounded to `dtype` as prepare_inference leaves them"""
    (k, stride, pad, cout), b, h, w = EMBED_CASES[name]
    img = synth.synth_input(f"pembed_img_{name}", (b, 3, h, w)).to(dtype).to(DEV)
    conv = nn.Conv2d(3, cout, k, stride, pad)
    norm = nn.LayerNorm(cout)
    with torch.no_grad():
        conv.weight.copy_(synth.synth_tensor(f"pembed_{name}.proj.weight", conv.weight.shape))
        conv.bias.copy_(synth.synth_tensor(f"pembed_{name}.proj.bias", (cout,)).mul(5))
        norm.weight.copy_(synth.synth_tensor(f"pembed_{name}.norm.weight", (cout,)))
        norm.bias.copy_(synth.synth_tensor(f"pembed_{name}.norm.bias", (cout,)).mul(5))
    conv.to(DEV).to(dtype)
    norm.to(DEV)
    for p in list(conv.parameters()) + list(norm.parameters()):
        p.requires_grad_(False)
    wd, bd = conv.weight.double().reshape(cout, -1), conv.bias.double()
    cols = F.unfold(img.double(), k, padding=pad, stride=stride).transpose(1, 2)                # (B, L, 3 k k)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    assert cols.shape[1] == ho * wo
    c = cols @ wd.t() + bd
    mag = (cols.abs() @ wd.abs().t() + bd.abs()).amax(-1, keepdim=True)
    mean = c.mean(-1, keepdim=True)
    var = (c - mean).square().mean(-1, keepdim=True)
    assert float(var.min()) > 1e-3                                     # no constant rows
    z = (c - mean) / torch.sqrt(var + norm.eps)
    ref = z * norm.weight.double() + norm.bias.double()
    kk = 3 * k * k
    bound = (U[dtype] * ref.abs() + 2.0 ** -24 * (kk + 16) * (2 + z.abs()) * norm.weight.double().abs() * mag / var.sqrt()
             + 1e-6)
    shape = (b, ho, wo, cout)
    return img, conv, norm, ref.view(shape), bound.view(shape)


@pytest.mark.parametrize("f32_image", [True, False], ids=["img_f32", "img_16bit"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=_name)
@pytest.mark.parametrize("name", list(EMBED_CASES))
def test_patch_embed_ln_matches_fp64_and_beats_the_stock_path(name, dtype, f32_image):
    from tramba_amd import encoders, hip
    img, conv, norm, ref, bound = _embed_inputs(name, dtype)
    (k, stride, pad, cout), b, h, w = EMBED_CASES[name]
    assert hip.patch_embed_ln_supported(dtype, k, stride, pad, cout)
    got = hip.patch_embed_ln(img.float() if f32_image else img, conv.weight.float().contiguous(), conv.bias.float(),
                             norm.weight, norm.bias, norm.eps, stride, pad, dtype)
    assert got.dtype == dtype
    what = f"patch_embed_ln {name} {_name(dtype)} {'f32' if f32_image else '16-bit'} image"
    _within(got, ref, bound, what)
    with torch.no_grad():
        stock = encoders._ln(norm, encoders._conv(conv, img).flatten(2).transpose(1, 2)).view(ref.shape)
    e_lib, e_stock = attn_blocks.rel_l2(got, ref), attn_blocks.rel_l2(stock, ref)
    print(f"{what}: rel L2 library {e_lib:.4e} stock {e_stock:.4e}")
    assert e_lib <= e_stock


def test_patch_embed_ln_refuses_other_forms():
    from tramba_amd import hip
    img = torch.zeros(1, 3, 32, 32, device=DEV)
    ones = torch.ones(64, device=DEV)
    with pytest.raises(hip.TrambaHipError, match="neither"):
        hip.patch_embed_ln(img, torch.zeros(64, 3, 3, 3, device=DEV), ones, ones, ones, 1e-5, 2, 1, BF)
    with pytest.raises(hip.TrambaHipError, match="neither"):
        hip.patch_embed_ln(img, torch.zeros(64, 3, 7, 7, device=DEV), ones, ones, ones, 1e-5, 4, 2, BF)


# ----------------------------------------------------------------------------- reproducibility
# conv3x3s2_cl at PVT's patch_embed2..4 of a 384 x 384 image: (H = W, Cin, Cout)
S2_CASES = ((96, 64, 128), (48, 128, 320), (24, 320, 512))


def _ops():
    from tramba_amd import hip
    ops = {}
    for name in PATCH_CASES:
        x, wk, bias, _, _ = _patch_inputs(name, BF)
        ops[f"patch_conv {name}"] = functools.partial(hip.patch_conv_cl, x, wk, bias)
    for name in EMBED_CASES:
        img, conv, norm, _, _ = _embed_inputs(name, BF)
        ops[f"patch_embed_ln {name}"] = functools.partial(hip.patch_embed_ln, img, conv.weight.float().contiguous(),
                                                          conv.bias.float(), norm.weight, norm.bias, norm.eps,
                                                          EMBED_CASES[name][0][1], EMBED_CASES[name][0][2], BF)
    for side, cin, cout in S2_CASES:
        x = synth.synth_input(f"s2_x_{side}", (1, side, side, cin)).to(BF).to(DEV)
        wk = synth.synth_tensor(f"s2_{side}.weight", (cout, 9 * cin)).to(BF).to(DEV)
        bias = synth.synth_tensor(f"s2_{side}.bias", (cout,)).to(DEV)
        ops[f"conv3x3s2 {side}"] = functools.partial(hip.conv3x3s2_cl, x, wk, bias)
    return ops


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


def test_a_busy_second_stream_does_not_change_the_bits():
    ops = _ops()
    side = torch.cuda.Stream()
    for name, op in ops.items():
        ref = op().clone()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            keep = [sop() for _ in range(3) for sop in ops.values()]
        outs = [op() for _ in range(10)]
        torch.cuda.synchronize()
        assert all(torch.equal(o, ref) for o in outs), name
        del keep


# ----------------------------------------------------------------------------- module level
def _counting(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapper)
    return calls


def _parity_margin():
    """profiles/attn_parity.json["pvt"]["m"]: the stock path's measured seed-to-seed spread of this very block's error"""
    with open(os.path.join(ROOT, "profiles", "attn_parity.json")) as f:
        m = json.load(f)["pvt"]["m"]
    assert 0.0 < m < 0.1, m
    return m


def test_pvt_block_reaches_patch_conv_once_and_keeps_the_stock_error(monkeypatch):
    from tramba_amd import encoders, hip
    pcalls = _counting(monkeypatch, hip, "patch_conv_cl")
    ccalls = _counting(monkeypatch, encoders, "_conv")
    m = _parity_margin()
    for seed in range(8):
        blk, x = attn_blocks.pvt_block(seed)           # _PvtBlock(128, 2, 4, True, 0.0, 2, 1e-6), bf16 (2, 576, 128)
        assert encoders.set_library_convolutions(blk) == 1
        with torch.no_grad():
            p0, c0 = len(pcalls), len(ccalls)
            lib = blk(x, 24, 24)
            assert (len(pcalls) - p0, len(ccalls) - c0) == (1, 0)
            encoders.set_library_convolutions(blk, enabled=False)
            blk.attn.forward = blk.attn._forward_stock
            stock, ref = blk(x, 24, 24), blk(x.float(), 24, 24)
            assert len(pcalls) - p0 == 1 and len(ccalls) - c0 == 2
        e_lib, e_stock = attn_blocks.rel_l2(lib, ref), attn_blocks.rel_l2(stock, ref)
        print(f"pvt block seed {seed}: library {e_lib:.3e} stock {e_stock:.3e}")
        assert e_lib <= e_stock * (1 + m), (seed, e_lib, e_stock, m)


def test_pvt_block_keeps_conv_where_the_library_path_does_not_apply(monkeypatch):
    from tramba_amd import encoders, hip
    pcalls = _counting(monkeypatch, hip, "patch_conv_cl")
    blk, x = attn_blocks.pvt_block(0)
    ccalls = []                                        # `_conv` calls of the spatial-reduction conv (with autograd on the
    real = encoders._conv                              # MLP's depth-wise conv goes through `_conv` too)
    monkeypatch.setattr(encoders, "_conv", lambda m, t: (ccalls.append(1) if m is blk.attn.sr else None, real(m, t))[1])
    encoders.set_library_convolutions(blk)
    with torch.no_grad():
        blk(x.float(), 24, 24)                                                  # fp32
    assert (len(pcalls), len(ccalls)) == (0, 1)
    blk(x.clone().requires_grad_(), 24, 24)                                     # autograd on
    assert (len(pcalls), len(ccalls)) == (0, 2)
    blk.train()
    blk(x, 24, 24)                                                              # training mode: parameters require grad
    assert (len(pcalls), len(ccalls)) == (0, 3)
    blk.eval()
    encoders.set_library_convolutions(blk, enabled=False)
    with torch.no_grad():
        blk(x, 24, 24)                                                          # flag off
    assert (len(pcalls), len(ccalls)) == (0, 4)
    encoders.set_library_convolutions(blk)
    with torch.no_grad():
        blk(x, 24, 24)
    assert (len(pcalls), len(ccalls)) == (1, 4)


# ----------------------------------------------------------------------------- whole model
@pytest.mark.parametrize("name,counts", [("Tramba-P-TSOD", (1, 3, 38)), ("Tramba-S-TSOD", (1, 0, 0))])
def test_whole_model_calls_no_framework_convolution_and_replays_bitwise(monkeypatch, name, counts):
    """bf16, 384 x 384, batch 1, switch on: the forward succeeds with `encoders._conv` raising, reaches the entries the
    expected number of times, and two eager forwards and two `GraphedForward` replays agree bit for bit with no
    convolution pinned."""
    import tramba_amd as ta
    from tramba_amd import encoders, hip
    m = ta.bulid_model_enc(name)
    sd = m.state_dict()
    new = synth.synth_state_dict(((k, v.shape) for k, v in sd.items()), keep=synth.CONST_KEYS)
    for k in sd:
        new.setdefault(k, sd[k])
    m.load_state_dict(new, strict=True)
    m = ta.prepare_inference(m.to(DEV).eval(), torch.bfloat16)
    x = synth.synth_input("attn_whole", (1, 3, 384, 384)).to(DEV)
    with torch.no_grad():
        off = [o.clone() for o in m(x)]                                         # the model as it ships
    assert encoders.set_library_convolutions(m) == {"Tramba-P-TSOD": 42, "Tramba-S-TSOD": 1}[name]

    def refuse(*a, **k):
        raise AssertionError("encoders._conv reached with the library convolutions switched on")
    monkeypatch.setattr(encoders, "_conv", refuse)
    calls = [_counting(monkeypatch, hip, e) for e in ("patch_embed_ln", "conv3x3s2_cl", "patch_conv_cl")]
    with torch.no_grad():
        eager = [o.clone() for o in m(x)]
        assert tuple(len(c) for c in calls) == counts
        again = m(x)
    assert all(torch.isfinite(o).all() for o in eager)
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    for i, (a, b) in enumerate(zip(eager, off)):
        print(f"{name} output {i}: rel L2 from the switch-off forward {attn_blocks.rel_l2(a, b):.3e}")
    graphed = ta.GraphedForward(m, strict=True)
    for _ in range(2):
        replay = graphed(x)
        torch.cuda.synchronize()
        for a, b in zip(eager, replay):
            assert torch.equal(a, b)
