"""GPU tests of the backward of the kernel = stride convolution (csrc/patch_conv_bwd.hip), of `encoders._PatchConvFn` and of
the encoder training path behind `encoders.set_library_training`.

References are fp64 autograd of `F.conv2d` on the same 16-bit inputs; every element is compared against a bound that is
derived, not measured.  Products of two 16-bit numbers are exact in f32, so the only errors are the f32 additions, in any
order, and one output rounding:

dgrad           |gx - ref| <= u |ref| + (Cout + 2) 2^-24 A + 1e-6,  A = sum_co |gy| |W|
wgrad, bias     |g  - ref| <= (M + 2) 2^-24 A + 1e-6,               A = the same contraction over magnitudes, M = B Ho Wo

u is the unit round-off of the activation format: 2^-8 for bf16, 2^-11 for fp16.  The worst ratio to the bound is printed
per case."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import enc_train_blocks
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF, HF = torch.bfloat16, torch.float16
NAN = float("nan")

# name: (B, H, W, Cin, Cout, r)
CASES = {
    "r8_20x28": (1, 20, 28, 64, 64, 8),            # M = 6: one ragged tile; rows 16-19 and columns 24-27 of gx are zeros
    "r4_24x24": (2, 24, 24, 128, 128, 4),          # M = 72: a ragged last tile
    "r2_26x22_c320": (2, 26, 22, 320, 320, 2),     # a tile across two images, Cout no multiple of 64, odd trailing row / column
    "r2_8x8_cout8": (1, 8, 8, 64, 8, 2),           # the smallest Cout
    "r8_96x96_stage1": (1, 96, 96, 64, 64, 8),     # the workload's stage-1 call, K = 4096
}
PARAMS = [(n, BF) for n in CASES] + [("r2_26x22_c320", HF), ("r8_96x96_stage1", HF)]
IDS = [f"{n}-{str(d)[6:]}" for n, d in PARAMS]


def _bwd64(x, w, gy, r):
    """fp64 autograd of F.conv2d on the host: x (B, H, W, Cin), w (Cout, Cin, r, r), gy (B, Ho, Wo, Cout) ->
    (gx (B, H, W, Cin), gw K-major (Cout, r, r, Cin), gb (Cout))"""
    xd = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    wd = w.clone().requires_grad_()
    bd = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, wd, bd, stride=r).backward(gy.permute(0, 3, 1, 2).contiguous())
    return xd.grad.permute(0, 2, 3, 1).contiguous(), wd.grad.permute(0, 2, 3, 1).contiguous(), bd.grad


@functools.lru_cache(maxsize=None)
def _inputs(name, dtype):
    """device tensors (x with NaN where no patch reaches, weight in the reference layout, its K-major copy, gy) and the
    fp64 references and bounds {gx, gw, gb}; computed once, never written to"""
    b, h, w, cin, cout, r = CASES[name]
    ho, wo = h // r, w // r
    m = b * ho * wo
    x = synth.synth_input(f"pcb_x_{name}", (b, h, w, cin)).to(dtype)
    wt = synth.synth_tensor(f"pcb_{name}.weight", (cout, cin, r, r)).to(dtype)
    gy = synth.synth_input(f"pcb_gy_{name}", (b, ho, wo, cout)).to(dtype)
    ref = _bwd64(x.double(), wt.double(), gy.double(), r)
    mag = _bwd64(x.double().abs(), wt.double().abs(), gy.double().abs(), r)
    bounds = (U[dtype] * ref[0].abs() + (cout + 2) * 2.0 ** -24 * mag[0] + 1e-6,
              (m + 2) * 2.0 ** -24 * mag[1] + 1e-6, (m + 2) * 2.0 ** -24 * mag[2] + 1e-6)
    x = x.to(DEV)
    x[:, r * ho:] = NAN                                                # what the weight gradient must never read
    x[:, :, r * wo:] = NAN
    return dict(x=x, wt=wt.to(DEV), wk=wt.permute(0, 2, 3, 1).contiguous().to(DEV), gy=gy.to(DEV),
                ref=dict(zip(("gx", "gw", "gb"), (t.to(DEV) for t in ref))),
                bound=dict(zip(("gx", "gw", "gb"), (t.to(DEV) for t in bounds))))


def _raw_dgrad(gy, wk, gx):
    from tramba_amd import hip
    b, h, w, cin = gx.shape
    rc = hip.lib().tramba_patch_conv_dgrad_cl(gy.data_ptr(), wk.data_ptr(), gx.data_ptr(), b, h, w, cin, wk.shape[0],
                                              wk.shape[1], hip.dt(gy), hip._stream())
    assert rc == 0, hip.lib().tramba_last_error()


def _raw_wgrad(gy, x, r, want_bias):
    """the entry on a NaN-filled workspace of exactly the size it asks for, its slabs added in index order"""
    from tramba_amd import hip
    b, h, w, cin = x.shape
    cout = gy.shape[-1]
    lib = hip.lib()
    nsplit = lib.tramba_patch_conv_wgrad_split(b, h, w, cin, cout, r)
    nbytes = lib.tramba_patch_conv_wgrad_work(b, h, w, cin, cout, r)
    slab = cout * r * r * cin + cout
    assert nsplit >= 1 and nbytes == nsplit * slab * 4
    work = torch.full((nsplit, slab), NAN, dtype=torch.float32, device=DEV)
    rc = lib.tramba_patch_conv_wgrad_cl(gy.data_ptr(), x.data_ptr(), work.data_ptr(), nbytes, b, h, w, cin, cout, r,
                                        int(want_bias), hip.dt(gy), hip._stream())
    assert rc == 0, lib.tramba_last_error()
    out = hip.slab_sum(work) if nsplit > 1 else work[0]
    return out[:slab - cout].view(cout, r, r, cin), out[slab - cout:]


def _within(got, ref, bound, what):
    g = got.double()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output (an element not written, or a poisoned element read)"
    ratio = (g - ref).abs() / bound
    worst = float(ratio.max())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound, worst {worst:.3f}"


# ----------------------------------------------------------------------------- the two entries
@pytest.mark.parametrize("name,dtype", PARAMS, ids=IDS)
def test_dgrad_matches_fp64_and_writes_every_element(name, dtype):
    from tramba_amd import hip
    d = _inputs(name, dtype)
    b, h, w, cin, cout, r = CASES[name]
    assert hip.patch_conv_train_supported(dtype, cin, cout, r)
    gx = torch.full((b, h, w, cin), NAN, dtype=dtype, device=DEV)      # poisoned: every element must be written
    _raw_dgrad(d["gy"], d["wk"], gx)
    _within(gx, d["ref"]["gx"], d["bound"]["gx"], f"dgrad {name} {str(dtype)[6:]}")
    ho, wo = h // r, w // r
    assert not gx[:, r * ho:].any() and not gx[:, :, r * wo:].any()    # exact zeros where no patch reaches
    if name == "r8_20x28":
        assert gx[:, 16:20].numel() > 0 and gx[:, :, 24:28].numel() > 0
        assert torch.equal(gx[:, 16:20], torch.zeros_like(gx[:, 16:20])) and torch.equal(gx[:, :, 24:28], torch.zeros_like(gx[:, :, 24:28]))
    got = hip.patch_conv_dgrad_cl(d["gy"], d["wk"], (b, h, w, cin))
    assert got.dtype == dtype and torch.equal(got, gx)


@pytest.mark.parametrize("name,dtype", PARAMS, ids=IDS)
def test_wgrad_and_bias_match_fp64(name, dtype):
    from tramba_amd import hip
    d = _inputs(name, dtype)
    b, h, w, cin, cout, r = CASES[name]
    gw, gb = _raw_wgrad(d["gy"], d["x"], r, True)
    _within(gw, d["ref"]["gw"], d["bound"]["gw"], f"wgrad {name} {str(dtype)[6:]}")
    _within(gb, d["ref"]["gb"], d["bound"]["gb"], f"bias grad {name} {str(dtype)[6:]}")
    gw0, gb0 = _raw_wgrad(d["gy"], d["x"], r, False)
    assert torch.equal(gw0, gw) and not gb0.any()                      # the same gw bits without the bias
    bw, bb = hip.patch_conv_wgrad_cl(d["gy"], d["x"], r, want_bias=True)
    assert bw.dtype == torch.float32 and torch.equal(bw, gw) and torch.equal(bb, gb)
    nw, nb = hip.patch_conv_wgrad_cl(d["gy"], d["x"], r)
    assert nb is None and torch.equal(nw, gw)


def test_bounds_are_sharp_enough_to_see_a_wrong_kernel():
    """fp64 references with (di, dj) exchanged in the weight, and with a kernel row dropped, lie outside the bounds"""
    d = _inputs("r4_24x24", BF)
    b, h, w, cin, cout, r = CASES["r4_24x24"]
    x = torch.nan_to_num(d["x"].double().cpu())
    wt, gy = d["wt"].double().cpu(), d["gy"].double().cpu()
    same = _bwd64(x, wt, gy, r)
    for got, key in zip(same, ("gx", "gw", "gb")):
        assert float(((got.to(DEV) - d["ref"][key]).abs() / d["bound"][key]).max()) < 1e-3
    swapped = _bwd64(x, wt.transpose(2, 3).contiguous(), gy, r)[0]
    cut = wt.clone()
    cut[:, :, r - 1] = 0
    dropped = _bwd64(x, cut, gy, r)[0]
    for wrong in (swapped, dropped):
        assert float(((wrong.to(DEV) - d["ref"]["gx"]).abs() / d["bound"]["gx"]).max()) > 1
    gw = same[1]                                                       # K-major (Cout, di, dj, Cin)
    gw_swapped = gw.transpose(1, 2).contiguous()
    gw_dropped = gw.clone()
    gw_dropped[:, r - 1] = 0
    for wrong in (gw_swapped, gw_dropped):
        assert float(((wrong.to(DEV) - d["ref"]["gw"]).abs() / d["bound"]["gw"]).max()) > 1


def test_backward_is_linear_in_gy_bit_for_bit():
    """bwd(2 gy) == 2 bwd(gy): doubling is exact in every format and commutes with every rounding unless a value overflows
    or a result falls into the denormals of its format; such results (counted, and few) are left out of the comparison"""
    from tramba_amd import hip
    for name, dtype in (("r2_26x22_c320", BF), ("r2_26x22_c320", HF), ("r8_20x28", BF)):
        d = _inputs(name, dtype)
        b, h, w, cin, cout, r = CASES[name]
        gy = d["gy"]
        tiny = 2.0 ** -13 if dtype == HF else 1e-30
        assert torch.isfinite(gy * 2).all() and float(gy.abs().max()) < 1e3      # (doubling a 16-bit denormal is exact)
        one = hip.patch_conv_dgrad_cl(gy, d["wk"], (b, h, w, cin))
        two = hip.patch_conv_dgrad_cl(gy * 2, d["wk"], (b, h, w, cin))
        ok = (one == 0) | ((one.abs().float() > tiny) & (one.abs().float() < 1e4))
        assert float(ok.float().mean()) > 0.99 and float(one.abs().max()) > 0
        assert torch.equal((one * 2)[ok], two[ok])
        w1, b1 = hip.patch_conv_wgrad_cl(gy, d["x"], r, want_bias=True)
        w2, b2 = hip.patch_conv_wgrad_cl(gy * 2, d["x"], r, want_bias=True)
        assert float(w1.abs().max()) < 1e30 and float(w1.abs()[w1 != 0].min()) > 1e-30
        assert torch.equal(w1 * 2, w2) and torch.equal(b1 * 2, b2) and float(w1.abs().max()) > 0


def _both(d, name):
    from tramba_amd import hip
    b, h, w, cin, cout, r = CASES[name]
    gx = hip.patch_conv_dgrad_cl(d["gy"], d["wk"], (b, h, w, cin))
    gw, gb = hip.patch_conv_wgrad_cl(d["gy"], d["x"], r, want_bias=True)
    return gx, gw, gb


@pytest.mark.parametrize("name", ["r2_26x22_c320", "r8_96x96_stage1"])
def test_two_runs_and_a_graph_replay_give_the_same_bits(name):
    d = _inputs(name, BF)
    first = _both(d, name)
    again = _both(d, name)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _both(d, name)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # no allocation of the entries' own, no synchronisation
        captured = _both(d, name)
    for _ in range(2):
        for t in captured:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, captured))


def test_ten_runs_beside_a_second_stream_give_the_first_runs_bits():
    name = "r2_26x22_c320"
    d = _inputs(name, BF)
    first = _both(d, name)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(10):
        with torch.cuda.stream(side):
            keep = [_both(d, name) for _ in range(3)]
        got = _both(d, name)
        assert all(torch.equal(a, b) for a, b in zip(first, got))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for k in keep for a, b in zip(first, k))


def test_patch_conv_function_passes_the_gradient_check():
    """x, weight and bias together, against the same fp64 references and bounds"""
    from tramba_amd import encoders, hip
    for name, dtype in (("r4_24x24", BF), ("r2_26x22_c320", HF)):
        d = _inputs(name, dtype)
        b, h, w, cin, cout, r = CASES[name]
        x = torch.nan_to_num(d["x"]).requires_grad_()                  # (autograd multiplies nothing by the trailing pixels)
        weight = d["wt"].float().requires_grad_()                      # an fp32 parameter holding 16-bit values
        bias = synth.synth_tensor(f"pcb_{name}.bias", (cout,)).to(DEV).requires_grad_()
        y = encoders._PatchConvFn.apply(x, weight, bias)
        assert torch.equal(y, hip.patch_conv_cl(x.detach(), d["wk"], bias.detach()))
        y.backward(d["gy"])
        assert x.grad.dtype == dtype and weight.grad.dtype == torch.float32 and weight.grad.shape == weight.shape
        _within(x.grad, d["ref"]["gx"], d["bound"]["gx"], f"_PatchConvFn gx {name}")
        _within(weight.grad.permute(0, 2, 3, 1), d["ref"]["gw"], d["bound"]["gw"], f"_PatchConvFn gw {name}")
        _within(bias.grad, d["ref"]["gb"], d["bound"]["gb"], f"_PatchConvFn gb {name}")
        # needs_input_grad skips either entry
        x2 = x.detach().requires_grad_()
        encoders._PatchConvFn.apply(x2, weight.detach(), bias.detach()).backward(d["gy"])
        assert torch.equal(x2.grad, x.grad)


# ----------------------------------------------------------------------------- blocks
def _counting(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapper)
    return calls


def _count_all(monkeypatch):
    from tramba_amd import encoders, hip
    return dict(linear=_counting(monkeypatch, F, "linear"), layer_norm=_counting(monkeypatch, F, "layer_norm"),
                conv=_counting(monkeypatch, encoders, "_conv"), sdpa=_counting(monkeypatch, F, "scaled_dot_product_attention"),
                fwd=_counting(monkeypatch, hip, "patch_conv_cl"), dgrad=_counting(monkeypatch, hip, "patch_conv_dgrad_cl"),
                wgrad=_counting(monkeypatch, hip, "patch_conv_wgrad_cl"))


def _parity_margins(kind):
    """profiles/enc_train_parity.json (scripts/measure_enc_train_parity.py, 16 seeds on an MI355X, the blocks of
    tests/golden/enc_train_blocks.py): per gradient tensor, m = (largest / smallest stock error) - 1 over the seeds -- the
    stock 16-bit path's own seed-to-seed spread is the yardstick, never the library path."""
    with open(os.path.join(ROOT, "profiles", "enc_train_parity.json")) as f:
        m = json.load(f)[kind]["m"]
    for name, v in m.items():
        assert 0.0 < v < 1.0, (name, v)
    return m


@pytest.mark.parametrize("kind", ["swin", "pvt"])
def test_block_gradients_keep_the_stock_error(kind):
    margins = _parity_margins(kind)
    for seed in range(8):
        errors = enc_train_blocks.block_errors(kind, seed)
        assert set(errors) == set(margins)
        for name, (lib, stock) in errors.items():
            print(f"{kind} seed {seed} {name}: library {lib:.3e} stock {stock:.3e}")
            assert lib <= stock * (1 + margins[name]), (kind, seed, name, lib, stock, margins[name])


def test_pvt_block_gradients_are_reproducible_with_the_switch_on_only():
    one, two = (enc_train_blocks.block_grads("pvt", 0, "library") for _ in range(2))
    assert all(torch.equal(one[k], two[k]) for k in one), [k for k in one if not torch.equal(one[k], two[k])]
    runs = [enc_train_blocks.block_grads("pvt", 0, "stock") for _ in range(4)]
    assert any(not torch.equal(runs[0][k], r[k]) for r in runs[1:] for k in r)      # the framework's sr backward


@pytest.mark.parametrize("kind", ["swin", "pvt"])
def test_switch_on_reaches_no_stock_op_and_each_new_entry_once(monkeypatch, kind):
    calls = _count_all(monkeypatch)
    grads = enc_train_blocks.block_grads(kind, 0, "library")
    assert not calls["linear"] and not calls["layer_norm"] and not calls["conv"] and not calls["sdpa"]
    want = 1 if kind == "pvt" else 0
    assert (len(calls["fwd"]), len(calls["dgrad"]), len(calls["wgrad"])) == (want, want, want)
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in grads.values())


@pytest.mark.parametrize("kind", ["swin", "pvt_sr1"])
def test_switch_off_is_the_never_switched_block_bit_for_bit(monkeypatch, kind):
    """(PVT: the sr 1 block, because two runs of the framework's sr backward need not agree with each other, see
    test_pvt_block_gradients_are_reproducible_with_the_switch_on_only)"""
    from tramba_amd import encoders
    from tramba_amd.encoders import _PvtBlock
    calls = _count_all(monkeypatch)
    lin_lib = _counting(monkeypatch, encoders._LinearTrainCL, "apply")

    def on_then_off(blk):
        assert encoders.set_library_training(blk, True) == encoders.set_library_training(blk, False) > 0
    if kind == "swin":
        never = enc_train_blocks.block_grads(kind, 0, "stock", prepare=lambda blk: None)     # the attribute was never set
        off = enc_train_blocks.block_grads(kind, 0, "stock", prepare=on_then_off)
    else:
        x = synth.synth_input("enc_train_off", (1, 576, 128)).to(DEV).bfloat16()
        dy = synth.synth_input("enc_train_off_dy", (1, 576, 128)).to(DEV).bfloat16()

        def run(prepare):
            blk = enc_train_blocks.seeded(_PvtBlock(128, 2, 4, True, 0.0, 1, 1e-6), 0).train()
            prepare(blk)
            inp = x.detach().requires_grad_()
            blk(inp, 24, 24).backward(dy)
            return dict([("x", inp.grad)] + [(k, p.grad) for k, p in blk.named_parameters()])
        never, off = run(lambda blk: None), run(on_then_off)
    assert all(torch.equal(never[k], off[k]) for k in never), [k for k in never if not torch.equal(never[k], off[k])]
    assert not calls["dgrad"] and not calls["wgrad"] and not calls["fwd"] and not lin_lib and calls["linear"]


def test_fp32_and_576_keys_keep_the_stock_ops(monkeypatch):
    from tramba_amd import encoders, hip
    from tramba_amd.encoders import _PvtBlock
    calls = _count_all(monkeypatch)
    kv_bwd = _counting(monkeypatch, hip, "kv_attention_bwd_cl")
    lin_lib = _counting(monkeypatch, encoders._LinearTrainCL, "apply")
    ln_lib = _counting(monkeypatch, encoders._LayerNormCL, "apply")
    x = synth.synth_input("enc_train_stock", (1, 576, 128)).to(DEV)
    dy = synth.synth_input("enc_train_stock_dy", (1, 576, 128)).to(DEV)

    def run(blk, inp):
        blk.zero_grad(set_to_none=True)
        inp = inp.detach().requires_grad_()
        blk(inp, 24, 24).backward(dy.to(inp.dtype))
        return [inp.grad] + [p.grad for p in blk.parameters()]
    # fp32 activations: the stock ops, switch on or off, bit for bit (sr 1: no framework convolution backward in the way)
    blk = enc_train_blocks.seeded(_PvtBlock(128, 2, 4, True, 0.0, 1, 1e-6), 0).train()
    stock = run(blk, x)
    n = {k: len(v) for k, v in calls.items()}
    assert n["linear"] > 0 and n["layer_norm"] > 0 and n["sdpa"] == 1 and n["conv"] == 1       # (conv: the depth-wise 3x3)
    assert encoders.set_library_training(blk) > 0
    again = run(blk, x)
    assert all(torch.equal(a, b) for a, b in zip(stock, again))
    assert {k: len(v) for k, v in calls.items()} == {k: 2 * v for k, v in n.items()} and not lin_lib and not ln_lib
    # 576 keys in bf16 (sr 1 on 24 x 24): stock SDPA for the attention only, the Linears and LayerNorms move
    for v in calls.values():
        del v[:]
    got = run(blk, x.bfloat16())
    assert len(calls["sdpa"]) == 1 and not kv_bwd
    assert not calls["linear"] and not calls["layer_norm"] and not calls["conv"] and lin_lib and ln_lib
    assert all(torch.isfinite(g).all() for g in got)


# ----------------------------------------------------------------------------- whole model
def _train_model(name, library, frozen=False, drop_path=True):
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
    if not drop_path:
        for mod in m.modules():
            if isinstance(mod, ta.DropPath):
                mod.drop_prob = 0.0
    on, off = encoders.set_library_training(m, True), encoders.set_library_training(m, library)
    assert on == off > 0
    return m


def _batch():
    x = synth.synth_input("enc_train_whole", (1, 3, 384, 384)).to(DEV)
    y = (synth.synth_input("enc_train_whole_y", (1, 1, 384, 384)).to(DEV) > 0).float()
    return x, y


@functools.lru_cache(maxsize=None)
def _stock_grad_names(name):
    from tramba_amd import train
    m = _train_model(name, library=False)
    train.train_step(m, train.get_opt(1e-4, m), *_batch())
    return frozenset(k for k, p in m.named_parameters() if p.grad is not None)


@pytest.mark.parametrize("name,count", [("Tramba-S-TSOD", 0), ("Tramba-P-TSOD", 38)])
def test_whole_model_train_step_on_the_library(monkeypatch, name, count):
    from tramba_amd import encoders, hip, train
    x, y = _batch()
    have = _stock_grad_names(name)
    assert have

    def forbidden(*a, **k):
        raise AssertionError("encoders._conv reached with the library training switch on")
    real_linear, real_ln = F.linear, F.layer_norm
    from_encoders = []

    def watch(real, what):
        import sys

        def wrapper(*a, **k):
            if sys._getframe(1).f_code.co_filename == encoders.__file__:
                from_encoders.append(what)
            return real(*a, **k)
        return wrapper
    monkeypatch.setattr(encoders, "_conv", forbidden)
    monkeypatch.setattr(F, "linear", watch(real_linear, "linear"))
    monkeypatch.setattr(F, "layer_norm", watch(real_ln, "layer_norm"))
    monkeypatch.setattr(F, "scaled_dot_product_attention", watch(F.scaled_dot_product_attention, "sdpa"))
    fwd = _counting(monkeypatch, hip, "patch_conv_cl")
    dgrad = _counting(monkeypatch, hip, "patch_conv_dgrad_cl")
    wgrad = _counting(monkeypatch, hip, "patch_conv_wgrad_cl")
    m = _train_model(name, library=True)
    loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
    assert torch.isfinite(loss).all()
    assert not from_encoders
    assert (len(fwd), len(dgrad), len(wgrad)) == (count, count, count)
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert have <= got
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    # a frozen encoder: no gradient for any weight that freeze_encoder() froze, and the step still runs
    del m, fwd[:], dgrad[:], wgrad[:]
    m = _train_model(name, library=True, frozen=True)
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert frozen and all(k.startswith("encoder.") for k in frozen)
    loss = train.train_step(m, train.get_opt(1e-4, m), x, y)
    assert torch.isfinite(loss).all() and not from_encoders
    assert all(p.grad is None for k, p in m.named_parameters() if not p.requires_grad)
    assert len(fwd) == count and not wgrad                              # no weight gradient of a frozen sr conv


@pytest.mark.parametrize("name", ["Tramba-P-TSOD", "Tramba-S-TSOD"])
def test_graphed_train_step_follows_the_eager_step(name):
    """the yardsticks of tests/test_gpu_e2e.py's test of the same name, on Tramba-P / -S with the switch on"""
    import tramba_amd as ta
    from tramba_amd import train
    x, y = _batch()
    m = _train_model(name, library=True, drop_path=False)
    opt = train.get_opt(1e-4, m)
    eager = [float(train.train_step(m, opt, x, y)) for _ in range(6)]
    del m, opt
    m = _train_model(name, library=True, drop_path=False)
    step = ta.GraphedTrainStep(m, train.get_opt(1e-4, m, capturable=True))
    probe = next(p for n, p in m.named_parameters() if n.startswith("encoder.") and n.endswith("weight") and p.ndim == 2)
    start = probe.detach().clone()
    got = [float(step(x, y))]                # eager warm-up steps (undone), capture, replay: exactly step 1
    after_one = probe.detach().clone()
    assert not torch.equal(start, after_one)
    got += [float(step(x, y)) for _ in range(5)]
    assert not torch.equal(after_one, probe)                           # the replay really updates the weights
    print(f"{name}: graphed {got} eager {eager}")
    assert got[0] == pytest.approx(eager[0], rel=1e-5)                 # same initial weights, same batch: same first loss
    assert np.allclose(got, eager, rtol=3e-2), (got, eager)
    assert len(step._graphs) == 1
