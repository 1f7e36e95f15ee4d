"""CPU side of the pointwise probes (tests/golden/pointwise_cases.py): E32 -- what a numpy float32 evaluation of each DOCUMENTED
formula loses against fp64 over the SWEEP, in the measure e = |got - want| / max(1, |want|) -- is measured and every emulation
shown finite over the whole sweep (the documented formulas have no tail defect); faults injected into the emulations (never
into a kernel) are shown to exceed 8 x E32 or to turn non-finite; the 16-bit subsets of the sweep still reach past every
switch-over; and every probe builder is shown, against the fp64 oracle, to put each sweep value where
tests/test_gpu_pointwise.py reads it.  profiles/pointwise_parity.json (scripts/measure_pointwise_parity.py) records the same
host numbers beside the GPU records; this file checks that the committed copy still says what it computes."""
import json
import math
import os

import numpy as np
import pytest
import torch

import pointwise_cases as pc

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_holds_every_switch_over_point():
    s = set(pc.SWEEP.tolist())
    f = lambda v: float(np.float32(v))
    for a in (2.0 ** -30, 1e-6, 1e-3, 0.5, 1, 2, 3, 5, 8, 10, 13.86, 15, 16.6, 17.4, 19.99, 25, 30, 41.6, 60, 87, 88.7, 88.8, 89, 100,
              103.9, 104, 200, 1e4):
        assert f(a) in s and f(-a) in s, a
    for v in (0.0, 20.0, float(np.nextafter(np.float32(20), np.float32(np.inf))), float(np.nextafter(np.float32(60), np.float32(np.inf)))):
        assert v in s, v
    rnd = pc.SWEEP[-256:]
    assert len(pc.SWEEP) == 316 and float(np.abs(rnd).max()) <= 110 and len(set(rnd.tolist())) == 256
    assert bool(np.isfinite(pc.SWEEP).all())
    assert np.array_equal(pc.SWEEP, pc._sweep())                       # seeded


@pytest.mark.parametrize("dtype,sub", [(BF16, pc.SWEEP_BF16), (F16, pc.SWEEP_F16)], ids=["bf16", "f16"])
def test_16_bit_subsets_reach_past_every_switch_over(dtype, sub):
    """operands that have to be 16-bit (the residual of GELU_GRAD_MUL, logits_to_u8's 16-bit logits) still see a point beyond
    where 1 + exp(x) rounds to 1 (+-16.6), the softplus threshold 20, the clamp 60 and the overflow of exp (+-88.7)"""
    t = torch.from_numpy(sub)
    assert torch.equal(t.to(dtype).float(), t) and set(sub.tolist()) <= set(pc.SWEEP.tolist())
    v = sub.astype(np.float64)
    assert (v > 16.6).any() and (v < -16.6).any()
    assert ((v > 20) & (v < 60)).any() and (v == 20).any()
    assert ((v > 60) & (v < 88.7)).any()
    assert (v > 88.7).any() and (v < -88.7).any()
    assert (np.abs(v) <= 5).sum() >= 9 and (v == 0).any()


def test_documented_formulas_are_finite_and_e32_is_fp32_level():
    """E32_F = max(max over SWEEP of e(emulation, fp64), 2^-24); every emulation finite over the whole sweep.  All of them sit
    between 2^-24 and 2^-20: an fp32 evaluation of the documented formula IS an fp32-level evaluation of the function, tails
    included (the largest, silu' = s (1 + x (1 - s)), loses 16 ulp to 1 - s at x = 16.6)."""
    table = pc.e32_table()
    for name, (e, x, finite) in table.items():
        print(f"E32 {name}: {e:.3e} at x = {x:.6g}")
        assert finite, name
        assert pc.FLOOR <= e <= 2.0 ** -20, (name, e, x)
    assert set(table) == set(pc.FORMULAS) | set(pc.FORMULAS2) | {"softmax"}


def test_reference_softplus_and_the_three_forms_differ_below_fp32_resolution():
    """the reference switches to x above 20; softplus_lean max-es with x and clamps the exponent at 60; the fused form takes the
    median with x' and 128.  In fp64 log1p(exp(x)) - x = 2e-9 at x = 20: the switch is invisible in fp32, all three agree with
    the threshold form to E32 on the whole sweep, including nextafter(20) and nextafter(60)"""
    want = pc.ref_softplus(pc.SWEEP)
    exact = torch.where(torch.from_numpy(pc.SWEEP).double() > 30, torch.from_numpy(pc.SWEEP).double(),
                        torch.log1p(torch.exp(torch.from_numpy(pc.SWEEP).double().clamp(max=30))))
    assert float(pc.err(exact, want).max()) < 2.0 ** -28
    for f in (pc.emu_softplus20, pc.emu_softplus_lean, pc.emu_softplus_med3):
        assert float(pc.err(torch.from_numpy(f(pc.SWEEP)), want).max()) <= 2.0 ** -22


def test_every_injected_fault_is_caught():
    """each fault in the emulation only: beyond 8 x E32 of its formula at some sweep point, or non-finite there; the factor is
    recorded (profiles/pointwise_parity.json)"""
    faults = pc.fault_table()
    assert len(faults) == 6
    for name, f in faults.items():
        print(f"{name}: error {f['error']} at x = {f['worst_x']:.6g}, {f['factor']} x the bound, non-finite: {f['nonfinite']}")
        assert f["nonfinite"] or f["factor"] is None or f["factor"] > 1.0, name
        assert f["nonfinite"] == (f["error"] is None)
    assert 100 < faults["tanh-GELU for erf-GELU"]["factor"] < 1e4 and not faults["tanh-GELU for erf-GELU"]["nonfinite"]
    for name in ("softplus = log(1 + exp(x)), no large-x guard", "sigmoid = exp(x) / (1 + exp(x))", "BCE = -log(sigmoid)",
                 "softmax without the row maximum"):
        assert faults[name]["nonfinite"], name
    assert faults["fp16 store clamped to 65504"]["error"] == 6          # +-65520, +-65536, +-7e4 come out finite


def test_check_rule_has_teeth():
    """the rule of the GPU file on CPU values: the emulation passes, the tanh-GELU fails as an fp32 output AND as a bf16 one
    below |x| = 3 (u |want| is 1e-2 |want| there, the fault 4.7e-4 absolute on |want| ~ 1e-3), an inf fails, an inf where the
    reference itself overflows the output dtype is skipped"""
    xs = torch.from_numpy(pc.SWEEP)
    want = pc.ref_gelu(xs)
    assert pc.check(torch.from_numpy(pc.emu_gelu(pc.SWEEP)), want, xs, "gelu")["ok"]
    bad = pc.check(torch.from_numpy(pc.fault_gelu_tanh(pc.SWEEP)), want, xs, "gelu")
    assert not bad["ok"] and bad["error"] > 100 * bad["bound"]
    assert not pc.check(torch.from_numpy(pc.fault_gelu_tanh(pc.SWEEP)).to(BF16), want, xs, "gelu", BF16)["ok"]
    assert pc.check(torch.from_numpy(pc.emu_gelu(pc.SWEEP)).to(BF16), want, xs, "gelu", BF16)["ok"]
    got = torch.from_numpy(pc.emu_gelu(pc.SWEEP)).clone()
    got[5] = float("inf")
    r = pc.check(got, want, xs, "gelu")
    assert not r["ok"] and not r["finite"]
    big = torch.tensor([7e4], dtype=torch.float64)
    assert pc.check(torch.tensor([float("inf")]), big, big, "identity", F16)["ok"]
    assert not pc.check(torch.tensor([float("inf")]), big, big, "identity", F32)["ok"]


# ----------------------------------------------------------------------------- placement of the probes
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,l,all_states", [(1, 37, False), (4, 40, False), (3, 37, True), (16, 40, True), (16, 37, False)])
def test_scan_probe_places_the_sweep(n, l, all_states, dtype):
    """the fp64 oracle on the probe's operands: out[r, t >= s_r] = N' softplus(x_r), 0 before; ddelta[r, s_r] = N' softplus'(x_r),
    0 elsewhere; du[r, s_r] = N' softplus(x_r); dbias = ddelta's row sum; dA = 0, dD = 1; every sweep value owns a row"""
    o = pc.scan_probe(n, l, dtype, all_states=all_states)
    assert set(o.xs.tolist()) == set(pc.SWEEP.tolist()) and o.kd >= len(pc.SWEEP)
    if dtype != F32:
        assert torch.equal(o.delta.float().to(dtype), o.delta)
    out, (du, ddelta, dA, dB, dC, dD, dbias) = pc.scan_probe_oracle(o)
    ex = pc.scan_probe_expected(o)
    rows, t = torch.arange(o.kd), torch.arange(l)[None]
    after = t >= o.pos[:, None]
    tol = lambda w: 1e-12 * w.abs().clamp_min(1.0)
    assert bool(((out[0] - torch.where(after, ex["out"][:, None], torch.zeros(()).double())).abs() <= tol(ex["out"])[:, None]).all())
    at = t == o.pos[:, None]
    assert bool(((ddelta[0] - torch.where(at, ex["ddelta"][:, None], torch.zeros(()).double())).abs() <= 1e-12).all())
    assert bool(((du[0, rows, o.pos] - ex["du"]).abs() <= tol(ex["du"])).all())
    assert bool(((dbias - ex["ddelta"]).abs() <= 1e-12).all())
    assert float(dA.abs().max()) == 0.0 and bool((dD == 1).all())
    ns = n if all_states else 1
    grp = rows // o.dper
    assert bool(((dB[0, grp, 0, o.pos] - ex["du"] / ns).abs() <= tol(ex["du"])).all())       # one row per (group, position)
    assert bool(((dC[0, grp, 0, o.pos] - ex["out"] / ns).abs() <= tol(ex["out"])).all())
    assert len(set(zip(grp.tolist(), o.pos.tolist()))) == o.kd


def test_scan_probe_without_softplus_stays_within_100():
    o = pc.scan_probe(4, 37, BF16, softplus=False)
    assert float(o.xs.abs().max()) <= 100 and float(o.xs.abs().max()) > 89
    out, grads = pc.scan_probe_oracle(o)
    rows = torch.arange(o.kd)
    assert torch.equal(out[0, rows, o.pos], o.xs.double()) and torch.equal(grads[1][0, rows, o.pos], torch.ones(o.kd).double())


@pytest.mark.parametrize("act", pc.GEMM_ACTS)
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
def test_gemm_probe_places_the_sweep(dtype, act):
    """a plain fp64 GEMM + epilogue on the probe's operands gives act(sweep value) in every column (every element for
    gelu'(residual)), and every value of the sweep (of the dtype's subset for the residual) is there"""
    for m, n, k in list(pc.GEMM_SHAPES.values()) + [(100, 520, 72), (100, 520, 50)]:
        o = pc.gemm_probe(m, n, k, dtype, act)
        got = pc.gemm_probe_cpu(o)
        want = pc.act_reference(act, o.xs)
        assert bool(((got - want).abs() <= 1e-15 * want.abs().clamp_min(1.0)).all())
        vals = pc.sweep_for(dtype) if act == pc.ACT_GELU_GRAD_MUL else pc.SWEEP
        assert set(o.xs.reshape(-1).tolist()) == set(vals.tolist())
        assert bool(torch.isfinite(o.w.float()).all()) and float(o.x.float().abs().max()) == 0.0


def test_norm_and_stencil_probes_place_the_sweep():
    for c in (64, 200):
        pieces = pc.chunks(c)
        assert set(torch.cat(pieces).tolist()) == set(pc.SWEEP.tolist()) and all(p.numel() == c for p in pieces)
        x, w, b = pc.norm_probe(5, c, BF16, pieces[0])
        y = torch.nn.functional.layer_norm(x.double(), (c,), w.double(), b.double())
        assert torch.equal(y, b.double()[None].expand(5, c))
    for dtype in (F32, BF16, F16):
        for ks in (3, 7):
            o = pc.dw_probe(dtype, ks)
            pre = torch.nn.functional.conv2d(o.x.double().permute(0, 3, 1, 2), o.wt.double().t().reshape(pc.DW_C, 1, ks, ks),
                                             o.bt.double(), padding=ks // 2, groups=pc.DW_C).permute(0, 2, 3, 1)
            assert torch.equal(pre, o.xs.double()) and set(o.xs.reshape(-1).tolist()) == set(pc.SWEEP.tolist())
            assert o.x.dtype == dtype


@pytest.mark.parametrize("mode", ["bias", "mfma"])
@pytest.mark.parametrize("fam", ["raster", "helix"])
def test_fused_scan_probe_places_the_sweep(fam, mode):
    """the fp64 reference of scan_memory_cases on the probe: ys = softplus(x_kc) x (visits so far), graw = softplus'(x_kc) x
    (visits from there on) at a visit and 0 elsewhere, gbias its sum; a raster direction passes every position once; over the
    pieces every sweep value (|x log2e| <= 1e4 where the MFMA forms x') is placed; what the MFMA reads is a bf16 value to an fp32 ulp"""
    import scan_memory_cases as smc
    kd = (4 if fam == "raster" else 8) * pc.SS2D_D
    seen = set()
    pieces = pc.ss2d_values(mode, kd)
    for i, values in enumerate(pieces):
        seen |= set(values.tolist())
        if i:
            continue                                     # (the operands differ only in the values: one piece through the oracle)
        for dtype, dma in ((BF16, False), (F16, True), (F32, False)):       # (dma: the 32 x 32 map of the LDS-DMA test)
            c = pc.ss2d_probe(fam, dtype, mode, values, form_dma=dma, h=pc.SS2D_H_DMA if dma else pc.SS2D_H)
            assert pc.ss2d_dma_runs(c.l, c.d, c.r, c.k, dtype) == dma
            ex = pc.ss2d_expected(c)
            ref = smc.reference(c)
            ref.update(smc.reference_bwd(c))
            for name in ("ys", "graw", "gbias"):
                assert float((ref[name] - ex[name]).abs().max()) <= 1e-12 * max(1.0, float(ex[name].abs().max())), name
            if fam == "raster":
                assert bool((c.visits.sum(1) == 1).all())
            rel = (c.xs - values.reshape(c.k, c.d)).abs() / values.reshape(c.k, c.d).abs().clamp_min(1e-30)
            assert float(rel.max()) <= (2.0 ** -8 if mode == "mfma" else 2.0 ** -15 if dma else 0.0)
            if mode == "mfma":
                w2 = c.dt_w * smc.LOG2E_F
                assert bool(((w2.to(BF16).float() - w2).abs() <= 2.0 ** -23 * w2.abs()).all()) and float(w2.abs().max()) <= pc.SS2D_MFMA_MAX
    want = set(pc.SWEEP.tolist()) if mode == "bias" else {v for v in pc.SWEEP.tolist() if abs(v) * pc.LOG2E <= pc.SS2D_MFMA_MAX}
    assert seen == want and (mode == "bias" or 1e4 not in seen)


@pytest.mark.parametrize("resized", [False, True])
@pytest.mark.parametrize("label", ["zeros", "ones", "checker"])
def test_loss_probe_and_reference(label, resized):
    """logits = the sweep tiled; the fp64 reference is finite, its closed-form gradient equals autograd (asserted inside), and
    the BCE term equals torch's own binary_cross_entropy_with_logits"""
    z, y = pc.loss_probe(label, resized)
    assert set(z.reshape(-1).tolist()) == set(pc.SWEEP[:z.numel()].tolist()) and (resized or z.numel() >= len(pc.SWEEP))
    loss, grad = pc.loss_reference(z, y)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all()) and grad.shape == z.shape
    zz = torch.nn.functional.interpolate(z.double(), y.shape[-2:], mode="bilinear") if resized else z.double()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(zz, y.double(), reduction="none")
    assert float((pc.ref_bce(zz, y) - bce).abs().max()) <= 1e-12 * float(bce.max())
    w = 1 + 5 * torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(1))
    for eps in (0.0, 0.1):
        for iou in (True, False):
            for pixel in (False, True):
                lw, gw = pc.loss_reference(z, y, w, eps, iou, pixel)
                assert math.isfinite(float(lw)) and bool(torch.isfinite(gw).all())


def test_range_probe():
    a, b, want = pc.range_probe()
    sums = a.double() + b.double()
    assert sorted(set(sums.abs().tolist())) == sorted(pc.RANGE_SUMS)
    assert want.tolist()[:6] == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, -65504.0]
    assert bool(torch.isinf(want[6:]).all()) and torch.equal(torch.sign(want), torch.sign(sums).to(F16))
    assert torch.equal((a.float() + b.float()).double(), sums)             # exact in the fp32 accumulator


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_attention_probes_span_300(dtype):
    """scaled scores on the fp64 reference reach beyond +-300; rows with one dominant key (P one-hot to 1e-30: a masked dominant key at 624 against 543), rows with all
    scores equal (P uniform over the keys of the row's region), the -100 mask present with shift 6; everything finite"""
    for shift in (0, 6):
        o = pc.window_attn_probe(dtype, shift)
        out, s = pc.window_attn_reference(o)
        lo, hi = pc.score_span(s)
        assert lo <= -pc.ATTN_SPAN and hi >= pc.ATTN_SPAN and bool(torch.isfinite(out).all())
        p = torch.softmax(s, -1)
        top = p.max(-1).values
        assert int((top == 1).sum()) > 500 and int((top < 0.03).sum()) > 500
        assert bool(((p == 0) | (p > 1e-3) | (p < 1e-30)).all())           # nothing in between: P is exact in any precision
        if shift:
            assert float(pc.shift_mask(24, 24, 12, shift).min()) == -100.0
        g = pc.attn_grads(pc.window_attn_reference, o, ("qkv",))["qkv"]
        assert bool(torch.isfinite(g).all())
    o = pc.kv_attn_probe(dtype)
    out, s = pc.kv_attn_reference(o)
    lo, hi = pc.score_span(s)
    assert lo <= -pc.ATTN_SPAN and hi >= pc.ATTN_SPAN and bool(torch.isfinite(out).all())
    p = torch.softmax(s, -1)
    assert bool(((p == 0) | (p > 1e-3) | (p < 1e-30)).all())


def test_shift_mask_is_the_blocks_own():
    from tramba_amd.encoders import SwinTransformerBlock
    blk = SwinTransformerBlock(128, (24, 24), 4, 12, 6, 1.0, 0.0)
    assert torch.equal(blk.attn_mask.double(), pc.shift_mask(24, 24, 12, 6))


def test_u8_reference_and_emulation_agree_on_the_sweep():
    """uint8(sigmoid * 255): torch's fp32 CPU sigmoid and the numpy restatement of the kernel's expression"""
    assert np.array_equal(pc.ref_u8(pc.SWEEP).numpy(), pc.emu_u8(pc.SWEEP))
    assert set(pc.ref_u8(pc.SWEEP).tolist()) >= {0, 127, 255}


# ----------------------------------------------------------------------------- the committed profile
def test_committed_profile_records_these_numbers():
    """profiles/pointwise_parity.json: the host section is what this machine computes (E32 within 2 x: numpy's float32 exp / log
    differ by an ulp between SIMD builds), every GPU record is within its bound, and every forced GEMM form is there with
    GELU checked into an fp32 output"""
    with open(os.path.join(ROOT, "profiles", "pointwise_parity.json")) as f:
        prof = json.load(f)
    mine = pc.host_profile()
    assert set(prof["host"]["e32"]) == set(mine["e32"]) and set(prof["host"]["faults"]) == set(mine["faults"])
    for name, v in mine["e32"].items():
        assert 0.5 <= prof["host"]["e32"][name]["e32"] / v["e32"] <= 2.0, name
    recs = prof["records"]                                 # the worst case per kernel, form, function and output width
    assert prof["cases"] >= len(recs)
    assert recs and all(r["ok"] for r in recs) and prof["all_within_bounds"]
    gelu32 = {r["form"].split(" M=")[0] for r in recs if r["kernel"] == "linear_cl" and r["function"] == "gelu" and r["bound"] < 1e-5}
    assert {"DMA4", "DMA2", "DMA3", "PC3", "PC4", "rule-no-PC/WS"} <= gelu32
    assert any(r["form"].startswith("WS") and r["function"] == "gelu" for r in recs)
    kernels = {r["kernel"] for r in recs}
    assert {"selective_scan_fwd", "selective_scan_bwd", "ss2d_scan_cl", "ss2d_scan_bwd_cl", "linear_cl", "linear_dual_cl", "linear2_cl",
            "layernorm_cl", "add_layernorm_cl", "ss2d_merge_norm_cl", "dwconv_cl", "dwconv_dual_cl", "sod_loss", "sod_loss_grad",
            "sod_wloss", "sod_wloss_grad", "window_attention_cl", "window_attention_bwd_cl", "kv_attention_cl", "kv_attention_bwd_cl",
            "logits_to_u8"} <= kernels
