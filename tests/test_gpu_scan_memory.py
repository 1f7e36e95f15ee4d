"""The scans that carry a recurrence state across tile and workgroup-step boundaries, where that state OUTLIVES many tiles:
every schedule against an independent fp64 reference in the regimes of tests/golden/scan_memory_cases.py (`slow`: memory of 70
.. 1600 positions; `undamped`: A = 0, a cumulative sum; `init`: the model's own initialisation, dt 1e-3 .. 1e-1, A = -1).

Bounds (tests/test_scan_memory_host.py measures them and shows a wrong hand-over exceeds them >= 100-fold): an fp32 output must
stay within 8 x E32 of the fp64 reference, E32 being what a plain fp32 evaluation of the same formulas loses on the same case
-- about 1e-6 of the largest output for ys (0.8e-6 .. 2e-6 on 16-bit pre-rounded inputs, 2e-6 .. 3.7e-6 on fp32 inputs with
their split-bf16 dt_proj), so bounds of 0.6e-5 .. 3e-5; up to 1e-5 for the gradients of `init`.  A 16-bit output must have
EVERY element within u |want| + (that fp32 bound) max |want|, u = 2^-8 (bf16) / 2^-11 (fp16).  Gradients are held to the same
rule on the max-relative and the RMS-relative measure; gA alone gets 2.5 x 8 x E32 (an error of the per-position decay enters
it twice, through h and through the adjoint, and the hardware exp2 is within an ulp but not correctly rounded: measured 9 x E32
on the slowest channel of one case where ys shows 3.6 x; scan_memory_cases.FACTOR_FOR and the host test beside it).
profiles/scan_memory_parity.json has E32, bound and measured error per case, output and regime
(scripts/measure_scan_memory_parity.py).

No test here withholds a hand-over or provokes a time-out: faults are injected into the CPU emulation only."""
import pytest
import torch

import scan_memory_cases as smc

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
RING, SEGMENT, LDS_DMA = 1, 2, 3        # TRAMBA_TUNE_SCAN_FORM


def hip():
    from tramba_amd import hip as h
    return h


def _dev():
    return torch.device("cuda")


def _hold(recs):
    for r in recs:
        print({k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in r.items()})
    for r in recs:
        assert r["ok"], r


def _ys_dtypes(dtype):
    return (F32,) if dtype == F32 else (F32, dtype)


def _forward(name, regime, dtype, form, a_log=False, ws=(0,)):
    H = hip()
    c, ref, e = smc.fwd_e32(name, regime, dtype, a_log, segment=form == SEGMENT)
    recs = []
    for w in ws:
        for ys_dtype in _ys_dtypes(dtype):
            ys = smc.run_scan(H, c, _dev(), form, ys_dtype, w)
            assert bool(torch.isfinite(ys.float()).all())
            recs.append(smc.record(f"fwd {name} {regime} form={form} W={w}", "ys", ys, ref["ys"], e["ys"], ys_dtype))
    _hold(recs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("regime", ["slow", "undamped", "init"])
def test_ring_form_across_super_chunks(regime, dtype):
    """Rows 1 and 2: register-ring chained form, raster 37 x 37 (L = 1369 = 42 tiles + 25 positions), D = 64, dt_rank 4, batch 1:
    8 sequences -> the library's W = 8 (5.4 super-chunks of 8 tiles, ragged end), and W forced to 1, 2, 4 (43 / 21.5 / 10.75
    steps; wave 0 takes its carry from wave W - 1 of the step before).  ys in fp32 and in the input dtype.  `init` passes
    A_logs (a_log)."""
    _forward("raster37", regime, dtype, RING, a_log=regime == "init", ws=(0, 1, 2, 4) if regime != "init" else (0,))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("regime", ["slow", "undamped", "init"])
def test_segment_form_folds_fifteen_segments(regime, dtype):
    """Row 3: two-pass wave-segment form on the case of row 1: 8 row-tiles -> seg_plan gives NT = 3 tiles per segment, NSEG =
    15; the state entering segment j is the fold of j aggregates.  (The form takes A, not A_logs: `init` passes A = -1.)"""
    _forward("raster37", regime, dtype, SEGMENT)


@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_segment_form_long_segments(regime):
    """Row 4: helix 37 x 37, D = 2048, dt_rank 64 (NK = 4 MFMA steps), batch 2: 2 * 8 * 64 = 1024 row-tiles -> NT = 12, NSEG = 4
    (the last segment holds 7 tiles)."""
    _forward("helix37_wide", regime, BF16, SEGMENT)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("r", [8, 16, 32])
@pytest.mark.parametrize("regime", ["slow", "undamped", "init"])
def test_lds_dma_form_sixteen_waves(regime, r, dtype):
    """Row 5: chained form on LDS-DMA staged operands, helix 40 x 40 (L = 1600 = 50 tiles = 3.125 super-chunks of 16), D = 64,
    batch 1: 16 sequences -> wdma = 16; padded dt_rank R8 = 8 (the bias rides in the MFMA), 16, 32 (two MFMA steps)."""
    _forward(f"helix40_r{r}", regime, dtype, LDS_DMA, a_log=regime == "init")


@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_lds_dma_form_eight_waves(regime):
    """Row 6: helix 37 x 37, D = 576, dt_rank 8, batch 2: 2 * 8 * 18 = 288 sequences -> wdma = 8 (288 * 16 > 4096 wave slots),
    5.35 super-chunks of 8 tiles, ragged end."""
    _forward("helix37_d576", regime, BF16, LDS_DMA)


@pytest.mark.parametrize("name,dtype,form", [("raster37", F32, RING), ("raster37", BF16, RING), ("helix40_r8", BF16, LDS_DMA),
                                             ("helix40_r8", F16, LDS_DMA), ("helix40_r32", BF16, LDS_DMA)],
                         ids=["ring-f32", "ring-bf16", "dma-bf16", "dma-f16", "dma-r32-bf16"])
@pytest.mark.parametrize("regime", ["slow", "undamped", "init"])
def test_saved_states_are_the_states_entering_every_tile(regime, name, dtype, form):
    """Row 7: ss2d_scan_cl(states=...) on cases 1 and 5, ys in the input dtype, the buffer prefilled with NaN: every saved state
    (fp32) within 8 x E32 of the fp64 state entering that tile -- a state saved one tile off is wrong by 0.4 of the largest --
    and ys bit-equal to the plain launch of the same form."""
    H = hip()
    c, ref, e = smc.fwd_e32(name, regime, dtype, regime == "init")
    ys, states = smc.run_scan(H, c, _dev(), form, dtype, states=True)
    plain = smc.run_scan(H, c, _dev(), form, dtype)
    assert bool(torch.isfinite(states).all())
    assert torch.equal(ys, plain)
    _hold([smc.record(f"states {name} {regime} form={form}", "states", states, ref["states"], e["states"]),
           smc.record(f"states {name} {regime} form={form}", "ys", ys, ref["ys"], e["ys"], dtype)])


@pytest.mark.parametrize("name,dtype", [("raster37", F32), ("raster37", BF16), ("helix40_r8", BF16)], ids=["raster-f32", "raster-bf16", "helix40"])
def test_library_choice_is_the_ring_form(name, dtype):
    """Knob 0 on cases 1 and 5: 8 and 16 sequences fill neither the LDS-DMA rule (>= 2048 waves) nor the wave-segment rule (>=
    128 tiles), so the library runs the register ring at W = 8: bit-equal to the forced form."""
    H = hip()
    c = smc.fused_case("fwd", name, "slow", dtype)
    for ys_dtype in _ys_dtypes(dtype):
        assert torch.equal(smc.run_scan(H, c, _dev(), 0, ys_dtype), smc.run_scan(H, c, _dev(), RING, ys_dtype))


@pytest.mark.parametrize("a_log", [False, True], ids=["A", "A_logs"])
@pytest.mark.parametrize("name,dtype", [("raster37", F32), ("raster37", BF16), ("helix40_d96", BF16), ("helix40_d96", F16),
                                        ("helix37_d576", BF16)], ids=["raster-f32", "raster-bf16", "helix40-bf16", "helix40-f16", "d576-bf16"])
@pytest.mark.parametrize("regime", ["slow", "init"])
def test_backward_chains_across_super_chunks(regime, name, dtype, a_log):
    """ss2d_scan_bwd_cl, forward and reverse chain: raster 37 x 37 D = 64 r 4 batch 1 (8 sequences, W = 8, 5.4 super-chunks,
    ragged); helix 40 x 40 D = 96 r 8 batch 2 (48 sequences, W = 8, 6.25 super-chunks); helix 37 x 37 D = 576 r 8 batch 2 (288
    sequences -> W = 4, 10.75 super-chunks).  With the states the forward launch saved and with the sweep that recomputes them,
    A and A_logs, dB / dC as per-channel-tile partials summed here.  Every output -- gu, graw (activation dtype), gB, gC, gA (or
    gA_logs), gD, gbias (fp32) -- against oracle.selective_scan.selective_scan_bwd on the gathered operands.  Bounds: 8 x E32 per
    output and measure (E32 0.5e-6 .. 1.6e-6 in `slow`, 2.4e-6 .. 1e-5 in `init`), 20 x E32 for gA (module docstring)."""
    _hold(smc.bwd_records(hip(), _dev(), name, regime, dtype, a_log))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_boundary_op_across_chunk_checkpoints(regime, n, dtype):
    """selective_scan_fwd / _bwd, rows = 2 x 4 x 8, d_state 1 and 4, L = 1561 (fp32, scalar accesses) / 1600 (bf16, 16-byte
    accesses): 4 chunks of 512 positions, the last ragged.  `undamped` is the closed form (a cumulative sum) for the backward that
    only the forward had.  All seven gradients and the output against oracle.selective_scan; the forward also against the
    oracle's fp32-arithmetic form."""
    _hold(smc.boundary_records(hip(), _dev(), regime, n, dtype))
