"""CPU side of the long-memory scan tests (tests/golden/scan_memory_cases.py): the fp64 reference loop is pinned to the oracle
the rest of the suite trusts, E32 -- what a plain fp32 evaluation of the same formulas loses against fp64 -- is measured for
every GPU case of tests/test_gpu_scan_memory.py, and faults injected into the tile-wise fp32 emulation (never into a kernel)
show that the bounds of that file, FACTOR * E32, separate a right hand-over from a wrong one by at least 100x."""
import pytest
import torch

import scan_memory_cases as smc
from oracle import selective_scan as oss

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _oracle_ys(c):
    """oracle.selective_scan.selective_scan_fwd on the gathered operands -> (B, K, L, D)"""
    k, l, d, r, rg, tbl = c.k, c.l, c.d, c.r, c.rg, c.table
    a_neg = (-torch.exp(c.A.double()) if c.a_log else c.A.double()).reshape(k * d, 1)
    out = []
    for i in range(c.b):
        xi, ri = c.x[i].double(), c.xdbl[i].double().view(l, k, rg)
        u = torch.stack([xi[tbl[j]].t() for j in range(k)]).reshape(1, k * d, l)
        rows = torch.stack([ri[tbl[j], j] for j in range(k)])
        delta = torch.einsum("klr,kdr->kdl", rows[..., :r], c.dt_w.double()).reshape(1, k * d, l)
        Bm, Cm = rows[..., rg - 4].reshape(1, k, 1, l), rows[..., rg - 3].reshape(1, k, 1, l)
        y = oss.selective_scan_fwd(u.contiguous(), delta.contiguous(), a_neg, Bm.contiguous(), Cm.contiguous(), c.ds.double(),
                                   c.dt_b.double(), True)
        out.append(y.reshape(k, d, l).permute(0, 2, 1))
    return torch.stack(out)


@pytest.mark.parametrize("regime,a_log", [("slow", False), ("slow", True), ("undamped", False), ("init", True)])
def test_reference_loop_equals_the_oracle(regime, a_log):
    """13 x 13 = 169 positions (5 tiles + 9), both families' K, 16-bit pre-rounded and fp32 operands: 1e-12 of the largest output"""
    for fam, dtype in (("raster", F32), ("helix", BF16)):
        c = smc.make(regime, fam, 13, 2, 24, 3, dtype, seed=1, a_log=a_log)
        got, want = smc.reference(c)["ys"], _oracle_ys(c)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        if regime == "undamped":       # the closed form: h = cumsum(dt B u)
            t = smc._terms64(c, 0)
            h = torch.cumsum(t["bb"], 0)
            y = (t["C"] * h).sum(-1) + t["Du"]
            want0 = want[0].permute(1, 0, 2).reshape(c.l, -1)
            assert float((y - want0).abs().max()) <= 1e-12 * float(want0.abs().max())


def _fwd_keys():
    """(case, regime, input dtype, a_log, wave-segment fold) of every forward launch of tests/test_gpu_scan_memory.py: `init`
    goes in as A_logs where the form takes it (ring, LDS-DMA) and as A = -1 on the wave-segment form"""
    for name, (fam, h, d, r, b, dtypes) in smc.FWD_CASES.items():
        for dtype in dtypes:
            chained = name != "helix37_wide"
            segment = name in ("raster37", "helix37_wide")
            for regime in ("slow", "undamped"):
                if chained:
                    yield name, regime, dtype, False, False
                if segment:
                    yield name, regime, dtype, False, True
            if name in ("raster37", "helix40_r8", "helix40_r16", "helix40_r32"):
                yield name, "init", dtype, True, False
            if name == "raster37":
                yield name, "init", dtype, False, True


def test_segment_plans_of_the_gpu_cases():
    """rows 3 and 4 of the forward table: NT = 3 / NSEG = 15 and NT = 12 / NSEG = 4"""
    assert smc.nt_seg_of("raster37") == (3, 15)
    assert smc.nt_seg_of("helix37_wide") == (12, 4)


_ids = lambda v: str(v).replace("torch.", "")


@pytest.mark.parametrize("name,regime,dtype,a_log,segment", list(_fwd_keys()), ids=_ids)
def test_e32_of_the_forward_cases(name, regime, dtype, a_log, segment):
    """E32 per case and regime, chained or wave-segment fold; printed, and sane: an fp32 evaluation of a 1369 .. 1600-position
    recurrence stays within 1e-5 of fp64, `init` with its small-dt softplus included"""
    _, _, e = smc.fwd_e32(name, regime, dtype, a_log, segment)
    print(f"E32 fwd {name} {regime} {str(dtype)[6:]} a_log={int(a_log)} segment={int(segment)}: ys {e['ys'][0]:.3e} "
          f"(bound {smc.bound(e['ys'][0]):.3e}) states {e['states'][0]:.3e}")
    assert 0 < e["ys"][0] < 1e-5 and e["states"][0] < 1e-5, e


def _bwd_keys():
    for name, (fam, h, d, r, b, dtypes) in smc.BWD_CASES.items():
        for dtype in dtypes:
            for regime in ("slow", "init"):
                for a_log in (False, True):
                    yield name, regime, dtype, a_log


@pytest.mark.parametrize("name,regime,dtype,a_log", list(_bwd_keys()), ids=_ids)
def test_e32_of_the_backward_cases(name, regime, dtype, a_log):
    """per gradient, max-relative / RMS-relative; gB and gC summed over the channels in a shuffled order"""
    _, _, e = smc.bwd_e32(name, regime, dtype, a_log)
    print(f"E32 bwd {name} {regime} {str(dtype)[6:]} a_log={int(a_log)}: " + " ".join(f"{n} {e[n][0]:.2e}/{e[n][1]:.2e}" for n in smc.BWD_OUTPUTS))
    for n in smc.BWD_OUTPUTS:
        assert e[n][0] < 2e-5, (n, e[n])


FWD_FAULTS = ("drop_old", "edge8", "edge16", "atile", "seg_skip", "state_shift")
ADJ_FAULTS = ("adj_edge8", "adj_atile")


def _fault_ratios(regime, a_log=False):
    """smallest (fault error / bound) per fault on the raster 37 x 37 bf16 case (L = 1369 = 42 tiles + 25, NT = 3)"""
    c, ref, e = smc.bwd_e32("raster37", regime, BF16, a_log)
    _, e_seg = smc.e32(c, ("bwd", "raster37", regime, BF16, a_log), nt_seg=3)
    ratios = {}
    for fault in FWD_FAULTS:
        seg = fault == "seg_skip"
        got = smc.emulate(c, True, nt_seg=3 if seg else None, fault=fault)
        name = "states" if fault == "state_shift" else "ys"
        err = smc.rel_errors(got[name], ref[name])[0]
        b = smc.bound((e_seg if seg else e)[name][0], name)
        ratios[fault] = (err, b, err / b)
    for fault in ADJ_FAULTS:
        got = smc.emulate(c, True, backward=True, fault=fault, shuffle_seed=5)
        worst = None
        for n in smc.BWD_OUTPUTS:        # the output that shows the fault LEAST among those it reaches (gC, gD: forward only)
            if n in ("gC", "gD"):
                continue
            err, b = smc.rel_errors(got[n], ref[n])[0], smc.bound(e[n][0], n)
            if worst is None or err / b < worst[2]:
                worst = (err, b, err / b, n)
        ratios[fault] = worst
    return ratios


@pytest.mark.parametrize("regime", ["slow", "undamped"])
def test_every_injected_fault_exceeds_the_bound_a_hundredfold(regime):
    """Teeth.  Each fault breaks one hand-over rule of the tile-wise emulation: the state older than one tile dropped; the carry
    lost at each super-chunk edge (W = 8, W = 16); A_tile missing its last factor; the segment fold one segment short; every
    saved state one tile off; the adjoint's reverse carry lost at a super-chunk edge; the adjoint A_tile missing a factor.  In
    `slow` every one of them exceeds FACTOR * E32 of the output it reaches at least 100-fold.  In `undamped` a = 1 everywhere, so
    the two A_tile faults change nothing at all (asserted: the error stays within the bound); all the others are held to the
    same 100x."""
    ratios = _fault_ratios(regime)
    for fault, r in ratios.items():
        print(f"teeth {regime} {fault}: error {r[0]:.3e} bound {r[1]:.3e} ratio {r[2]:.1f}" + (f" ({r[3]})" if len(r) > 3 else ""))
    for fault, r in ratios.items():
        if regime == "undamped" and fault in ("atile", "adj_atile"):
            assert r[2] <= 1.0, (fault, r)
        else:
            assert r[2] >= 100.0, (fault, r)


def test_every_injected_fault_exceeds_the_init_bound_a_hundredfold():
    """`init` (dt 1e-3 .. 1e-1, A = -1, as A_logs) has its own E32 -- the gradients' is up to 10 times that of `slow`, the
    small-dt softplus -- and its own bounds; every fault still exceeds them 100-fold.  The A_tile faults come closest (one
    factor exp(-dt) = 0.9 .. 0.999 of a tile's decay): about 440x on ys, 110x on the adjoint."""
    ratios = _fault_ratios("init", a_log=True)
    for fault, r in ratios.items():
        print(f"teeth init {fault}: error {r[0]:.3e} bound {r[1]:.3e} ratio {r[2]:.1f}" + (f" ({r[3]})" if len(r) > 3 else ""))
    for fault, r in ratios.items():
        assert r[2] >= 100.0, (fault, r)


def test_ga_is_the_output_most_sensitive_to_the_decay():
    """Why gA alone is held to 2.5 x 8 x E32 (scan_memory_cases.FACTOR_FOR): with every decay a = exp2(t A) off by up to one
    ulp in one direction -- what a hardware exp2 that is accurate to an ulp but not correctly rounded may do -- gA moves 2 .. 2.5
    times as far from fp64 as ys, measured in units of their own E32; no other gradient moves a quarter further than ys does."""
    c, ref, e = smc.bwd_e32("raster37", "slow", BF16, False)
    got = smc.emulate(c, True, backward=True, shuffle_seed=5, biased_exp=True)
    move = {n: smc.rel_errors(got[n], ref[n])[0] / e[n][0] for n in ("ys",) + smc.BWD_OUTPUTS}
    print("moved by a one-sided ulp of the decay, in E32:", {n: round(v, 2) for n, v in move.items()})
    assert 2.0 <= move["gA"] / move["ys"] <= 2.5
    assert all(move[n] <= 1.25 * move["ys"] for n in smc.BWD_OUTPUTS if n != "gA")
    assert smc.FACTOR_FOR == {"gA": 2.5 * smc.FACTOR}


def test_the_older_recipe_hides_a_wrong_a_tile():
    """Why this file exists: on the input recipe of the older scan tests (decay 0.7 .. 0.9 per position) an A_tile that lacks a
    factor moves ys by less than the 2e-2 * scale those tests allow a 16-bit output."""
    c = smc.make("existing", "helix", 40, 1, 64, 8, BF16, seed=0)
    ref = smc.reference(c)
    got = smc.emulate(c, True, fault="atile")
    err = smc.rel_errors(got["ys"], ref["ys"])[0]
    print(f"older recipe, A_tile fault: {err:.3e} of scale")
    assert err < 2e-2


@pytest.mark.parametrize("regime", ["slow", "undamped"])
@pytest.mark.parametrize("n", [1, 4])
def test_e32_of_the_boundary_cases(regime, n):
    for dtype, l in smc.BOUNDARY_L.items():
        o = smc.make_boundary(regime, 2, 4, 8, n, l, dtype)
        _, e = smc.boundary_e32(o, (regime, n, l, dtype))
        print(f"E32 boundary {regime} N={n} {str(dtype)[6:]}: " + " ".join(f"{k} {v[0]:.2e}/{v[1]:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v[0] < 1e-5, (k, v)
