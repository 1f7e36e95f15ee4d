"""CPU, fp64: everything tests/test_gpu_fp16_range.py takes for granted about tests/golden/fp16_range_cases.py -- the
references equal autograd through the oracle, they are exactly linear in dy over the ladder, dy is a normal fp16 number at
every level, the overflow level hits between 1 % and 50 % of a 16-bit output, the poison masks are never empty -- and the
mutation check: the emulated ideal kernel passes every assertion of the GPU test, each of its three mutants fails the
assertion that is there for it.  e_store is printed per (case, output, level): the reference's own statement of which
quantities fit fp16 at the working point (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import fp16_range_cases as rc

F16, BF16, F32 = rc.F16, rc.BF16, rc.F32
CHEAP = [n for n in rc.NAMES if not n.startswith(("scan_", "fn_"))]
SCANS = [n for n in rc.NAMES if n.startswith("scan_")]


def _maxrel(a, b):
    return rc.metric_err("maxrel", a, b)


# the scan cases hold x_dbl as the fp32 rows the x_proj GEMM hands the kernel (ss2d_dstate_cases.core_as_scan_case), the oracle
# forms them in fp64: the two agree to fp32's rounding of those rows, not to fp64's
XDBL_F32 = 2e-6


# ----------------------------------------------------------------------------- references
@pytest.mark.parametrize("name", SCANS)
def test_scan_references_equal_autograd_through_the_oracle(name):
    """the kernel-level adjoint, carried to the leaves by the linear maps around the kernel, against autograd through
    oracle.ops.ss2d_core + cross_merge with dy0 as the merged map's gradient"""
    c = rc.case(name, F16)
    got, want = c.leaves(c.ref0), c.oracle_leaves(c.dy0)
    for k in want:
        assert _maxrel(got[k], want[k]) <= XDBL_F32, (name, k, _maxrel(got[k], want[k]))


@pytest.mark.parametrize("name", [n for n in rc.NAMES if n.startswith("fn_")])
def test_function_references_are_the_scan_references_at_the_leaves(name):
    c = rc.case(name, F16)
    want = rc.ScanCase.oracle_leaves(c, c.dy0)
    ref = c.ref0
    a = want["a_logs"] if c.c.n > 1 else (want["a_logs"] / c.c.A.double()).reshape(-1)
    for k, w in (("dt_w", want["dt_w"]), ("dt_b", want["dt_b"]), ("a", a), ("ds", want["ds"])):
        assert _maxrel(ref[k], w) <= XDBL_F32, (name, k, _maxrel(ref[k], w))


def test_closed_form_references_equal_autograd():
    c = rc.case("rowdot", F16)
    x, w = c.x.double().requires_grad_(), c.w.double().requires_grad_()
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    ((x @ w + b) * c.dy0).sum().backward()
    for k, g in (("gx", x.grad), ("gw", w.grad), ("gb", b.grad)):
        assert _maxrel(c.ref0[k], g) <= 1e-12, k
    for name in [n for n in rc.NAMES if n.startswith("gelu_grad_gemm")]:
        c = rc.case(name, F16)
        h = c.h.double().requires_grad_()
        ((F.gelu(h) @ c.w.double()) * c.dy0).sum().backward()            # Linear(GELU(h)) with weight w^T
        assert _maxrel(c.ref0["y"], h.grad) <= 1e-12, name
    c = rc.case("shuffle_norm_head", F16)
    from oracle import ops as oo
    coef = torch.ones(c.c, dtype=torch.float64, requires_grad=True)
    xs = oo.pixel_shuffle_groups(c.x.double().permute(0, 3, 1, 2), c.p)
    xhat = (xs - xs.mean(1, keepdim=True)) / torch.sqrt(xs.var(1, unbiased=False, keepdim=True) + 1e-5)
    ((xhat * coef.view(1, -1, 1, 1)).sum(1) * c.dy0).sum().backward()
    assert _maxrel(c.ref0["A"], coef.grad) <= 1e-12
    # and the whole head against the oracle's LayerNorm: logits = head(LN(shuffle(x)))
    xr = c.x.double().permute(0, 3, 1, 2).requires_grad_()
    y = oo.layernorm2d(oo.pixel_shuffle_groups(xr, c.p), c.w.double(), c.b.double())
    ((y * c.hw.double().view(1, -1, 1, 1)).sum(1) * c.dy0).sum().backward()
    assert _maxrel(c.ref0["dx"], xr.grad.permute(0, 2, 3, 1)) <= 1e-9


@pytest.mark.parametrize("name", list(rc.TAIL_CFGS))
def test_tail_references_equal_autograd_of_the_forward_map(name):
    """the tail is the adjoint of the scan's gather: x_dbl rows (B, L, K, RG) -> for direction k and position i the row of pixel
    table[k][i]; its first R columns times dt_w give raw, columns R8 .. are B and C.  g_xd must be autograd's gradient of
    sum(graw raw) + sum(dB B) + sum(dC C) with respect to the rows; with graw = 0 that is the assemble entry's reference"""
    c = rc.case(name, F16)
    b, h, d, r, fam, n, k, l = c.geo
    r8 = c.r8
    pb, pc = (p.sum(2) for p in c.part0)                                              # (B, K, N, L)

    def grad(graw, gseq_extra=None):
        xd = torch.zeros(b, l, k, c.rg, dtype=torch.float64, requires_grad=True)
        loss = 0
        for j in range(k):
            rows = xd[:, c.table[j], j]                                                  # (B, L, RG)
            if graw is not None:
                loss = loss + (graw[:, j] * (rows[..., :r] @ c.dt_w[j].double().t())).sum()
                loss = loss + (pb[:, j].transpose(1, 2) * rows[..., r8:r8 + n]).sum()
                loss = loss + (pc[:, j].transpose(1, 2) * rows[..., r8 + n:r8 + 2 * n]).sum()
            else:
                loss = loss + (gseq_extra[:, j] * rows).sum()
        loss.backward()
        return xd.grad.view(b, l, k * c.rg)

    assert _maxrel(c.ref0["g_xd"], grad(c.dy0)) <= 1e-12
    a = rc.case(f"assemble:{name}", F16)
    live = torch.zeros(c.rg, dtype=torch.float64)
    live[:r] = 1.0
    live[r8:r8 + 2 * n] = 1.0                                                            # the padding columns carry no gradient
    assert _maxrel(a.ref0["g_xd"], grad(None, a.dy0 * live)) <= 1e-12
    assert float(a.dy0[..., live == 0].abs().min()) >= 2.0 ** -8                       # ... though dy is non-zero there
    rows = rc.case(f"rows:{name}", F16)
    coef = torch.ones(b, k, l, r, dtype=torch.float64, requires_grad=True)         # the rows are the gradient of sum(coef raw) in coef
    (coef * torch.stack([rows.dy0[:, j] @ c.dt_w[j].double() for j in range(k)], 1)).sum().backward()
    assert _maxrel(rows.ref0["rows"], coef.grad.reshape(b * k, l, r)) <= 1e-12
    prep = rc.case(f"prep:{name}", F16)
    assert torch.equal(prep.ref0["bc"][..., :n], pb.transpose(2, 3)) and torch.equal(prep.ref0["bc"][..., n:], pc.transpose(2, 3))


def test_merge_grad_and_dct_references_equal_autograd():
    for name in rc.MERGE_CFGS:
        c = rc.case(name, F16)
        fam, h, d, b, k, l = c.geo
        z = c.z.double().requires_grad_()
        xs = F.silu(z)
        loss = (c.t0 * xs).sum()
        for j in range(k):
            loss = loss + (c.dy0[:, j] * xs[:, c.table[j]]).sum()                          # the scan's gather of silu(z), direction j
        loss.backward()
        assert _maxrel(c.ref0["gz"], z.grad) <= 1e-12, name
    c = rc.case("dct_split", F16)                                                          # (its reference is autograd through
    n = c.w.shape[0]                                                                       # oracle.ops.dct2d_split; restated here)
    w, x = c.w.double(), c.x.double().requires_grad_()
    y = torch.einsum("vh,bhwc,uw->bvuc", w, x, w)
    ((y[:, :n // 2, :n // 2] * c.dy0).sum() + (y[:, n // 2:, n // 2:] * c.gh0).sum()).backward()
    assert _maxrel(c.ref0["gx"], x.grad) <= 1e-12


@pytest.mark.parametrize("name", rc.NAMES)
def test_references_are_exactly_linear_over_the_ladder(name):
    c = rc.case(name, F16)
    levels = set(rc.LEVELS[F16])
    if rc.stored16(c) and c.overflow:
        levels.add(rc.overflow_level(c)[0])
    for level in sorted(levels - {0}):
        ref = c.reference(c.dy0 * 2.0 ** level)
        for k, v in c.ref0.items():
            assert torch.equal(ref[k], v * 2.0 ** level), (name, k, level)


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("name,dtype", rc.PARAMS, ids=rc.IDS)
def test_dy_is_a_normal_number_of_its_dtype_at_every_level(name, dtype):
    c = rc.case(name, dtype)
    assert float(c.dy0.abs().max()) == 1.0 and float(c.dy0.abs().min()) >= 2.0 ** -8
    assert torch.equal(c.dy0, rc.rnd(c.dy0, dtype))
    for level in rc.LEVELS[dtype]:
        dy = c.dy_device(level, "cpu")                    # asserts the scaled dy is exact in the dtype it travels in
        assert dy.dtype == c.up_dtype
        lo, hi = float(dy.double().abs().min()), float(dy.double().abs().max())
        assert lo >= rc.FP16_MIN_NORMAL and hi == 2.0 ** level <= 65504.0, (name, level, lo, hi)
        if getattr(c, "gres0", None) is not None:
            g = c.gres0 * 2.0 ** level
            assert float(g.abs().min()) >= rc.FP16_MIN_NORMAL and torch.equal(g, rc.rnd(g, dtype))
    for value in (float("inf"), float("nan")):
        dy = c.dy_device(0, "cpu", poison=value)
        assert int((~torch.isfinite(dy)).sum()) == 1


OVERFLOW_NAMES = rc.OVERFLOW_NAMES


def test_overflow_is_left_out_only_where_it_cannot_happen():
    """every case with a 16-bit output has an overflow level, except those whose upstream gradient must itself fit fp16 and
    whose gain is too small: at 2^15, the last level at which dy is finite in fp16, not 1 % of the output reaches 2^17"""
    for name in rc.NAMES:
        c = rc.case(name, F16)
        assert (name in OVERFLOW_NAMES) == bool(rc.stored16(c) and c.overflow), name
        if rc.stored16(c) and not c.overflow:
            assert c.up_dtype == F16 and c.over_dtype is None
            assert not bool(torch.isfinite((c.dy0 * 2.0 ** 16).half()).all())
            for k in rc.stored16(c):
                share = float((c.ref0[k].abs() * 2.0 ** 15 >= rc.OVERFLOW_AT).double().mean())
                print(name, k, "share reaching 2^17 at the last level dy fits fp16:", share)
                assert share < rc.SHARE[0], (name, k, share)


@pytest.mark.parametrize("name", OVERFLOW_NAMES)
def test_overflow_level_hits_between_1_and_50_percent(name):
    c = rc.case(name, F16)
    level, shares = rc.overflow_level(c)
    print(name, "overflow level", level, {k: f"{v:.3f}" for k, v in shares.items()})
    assert rc.SHARE[0] <= max(shares.values()) and all(v <= rc.SHARE[1] for v in shares.values()), (level, shares)
    dy = c.dy_device(level, "cpu", overflow=True)         # exact in the dtype it travels in at that level
    assert bool(torch.isfinite(dy).all())
    below = {k: float((c.ref0[k].abs() * 2.0 ** (level - 1) >= rc.OVERFLOW_AT).double().mean()) for k in shares}
    assert max(below.values()) < rc.SHARE[0]
    for k, m in rc.overflow_masks(c, level).items():
        assert bool(torch.isinf(rc.rnd(c.ref0[k] * 2.0 ** level, F16)[m]).all())


def test_function_cases_have_no_16_bit_output():
    assert all(not rc.stored16(rc.case(n, F16)) for n in rc.NAMES if n.startswith(("fn_", "prep:", "rows:")))


@pytest.mark.parametrize("name", rc.NAMES)
def test_poison_masks_are_never_empty(name):
    c = rc.case(name, F16)
    for k, m in c.poison_masks.items():
        assert m.shape == c.ref0[k].shape and bool(m.any()), (name, k)
    assert set(c.poison_masks) == set(c.outputs)
    # what the dependency set leaves out of the reference's NaN mask: nothing, except (a) the taps of the depth-wise weight
    # gradient that meet only zero padding at the poisoned pixel (a corner of the 9 x 9 map: 16 of 25; 24 x 24, k 7: 21 of 49)
    # and (b) dA of the two raster directions that START at the poisoned pixel (pixel 0 of the second image): there the adjoint
    # is NaN at sequence position 0 alone, where it multiplies the state before the first step -- the zero initial state
    nan = {k: int(torch.isnan(v).sum()) for k, v in c.poison_ref(float("nan")).items()}
    dropped = {k: nan[k] - int(m.sum()) for k, m in c.poison_masks.items() if nan[k] != int(m.sum())}
    print(name, "NaN mask", nan, "dropped", dropped)
    expect = {"dwconv:2x9x32_k5": {"gw": 16}, "dwconv:1x24x130_k7": {"gw": 21}, "scan_n1_raster": {"gA": 2},
              "scan_n1_raster_trained": {"gA": 2}, "fn_core_raster": {"a": 2}}
    assert dropped == expect.get(name, {}), (name, dropped)
    assert not bool(torch.isnan(c.ref0[next(iter(c.outputs))]).any())


@pytest.mark.parametrize("name,dtype", rc.PARAMS, ids=rc.IDS)
def test_e_store_is_finite_and_printed(name, dtype):
    c = rc.case(name, dtype)
    for k, o in c.outputs.items():
        es = {level: rc.e_store(c, k, level) for level in rc.LEVELS[dtype]}
        print(f"{name} {str(dtype)[6:]} {k}: max |R| {float(c.ref0[k].abs().max()):.3e}  T_unit {o.tol:.1e}  e_store "
              + "  ".join(f"2^{level}: {v:.2e}" for level, v in es.items()))
        assert all(v == v and v < float("inf") for v in es.values()), (name, k, es)
        if o.store == F32:          # (in units of u A for the attention cases)
            assert max(es.values()) <= (1e-3 if o.metric == "uA" else 2.0 ** -23)


# ----------------------------------------------------------------------------- the mutation check
def _ladder_failures(c, mutant):
    bad = {}
    for level in rc.LEVELS[c.dtype]:
        got = rc.ideal(c, level, mutant)
        for k in c.outputs:
            err, bnd = rc.err_at(c, k, level, got[k]), rc.bound(c, k, level)
            if not err <= bnd:
                bad[(k, level)] = (err, bnd)
    return bad


def _overflow_failures(c, mutant):
    level = rc.overflow_level(c)[0]
    got = rc.ideal(c, level, mutant)
    return {k: int(torch.isfinite(got[k][m]).sum()) for k, m in rc.overflow_masks(c, level).items()
            if bool(torch.isfinite(got[k][m]).any())}


def _poison_failures(c, mutant):
    bad = {}
    for value in (float("inf"), float("nan")):
        got = rc.ideal(c, 0, mutant, poison=value)
        for k, m in c.poison_masks.items():
            if bool(torch.isfinite(got[k][m]).any()):
                bad[(k, value)] = int(torch.isfinite(got[k][m]).sum())
    return bad


@pytest.mark.parametrize("name,dtype", rc.PARAMS, ids=rc.IDS)
def test_the_ideal_kernel_passes_every_assertion(name, dtype):
    c = rc.case(name, dtype)
    assert not _ladder_failures(c, None)
    if dtype == F16:
        assert not _poison_failures(c, None)
        if rc.stored16(c) and c.overflow:
            assert not _overflow_failures(c, None)


SMALL = 2.0 ** -7      # an output whose largest element is below this sits, 2^-10 further down and at dy's level 2^-6, entirely
                       # below 2^-23: in fp16's last two subnormal steps


@pytest.mark.parametrize("name", rc.NAMES)
def test_a_16_bit_intermediate_below_the_output_fails_at_the_working_point(name):
    """fp16: the mutant passes wherever its intermediate is a normal fp16 number, and fails at 2^-6 on every output small
    enough for the intermediate to fall among fp16's last subnormals (graw in the trained regime); the Function cases restate
    their real intermediate (graw in the activation dtype) and fail on dt_w at 2^-6 while passing at 2^0 and 2^6.  With the
    max-type metrics and tolerances of the existing tests an output of dy's own magnitude hides such an intermediate: its
    error is 2^-9 of the output's largest element at most.  bf16, the control, passes throughout."""
    c = rc.case(name, F16)
    bad = _ladder_failures(c, "intermediate")
    print(name, {k: (f"{e:.2e}", f"{b:.2e}") for k, (e, b) in bad.items()})
    small = [] if name.startswith("fn_") else [k for k in c.outputs if float(c.ref0[k].abs().max()) <= SMALL]
    assert all((k, -6) in bad for k in small), (small, bad)
    if name.startswith(("kv_", "window_")):
        # the attention tests bound every element by its own magnitude A: there the mutant shows even on outputs of dy's size
        assert all((k, -6) in bad for k in ("dq", "dv")), bad
    elif name.startswith("rows:"):
        # held to 1e-5 (exact 16-bit operands, fp32 sums): any 16-bit rounding on the way shows at every level
        assert set(bad) == {("rows", level) for level in rc.LEVELS[F16]}, bad
        return
    else:
        assert all(level == -6 or k in small for k, level in bad), bad
    if name.endswith("_trained"):
        assert "graw" in small and "gu" not in small, small
    if name.startswith("fn_"):
        assert set(bad) == {("dt_w", -6)}, bad
    assert not _ladder_failures(rc.case(name, BF16), "intermediate")


@pytest.mark.parametrize("name", OVERFLOW_NAMES)
def test_a_saturating_store_fails_the_overflow_level(name):
    c = rc.case(name, F16)
    assert _overflow_failures(c, "clamp") and not _ladder_failures(c, "clamp")


@pytest.mark.parametrize("name", rc.NAMES)
def test_swallowing_non_finite_values_fails_the_poison_level(name):
    c = rc.case(name, F16)
    bad = _poison_failures(c, "nan_to_num")
    assert {k for k, _ in bad} == set(c.outputs), bad
