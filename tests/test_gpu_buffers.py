"""No kernel result may depend on what torch.empty hands back (tests/golden/buffer_cases.py; CPU side:
tests/test_buffers_host.py).  Every case runs under NaN, zero and seeded-noise fills of every uninitialised allocation of the
library and once unpatched; the documented payload of every result must be finite and bit-identical across the four runs.
The entries that add floats with atomics are held to the tolerance of their own tests against the same fp64 oracles instead:

  selective_scan_bwd            dA, dB, dC, dD, dbias (csrc/selective_scan.hip atomicAdd; test_selective_scan_bwd's measure)
  ss2d_scan_bwd_cl              gB, gC without bc_partials (csrc/ss2d_fused.hip ~1099; test_ss2d_core_training_gradients' 5e-4 /
                                5e-2 of the largest entry), alone and inside _SS2DCoreCL

A: the chains (blocks, training blocks, losses, metrics, frames, augment); B: wrappers at the smallest shapes with a ragged
tail, more than one partial row or a pad; C: persistent workspaces and stale contents.

Shapes of the plan that an entry refuses are replaced by the nearest shape it takes (csrc/train_gemm.hip: the weight-gradient
GEMMs need N % 8 == 0 and K % 8 == 0, rows_gemm_cl N <= 64; csrc/linear.hip: linear2_cl / linear_ln_cl / linear_dual_cl need
K % 64 == 0, the last two N % 8 == 0): (37, 8, 16), (513, 136, 72) for the weight gradients, N = 5 and 61 for rows_gemm_cl,
K = 64 / 128 for the three fused GEMMs."""

import numpy as np
import pytest
import torch

import buffer_cases as bc
import scan_dstate_cases as sdc
import scan_memory_cases as smc
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def H():
    from tramba_amd import hip
    return hip


def rnd(seed, *shape, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# ============================================================================= A. chains
from test_gpu_model import TAGS  # noqa: E402


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("path", ["inference", "training"])
@pytest.mark.parametrize("tag", TAGS)
def test_blocks(tag, path, dtype):
    """the nine golden blocks: outputs, every parameter gradient and the input gradient.  A fresh module per run, so that its
    standing packs and caches are allocated under every fill"""
    import tramba_amd as ta
    from test_gpu_model import _blocks, _load_synth
    ctor, shape = _blocks()[tag]
    x = synth.synth_input("g4_" + tag, shape)

    def run():
        m = _load_synth(ctor())
        if path == "inference":
            if dtype != F32:
                for mod in m.modules():            # the prepare_inference policy on a bare block (test_gpu_model.py)
                    if isinstance(mod, ta.Linear2d):
                        mod.weight.data = mod.weight.data.to(dtype)
                    elif isinstance(mod, ta.SS2D):
                        mod.x_proj_weight.data = mod.x_proj_weight.data.to(dtype)
            with torch.no_grad():
                return m(x.to(DEV, dtype))
        xin = x.to(DEV).to(dtype).requires_grad_()
        y = m(xin)
        gy = synth.synth_input("g4_gy_" + tag, tuple(y.shape)).to(DEV).to(y.dtype)
        return [y.detach()] + list(torch.autograd.grad(y, [xin] + list(m.parameters()), gy))
    bc.check_independent(run, what=f"{tag} {path} {dtype}")


@pytest.mark.parametrize("family,kind,mode", [("attn", "swin", "fused"), ("attn", "pvt", "fused"), ("enc", "swin", "library"),
                                              ("enc", "pvt", "library"), ("resnet", "layer1", "library"),
                                              ("resnet", "layer2", "library")])
def test_training_blocks(family, kind, mode):
    """the attention, patch-conv and bottleneck training blocks of the existing builders at their existing shapes: the input
    gradient and every parameter gradient.

    ("attn", "pvt") is held to its own test's bound instead of bit for bit: with only the attention fused, the block's
    spatial-reduction Conv2d and its LayerNorms run on the framework's kernels, whose backward is not the same run to run
    (measured unpatched on an MI355X: norm1.weight, norm1.bias and attn.sr.weight differ between two runs of the same
    process).  Every run must be finite and keep test_block_gradients_keep_the_stock_error's bound (error against the fp32
    gradients <= the stock 16-bit path's, times 1 + its recorded spread; attn_blocks.gemm_conv names the cause: the framework's
    convolution may add its split reduction with atomics).  The library's part of that chain is held bit for bit:
    kv_attention_cl and kv_attention_bwd_cl run below on the operands the block hands them, test_attention_and_its_backward runs
    both at the block's shapes (2 x 576 queries on 144 keys, 2 heads of 64) on operands of its own, and the ("enc", "pvt")
    block, where every layer runs on the library, is exact as a whole."""
    import attn_train_blocks
    import enc_train_blocks
    import resnet_train_blocks
    mod = {"attn": attn_train_blocks, "enc": enc_train_blocks, "resnet": resnet_train_blocks}[family]
    if (family, kind) != ("attn", "pvt"):
        bc.check_independent(lambda: mod.block_grads(kind, 0, mode), what=f"{family} {kind}")
        return
    from test_gpu_attn_train import _parity_margins
    margins = _parity_margins(kind)
    stock, ref = (mod.block_grads(kind, 0, m) for m in ("stock", "fp32"))
    names = list(ref)
    assert set(names) == set(margins)

    def close(ts):
        for name, got in zip(names, ts):
            fused, base = mod.rel_l2(got.to(DEV), ref[name]), mod.rel_l2(stock[name], ref[name])
            assert fused <= base * (1 + margins[name]), (name, fused, base, margins[name])
    bc.check_independent(lambda: mod.block_grads(kind, 0, mode), payload=lambda d: [d[n] for n in names], exact=False, close=close,
                         what=f"{family} {kind}")

    # what the library itself computes inside that block, bit for bit: kv_attention_cl and kv_attention_bwd_cl on the very
    # operands the block hands them (tapped from an unpatched run; between two runs of the block the operands themselves
    # differ, since k and v come out of the framework's spatial-reduction convolution)
    hip = H()
    calls = {}

    def tap(name):
        orig = getattr(hip, name)

        def tapped(*a, **k):
            calls[name] = (tuple(t.detach().clone() if torch.is_tensor(t) else t for t in a), dict(k))
            return orig(*a, **k)
        return orig, tapped
    saved = {n: tap(n) for n in ("kv_attention_cl", "kv_attention_bwd_cl")}
    try:
        for n, (_, t) in saved.items():
            setattr(hip, n, t)
        mod.block_grads(kind, 0, mode)
    finally:
        for n, (o, _) in saved.items():
            setattr(hip, n, o)
    assert set(calls) == set(saved)
    (fa, fk), (ba, bk) = calls["kv_attention_cl"], calls["kv_attention_bwd_cl"]
    assert tuple(fa[0].shape) == (2, 576, 128) and tuple(fa[1].shape) == (2, 144, 256) and not bk.get("out")
    bc.check_independent(lambda: [hip.kv_attention_cl(*fa, **fk), *hip.kv_attention_bwd_cl(*ba, **bk)],
                         what=f"{family} {kind}, the attention inside")


def test_adam_step_with_weight_decay():
    from tramba_amd import train
    from test_gpu_step_ends import ADAM_SHAPES
    g = torch.Generator().manual_seed(7)
    ps = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    gs = [[torch.randn(s, generator=g) * (10.0 ** (i % 3 - 2)) for i, s in enumerate(ADAM_SHAPES)] for _ in range(2)]

    def run():
        params = [torch.nn.Parameter(p.to(DEV)) for p in ps]
        opt = train.Adam(params, 1e-2, weight_decay=0.01)
        for grads in gs:
            for p, gr in zip(params, grads):
                p.grad = gr.to(DEV)
            opt.step()
        return [p.detach() for p in params] + [opt.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")]
    bc.check_independent(run, what="Adam")


LOSS_LABEL = (2, 1, 37, 45)                       # 1665 pixels: two loss blocks, the second ragged
LOSS_SIZES = [(7, 9), (12, 15), (37, 45)]


@pytest.mark.parametrize("form", ["sod_loss", "structure", "wbce", "raw_weight"])
def test_losses_and_their_gradients(form):
    hip = H()
    outs = [synth.synth_input(f"buf_loss_{i}", LOSS_LABEL[:2] + s, scale=3.0).to(DEV) for i, s in enumerate(LOSS_SIZES)]
    lab = (synth.synth_input("buf_loss_y", LOSS_LABEL) > 0.2).float().to(DEV)
    assert hip._loss_nblk(LOSS_LABEL[2] * LOSS_LABEL[3]) > 1 and (LOSS_LABEL[2] * LOSS_LABEL[3]) % 1024
    gscale = torch.tensor(0.5, device=DEV)

    def run():
        if form == "sod_loss":
            loss, coefs = hip.sod_loss(outs, lab, weights=(0.25, 2.0, 1.0))
            return [loss, coefs] + [hip.sod_loss_grad(o, lab, coefs[i], gscale) for i, o in enumerate(outs)]
        if form == "raw_weight":
            wmap = torch.sigmoid(synth.synth_input("buf_loss_w", LOSS_LABEL)).to(DEV)
            kw = dict(eps=0.001, weight_is_raw=True)
            extra = []
        else:
            wmap = hip.loss_weight_map(lab, 31 if form == "structure" else 15)
            kw = dict(eps=0.001 if form == "structure" else 0.0)
            extra = [wmap]
        loss, coefs = hip.sod_wloss(outs, lab, wmap, with_iou=form != "wbce", per_pixel=form == "wbce", **kw)
        return extra + [loss, coefs] + [hip.sod_wloss_grad(o, lab, wmap, coefs[i], gscale, **kw) for i, o in enumerate(outs)]
    bc.check_independent(run, what=form)


@pytest.mark.parametrize("hw", [(48, 80), (1, 1)])
def test_metrics(hw):
    hip = H()
    pred = torch.sigmoid(synth.synth_input(f"buf_metric_{hw[0]}", (2,) + hw, scale=2.0)).to(DEV)
    gt = (synth.synth_input(f"buf_metric_gt_{hw[0]}", (2,) + hw) > 0.3).to(DEV)
    gt[1] = False                                 # an empty mask: idx = dist2 = -1 everywhere

    def payload(res):
        """on a one-pixel image three of the four S-measure quadrants are empty and their centred moments (slots 32 .. 45 of
        the fp64 record) are 0 / 0 whatever the memory held; nothing reads them there: the mask is empty or full, and
        evaluate.ImageStats.smeasure returns on its first lines (`area == 0`, `area == n`) before it looks at a quadrant"""
        if hw == (1, 1):
            res = [res[0], res[1][:, :32], res[1][:, 46:]] + list(res[2:])
        return res
    bc.check_independent(lambda: list(hip.saliency_stats(pred, gt)) + list(hip.feature_transform(gt)) +
                         [hip.weighted_f_sums(pred, gt)], payload=payload, what=f"metrics {hw}")


FRAME_SIZES = [(37, 53), (120, 64), (5, 200)]


def _frame(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_frames_and_maps():
    """frames_to_input / logits_to_u8 and their ragged forms on a mixed list of three sizes; of the ragged output buffer only
    the maps are payload (the bytes between them belong to nobody: infer._map_views reads the maps alone)"""
    from tramba_amd import infer
    hip = H()
    s = 48
    frames = [_frame(h, w, 7 * h + w) for h, w in FRAME_SIZES]
    logits = rnd(3, 3, 1, s, s, scale=3.0)
    uni = torch.from_numpy(np.stack([_frame(37, 53, i) for i in range(2)])).to(DEV)

    def run():
        a = infer.preprocess(frames, s)
        b = infer.preprocess(uni, s)
        maps = infer.postprocess(logits, FRAME_SIZES)
        one = infer.postprocess(logits.to(BF16), FRAME_SIZES[0])
        return [a, b, one] + list(maps)
    bc.check_independent(run, what="frames")


def _aug_samples(size, n, seed=99):
    from tramba_amd import augment
    from test_gpu_augment import SOURCES, _pair
    rec = augment.DrawRecorder(np.random.RandomState(seed))
    pairs = [_pair(h, w, h + 3 * w) for h, w in SOURCES]
    return [(*pairs[i % len(pairs)], rec(size)) for i in range(n)]


def _aug_run(samples, size):
    from tramba_amd import augment
    batch = augment.pack(samples, size)
    desc = augment.bind(augment.descriptors(batch), size, torch.device(DEV, torch.cuda.current_device()))
    return augment.transform(batch["packed"].to(DEV), desc, size)


def test_augment_transform():
    samples = _aug_samples(256, 8)
    bc.check_independent(lambda: list(_aug_run(samples, 256)), what="augment.transform")


# ============================================================================= B. wrappers
NORM_ROWS, NORM_C = (37, 4609), (16, 200, 1024)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", NORM_C)
@pytest.mark.parametrize("rows", NORM_ROWS)
def test_layernorm_backward_family(rows, c, dtype):
    """layernorm_bwd_cl, layernorm_bwd_res_cl (masked, with the incoming residual gradient), their deferred forms; the rows
    form, the generic form and the wide 16-bit form; one and several rows of the partial table"""
    hip = H()
    b = 1 if rows == 37 else 11                   # 4609 = 11 * 419
    x, dy, gres = (rnd(s, b, rows // b, c, dtype=dtype) for s in (1, 2, 3))
    w = rnd(4, c) * 0.1 + 1
    mask = (torch.arange(b) % 2).float().to(DEV) * 2
    parts = hip.lib().tramba_layernorm_bwd_parts(rows, c, hip.dt(x))
    assert parts >= 1 and (rows == 37 or parts > 1), parts

    def run():
        out = list(hip.layernorm_bwd_cl(x, dy, w))
        out += list(hip.layernorm_bwd_res_cl(x, dy, w, gres=gres, mask=mask, want_masked=True))
        with hip.deferred_sums():
            late = list(hip.layernorm_bwd_cl(x, dy, w, defer=True))[1:]
        return out + late
    bc.check_independent(run, what=f"layernorm_bwd {rows}x{c}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", NORM_C)
@pytest.mark.parametrize("hw", [(3, 3), (1, 1153)])
def test_shuffle_norm_backward(hw, c, dtype):
    """the grid of the LayerNorm backwards through the pixel shuffle (p = 2: the rows are 4 per input pixel, so 36 and 4612
    stand for 37 and 4609): the rows form, the generic form and the wide 16-bit form, with dx addressed through the shuffle"""
    hip = H()
    p, (h, w_) = 2, hw
    rows = h * w_ * p * p
    assert rows in (36, 4612)
    x = rnd(5, 1, h, w_, p * p * c, dtype=dtype)
    dy = rnd(6, 1, h * p, w_ * p, c, dtype=dtype)
    w, b = rnd(7, c) * 0.1 + 1, rnd(8, c) * 0.1
    parts = hip.lib().tramba_layernorm_bwd_parts(rows, c, hip.dt(x))
    assert parts >= 1 and (rows == 36 or parts > 1), parts
    bc.check_independent(lambda: [hip.shuffle_norm_cl(x, w, b, p)] + list(hip.shuffle_norm_bwd_cl(x, dy, w, p)),
                         what=f"shuffle_norm {rows}x{c}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_head_backwards(dtype):
    """shuffle_norm_head_bwd_cl: of `part` only slots 0 .. C are payload (A_c and G; the three slots behind them pad the row to
    16 bytes and nothing reads them: modules._ShuffleNormHeadCL.backward takes s[:c] and s[c] of the slab sum);
    rowdot_bwd_cl returns the summed slots itself"""
    hip = H()
    c, p = 16, 4
    x = rnd(9, 2, 6, 6, p * p * c, dtype=dtype)
    g = rnd(10, 2, 6 * p, 6 * p)
    lw, hw = rnd(11, c) * 0.1 + 1, rnd(12, c)
    bc.check_independent(lambda: hip.shuffle_norm_head_bwd_cl(x, g, lw, hw, p), payload=lambda r: [r[0], r[1][:, :c + 1]],
                         what="shuffle_norm_head_bwd")
    xr = rnd(13, 2, 37, 19, 64, dtype=dtype)
    gy = rnd(14, 2, 37, 19)
    wr = rnd(15, 64)
    assert hip.rowdot_bwd_ok(xr)
    bc.check_independent(lambda: [hip.rowdot_cl(xr, wr, 0.25)] + list(hip.rowdot_bwd_cl(xr, gy, wr)), what="rowdot")


def _dw_parts_shape(hip, ks):
    """the smallest (B, H, H, 32) map with more than one row of partial sums"""
    for b, h in [(b, h) for h in (12, 16, 24, 32, 48, 64, 96) for b in (1, 2, 4)]:
        if hip.lib().tramba_dwconv_wgrad_parts(b, h, h, 32, ks) > 1:
            return b, h, 32
    raise AssertionError("no small shape with more than one partial row")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ks", [3, 5, 7])
def test_depthwise_weight_gradients(ks, dtype):
    hip = H()
    shapes = [(1, 5, 4), (1, 7, 6), (2, 12, 32), _dw_parts_shape(hip, ks)]
    assert hip.lib().tramba_dwconv_wgrad_parts(shapes[-1][0], shapes[-1][1], shapes[-1][1], 32, ks) > 1
    for b, h, c in shapes:
        x, gy = rnd(16 + h, b, h, h, c, dtype=dtype), rnd(17 + h, b, h, h, c, dtype=dtype)

        def run():
            out = list(hip.dwconv_wgrad_cl(x, gy, ks))
            out += [t for t in hip.dw_unpack_grad(hip.dwconv_wgrad_table(x, gy, ks), ks, multiscale=ks == 7, nbias=3 if ks == 7 else 1)]
            with hip.deferred_sums():
                late = hip.dw_unpack_grad(hip.dwconv_wgrad_table(x, gy, ks, defer=True), ks, nbias=1, defer=True)
            return out + list(late)
        bc.check_independent(run, what=f"dwconv_wgrad ks {ks} {(b, h, c)}")


def _multi_slab_m(hip, n, k):
    """the smallest m (a multiple of 64 plus 1, so that the last chunk is ragged) at which wgrad_cl leaves several slabs"""
    one = (n * k + n) * 4
    for m in range(513, 8192, 64):
        if hip.lib().tramba_wgrad_workspace(m, n, k, 1, 1) > one:
            return m
    raise AssertionError("no multi-slab shape below 8192 rows")


WGRAD_SHAPES = [(37, 8, 16), (513, 136, 72)]


@pytest.mark.parametrize("case", ["small", "ragged", "multi_slab"])
def test_weight_gradient_gemms(case):
    hip = H()
    if case == "multi_slab":
        n, k = 136, 72
        m = _multi_slab_m(hip, n, k)
        assert hip.lib().tramba_wgrad_workspace(m, n, k, 1, 1) >= 2 * (n * k + n) * 4        # the multi-slab path
        assert m > 513 and hip.lib().tramba_wgrad_workspace(m - 64, n, k, 1, 1) == (n * k + n) * 4
    else:
        m, n, k = WGRAD_SHAPES[0 if case == "small" else 1]
        assert hip.lib().tramba_wgrad_workspace(m, n, k, 1, 1) == (n * k + n) * 4            # a single slab
    gy, x = rnd(20, m, n, dtype=BF16), rnd(21, m, k, dtype=BF16)
    ggy, gx = rnd(22, 2, 3, m, 8, dtype=BF16), rnd(23, 2, 3, m, 16, dtype=BF16)
    a, xs = rnd(24, m, 8, dtype=BF16), rnd(25, 3, m, 16, dtype=BF16)
    segs = [(n - 8, 8), (0, 8)]

    def run():
        out = []
        for want_bias in (False, True):
            out += list(hip.wgrad_cl(gy, x, want_bias=want_bias))
        out += [hip.wgrad_rows_cl(gy, x, segs), hip.wgrad_grouped_cl(ggy, gx), hip.tn_shared_cl(a, xs)]
        with hip.deferred_sums():
            late = list(hip.wgrad_cl(gy, x, want_bias=True, defer=True)) + [hip.wgrad_rows_cl(gy, x, segs, defer=True),
                                                                           hip.wgrad_grouped_cl(ggy, gx, defer=True)]
        return out + late
    bc.check_independent(run, what=f"wgrad {case} m={m}")


@pytest.mark.parametrize("m,n,k", [(37, 5, 16), (513, 61, 72), (130, 8, 512)])
def test_rows_gemm_writes_its_columns_only(m, n, k):
    """payload: columns :n of y.  The columns behind them are not rows_gemm_cl's: in the SS2D backward they are the B / C / pad
    columns of g_seq, written by ss2d_bwd_prep before it (checked in test_ss2d_backward_pieces) -- so they must come back
    untouched, which the test checks by handing in a marked table"""
    hip = H()
    ldy = (n + 7) // 8 * 8 + 4
    x, w = rnd(26, 4, m, k, dtype=BF16), rnd(27, 2, n, k, dtype=BF16)

    def run():
        y = torch.full((4, m, ldy), 7.0, device=DEV)
        return hip.rows_gemm_cl(x, w, y, n)
    base = bc.check_independent(run, what="rows_gemm")
    assert bool((base[0][..., n:] == 7.0).all())


LINEAR_SHAPES = [(37, 5, 16), (513, 130, 72), (64, 1, 128)]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("m,n,k", LINEAR_SHAPES)
def test_linear(m, n, k, dtype):
    hip = H()
    x, w, res = rnd(28, m, k, dtype=dtype), rnd(29, n, k, dtype=dtype, scale=k ** -0.5), rnd(30, m, n, dtype=dtype)
    bias = rnd(31, n)
    bc.check_independent(lambda: [hip.linear_cl(x, w), hip.linear_cl(x, w, bias, res, hip.ACT_GELU),
                                  hip.linear_cl(x, w, bias, out_dtype=F32)], what=f"linear {(m, n, k)}")


@pytest.mark.parametrize("m,n,k", [(37, 8, 64), (513, 136, 128), (64, 8, 128)])
def test_fused_linears(m, n, k):
    hip = H()
    x, w = rnd(32, m, k, dtype=BF16), rnd(33, n, k, dtype=BF16, scale=k ** -0.5)
    x2, w2 = rnd(34, m, 64, dtype=BF16), rnd(35, n, k + 64, dtype=BF16, scale=k ** -0.5)
    bias, colsum = rnd(36, n), w.float().sum(1).contiguous()
    bc.check_independent(lambda: [hip.linear2_cl(x, x2, w2, bias, act=hip.ACT_SILU), hip.linear_ln_cl(x, w, colsum, bias, 1e-5),
                                  *hip.linear_dual_cl(x, w, bias, hip.ACT_GELU)], what=f"fused linears {(m, n, k)}")


FORCED_RAGGED = (100, 520, 64)       # pointwise_cases.GEMM_SHAPES["ragged"]: one 64-deep K step, ragged last row and column tiles
WS_SHAPES = [(100, 128, 128), (100, 256, 128), (100, 128, 256)]       # NCW 1, 2 at K = 128, NCW 1 at K = 256


@pytest.mark.parametrize("form", [7, 13, 14, 16, 17, 18])
def test_gemms_under_every_forced_form(form):
    """the TUNE_GEMM_TILE values test_gpu_pointwise.test_gemm_epilogues_of_every_forced_form forces, each at the smallest shape
    gemm_plan (csrc/linear.hip) honours it on with a ragged tail: the LDS-DMA (7, 13, 14) and producer / consumer (16, 17)
    forms and the rule without PC / WS (18) run wherever K % 64 == 0, so M = 100, N = 520, K = 64 serves all six.  The knob also
    steers linear_ln_cl and linear_dual_cl (7 leaves those two on their rule: they have no 4-stage kernel)."""
    import pointwise_cases as pc
    hip = H()
    assert form in pc.GEMM_FORMS and pc.GEMM_SHAPES["ragged"] == FORCED_RAGGED
    m, n, k = FORCED_RAGGED
    x, w, bias = rnd(37, m, k, dtype=BF16), rnd(38, n, k, dtype=BF16, scale=k ** -0.5), rnd(39, n)
    res, colsum = rnd(40, m, n, dtype=BF16), w.float().sum(1).contiguous()

    def run():
        try:
            hip.tune_set(hip.TUNE_GEMM_TILE, form)
            return [hip.linear_cl(x, w, bias, res, hip.ACT_SILU), hip.linear_cl(x, w, out_dtype=F32),
                    hip.linear_ln_cl(x, w, colsum, bias, 1e-5, res, hip.ACT_GELU), *hip.linear_dual_cl(x, w, bias, hip.ACT_GELU)]
        finally:
            hip.tune_set(hip.TUNE_GEMM_TILE, 0)
    bc.check_independent(run, what=f"GEMMs under form {form}")


@pytest.mark.parametrize("m,n,k", WS_SHAPES)
def test_gemms_on_the_weight_stationary_form(m, n, k):
    """TUNE_GEMM_TILE 19 reaches linear_ws_kernel only where ws_ncw() (csrc/linear.hip) is non-zero and M >= 64: K = 128 or
    256, N a multiple of 128, output in the input dtype, act NONE / GELU / SiLU.  The smallest such shapes with a ragged last
    32-row tile: M = 100 (three whole tiles and four rows), N = 128 and 256 at K = 128 (one and two column blocks per wave), N = 128
    at K = 256; with and without a residual (two instantiations), and the LayerNorm-folded and dual-output entries, which
    the knob steers too.  Below, the same calls with an fp32 output or a sigmoid gate, which gemm_plan sends to the rule."""
    hip = H()
    assert k in (128, 256) and n % 128 == 0 and m >= 64 and m % 32
    x, w, bias = rnd(88, m, k, dtype=BF16), rnd(89, n, k, dtype=BF16, scale=k ** -0.5), rnd(90, n)
    res, colsum = rnd(91, m, n, dtype=BF16), w.float().sum(1).contiguous()

    def run():
        try:
            hip.tune_set(hip.TUNE_GEMM_TILE, 19)
            return [hip.linear_cl(x, w), hip.linear_cl(x, w, bias, act=hip.ACT_GELU), hip.linear_cl(x, w, bias, res, hip.ACT_SILU),
                    hip.linear_ln_cl(x, w, colsum, bias, 1e-5, act=hip.ACT_GELU), hip.linear_ln_cl(x, w, colsum, bias, 1e-5, res),
                    *hip.linear_dual_cl(x, w, bias, hip.ACT_SILU),
                    hip.linear_cl(x, w, bias, out_dtype=F32), hip.linear_cl(x, w, bias, res, hip.ACT_SIGMOID_GATE)]
        finally:
            hip.tune_set(hip.TUNE_GEMM_TILE, 0)
    bc.check_independent(run, what=f"weight-stationary GEMMs {(m, n, k)}")


@pytest.mark.parametrize("fam", ["raster", "helix"])
@pytest.mark.parametrize("h", [5, 12])
def test_cross_scan_and_merge(fam, h):
    """the boundary ops of the plugin path: (B, C, H, W) -> (B, K, C, L) and back"""
    hip = H()
    order = hip.scan_order(fam, h, h, torch.device(DEV))
    for dtype in (F32, BF16):
        x, ys = rnd(76, 2, 5, h, h, dtype=dtype), rnd(77, 2, order.k, 5, h * h, dtype=dtype)
        bc.check_independent(lambda: [hip.cross_scan(x, order), hip.cross_merge(ys, order)], what=f"cross scan {fam} {h}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_norm_heads(dtype):
    """shuffle_norm_head_cl and (16-bit) expand_norm_head_cl: one fp32 logit per shuffled pixel"""
    hip = H()
    c, p = 16, 4
    x = rnd(78, 2, 5, 7, p * p * c, dtype=dtype)
    lw, lb, hw = rnd(79, c) * 0.1 + 1, rnd(80, c) * 0.1, rnd(81, c)
    bc.check_independent(lambda: hip.shuffle_norm_head_cl(x, lw, lb, hw, 0.25, p), what="shuffle_norm_head")
    if dtype != F32:
        xe, we = rnd(82, 2, 5, 7, 64, dtype=dtype), rnd(83, p * p * 128, 64, dtype=dtype, scale=0.125)
        l128w, l128b, h128 = rnd(84, 128) * 0.1 + 1, rnd(85, 128) * 0.1, rnd(86, 128)
        bc.check_independent(lambda: hip.expand_norm_head_cl(xe, we, l128w, l128b, h128, -0.5, p), what="expand_norm_head")


@pytest.mark.parametrize("shift", [0, 6])
def test_attention_and_its_backward(shift):
    """window and key-value attention at the shapes of tests/golden/attn_blocks.py (24 x 24 map, window 12; 576 queries on 144
    keys), forward and backward, with and without the table gradient (whose partial bins are the workspace)"""
    hip = H()
    qkv, dy = rnd(70, 1, 24, 24, 3 * 128, dtype=BF16), rnd(71, 1, 24, 24, 128, dtype=BF16)
    table = rnd(72, 23 * 23, 4) * 0.1
    q, kv, dq = rnd(73, 2, 576, 128, dtype=BF16), rnd(74, 2, 144, 256, dtype=BF16), rnd(75, 2, 576, 128, dtype=BF16)

    def run():
        return [hip.window_attention_cl(qkv, table, 12, shift, 4), *hip.window_attention_bwd_cl(qkv, table, dy, 12, shift, 4),
                hip.window_attention_bwd_cl(qkv, table, dy, 12, shift, 4, need_table=False)[0],
                hip.kv_attention_cl(q, kv, 2), *hip.kv_attention_bwd_cl(q, kv, dq, 2)]
    bc.check_independent(run, what=f"attention shift {shift}")


SS2D_CASES = [("raster", 5, 5, 1), ("raster", 12, 24, 3), ("raster", 12, 40, 8), ("helix", 5, 24, 8), ("helix", 12, 5, 1),
              ("helix", 12, 40, 3)]


def _ss2d(fam, h, d, r, dtype):
    c = smc.make("existing", fam, h, 2, d, r, dtype)
    return c, smc._device(H(), c, torch.device(DEV))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fam,h,d,r", SS2D_CASES)
def test_ss2d_forward(fam, h, d, r, dtype):
    """segmented and chained, with and without `states`; the merges.  Of the states buffer the payload is what
    test_ss2d_saved_states_equal_the_recomputed_ones reads through the backward: the state entering each of the ceil(L / 32)
    tiles (the 8 tiles of slack behind them are the backward's own scratch)"""
    hip = H()
    c, (order, x, xdbl, gym, par) = _ss2d(fam, h, d, r, dtype)
    ntile = (c.l + 31) // 32
    lw, lb = rnd(41, d) * 0.1 + 1, rnd(42, d) * 0.1

    def run():
        ys = hip.ss2d_scan_cl(x, xdbl, order, *par, dtype)
        yc = hip.ss2d_scan_cl(x, xdbl, order, *par, dtype, segmented=False)
        st = hip.ss2d_scan_states(x, order)
        yst = hip.ss2d_scan_cl(x, xdbl, order, *par, dtype, states=st)
        tiles = st.view(F32).view(c.b, c.k, ntile + 8, d)[:, :, :ntile]
        return [ys, yc, yst, tiles, hip.ss2d_merge_sum_cl(ys, order, dtype), hip.ss2d_merge_norm_cl(ys, order, lw, lb, 1e-5, hip.ACT_GELU, dtype),
                hip.ss2d_merge_grad_cl(ys, order, gym, x)]
    bc.check_independent(run, what=f"ss2d forward {fam} {h} {d} {r}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fam,h,d,r", SS2D_CASES)
def test_ss2d_backward_pieces(fam, h, d, r, dtype):
    """ss2d_scan_bwd_cl with bc_partials (recomputing and from saved states), ss2d_bwd_prep, rows_gemm_cl into its rank
    columns, ss2d_bwd_assemble.  ss2d_bwd_prep's payload is `ranks` in full and columns R8 .. R8 + 3 of g_seq; the rank
    columns are rows_gemm_cl's: :R is checked after it, and R .. R8 -- which nobody writes -- must not reach the assembled
    gradient (ss2d_bwd_assemble's live mask), which is checked in full"""
    hip = H()
    c, (order, x, xdbl, gym, par) = _ss2d(fam, h, d, r, dtype)
    r8, rg = c.rg - 4, c.rg
    cd = BF16 if dtype == F32 else dtype
    dtw_t = par[0].transpose(1, 2).contiguous().to(cd)

    def run():
        st = hip.ss2d_scan_states(x, order)
        hip.ss2d_scan_cl(x, xdbl, order, *par, dtype, states=st)
        with_st = hip.ss2d_scan_bwd_cl(x, xdbl, order, *par, gym, states=st, bc_partials=True)
        gu, graw, bpart, cpart, gpar = hip.ss2d_scan_bwd_cl(x, xdbl, order, *par, gym, bc_partials=True)
        ranks, gseq = hip.ss2d_bwd_prep(xdbl, order, bpart, cpart, r, cd)
        prep = [ranks, gseq[..., r8:].clone()]
        if d % 8 == 0:
            hip.rows_gemm_cl(graw.to(cd).view(c.b * c.k, c.l, d), dtw_t, gseq.view(c.b * c.k, c.l, rg), r)
        else:                                     # (rows_gemm_cl takes K % 8 == 0: the rank columns are filled by hand)
            gseq[..., :r] = 1.0
        return list(with_st) + [gu, graw, bpart, cpart, gpar] + prep + [gseq[..., :r].clone(), gseq[..., r8:].clone(),
                                                                         hip.ss2d_bwd_assemble(gseq, order, r, dtype)]
    bc.check_independent(run, what=f"ss2d backward {fam} {h} {d} {r}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["zeroed", "g_seq"])
@pytest.mark.parametrize("fam,h,d,r", [("raster", 12, 40, 3), ("helix", 5, 24, 8)])
def test_ss2d_backward_with_atomic_b_and_c(fam, h, d, r, mode, dtype):
    """ss2d_scan_bwd_cl without bc_partials adds gB / gC with float atomics: gu, graw and gpar are held bit for bit, gB and gC
    to the tolerance of test_ss2d_core_training_gradients (5e-4 of the largest entry in fp32, 5e-2 in bf16) against the fp64
    gradients of the oracle's selective scan on the gathered operands (scan_memory_cases.reference_bwd)"""
    hip = H()
    c, (order, x, xdbl, gym, par) = _ss2d(fam, h, d, r, dtype)
    want = smc.reference_bwd(c)
    rel = 5e-4 if dtype == F32 else 5e-2

    def run():
        g_seq = torch.zeros((c.b, c.k, c.l, c.rg), device=DEV) if mode == "g_seq" else None
        gu, graw, gB, gC, gpar = hip.ss2d_scan_bwd_cl(x, xdbl, order, *par, gym, g_seq=g_seq)
        return [gu, graw, gpar, gB.contiguous(), gC.contiguous()]

    def close(ts):
        for name, got in zip(("gB", "gC"), ts):
            w = want[name]
            err = float((got.double() - w).abs().max()) / (float(w.abs().max()) + 1e-12)
            print(f"{fam} {h} {d} {r} {mode} {dtype} {name}: {err:.3e} of {rel:.0e}")
            assert err < rel, (name, err)
    bc.check_independent(run, payload=lambda t: t[:3], what="ss2d_scan_bwd, exact part")
    bc.check_independent(run, payload=lambda t: t[3:], exact=False, close=close, what="ss2d_scan_bwd, gB / gC")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_ss2d_core_with_atomic_b_and_c(dtype):
    """modules._SS2DCoreCL (the training path of a custom-merge SS2D): forward, atomic gB / gC, the rank projections and their
    scratch, the inverse permutation.  Only the B / C columns of the x_dbl gradient come from float atomics: the merged
    output, the gradients of x, dt_w, dt_bias, A and D and the rank columns of the x_dbl gradient are held bit for bit, the
    x_dbl gradient as a whole to test_ss2d_core_training_gradients' bound against its fp64 restatement of the graph.  Every run
    builds a ScanOrder of its own (not the cached one the process shares), so that its index tables are allocated under
    every fill and no cache is touched"""
    from tramba_amd import modules as M
    from test_gpu_kernels import _ref_core_fp64
    hip = H()
    fam, h, d, r, b = "window", 24, 40, 3, 1
    dev = torch.device(DEV)
    table = hip.scan_order(fam, h, h, dev).table.cpu()
    k, l, rg = table.shape[0], h * h, hip.ss2d_group_stride(r)
    g = torch.Generator().manual_seed(h * d + r)
    x = torch.randn(b, l, d, generator=g).to(dtype)
    xdbl = torch.zeros(b, l, k, rg)
    xdbl[..., :r] = 0.5 * torch.randn(b, l, k, r, generator=g)
    xdbl[..., rg - 4:rg - 2] = torch.randn(b, l, k, 2, generator=g)
    xdbl = xdbl.view(b, l, k * rg)
    dt_w = torch.randn(k, d, r, generator=g) * r ** -0.5
    dt_b = torch.randn(k, d, generator=g) * 0.5 - 1.0
    a_neg = -(torch.rand(k, d, generator=g) * 0.8 + 0.2)
    ds = 1 + 0.1 * torch.randn(k, d, generator=g)
    gym = torch.randn(b, l, d, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (x.float(), xdbl, dt_w, dt_b, a_neg, ds)]
    ymr = _ref_core_fp64(leaves[0], leaves[1], table, leaves[2], leaves[3], leaves[4], leaves[5], r)
    ymr.backward(gym.double())
    want = [ymr.detach()] + [t.grad for t in leaves]
    f32 = dtype == F32
    rels = [2e-4 if f32 else 2e-2, 3e-4 if f32 else 3e-2] + [5e-4 if f32 else 5e-2] * 5

    def run():
        order = hip.ScanOrder(fam, h, h, 0, dev)
        assert not hasattr(order, "_flat_inverse") and torch.equal(order.table.cpu(), table)
        dl = [x.to(dev).requires_grad_(True), xdbl.to(dev).requires_grad_(True), dt_w.to(dev).requires_grad_(True),
              dt_b.reshape(-1).to(dev).requires_grad_(True), a_neg.reshape(-1).to(dev).requires_grad_(True),
              ds.reshape(-1).to(dev).requires_grad_(True)]
        ym = M._SS2DCoreCL.apply(*dl, order)
        ym.backward(gym.to(dev))
        return [ym.detach()] + [t.grad for t in dl]

    def exact_part(ts):
        gxdbl = ts[2].view(b, l, k, rg)
        return [ts[0], ts[1], gxdbl[..., :r].contiguous()] + list(ts[3:])

    def close(ts):
        got, w, rel = ts[0], want[2], rels[2]
        err = float((got.double().reshape(w.shape) - w).abs().max()) / (float(w.abs().max()) + 1e-12)
        assert err < rel, (tuple(w.shape), err, rel)
    bc.check_independent(run, payload=exact_part, what="_SS2DCoreCL, exact part")
    bc.check_independent(run, payload=lambda ts: [ts[2]], exact=False, close=close, what="_SS2DCoreCL, x_dbl gradient")
    for got, w, rel in zip(run(), want, rels):                        # and the whole of it against the fp64 graph, once
        err = float((got.double().cpu().reshape(w.shape) - w).abs().max()) / (float(w.abs().max()) + 1e-12)
        assert err < rel, (tuple(w.shape), err, rel)


SCAN_SHAPES = [(2, 2, 3, 1, 37), (1, 2, 3, 4, 1000), (1, 4, 4, 16, 1153), (2, 2, 3, 16, 37), (1, 2, 3, 1, 1153), (1, 2, 3, 16, 1000)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SCAN_SHAPES)
def test_selective_scan(shape, dtype):
    """selective_scan_fwd (output and checkpoints) and du / ddelta of selective_scan_bwd bit for bit; dA, dB, dC, dD, dbias
    are added with float atomics: every run within test_selective_scan_bwd's bound (max |err| / max(1, max |want|) < 3e-4)
    of the fp64 oracle"""
    hip = H()
    a, dout, want = sdc.bwd_case(shape, dtype)
    g = {k_: v.to(DEV) for k_, v in a.items()}
    dd = dout.to(DEV)

    def run():
        out, ckpt = hip.selective_scan_fwd(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["delta_bias"], True, True)
        out2, _ = hip.selective_scan_fwd(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["delta_bias"], True, False)
        grads = hip.selective_scan_bwd(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["delta_bias"], dd, ckpt, True)
        return [out, ckpt, out2] + list(grads)

    def close(ts):
        for name, got, w in zip(sdc.GRADS[2:], ts, want[2:]):
            err = sdc.grad_error(got, w)
            assert err < 3e-4, (name, err)
    bc.check_independent(run, payload=lambda t: t[:5], what=f"selective scan {shape}, exact part")
    bc.check_independent(run, payload=lambda t: t[5:], exact=False, close=close, what=f"selective scan {shape}, atomic sums")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", [3, 5])
def test_im2col_and_back(c, stride, dtype):
    """the whole of `cols` is payload, alignment columns included: the docstring promises zeros there"""
    hip = H()
    for h in (5, 6):
        x = rnd(43 + h, 2, h, h, c, dtype=dtype)
        ckp = (9 * c + 7) // 8 * 8
        assert ckp > 9 * c
        ho = (h + 2 - 3) // stride + 1
        gcols = rnd(44 + h, 2 * ho * ho, ckp, dtype=dtype)

        def run():
            cols = hip.im2col3x3_cl(x, stride, 1, ckp)
            assert bool((cols[:, 9 * c:] == 0).all())
            return [cols, hip.col2im3x3_cl(gcols, (2, h, h, c), stride, 1)]
        bc.check_independent(run, what=f"im2col c {c} stride {stride} h {h}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,c", [(24, 16), (24, 32), (48, 16), (48, 32)])
def test_dct_split_and_its_backward(n, c, dtype):
    from tramba_amd import modules as M
    xs = rnd(45, 2, n, n, c, dtype=dtype)
    gh, gl = rnd(46, 2, n // 2, n // 2, c, dtype=dtype), rnd(47, 2, n // 2, n // 2, c, dtype=dtype)

    def run():
        w = M._dct_filter(n).to(DEV)              # a table of its own per run: its 16-bit pieces are cached by address
        x = xs.clone().requires_grad_()
        high, low = M._DCTSplitCL.apply(x, w, w)
        gx, = torch.autograd.grad([high, low], [x], [gh, gl])
        return [high.detach(), low.detach(), gx]
    bc.check_independent(run, what=f"dct {n} {c}")


def test_upsample_bilinear_backward():
    hip = H()
    for (h, w), (hh, ww) in (((7, 9), (37, 45)), ((1, 1), (16, 16)), ((12, 15), (37, 45))):
        gout = rnd(48 + h, 2, 1, hh, ww)
        bc.check_independent(lambda: hip.upsample_bilinear_bwd(gout, h, w), what=f"upsample_bwd {(h, w)}")


@pytest.mark.parametrize("c", [8, 72])
@pytest.mark.parametrize("m", [130, 300])
def test_batchnorm(m, c):
    """one and two row runs; work rows padded to 64 floats"""
    hip = H()
    assert hip.bn_parts(m, c) == (1 if m == 130 else 2) and hip.bn_work_floats(m, c) % 64 == 0
    x, dy, res = rnd(49, m, c, dtype=BF16), rnd(50, m, c, dtype=BF16), rnd(51, m, c, dtype=BF16)
    gamma, beta = rnd(52, c) * 0.1 + 1, rnd(53, c) * 0.1

    def run():
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        mean, rstd = hip.bn_stats_cl(x, 1e-5, rm, rv)
        y = hip.bn_act_cl(x, mean, rstd, gamma, beta, res, relu=True)
        return [mean, rstd, rm, rv, y] + list(hip.bn_act_bwd_cl(dy, x, y, mean, rstd, gamma, relu=True, want_dres=True))
    bc.check_independent(run, what=f"batchnorm {m} {c}")


def test_maxpool_and_its_backward():
    hip = H()
    for h, w, c in ((5, 6, 8), (24, 24, 64), (1, 1, 8)):
        x = rnd(54 + h, 2, h, w, c, dtype=BF16)
        gy = rnd(55 + h, 2, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=BF16)
        bc.check_independent(lambda: [hip.maxpool3s2_cl(x), hip.maxpool3s2_bwd_cl(gy, x)], what=f"maxpool {(h, w, c)}")


@pytest.mark.parametrize("n", [1024, 1026, 7])
def test_slab_sum(n):
    """immediate and deferred; n % 4 != 0 takes the framework's sum"""
    hip = H()
    part = rnd(56, 5, n)

    def run():
        with hip.deferred_sums():
            late = hip.slab_sum(part, defer=True)
        return [hip.slab_sum(part), late]
    bc.check_independent(run, what=f"slab_sum {n}")


def test_stems_and_strided_convs():
    """each at the smallest cfg of its own test: conv3x3s2_cl (2, 12, 12, 64) -> 40 channels (test_conv3x3s2_cl),
    stem_conv_ln_gelu on (2, 3, 24, 24) (test_stem_conv_ln_gelu), patch_embed_ln on PVT's (2, 3, 21, 30) and Swin's (2, 3, 24, 24)
    (test_gpu_conv.EMBED_CASES), stem7_affine_relu_pool on (2, 3, 18, 22) (test_gpu_resnet_conv.STEM_CASES)"""
    hip = H()
    x64 = rnd(58, 2, 12, 12, 64, dtype=BF16)
    w3, b40 = rnd(59, 40, 9 * 64, dtype=BF16, scale=0.05), rnd(60, 40)
    img24, img_pvt, img_stem = rnd(57, 2, 3, 24, 24), rnd(92, 2, 3, 21, 30), rnd(93, 2, 3, 18, 22)
    ws, bs, lw, lb = rnd(61, 64, 3, 3, 3, scale=0.2), rnd(62, 64) * 0.1, rnd(63, 64) * 0.1 + 1, rnd(64, 64) * 0.1
    w7, w4 = rnd(65, 64, 3, 7, 7, scale=0.1), rnd(66, 128, 3, 4, 4, scale=0.1)
    l128w, l128b, b128 = rnd(67, 128) * 0.1 + 1, rnd(68, 128) * 0.1, rnd(69, 128) * 0.1

    def run():
        return [hip.conv3x3s2_cl(x64, w3, b40), hip.stem_conv_ln_gelu(img24, ws, bs, lw, lb, 1e-5, BF16),
                hip.patch_embed_ln(img_pvt, w7, bs, lw, lb, 1e-5, 4, 3, BF16), hip.patch_embed_ln(img24, w4, b128, l128w, l128b, 1e-5, 4, 0, BF16),
                hip.stem7_affine_relu_pool(img_stem, w7, lw, lb, BF16)]
    bc.check_independent(run, what="stems")


# ============================================================================= C. persistent workspaces, stale contents
@pytest.mark.parametrize("which", ["forward", "backward"])
def test_scan_workspace_across_shapes(which):
    """a workspace allocated under poison (a new stream gives _scan_workspace a new key), then shape S1, S2 (larger batch,
    other L and D: another layout of the same bytes), S1 again: the second S1 equals the first and the unpatched run"""
    hip = H()
    dev = torch.device(DEV)
    c1 = smc.make("existing", "raster", 12, 1, 24, 3, BF16)
    c2 = smc.make("existing", "helix", 16, 3, 40, 8, BF16, seed=1)
    smc._device(hip, c1, dev), smc._device(hip, c2, dev)

    def one(c):
        order, x, xdbl, gym, par = c.dev
        if which == "forward":
            return [hip.ss2d_scan_cl(x, xdbl, order, *par, c.dtype)]
        return list(hip.ss2d_scan_bwd_cl(x, xdbl, order, *par, gym, bc_partials=True))
    base = [t.cpu() for t in one(c1)]
    torch.cuda.synchronize()
    for fill in bc.FILLS:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with bc.poisoned_allocations(fill) as st:
                first = one(c1)
                one(c2)
                second = one(c1)
            stream.synchronize()
        bc.HIT.update(st.device_sites)
        if which == "forward":
            assert ("hip.py", _line("hip.py", "ws = _scan_ws[key] = torch.empty")) in st.device_sites      # a fresh workspace
        for a, b_, u in zip(first, second, base):
            assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b_) and torch.equal(a.cpu(), u), (which, fill)
        torch.cuda.current_stream().wait_stream(stream)


def _line(fname, frag):
    hits = [k[1] for k, s in bc.SITE_LINES.items() if k[0] == fname and frag in s]
    assert len(hits) == 1, (fname, frag, hits)
    return hits[0]


def test_augment_workspace_across_batches():
    """a workspace allocated under poison, then batch 8, batch 3, batch 8: the second batch of 8 equals the first and the
    unpatched result.  augment keeps one workspace per (output size, device): a size per fill that nothing else in the suite
    uses gives each fill an allocation of its own, whatever ran before"""
    site = ("augment.py", _line("augment.py", "_workspace[key] = torch.empty"))
    for size, fill in zip((96, 104, 112), bc.FILLS):
        s8, s3 = _aug_samples(size, 8, seed=5), _aug_samples(size, 3, seed=6)
        with bc.poisoned_allocations(fill) as st:
            first = [t.cpu() for t in _aug_run(s8, size)]
            _aug_run(s3, size)
            second = [t.cpu() for t in _aug_run(s8, size)]
        bc.HIT.update(st.device_sites)
        assert site in st.device_sites, "the workspace was not allocated anew"
        base = [t.cpu() for t in _aug_run(s8, size)]
        for a, b_, u in zip(first, second, base):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b_) and torch.equal(a, u), fill


class _TinyNet(torch.nn.Module):
    """(B, 3, S, S) -> [(B, 1, S, S)]: three weights, no framework library behind it (nothing to tune under capture)"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, -0.25, 1.0]).view(1, 3, 1, 1))

    def forward(self, x):
        return [(x * self.w).sum(1, keepdim=True)]


def test_frame_predictor_static_buffers():
    """the graphs' static buffers are allocated under poison (allocations made while the stream captures are passed through
    unfilled); the first replay equals the eager result byte for byte, as test_gpu_frames.py defines equal"""
    from tramba_amd import infer
    model = _TinyNet().to(DEV).eval()
    frames = [_frame(h, w, 3 * h + w) for h, w in FRAME_SIZES]
    uni = np.stack([_frame(37, 53, i) for i in range(2)])
    eager = infer.FramePredictor(model, 48, graph=False)
    want = [m.cpu() for m in eager(frames)]
    want_u = eager(uni).cpu()
    for fill in bc.FILLS:
        with bc.poisoned_allocations(fill) as st:
            graphed = infer.FramePredictor(model, 48, graph=True, strict=True)
            got = [m.cpu() for m in graphed(frames)]
            got_u = graphed(uni).cpu()
            again = [m.cpu() for m in infer.FramePredictor(model, 48, graph=False)(frames)]
        bc.HIT.update(st.device_sites)
        assert ("infer.py", _line("infer.py", "static_in = torch.empty(cap_in")) in st.device_sites
        assert len(got) == len(want) and all(torch.equal(a, b_) for a, b_ in zip(got, want)), fill
        assert all(torch.equal(a, b_) for a, b_ in zip(again, want)) and torch.equal(got_u, want_u), fill
        again2 = [m.cpu() for m in graphed(frames)]                     # a replay outside the context
        assert all(torch.equal(a, b_) for a, b_ in zip(again2, want)), fill


class _TinyTrain(torch.nn.Module):
    """a VSSBlock behind the interface train.train_step expects (test_gpu_model._TinyDP)"""

    def __init__(self):
        super().__init__()
        import tramba_amd as ta
        torch.manual_seed(11)
        self.encoder = ta.MultiScaleDecoderBlock(hidden_dim=32, drop_path=0.0, channel_first=True)
        self.compute_dtype = torch.bfloat16

    def forward(self, z):
        return [self.encoder(z).mean(dim=1, keepdim=True)]


def test_controlled_step_weight_shadows_and_packs():
    """two controlled steps (2 micro-batches, norm clipping) of a small block in bf16: the norm workspace of StepControl, the
    16-bit weight shadows and the standing depth-wise packs are all allocated under each fill; losses, weights and shadows
    equal those of the unpatched run, and every shadow equals the cast of its weight"""
    from tramba_amd import modules as M, train
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 24, 24, generator=g).to(DEV)
    y = (torch.rand(4, 1, 24, 24, generator=g) > 0.5).float().to(DEV)

    def run():
        model = _TinyTrain().to(DEV).train()
        opt = train.get_opt(1e-3, model)
        control = train.StepControl(accumulate=2, clip_norm=0.05, skip_nonfinite=True)
        losses = [train.train_step(model, opt, x, y, control=control).detach().clone() for _ in range(2)]
        shadows = []
        for p, kind in M._shadow_params(model):
            ent = M._lowp_shadow[id(p)]
            assert ent[1] == p._version
            if kind is None:
                w16 = p.detach().to(BF16)
                assert torch.equal(ent[0], w16) and torch.equal(ent[3], w16.t())
            shadows += [ent[0], ent[3]]
        return losses + [control.grad_norm.detach().clone()] + [p.detach() for p in model.parameters()] + shadows
    bc.check_independent(run, what="controlled step")


def test_graphed_controlled_step_built_under_poison():
    """GraphedTrainStep with a StepControl: the record's norm workspace, the shadows and the packs are allocated under each
    fill by one eager controlled step; the step is captured after the context is left, on those buffers, and its replays
    equal the eager steps as tests/test_gpu_e2e.py defines equal (first loss to 1e-5, the following ones to 3e-2)"""
    import tramba_amd as ta
    from tramba_amd import train
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 24, 24, generator=g).to(DEV)
    y = (torch.rand(4, 1, 24, 24, generator=g) > 0.5).float().to(DEV)
    make = lambda: train.StepControl(accumulate=2, clip_norm=0.05, skip_nonfinite=True)   # noqa: E731
    model = _TinyTrain().to(DEV).train()
    opt, control = train.get_opt(1e-3, model, capturable=True), make()
    eager = [float(train.train_step(model, opt, x, y, control=control)) for _ in range(4)]
    for fill in bc.FILLS:
        with bc.poisoned_allocations(fill) as st:
            model = _TinyTrain().to(DEV).train()
            opt, control = train.get_opt(1e-3, model, capturable=True), make()
            got = [float(train.train_step(model, opt, x, y, control=control))]
        bc.HIT.update(st.device_sites)
        assert ("train.py", _line("train.py", "self._workspace = torch.empty")) in st.device_sites
        workspace = control._workspace.data_ptr()
        step = ta.GraphedTrainStep(model, opt, control=control)
        got += [float(step(x, y)) for _ in range(3)]                     # capture and replays, outside the context
        assert control._workspace.data_ptr() == workspace                # the graph runs on the buffer made under poison
        assert int(control.skipped_steps) == 0 and all(np.isfinite(got)), (fill, got)
        assert got[:2] == pytest.approx(eager[:2], rel=1e-5) and np.allclose(got, eager, rtol=3e-2), (fill, got, eager)


def test_poison_reaches_the_device_buffers_of_the_library():
    """the harness itself on the device: a float workspace of the library comes back as NaN, a classified byte buffer as 0xFF
    bytes, an index buffer with its legal value, and each is recorded under its line"""
    hip = H()
    order = hip.scan_order("raster", 5, 5, torch.device(DEV))
    x = rnd(87, 1, 25, 8)
    with bc.poisoned_allocations("nan") as st:
        work, _ = hip._bn_workspace(130, 8, torch.device(DEV))
        states = hip.ss2d_scan_states(x, order)
        idx, dist2 = hip.feature_transform(torch.zeros(1, 3, 3, dtype=torch.bool, device=DEV))
    assert bool(torch.isnan(work).all()) and bool((states == 0xFF).all())
    assert bool((idx == -1).all()) and bool((dist2 == -1).all())            # an empty mask: written by the kernels
    assert {("hip.py", _line("hip.py", "return torch.empty(nbytes // 4")),
            ("hip.py", _line("hip.py", "return torch.empty(lib().tramba_ss2d_scan_bwd_workspace"))} <= st.device_sites
    with bc.poisoned_allocations("zero"):
        with pytest.raises(RuntimeError, match="nest"):
            with bc.poisoned_allocations("nan"):
                pass


# ============================================================================= D. the coverage gate
def test_every_device_site_of_the_census_was_reached():
    """the union of the sites that allocated under poison in the cases above holds every device-memory site of the census
    (an `ast` walk over tramba_amd/*.py) but the reasoned exclusions of buffer_cases.EXCLUSIONS: a later change that adds an
    allocation adds a case, or an exclusion with its reason.  It reads what the other cases of this module recorded, so it
    runs with the whole module and as its last test."""
    missing = [s for s in bc.device_sites() if s not in bc.HIT]
    for f, line in missing:
        print(f"not reached: {f}:{line}  {bc.SITE_LINES[(f, line)]}")
    assert len(bc.EXCLUDED_SITES) <= bc.MAX_EXCLUSIONS
    assert not missing, f"{len(missing)} device sites were not reached under poison (run the whole module): {missing}"
