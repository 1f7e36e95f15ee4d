"""GPU tests of the forward's last register-staged launches moved onto the LDS-DMA tile (implicit-GEMM 3x3 / stride-2
convolution and two-source GEMM on linear_pc_kernel) and of the streaming merge's pixels per wave.  Each new route is held
bit for bit against the kernel it replaces (TRAMBA_TUNE_GEMM_TILE 18 / TRAMBA_TUNE_MERGE_PW 16) and against fp64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def hip():
    from tramba_amd import hip as h
    return h


class _tuned:
    """tune_set(knob, value) for the body, 0 again after it"""

    def __init__(self, *pairs):
        self.pairs = pairs

    def __enter__(self):
        for knob, value in self.pairs:
            hip().tune_set(knob, value)

    def __exit__(self, *exc):
        for knob, _ in self.pairs:
            hip().tune_set(knob, 0)


MODEL_CONVS = [(192, 64, 128), (96, 128, 256), (48, 256, 512), (24, 512, 1024)]     # (input side, Cin, Cout)
CONV_CASES = [(b, h, ci, co) for b in (4, 1) for h, ci, co in MODEL_CONVS] + [(1, 13, 64, 64), (2, 12, 64, 40), (1, 48, 256, 130)]


def _conv_operands(dtype, cfg):
    b, h, cin, cout = cfg
    g = torch.Generator().manual_seed(cin + cout + b)
    x = torch.randn(b, h, h, cin, generator=g).to(dtype)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).to(dtype)
    bias = torch.randn(cout, generator=g)
    return x, w, bias


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", CONV_CASES)
def test_conv_on_lds_dma_tile_matches_tiled_kernel_and_fp64(dtype, cfg):
    """tramba_conv3x3s2_cl under the rule (linear_pc_kernel<.., A_CONV>) == under knob 18 (linear_tiled_kernel<.., CONV>) bit for
    bit -- both run 64-deep K steps in (tap, cin) order through the same MFMA sequence and epilogue -- and both within
    test_conv3x3s2_cl's tolerance of F.conv2d in fp64."""
    H = hip()
    x, w, bias = _conv_operands(dtype, cfg)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(DEV)
    xd, bd = x.to(DEV), bias.to(DEV)
    new = H.conv3x3s2_cl(xd, wk, bd)
    with _tuned((H.TUNE_GEMM_TILE, 18)):
        old = H.conv3x3s2_cl(xd, wk, bd)
    torch.cuda.synchronize()
    assert new.shape == want.shape
    print(f"conv {cfg} {dtype}: max |new - old| = {float((new.float() - old.float()).abs().max()):.3e}, "
          f"max |new - fp64| = {float((new.cpu().double() - want).abs().max()):.3e}")
    np.testing.assert_allclose(new.cpu().double().numpy(), want.numpy(), rtol=2e-2, atol=2e-2)
    assert torch.equal(new, old)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [(2, 24, 64, 64), (1, 13, 128, 72), (3, 7, 64, 64), (1, 1, 64, 64), (1, 2, 64, 64)])
def test_conv_zero_padding_counts_taps(dtype, cfg):
    """A constant map of ones under an all-ones weight: every output equals Cin times the number of its taps that lie inside
    the map (4 / 6 / 9 at a corner / edge / inside, fewer on odd sizes' last row and on 1- and 2-pixel maps), exactly -- the
    sums are small integers.  A border tap read from a neighbouring pixel, row or image instead of as zero shows as a wrong
    count."""
    H = hip()
    b, h, cin, cout = cfg
    x = torch.ones(b, h, h, cin, dtype=dtype, device=DEV)
    wk = torch.ones(cout, 9 * cin, dtype=dtype, device=DEV)
    ho = (h + 1) // 2
    idx = torch.arange(ho)
    n1 = sum(((2 * idx - 1 + d >= 0) & (2 * idx - 1 + d < h)).long() for d in range(3))     # taps inside, per axis
    want = (cin * n1[:, None] * n1[None, :]).float()[None, :, :, None].expand(b, ho, ho, cout)
    got = H.conv3x3s2_cl(x, wk, torch.zeros(cout, device=DEV))
    with _tuned((H.TUNE_GEMM_TILE, 18)):
        old = H.conv3x3s2_cl(x, wk, torch.zeros(cout, device=DEV))
    assert torch.equal(got.float().cpu(), want.to(dtype).float())
    assert torch.equal(got, old)
    # and a map whose images differ, so that a tap that leaves one image for its neighbour is seen
    x2 = x * torch.arange(1, b + 1, device=DEV, dtype=dtype).view(b, 1, 1, 1)
    got2 = H.conv3x3s2_cl(x2, wk, torch.zeros(cout, device=DEV))
    want2 = want * torch.arange(1, b + 1).view(b, 1, 1, 1)
    assert torch.equal(got2.float().cpu(), want2.to(dtype).float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [(2304, 512, 512, 512), (9216, 256, 256, 256), (36864, 128, 128, 128), (576, 512, 512, 512),
                                 (300, 128, 64, 192), (1000, 72, 128, 64), (2304, 512, 2048, 1024)])
def test_two_source_gemm_on_lds_dma_tile_matches_lean_kernel(dtype, cfg):
    """tramba_linear2_cl under the rule (linear_pc_kernel<.., A_TWO>) == under knob 18 (linear_lean_kernel) bit for bit, with
    the bias / GELU / residual epilogue, an fp32 output and the sigmoid gate; the decoder's and the gate's shapes at batch 4
    and 1, ragged M / N, unequal parts and the 288-tile K >= 2048 case the plain rule gives to linear_dma_kernel."""
    m, n, k1, k2 = cfg
    H = hip()
    g = torch.Generator().manual_seed(m + n + k1)
    x1 = torch.randn(m, k1, generator=g).to(dtype).to(DEV)
    x2 = torch.randn(m, k2, generator=g).to(dtype).to(DEV)
    w = (torch.randn(n, k1 + k2, generator=g) * (k1 + k2) ** -0.5).to(dtype).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(m, n, generator=g).to(dtype).to(DEV)
    calls = [lambda: H.linear2_cl(x1, x2, w, bias, res, 2), lambda: H.linear2_cl(x1, x2, w, None, None, 0, torch.float32),
             lambda: H.linear2_cl(x1, x2, w, None, res, H.ACT_SIGMOID_GATE)]
    new = [c() for c in calls]
    with _tuned((H.TUNE_GEMM_TILE, 18)):
        old = [c() for c in calls]
    for a, b_ in zip(new, old):
        assert torch.equal(a, b_)
    xc = torch.cat((x1, x2), dim=-1)
    assert torch.equal(new[0], H.linear_cl(xc, w, bias, res, 2))
    want = torch.sigmoid(xc.double() @ w.double().T) * res.double()
    np.testing.assert_allclose(new[2].cpu().double().numpy(), want.cpu().numpy(), rtol=2e-2, atol=2e-2)


def test_two_source_split_off_the_k_step_keeps_its_old_route():
    """Parts that are not whole 64-deep K steps never reach tramba_linear2_cl (it rejects them, as before): Linear2d's
    concatenated forward takes the route it always took, and gives the concatenated GEMM's result."""
    from tramba_amd import modules
    H = hip()
    g = torch.Generator().manual_seed(3)
    lin = modules.Linear2d(96 + 160, 128, bias=True).to(DEV).to(torch.bfloat16).eval()
    x1 = torch.randn(1, 24, 24, 96, generator=g).to(torch.bfloat16).to(DEV)
    x2 = torch.randn(1, 24, 24, 160, generator=g).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        got = lin._forward_cat_cl(x1, x2)
        want = lin._forward_cl(torch.cat((x1, x2), dim=-1))
    assert torch.equal(got, want)
    w = lin.weight.detach().reshape(128, 256).contiguous()
    with pytest.raises(H.TrambaHipError):
        H.linear2_cl(x1.contiguous(), x2.contiguous(), w)
    ref = torch.cat((x1, x2), dim=-1).double() @ w.double().T + lin.bias.detach().double()
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.cpu().numpy(), rtol=2e-2, atol=2e-2)


def _merge_reference(ys, order, lw, lb):
    """fp64: per pixel the sum of its listed rows of (K*L, D), LayerNorm, GELU"""
    b, k, l, d = ys.shape
    ptr, idx = order.inv_ptr.long(), order.inv_idx.long()
    pix = torch.repeat_interleave(torch.arange(l, device=ys.device), ptr[1:l + 1] - ptr[:l])
    rows = ys.double().reshape(b, k * l, d)[:, idx[:pix.numel()]]
    y = torch.zeros(b, l, d, dtype=torch.float64, device=ys.device).index_add_(1, pix, rows)
    return F.gelu(F.layer_norm(y, (d,), lw.double(), lb.double(), 1e-5))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fam,b,h,d,form", [("raster", 4, 48, 512, 0), ("window", 4, 48, 512, 0), ("dilation", 4, 48, 512, 0),
                                            ("raster", 1, 96, 256, 0), ("window", 1, 96, 256, 0), ("dilation", 4, 96, 256, 0),
                                            ("helix", 4, 48, 512, 2), ("raster", 2, 14, 128, 2), ("helix", 1, 14, 96, 2)])
def test_streaming_merge_does_not_depend_on_pixels_per_wave(dtype, fam, b, h, d, form):
    """ss2d_merge_norm_stream_kernel at 4 / 8 / 16 pixels per wave (TRAMBA_TUNE_MERGE_PW) and under the rule: pairwise equal
    bit for bit (a pixel's sum order and its wave-local LayerNorm do not know how many pixels the wave holds), and within
    16-bit rounding of the fp64 merge.  form 2 forces the streaming form where the rule would not take it (Helix tables, and
    14 x 14 maps whose 196 pixels are no multiple of 8 or 16)."""
    H = hip()
    dev = torch.device(DEV)
    order = H.scan_order(fam, h, h, dev)
    k, l = order.k, h * h
    g = torch.Generator().manual_seed(h * d + k + b)
    ys = torch.randn(b, k, l, d, generator=g).to(dtype).to(dev)
    lw, lb = (1 + 0.1 * torch.randn(d, generator=g)).to(dev), (0.1 * torch.randn(d, generator=g)).to(dev)
    outs = {}
    for pw in (0, 4, 8, 16):
        with _tuned((H.TUNE_MERGE_FORM, form), (H.TUNE_MERGE_PW, pw)):
            outs[pw] = H.ss2d_merge_norm_cl(ys, order, lw, lb, 1e-5, 2, dtype)
    torch.cuda.synchronize()
    for pw in (4, 8, 16):
        assert torch.equal(outs[pw], outs[0]), pw
    want = _merge_reference(ys, order, lw, lb)
    np.testing.assert_allclose(outs[0].double().cpu().numpy(), want.cpu().numpy(), rtol=2e-2, atol=2e-2)


def test_merge_pw_knob_rejects_other_values():
    H = hip()
    dev = torch.device(DEV)
    order = H.scan_order("raster", 14, 14, dev)
    ys = torch.zeros(1, 4, 196, 64, dtype=torch.bfloat16, device=dev)
    lw, lb = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    with _tuned((H.TUNE_MERGE_PW, 5)):
        with pytest.raises(H.TrambaHipError, match="MERGE_PW"):
            H.ss2d_merge_norm_cl(ys, order, lw, lb, 1e-5, 2, torch.bfloat16)


def test_new_routes_beside_a_second_stream_are_bitwise_stable():
    """The convolution on the LDS-DMA loaders and the 4-pixel streaming merge, each beside a busy second stream (a GEMM and
    a 96 x 96 merge, as in test_two_stream_concurrency_is_bitwise_stable): every result equals the one computed alone."""
    H = hip()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(11)
    dtype = torch.bfloat16
    x, w, bias = _conv_operands(dtype, (4, 48, 256, 512))
    xd, bd = x.to(dev), bias.to(dev)
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(dev)
    order = H.scan_order("raster", 48, 48, dev)
    ys = torch.randn(4, 4, 48 * 48, 512, generator=g).to(dtype).to(dev)
    lw, lb = torch.ones(512, device=dev), torch.zeros(512, device=dev)
    ops = {"conv": lambda: H.conv3x3s2_cl(xd, wk, bd), "merge": lambda: H.ss2d_merge_norm_cl(ys, order, lw, lb, 1e-5, 2, dtype)}
    xs = torch.randn(1, 192, 192, 128, generator=g).to(dev)
    ws = (torch.randn(256, 128, generator=g) * 0.1).to(dev)
    order96 = H.scan_order("window", 96, 96, dev)
    ys96 = torch.randn(1, 4, 96 * 96, 256, generator=g).to(dev)
    l96w, l96b = torch.ones(256, device=dev), torch.zeros(256, device=dev)
    side_ops = [lambda: H.linear_cl(xs, ws, None, None, 2),
                lambda: H.ss2d_merge_norm_cl(ys96, order96, l96w, l96b, 1e-5, 2, torch.float32)]
    side = torch.cuda.Stream()
    with _tuned((H.TUNE_MERGE_PW, 4)):
        for name, op in ops.items():
            ref = op().clone()
            torch.cuda.synchronize()
            for sop in side_ops:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    keep = [sop() for _ in range(30)]
                outs = [op() for _ in range(10)]
                torch.cuda.synchronize()
                assert all(torch.equal(o, ref) for o in outs), name
                del keep
