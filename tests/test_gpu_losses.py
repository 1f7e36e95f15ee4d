"""GPU tests of the weighted losses (reference utils/loss.py:14-42: structure_loss, wbce) in the library: the weight map
against an fp64 avg_pool2d, values and gradients of both losses in both readings of the BCE term against fp64 autograd of a
restatement and against the reference's own results (tests/golden/golden_loss.npz), scaling, bitwise reproducibility, the
caller's weight tensor, what the bindings refuse, and the loss spec inside a captured training step."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases
import synth
from test_gpu_step_ends import LOSS_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"structure": (31, 0.001, True), "wbce": (15, 0.0, False)}


def _rel_l2(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-30))


def _weit(mask, k):
    return 1 + 5 * torch.abs(F.avg_pool2d(mask, kernel_size=k, stride=1, padding=k // 2) - mask)


def restated(kind, outs, mask, pixel, weight=None, loss_weights=None):
    """fp64 restatement of utils/loss.py:15-42 over deep-supervision outputs (each resized to the label, train.py:78-79):
    reduction='none' for the per-pixel reading, 'mean' for what the reference executes"""
    k, eps, iou = FORMS[kind]
    weit = _weit(mask, k) if weight is None else 1 + 5 * weight
    total = 0.0
    for i, o in enumerate(outs):
        if o.shape[-2:] != mask.shape[-2:]:
            o = F.interpolate(o, mask.shape[-2:], mode="bilinear")
        bce = F.binary_cross_entropy_with_logits(o, (1 - eps) * mask + eps / 2, reduction="none" if pixel else "mean")
        term = ((weit * bce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))).mean()
        if iou:
            p = torch.sigmoid(o)
            inter = ((p * mask) * weit).sum(dim=(2, 3))
            union = ((p + mask) * weit).sum(dim=(2, 3))
            term = term + (1 - (inter + 1) / (union - inter + 1)).mean()
        total = total + (term if loss_weights is None else loss_weights[i] * term)
    return total


def _label(tag, shape, soft):
    """hard: blobs (a weight map with structure, not noise); soft: the same edges blurred into [0, 1]"""
    hard = loss_cases._blob_label(tag, shape)
    if not soft:
        return hard.float()
    return (0.8 * F.avg_pool2d(hard, 5, 1, 2) + 0.2 * torch.sigmoid(synth.synth_input(tag + "_soft", shape).double())).float()


WMAP_SHAPES = {"training": (8, 1, 384, 384), "rect": (2, 1, 37, 45), "small": (2, 1, 16, 16), "one_pixel": (3, 1, 1, 1),
               "channels": (2, 3, 40, 52)}


@pytest.mark.parametrize("k", [31, 15])
@pytest.mark.parametrize("name", list(WMAP_SHAPES))
def test_weight_map_against_fp64(name, k):
    """0/1 labels: every box sum is an integer <= 961, exact in fp32 in any order -- what is left is the rounding of the
    division, of the product and of the result (<= 6): 1e-6 absolute.  Soft labels: fp32 sums of <= 961 terms in [0, 1],
    1e-5 relative (the map is >= 1)."""
    from tramba_amd import hip
    shape = WMAP_SHAPES[name]
    for soft in (False, True):
        lab = _label(f"wmap_{name}", shape, soft)
        if name == "one_pixel":
            lab = torch.tensor([0.0, 1.0, 0.25]).reshape(shape)
        want = _weit(lab.double(), k)
        got = hip.loss_weight_map(lab.to(DEV), k)
        assert got.shape == lab.shape and got.dtype == torch.float32
        err = (got.double().cpu() - want).abs()
        print(f"weight map {name} k={k} soft={soft}: max abs err {float(err.max()):.3e}, max rel {float((err / want).max()):.3e}")
        if soft:
            assert bool((err <= 1e-5 * want).all()), float((err / want).max())
        else:
            assert float(err.max()) <= 1e-6, float(err.max())
    # the largest window the kernel takes, and one larger than the image
    lab = _label("wmap_k63", (1, 2, 20, 70), False)
    got = hip.loss_weight_map(lab.to(DEV), 63)
    assert float((got.double().cpu() - _weit(lab.double(), 63)).abs().max()) <= 1e-6
    with pytest.raises(hip.TrambaHipError):
        hip.loss_weight_map(lab.to(DEV), 65)
    with pytest.raises(hip.TrambaHipError):
        hip.loss_weight_map(lab.to(DEV), 30)


@pytest.mark.parametrize("name", list(LOSS_CASES))
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("kind", ["structure", "wbce"])
@pytest.mark.parametrize("bce", ["reference", "pixel"])
def test_value_and_gradients_against_fp64(name, soft, kind, bce):
    """The bounds of test_loss_value_and_gradients_against_the_oracle: the weights rescale that arithmetic by at most 6."""
    from tramba_amd import train
    b, c, (hh, ww), sizes = LOSS_CASES[name]
    outs = [synth.synth_input(f"loss_{name}_{i}", (b, c, h, w), scale=3.0) for i, (h, w) in enumerate(sizes)]
    lab = _label(f"wloss_{name}", (b, c, hh, ww), soft)
    o64 = [o.double().requires_grad_() for o in outs]
    want = restated(kind, o64, lab.double(), bce == "pixel")
    want.backward()
    want = float(want.detach())
    od = [o.to(DEV).requires_grad_() for o in outs]
    got = train.SodLoss(kind, bce)(od, lab.to(DEV))
    assert got.dtype == torch.float32 and got.dim() == 0 and got.grad_fn is not None
    (got * 1.0).backward()
    errs = [_rel_l2(o.grad, ref.grad) for o, ref in zip(od, o64)]
    print(f"{kind}/{bce} {name} soft={soft}: loss {float(got.detach()):.8f} want {want:.8f} "
          f"err {abs(float(got.detach()) - want):.3e}, gradient rel L2 {['%.2e' % e for e in errs]}")
    assert abs(float(got.detach()) - want) < 2e-6 * max(1.0, abs(want)), (float(got.detach()), want)
    for i, (o, e) in enumerate(zip(od, errs)):
        assert o.grad.shape == o.shape
        assert e < 2e-5, (name, i, e)


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_the_reference_reading_against_the_reference(name):
    """structure_loss / wbce on the device against what the reference's own functions returned in fp64.  The golden holds
    the value, every 11th gradient element and the gradient's L2 norm: this is the comparison that is independent of this
    project's own restatement (bce="reference" only); every gradient element is compared in
    test_value_and_gradients_against_fp64, against the restatement that test_losses_host pins to the same golden."""
    from tramba_amd import train
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_loss.npz"))
    pred, mask, weight = loss_cases.case(name)
    for kind in ("structure",) if weight is not None else ("structure", "wbce"):
        p = pred.float().to(DEV).requires_grad_()
        m = mask.float().to(DEV)
        if kind == "structure":
            got = train.structure_loss(p, m, None if weight is None else weight.float().to(DEV))
        else:
            got = train.wbce(p, m)
        assert got.is_cuda and got.dtype == torch.float32
        want = float(gold[f"{kind}/{name}/value"])
        got.backward()
        d = loss_cases.digest(p.grad.cpu())
        ref = torch.from_numpy(gold[f"{kind}/{name}/grad_sample"])
        print(f"{kind} {name}: err {abs(float(got.detach()) - want):.3e}, gradient sample rel L2 {_rel_l2(d['sample'], ref):.2e}")
        assert abs(float(got.detach()) - want) < 2e-6 * max(1.0, abs(want))
        assert _rel_l2(d["sample"], ref) < 2e-5
        assert abs(d["norm"] - float(gold[f"{kind}/{name}/grad_norm"])) < 2e-5 * float(gold[f"{kind}/{name}/grad_norm"])


@pytest.mark.parametrize("kind,bce", [("structure", "reference"), ("structure", "pixel"), ("wbce", "pixel")])
def test_loss_weights_and_incoming_gradient(kind, bce):
    from tramba_amd import train
    outs = [synth.synth_input(f"lossw_{i}", (2, 1, s, s), scale=2.0) for i, s in enumerate((8, 16, 32))]
    lab = _label("wlossw", (2, 1, 32, 32), False)
    wts = (0.25, 2.0, 1.5)
    o64 = [o.double().requires_grad_() for o in outs]
    want = restated(kind, o64, lab.double(), bce == "pixel", loss_weights=wts)
    (want * 0.37).backward()
    od = [o.to(DEV).requires_grad_() for o in outs]
    got = train.SodLoss(kind, bce, loss_weights=wts)(od, lab.to(DEV))
    assert abs(float(got.detach()) - float(want.detach())) < 2e-6 * max(1.0, abs(float(want.detach())))
    (got * 0.37).backward()
    for o, ref in zip(od, o64):
        assert _rel_l2(o.grad, ref.grad) < 2e-5


@pytest.mark.parametrize("kind,bce", [("structure", "reference"), ("structure", "pixel"), ("wbce", "reference"), ("wbce", "pixel")])
def test_reproducible_and_no_gradient_where_none_is_needed(kind, bce):
    from tramba_amd import train
    outs = [synth.synth_input(f"lossr_{i}", (4, 1, s, s), scale=2.0).to(DEV) for i, s in enumerate((12, 48, 96))]
    lab = _label("wlossr", (4, 1, 96, 96), True).to(DEV)
    spec = train.SodLoss(kind, bce)
    runs = []
    for _ in range(3):
        od = [o.clone().requires_grad_(i != 1) for i, o in enumerate(outs)]
        loss = spec(od, lab)
        loss.backward()
        assert od[1].grad is None
        runs.append((loss.detach().clone(), od[0].grad.clone(), od[2].grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))       # fixed summation order, no atomics
    with torch.no_grad():
        assert torch.equal(spec(outs, lab), runs[0][0])


@pytest.mark.parametrize("bce", ["reference", "pixel"])
def test_callers_weight(bce):
    from tramba_amd import train
    outs = [synth.synth_input(f"lossc_{i}", (2, 2, h, w), scale=2.5) for i, (h, w) in enumerate(((9, 11), (37, 45)))]
    lab = _label("wlossc", (2, 2, 37, 45), False)
    weight = torch.sigmoid(synth.synth_input("wlossc_w", (2, 2, 37, 45)))
    o64 = [o.double().requires_grad_() for o in outs]
    want = restated("structure", o64, lab.double(), bce == "pixel", weight=weight.double())
    want.backward()
    od = [o.to(DEV).requires_grad_() for o in outs]
    got = train.SodLoss("structure", bce)(od, lab.to(DEV), weight=weight.to(DEV))
    assert got.is_cuda
    assert abs(float(got.detach()) - float(want.detach())) < 2e-6 * max(1.0, abs(float(want.detach())))
    got.backward()
    for o, ref in zip(od, o64):
        assert _rel_l2(o.grad, ref.grad) < 2e-5
    # one output through the reference's own signature
    p = outs[1].to(DEV).requires_grad_()
    one = train.structure_loss(p, lab.to(DEV), weight.to(DEV), bce=bce)
    w1 = restated("structure", [outs[1].double()], lab.double(), bce == "pixel", weight=weight.double())
    assert abs(float(one.detach()) - float(w1)) < 2e-6 * max(1.0, abs(float(w1)))


def test_bindings_reject_what_the_kernels_cannot_take():
    from tramba_amd import hip
    lab = torch.zeros(1, 1, 8, 8, device=DEV)
    wmap = hip.loss_weight_map(lab, 31)
    assert torch.equal(wmap, torch.ones_like(lab))
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss([torch.zeros(1, 1, 16, 16, device=DEV)], lab, wmap)                        # larger than the label
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss([torch.zeros(1, 1, 8, 8, device=DEV, dtype=torch.bfloat16)], lab, wmap)
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss([torch.zeros(1, 1, 8, 8)], lab, wmap)                                      # a host tensor: no fallback here
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss([torch.zeros(1, 1, 8, 8, device=DEV)], lab, wmap[..., :4].contiguous())    # a map of another shape
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss([torch.zeros(1, 1, 8, 8, device=DEV)], lab, wmap, eps=1.5)
    _, coefs = hip.sod_wloss([torch.zeros(1, 1, 8, 8, device=DEV)], lab, wmap)
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss_grad(torch.zeros(1, 1, 16, 16, device=DEV), lab, wmap, coefs[0])
    with pytest.raises(hip.TrambaHipError):
        hip.sod_wloss_grad(torch.zeros(1, 1, 8, 8), lab, wmap, coefs[0])
    with pytest.raises(hip.TrambaHipError):
        hip.loss_weight_map(lab.to(torch.bfloat16), 31)


@pytest.mark.parametrize("name", ["ragged", "one_pixel", "planes"])
@pytest.mark.parametrize("soft", [False, True])
def test_unit_weights_give_the_unweighted_loss(name, soft):
    """The unweighted and the weighted loss are two instantiations of the same kernels (3 and 5 sums per block, I and U in
    other slots).  With W = 1 (a raw weight of zeros, W = 1 + 5 * 0), eps = 0 and the IoU term on they are one function, in
    either reading of the BCE term: with planes of equal size the mean over planes of sum bce / npix is the batch mean.
    Each against the fp64 oracle at the bounds of test_loss_value_and_gradients_against_the_oracle (2e-6 max(1, |value|),
    2e-5 relative L2), among each other at twice those, relative to the fp64 result (triangle inequality); the coefficient
    tables within 4e-6 relative in a, cI, cU, and the selector exactly 0, 0, 1."""
    from oracle import ops as oo
    from tramba_amd import hip
    b, c, (hh, ww), sizes = LOSS_CASES[name]
    outs = [synth.synth_input(f"loss_{name}_{i}", (b, c, h, w), scale=3.0) for i, (h, w) in enumerate(sizes)]
    lab = _label(f"wloss_{name}", (b, c, hh, ww), soft)
    o64 = [o.double().requires_grad_() for o in outs]
    want = oo.tramba_loss(o64, lab.double())
    (want * 0.37).backward()
    want = float(want.detach())
    od, labd, gscale = [o.to(DEV) for o in outs], lab.to(DEV), torch.tensor(0.37, device=DEV)
    zeros = torch.zeros_like(labd)
    got = {"bce_iou": hip.sod_loss(od, labd)}
    for per_pixel in (False, True):
        got[f"w/pixel={per_pixel}"] = hip.sod_wloss(od, labd, zeros, eps=0.0, per_pixel=per_pixel, with_iou=True, weight_is_raw=True)
    grads = {"bce_iou": [hip.sod_loss_grad(o, labd, got["bce_iou"][1][i], gscale) for i, o in enumerate(od)]}
    for k in list(got)[1:]:
        grads[k] = [hip.sod_wloss_grad(o, labd, zeros, got[k][1][i], gscale, eps=0.0, weight_is_raw=True) for i, o in enumerate(od)]
    for k, (loss, coefs) in got.items():
        errs = [_rel_l2(g, ref.grad) for g, ref in zip(grads[k], o64)]
        print(f"{name} soft={soft} {k}: loss {float(loss):.8f} want {want:.8f} err {abs(float(loss) - want):.3e}, "
              f"gradient rel L2 {['%.2e' % e for e in errs]}")
        assert loss.dtype == torch.float32 and loss.dim() == 0 and coefs.shape == (len(od), b * c, 4)
        assert abs(float(loss) - want) < 2e-6 * max(1.0, abs(want)), (k, float(loss), want)
        for i, (g, e) in enumerate(zip(grads[k], errs)):
            assert g.shape == od[i].shape
            assert e < 2e-5, (k, i, e)
    names = list(got)
    for x, y in ((0, 1), (0, 2), (1, 2)):
        (la, ca), (lb, cb) = got[names[x]], got[names[y]]
        assert abs(float(la) - float(lb)) < 4e-6 * max(1.0, abs(want)), (names[x], names[y], float(la), float(lb))
        for ga, gb, ref in zip(grads[names[x]], grads[names[y]], o64):
            assert float((ga.double() - gb.double()).norm().cpu() / ref.grad.norm()) < 4e-5, (names[x], names[y])
        rel = ((ca[..., :3].double() - cb[..., :3].double()).abs() / cb[..., :3].double().abs()).max()
        print(f"{name} soft={soft} {names[x]} vs {names[y]}: coefficients max rel {float(rel):.3e}")
        assert float(rel) <= 4e-6, (names[x], names[y], float(rel))
    for k, sel in zip(names, (0.0, 0.0, 1.0)):
        assert bool((got[k][1][..., 3] == sel).all()), k


def _small_vss(capturable=True):
    import tramba_amd as ta
    from tramba_amd import train
    torch.manual_seed(5)
    m = ta.bulid_model(use_pretrain=False, img_size=64).to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, ta.DropPath):
            mod.drop_prob = 0.0          # no random numbers: the eager and the captured step see the same network
    m.compute_dtype = torch.bfloat16
    return m, train.get_opt(1e-3, m, capturable=capturable)


def _run(graphed, spec, make_control, steps=2, pass_loss=True):
    import tramba_amd as ta
    from tramba_amd import train
    x = synth.synth_input("wloss_step_x", (4, 3, 64, 64)).to(DEV)
    y = _label("wloss_step_y", (4, 1, 64, 64), False).to(DEV)
    m, opt = _small_vss()
    control = make_control()
    kw = {"loss": spec} if pass_loss else {}
    if graphed:
        step = ta.GraphedTrainStep(m, opt, control=control, **kw)
        losses = [step(x, y).clone() for _ in range(steps)]
    else:
        ckw = {} if control is None else {"control": control}
        losses = [train.train_step(m, opt, x, y, **ckw, **kw).clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in m.parameters()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


def test_captured_step_with_a_loss_spec():
    from tramba_amd import train
    spec = train.SodLoss("structure", bce="pixel")
    none = lambda: None                                                               # noqa: E731
    eager, graphed = _run(False, spec, none), _run(True, spec, none)
    assert all(bool(torch.isfinite(l)) for l in eager[0]) and not torch.equal(eager[0][0], eager[0][1])
    assert _same(eager, graphed), ([float(l) for l in eager[0]], [float(l) for l in graphed[0]])
    ctl = lambda: train.StepControl(accumulate=2, clip_norm=1.0)                      # noqa: E731
    eager_c, graphed_c = _run(False, spec, ctl), _run(True, spec, ctl)
    assert _same(eager_c, graphed_c), ([float(l) for l in eager_c[0]], [float(l) for l in graphed_c[0]])
    assert not _same(eager, eager_c)
    # the default spec is the step as it was
    plain, default = _run(True, None, none, pass_loss=False), _run(True, train.SodLoss(), none)
    assert _same(plain, default)
    assert not torch.equal(plain[0][0], graphed[0][0])                                # ... and another loss than the structure loss


def test_device_error_word_is_clear():
    from tramba_amd import hip
    torch.cuda.synchronize()
    assert hip.lib().tramba_device_error() == 0        # the word itself (reading it clears it) ...
    hip.device_error()                                 # ... and the binding, which raises when it is set
