"""CPU tests of structure_loss / wbce (reference utils/loss.py:14-42) and of the loss spec that train_step, fit and
GraphedTrainStep take: the torch composition (what runs off the device) against the reference's own fp64 results in
tests/golden/golden_loss.npz, the per-pixel reading against a restatement, and the plumbing through the training step."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases
import synth
from test_train_loop import Tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tramba_loss_weight_map", "tramba_sod_wloss_sums", "tramba_sod_wloss_finish", "tramba_sod_wloss_grad_workspace",
               "tramba_sod_wloss_grad")


@pytest.fixture(scope="module")
def golden_loss():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_loss.npz"))


def restated(kind, pred, mask, weight=None, pixel=True):
    """fp64 restatement of utils/loss.py:15-42 with reduction='none' (pixel) or 'mean' (what the reference executes)"""
    k, eps, iou = {"structure": (31, 0.001, True), "wbce": (15, 0.0, False)}[kind]
    weit = 1 + 5 * torch.abs(F.avg_pool2d(mask, kernel_size=k, stride=1, padding=k // 2) - mask) if weight is None else 1 + 5 * weight
    bce = F.binary_cross_entropy_with_logits(pred, (1 - eps) * mask + eps / 2, reduction="none" if pixel else "mean")
    bce = (weit * bce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))
    if not iou:
        return bce.mean()
    p = torch.sigmoid(pred)
    inter = ((p * mask) * weit).sum(dim=(2, 3))
    union = ((p + mask) * weit).sum(dim=(2, 3))
    return (bce + 1 - (inter + 1) / (union - inter + 1)).mean()


def _call(kind, pred, mask, weight, bce):
    from tramba_amd import train
    if kind == "structure":
        return train.structure_loss(pred, mask, weight, bce=bce)
    return train.wbce(pred, mask, bce=bce)


def _kinds(name):
    return ("structure",) if loss_cases.CASES[name][2] else ("structure", "wbce")


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_fallback_equals_the_reference_in_fp64(name, golden_loss):
    """the same arithmetic in the same precision: 1e-12 relative on the value and on the gradient"""
    pred, mask, weight = loss_cases.case(name)
    for kind in _kinds(name):
        p = pred.clone().requires_grad_()
        got = _call(kind, p, mask, weight, "reference")
        assert got.dtype == torch.float64 and got.dim() == 0
        want = float(golden_loss[f"{kind}/{name}/value"])
        assert abs(float(got.detach()) - want) <= 1e-12 * abs(want), (kind, name, float(got.detach()), want)
        got.backward()
        d = loss_cases.digest(p.grad)
        ref = torch.from_numpy(golden_loss[f"{kind}/{name}/grad_sample"])
        norm = float(golden_loss[f"{kind}/{name}/grad_norm"])
        assert d["sample"].shape == ref.shape
        assert float((d["sample"] - ref).norm()) <= 1e-12 * float(ref.norm()), (kind, name)
        assert abs(d["norm"] - norm) <= 1e-12 * norm
        assert abs(d["sum"] - float(golden_loss[f"{kind}/{name}/grad_sum"])) <= 1e-12 * norm * p.numel() ** 0.5


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_pixel_reading_equals_the_restatement(name):
    pred, mask, weight = loss_cases.case(name)
    for kind in _kinds(name):
        p, q = pred.clone().requires_grad_(), pred.clone().requires_grad_()
        got, want = _call(kind, p, mask, weight, "pixel"), restated(kind, q, mask, weight, pixel=True)
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        got.backward()
        want.backward()
        assert float((p.grad - q.grad).norm()) <= 1e-12 * float(q.grad.norm())


def test_the_two_readings_differ_on_a_blob_and_coincide_where_the_weight_is_flat():
    from tramba_amd import train
    pred, mask, _ = loss_cases.case("blob")
    assert abs(float(train.structure_loss(pred, mask, bce="pixel")) - float(train.structure_loss(pred, mask))) > 1e-4
    assert abs(float(train.wbce(pred, mask, bce="pixel")) - float(train.wbce(pred, mask))) > 1e-4
    # all-zero label: avg_pool(0) - 0 = 0, W == 1 everywhere
    pred, mask, _ = loss_cases.case("zeros")
    for fn in (train.structure_loss, train.wbce):
        a, b = float(fn(pred, mask, bce="pixel")), float(fn(pred, mask, bce="reference"))
        assert abs(a - b) <= 1e-12 * abs(b)
    # wbce as the reference executes it: the weight cancels, plain mean BCE is left
    for name in ("blob", "soft", "rect"):
        pred, mask, _ = loss_cases.case(name)
        a, b = float(train.wbce(pred, mask)), float(F.binary_cross_entropy_with_logits(pred, mask))
        assert abs(a - b) <= 1e-12 * abs(b)


def test_spec_over_deep_supervision_outputs():
    from tramba_amd import train
    outs = [synth.synth_input(f"spec_{i}", (2, 1, s, s), scale=2.0) for i, s in enumerate((8, 16, 32))]
    lab = (synth.synth_input("spec_y", (2, 1, 32, 32)) > 0).float()
    assert torch.equal(train.SodLoss("bce_iou")(outs, lab), train.tramba_loss(outs, lab))
    wts = (0.5, 2.0, 1.0)
    assert torch.equal(train.SodLoss("bce_iou", loss_weights=wts)(outs, lab), train.tramba_loss(outs, lab, wts))
    for kind in ("structure", "wbce"):
        for bce in ("reference", "pixel"):
            got = train.SodLoss(kind, bce, wts)(outs, lab)
            want = sum(w * restated(kind, F.interpolate(o, (32, 32), mode="bilinear").double(), lab.double(), pixel=bce == "pixel")
                       for w, o in zip(wts, outs))
            assert got.dtype == torch.float32
            assert abs(float(got) - float(want)) < 1e-5 * abs(float(want)), (kind, bce)
    w = torch.sigmoid(synth.synth_input("spec_w", (2, 1, 32, 32)))
    got = train.SodLoss("structure")(outs[2:], lab, weight=w)
    assert abs(float(got) - float(restated("structure", outs[2].double(), lab.double(), w.double(), pixel=False))) < 1e-5


def _batch():
    x = synth.synth_input("plumb_x", (4, 3, 8, 8))
    y = (synth.synth_input("plumb_y", (4, 1, 8, 8)) > 0).float()
    return x, y


def _fresh():
    from tramba_amd import train
    torch.manual_seed(0)
    m = Tiny()
    return m, train.get_opt(1e-2, m)


def test_train_step_takes_the_spec():
    from tramba_amd import train
    x, y = _batch()
    m0, o0 = _fresh()
    l0 = train.train_step(m0, o0, x, y)
    m1, o1 = _fresh()
    l1 = train.train_step(m1, o1, x, y, loss=None)
    m2, o2 = _fresh()
    l2 = train.train_step(m2, o2, x, y, loss=train.SodLoss("bce_iou"))
    for a, b, c in zip(m0.parameters(), m1.parameters(), m2.parameters()):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    m3, o3 = _fresh()
    before = copy.deepcopy(m3.state_dict())
    l3 = train.train_step(m3, o3, x, y, loss=train.SodLoss("structure"))
    with torch.no_grad():
        ref = Tiny()
        ref.load_state_dict(before)
        assert torch.equal(l3, train.SodLoss("structure")(ref(x), y))
    assert any(not torch.equal(before[k], v) for k, v in m3.state_dict().items())            # it steps
    assert any(not torch.equal(a, b) for a, b in zip(m0.parameters(), m3.parameters()))      # ... somewhere else


def test_controlled_step_returns_the_mean_micro_batch_loss():
    from tramba_amd import train
    x, y = _batch()
    spec = train.SodLoss("structure", bce="pixel")
    m, opt = _fresh()
    with torch.no_grad():
        want = sum(spec(m(xx), yy) for xx, yy in zip(x.chunk(2), y.chunk(2))) / 2
    before = copy.deepcopy(m.state_dict())
    got = train.train_step(m, opt, x, y, control=train.StepControl(accumulate=2), loss=spec)
    assert torch.allclose(got, want, rtol=1e-6, atol=0)
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())
    m2, opt2 = _fresh()
    train.train_step(m2, opt2, x, y, control=train.StepControl(accumulate=2))
    assert any(not torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))


def test_fit_takes_the_spec(tmp_path):
    from tramba_amd import train
    from test_train_loop import _data
    kw = dict(epochs=1, base_lr=1e-2, decay_epochs=[], decay_factors=[], save_model=str(tmp_path), method="T", is_main=False)
    m0, o0 = _fresh()
    h0 = train.fit(m0, o0, _data, **kw)
    m1, o1 = _fresh()
    h1 = train.fit(m1, o1, _data, loss=train.SodLoss("wbce", bce="pixel"), **kw)
    assert h0[0]["loss"] != h1[0]["loss"]
    assert any(not torch.equal(a, b) for a, b in zip(m0.parameters(), m1.parameters()))


def test_new_symbols_names_and_errors():
    import tramba_amd
    from tramba_amd import hip, train
    hdr = open(os.path.join(ROOT, "include", "tramba_hip.h")).read()
    declared = set(re.findall(r"\b(tramba_[a-z0-9_]+)\s*\(", hdr))
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    # bad arguments come back as codes, before any launch
    assert lib.tramba_loss_weight_map(None, None, 1, 8, 8, 31, None) < 0
    assert lib.tramba_loss_weight_map(1, 1, 1, 8, 8, 30, None) < 0 and b"odd" in lib.tramba_last_error()
    assert lib.tramba_loss_weight_map(1, 1, 1, 8, 8, 65, None) < 0
    assert lib.tramba_sod_wloss_grad_workspace(8, 24, 24, 384, 384) == lib.tramba_sod_loss_grad_workspace(8, 24, 24, 384, 384)
    assert tramba_amd.SodLoss is train.SodLoss and tramba_amd.structure_loss is train.structure_loss
    assert tramba_amd.wbce is train.wbce
    for bad in (dict(kind="ssim"), dict(kind="structure", bce="mean")):
        with pytest.raises(ValueError):
            train.SodLoss(**bad)
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        train.structure_loss(z, z, bce="none")
    with pytest.raises(ValueError):
        train.wbce(z, z, bce="")
    with pytest.raises(ValueError):
        train.SodLoss("wbce")([z], z, weight=z)
    with pytest.raises(ValueError):
        train.SodLoss("structure", loss_weights=(1.0, 2.0))([z], z)
    with pytest.raises(hip.TrambaHipError):
        hip.loss_weight_map(z, 31)                      # a host tensor: the binding has no fallback
    m, opt = _fresh()
    with pytest.raises(TypeError):                      # a step takes the spec, not any callable (it may be captured)
        train.train_step(m, opt, *_batch(), loss=train.tramba_loss)


def test_compat_shim_exports_the_reference_names():
    from tramba_amd import train
    compat = os.path.join(ROOT, "tramba_amd", "compat")
    saved_path, saved = list(sys.path), {k: v for k, v in sys.modules.items() if k == "utils" or k.startswith("utils.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, compat)
    try:
        from utils.loss import iou_loss, structure_loss, wbce
        assert structure_loss is train.structure_loss and wbce is train.wbce and iou_loss is train.iou_loss
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
        sys.modules.update(saved)
