"""The weighted F-measure on the GPU (Evaluation/metrics.py:379-441; csrc/saliency_wfm.hip): the feature transform
index for index against scipy's distance_transform_edt(return_indices=True), ties included; the weighted-F sums against
the reference fixture and the scipy path; the evaluation loop without the host path; the folder evaluator
(Evaluation/evaluate_TSOD.py) against the oracle."""
import json
import os

import numpy as np
import pytest
import torch

import synth
from oracle import metrics as om

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "metrics_golden.json")) as f:
        return json.load(f)


def _blob_mask(h, w, seed, n=3):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = np.zeros((h, w))
    for _ in range(n):
        cy, cx = rs.uniform(0.15, 0.85) * h, rs.uniform(0.15, 0.85) * w
        sy, sx = rs.uniform(0.05, 0.2) * h, rs.uniform(0.05, 0.2) * w
        z += rs.uniform(0.5, 1.5) * np.exp(-((yy - cy) ** 2 / (2 * sy * sy) + (xx - cx) ** 2 / (2 * sx * sx)))
    return z > 0.55, z, rs


def _blob_pair(h, w, seed):
    gt, z, rs = _blob_mask(h, w, seed)
    logit = 6.0 * (z - 0.55) + 1.2 * rs.standard_normal((h, w))
    return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32), gt


def _lattice(h, w, step, oy=0, ox=0):
    g = np.zeros((h, w), bool)
    g[oy::step, ox::step] = True
    return g


def _cross(h, w, seed):
    rs = np.random.RandomState(seed)
    g = np.zeros((h, w), bool)
    g[h // 2, :] = True
    g[:, w // 2] = True
    g[h // 3, w // 5:] = True
    return g & (rs.random_sample((h, w)) < 0.6)


def _masks():
    """(name, bool mask): the fixture's masks, tie-rich lattices and crosses, a single pixel, random sparse masks and
    degenerate / odd / large shapes"""
    out = [(n, g != 0) for n, _, g in synth.metric_cases()]
    rs = np.random.RandomState(11)
    for step, oy, ox in ((2, 0, 0), (3, 1, 2), (4, 0, 3), (5, 2, 2), (7, 3, 0), (16, 5, 9)):
        out.append((f"lattice{step}_{oy}{ox}", _lattice(61, 75, step, oy, ox)))
    out += [(f"cross{s}", _cross(57, 64, s)) for s in range(3)]
    one = np.zeros((40, 33), bool)
    one[17, 5] = True
    out.append(("single", one))
    out += [(f"sparse{p}", rs.random_sample((90, 70)) < p) for p in (0.0005, 0.003, 0.02, 0.2)]
    out.append(("row1xN", rs.random_sample((1, 300)) < 0.02))
    out.append(("colNx1", rs.random_sample((300, 1)) < 0.02))
    out.append(("odd383x385", _blob_mask(383, 385, 3)[0] | (rs.random_sample((383, 385)) < 0.001)))
    out.append(("sq384", _blob_mask(384, 384, 4)[0]))
    out.append(("hd1080x1920", _blob_mask(1080, 1920, 5)[0] | _lattice(1080, 1920, 97, 13, 41)))
    return out


def _scipy_ft(g):
    from scipy.ndimage import distance_transform_edt
    dist, idx = distance_transform_edt(~g, return_indices=True)
    rr, cc = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    return idx[0] * g.shape[1] + idx[1], (idx[0] - rr) ** 2 + (idx[1] - cc) ** 2, dist


def _check_ft(g, idx, d2, name):
    if not g.any():
        assert (idx == -1).all() and (d2 == -1).all(), name
        return
    ref_idx, ref_d2, ref_dist = _scipy_ft(g)
    bad = np.argwhere(idx != ref_idx)
    assert bad.size == 0, f"{name}: {len(bad)} indices differ, first at {bad[0].tolist()}"
    assert np.array_equal(d2, ref_d2), name
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), ref_dist), name


def test_feature_transform_equals_scipy_indices():
    from tramba_amd import hip
    for name, g in _masks():
        idx, d2 = hip.feature_transform(torch.from_numpy(g[None]).cuda())
        _check_ft(g, idx[0].cpu().numpy(), d2[0].cpu().numpy(), name)


def test_feature_transform_mixed_batch():
    """one launch over a tie-rich, a sparse, an empty, a full, a single-pixel and a blob mask"""
    from tramba_amd import hip
    h, w = 96, 80
    one = np.zeros((h, w), bool)
    one[h - 1, 0] = True
    gs = [_lattice(h, w, 3, 1, 1), np.random.RandomState(2).random_sample((h, w)) < 0.004, np.zeros((h, w), bool),
          np.ones((h, w), bool), one, _blob_mask(h, w, 9)[0], _cross(h, w, 7)]
    batch = torch.from_numpy(np.stack(gs)).cuda()
    idx, d2 = hip.feature_transform(batch)
    idx8, _ = hip.feature_transform(batch.to(torch.uint8) * 7)      # any non-zero byte is a mask pixel
    torch.cuda.synchronize()
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(idx, idx8.cpu().numpy())
    for i, g in enumerate(gs):
        _check_ft(g, idx[i], d2[i], f"batch[{i}]")


def _gpu_wfm(pairs, **kw):
    from tramba_amd import evaluate as E
    m = E.WeightedFmeasure(**kw)
    for pred, gt in pairs:
        m.step(pred=pred, gt=gt)
    return m.weighted_fms, m.get_results()["wfm"]


def test_weighted_f_matches_reference_fixture(golden):
    cases = synth.metric_cases()
    for name, pred, gt in cases:
        _, got = _gpu_wfm([(pred, gt)])
        assert abs(got - golden["cases"][name]["wfm"]) <= 2e-6, (name, got, golden["cases"][name]["wfm"])
    _, got = _gpu_wfm([(p, g) for _, p, g in cases])
    assert abs(got - golden["all"]["wfm"]) <= 2e-6


@pytest.mark.parametrize("h,w", [(384, 384), (1080, 1920), (61, 75)])
def test_weighted_f_matches_scipy_path(h, w):
    pairs = [_blob_pair(h, w, s) for s in range(2)]
    if (h, w) == (61, 75):      # tie-rich masks: a different nearest pixel would spread a different error
        pairs = [(p, _lattice(h, w, s, 1, 2)) for s, (p, _) in zip((3, 4), pairs)]
    got, _ = _gpu_wfm(pairs)
    want, _ = _gpu_wfm(pairs, host=True)
    for g, r in zip(got, want):
        assert abs(g - r) <= 2e-6, (g, r)
    for (p, gt), g in zip(pairs, got):
        assert abs(g - om.weighted_fmeasure(p, gt)) <= 2e-6


def test_weighted_f_sums_reproducible_and_batch_independent():
    from tramba_amd import hip
    pairs = [_blob_pair(200, 136, s) for s in range(3)]
    pairs[1] = (pairs[1][0], np.zeros_like(pairs[1][1]))                    # an empty mask inside the batch
    pred = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
    gt = torch.from_numpy(np.stack([g for _, g in pairs])).cuda()
    a = hip.weighted_f_sums(pred, gt).cpu()
    b = hip.weighted_f_sums(pred, gt).cpu()
    assert torch.equal(a, b)
    assert torch.equal(a[1], torch.zeros(3, dtype=torch.float64))
    for i in range(3):
        assert torch.equal(hip.weighted_f_sums(pred[i:i + 1], gt[i:i + 1]).cpu()[0], a[i]), i
    assert a[0, 0] == pairs[0][1].sum() and a[2, 0] == pairs[2][1].sum()


def test_test_one_epoch_weighted_takes_no_host_path(monkeypatch):
    """test_one_epoch(weighted=True) on a stand-in model, with scipy's distance transform made to raise"""
    import scipy.ndimage
    from tramba_amd import evaluate as E

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([0.9, -0.4, 0.3]).view(1, 3, 1, 1))

        def forward(self, x):
            full = (x * self.w).sum(1, keepdim=True) * 3.0
            return [full[:, :, ::4, ::4], full]

    model = Stub().cuda()
    g = torch.Generator().manual_seed(8)
    batches = []
    for _ in range(3):
        img = torch.nn.functional.avg_pool2d(torch.randn(2, 3, 64, 72, generator=g), 5, 1, 2)
        gt = ((img * torch.tensor([0.9, -0.4, 0.3]).view(1, 3, 1, 1)).sum(1, keepdim=True) > 0.05).float()
        batches.append({"image": img, "gt": gt})
    ev = om.Evaluator()
    with torch.no_grad():
        for b in batches:
            pred = torch.sigmoid(model(b["image"].cuda())[-1]).cpu().numpy()
            for j in range(2):
                ev.step(pred[j, 0], b["gt"][j, 0].numpy())
    r = ev.results()

    def no_host(*a, **k):
        raise AssertionError("the host distance transform was called")

    monkeypatch.setattr(scipy.ndimage, "distance_transform_edt", no_host)
    got = E.test_one_epoch(model, batches, weighted=True)
    assert got["Wmeasure_r"] is not None and abs(float(got["Wmeasure_r"]) - round(r["wfm"], 4)) <= 1e-4
    assert abs(float(got["Smeasure_r"]) - round(r["sm"], 4)) <= 1e-4
    assert abs(float(got["MAE_r"]) - round(r["mae"], 4)) <= 1e-4


def test_evaluate_folder_matches_oracle(tmp_path):
    pytest.importorskip("PIL.Image")
    from tramba_amd import evaluate as E
    sal, msk = tmp_path / "sal", tmp_path / "gt"
    sal.mkdir()
    msk.mkdir()
    rs = np.random.RandomState(4)
    arrays = []
    for i, (h, w) in enumerate([(96, 128), (72, 72), (130, 90), (64, 64)]):
        p, g = _blob_pair(h, w, 20 + i)
        p8 = (p * 255).astype(np.uint8)
        g8 = np.where(g, 255, 0).astype(np.uint8) if i != 3 else np.zeros((h, w), np.uint8)
        E.write_png_gray8(str(sal / f"im{i}.png"), p8)
        E.write_png_gray8(str(msk / f"im{i}.png"), g8)
        arrays.append((p8.astype(np.float32) / 255, g8.astype(np.float32) / (g8.max() + 1e-8)))
    E.write_png_gray8(str(sal / "only_pred.png"), (rs.random_sample((10, 10)) * 255).astype(np.uint8))
    got = E.evaluate_folder(str(sal), str(msk), model="m", dataset="d", save_dir=str(tmp_path / "npy"), workers=3)
    ev = om.Evaluator()
    for p, g in arrays:
        ev.step(p, g)
    r = ev.results()
    want = {"Smeasure_r": r["sm"], "Wmeasure_r": r["wfm"], "MAE_r": r["mae"], "adpEm_r": r["em_adp"],
            "meanEm_r": r["em_curve"].mean(), "maxEm_r": r["em_curve"].max(), "adpFm_r": r["fm_adp"],
            "meanFm_r": r["fm_curve"].mean(), "maxFm_r": r["fm_curve"].max(), "fnr_r": r["fnr"]}
    assert got["model"] == "m" and got["dataset"] == "d"
    for k, v in want.items():
        assert abs(float(got[k]) - round(float(v), 4)) <= 1e-4, (k, got[k], v)
    np.testing.assert_allclose(got["precision"], r["precision"].astype(np.float32), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["recall"], r["recall"].astype(np.float32), rtol=0, atol=1e-6)
    assert np.array_equal(np.load(str(tmp_path / "npy" / "precision.npy")), got["precision"])
