"""CPU tests of the weighted F-measure's host side (Evaluation/metrics.py:379-441): the two C entries are exported and
bound, bad arguments are rejected before any launch, the filter weights are the reference's, and the scipy path stays
reachable as WeightedFmeasure(host=True).  The GPU side: tests/test_gpu_wfm.py."""
import json
import os

import numpy as np
import pytest
import torch

import synth
from oracle import metrics as om

HERE = os.path.dirname(os.path.abspath(__file__))


def test_weighted_f_entries_are_exported_and_bound():
    from tramba_amd import hip
    lib = hip.lib()
    assert lib.tramba_abi_version() == 7
    for name in ("tramba_feature_transform", "tramba_weighted_f_workspace", "tramba_weighted_f_sums"):
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.tramba_weighted_f_workspace(2, 384, 384) > 0
    assert lib.tramba_weighted_f_workspace(1, hip.WFM_MAX_DIM + 1, 8) == 0


def test_weighted_f_bad_arguments_are_rejected_not_fatal():
    from tramba_amd import hip
    lib = hip.lib()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data          # never dereferenced: every call below is rejected before a launch
    assert lib.tramba_feature_transform(None, None, None, 1, 8, 8, None) < 0 and b"null" in lib.tramba_last_error()
    assert lib.tramba_feature_transform(p, p, p, 1, hip.WFM_MAX_DIM + 1, 8, None) < 0
    assert lib.tramba_feature_transform(p, p, p, 1, 8, 0, None) < 0
    g = hip._GAUSS7.ctypes.data
    assert lib.tramba_weighted_f_sums(p, p, p, p, g, p, p, 1 << 20, 1, 8, hip.WFM_MAX_DIM + 1, None) < 0
    assert lib.tramba_weighted_f_sums(p, p, p, p, g, p, p, 0, 1, 8, 8, None) < 0 and b"workspace" in lib.tramba_last_error()
    # the wrappers: CPU tensors (no host fallback), dtypes, shapes, the size limit
    pred, gt = torch.rand(2, 8, 8), torch.rand(2, 8, 8) > 0.5
    for call in (lambda: hip.feature_transform(gt), lambda: hip.weighted_f_sums(pred, gt),
                 lambda: hip.feature_transform(gt.float()), lambda: hip.feature_transform(gt[0]),
                 lambda: hip.weighted_f_sums(pred.double(), gt), lambda: hip.weighted_f_sums(pred, gt[:, :4]),
                 lambda: hip.weighted_f_sums(pred, gt.float()),
                 lambda: hip.feature_transform(torch.zeros(1, 2, hip.WFM_MAX_DIM + 1, dtype=torch.bool))):
        with pytest.raises(hip.TrambaHipError):
            call()


def test_filter_weights_are_the_reference_gaussian():
    """matlab_style_gauss2D((7, 7), 5) of Evaluation/metrics.py:429-441, as the oracle restates it"""
    from tramba_amd import hip
    assert np.array_equal(hip._GAUSS7.reshape(7, 7), om._gauss7())


def test_host_weighted_fmeasure_matches_reference_fixture():
    from tramba_amd.evaluate import WeightedFmeasure
    with open(os.path.join(HERE, "golden", "metrics_golden.json")) as f:
        golden = json.load(f)
    every = WeightedFmeasure(host=True)
    for name, pred, gt in synth.metric_cases():
        one = WeightedFmeasure(host=True)
        one.step(pred, gt)
        every.step(pred, gt)
        assert abs(one.get_results()["wfm"] - golden["cases"][name]["wfm"]) <= 1e-12, name
    assert abs(every.get_results()["wfm"] - golden["all"]["wfm"]) <= 1e-12
