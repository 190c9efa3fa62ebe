"""DeviceHDBSCAN with the minimum spanning tree from clift_emst on the GPU, against sklearn.cluster.HDBSCAN in the test process, and the
``hdbscan="device"`` switch of inference.cluster / cluster_segmentwise against ``"sklearn"``.  Labels and one-hot outputs exactly equal;
probabilities within 1e-12 (ratios in [0, 1], a few fp64 roundings), centroids within 1e-9."""
import numpy as np
import pytest
import torch

import hdbscan_cases as hc
from contrastive_lift_amd import inference
from contrastive_lift_amd.hdbscan import DeviceHDBSCAN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", [0, 2, 3, 7])
def test_device_fit_equals_sklearn(i):
    X, mcs, prim = hc.case(i)
    got = DeviceHDBSCAN(mcs, device="cuda").fit(X)
    labels, prob = hc.sklearn_fit(i)
    a, b, w = got.mst_
    assert hc.is_spanning_tree(len(X), a, b) and np.array_equal(np.sort(w), np.sort(prim[2]))
    assert 1 <= got.n_rounds_ <= int(np.ceil(np.log2(len(X))))
    assert np.array_equal(got.labels_, labels), int((got.labels_ != labels).sum())
    worst = float(np.abs(got.probabilities_ - prob).max())
    print("case", i, "rounds", got.n_rounds_, "max |dp|", worst)
    assert worst <= 1e-12


def thing_features():
    X = hc.blobs(2, 1500, 3)
    return np.concatenate([np.full((len(X), 1), -np.inf, dtype=np.float32), X], axis=1)


def test_cluster_switch():
    feats, out = thing_features(), {}
    for backend in ("device", "sklearn"):
        np.random.seed(11)
        out[backend] = inference.cluster(feats, 0.15, "cuda", 1, use_dbscan=True, cluster_size=25, hdbscan=backend)
    (oh_d, cen_d), (oh_s, cen_s) = out["device"], out["sklearn"]
    assert oh_d.shape == oh_s.shape and oh_d.shape[-1] >= 4 and torch.equal(oh_d, oh_s)
    assert cen_d.shape == cen_s.shape and float(np.abs(cen_d - cen_s).max()) <= 1e-9


def test_cluster_segmentwise_switch():
    feats, out = thing_features(), {}
    cls = (np.arange(len(feats)) % 5 < 2).astype(np.int64)                              # two thing classes of 900 and 600 points
    sem = [torch.nn.functional.one_hot(torch.as_tensor(cls), 3).float()]
    for backend in ("device", "sklearn"):
        np.random.seed(11)
        out[backend] = inference.cluster_segmentwise(feats, sem, 0.15, "cuda", 1, use_dbscan=True, cluster_size=15, hdbscan=backend)
    (oh_d, cen_d), (oh_s, cen_s) = out["device"], out["sklearn"]
    assert oh_d.shape == oh_s.shape and oh_d.shape[-1] >= 5 and torch.equal(oh_d, oh_s)
    assert cen_d.shape == cen_s.shape and float(np.abs(cen_d - cen_s).max()) <= 1e-9


def test_non_finite_input_is_an_error_not_a_loop():
    from contrastive_lift_amd import _lib
    X = np.array(hc.case(0)[0])
    X[17, 1] = np.nan
    with pytest.raises(_lib.CliftError, match="non-finite"):
        DeviceHDBSCAN(10, device="cuda").fit(X)
