"""Host side of DeviceHDBSCAN (contrastive_lift_amd/hdbscan.py) against sklearn.cluster.HDBSCAN, with the minimum spanning tree injected
from a numpy Prim (tests/hdbscan_cases.py) instead of clift_emst.  No GPU.

Bounds: labels exactly equal; probabilities within 1e-12 absolute -- they are ratios in [0, 1] of two lambdas = 1 / distance, a few fp64
roundings apart at most.  Centroids (probability-weighted means of points in the unit box) within 1e-9."""
import functools

import numpy as np
import pytest
import torch

import hdbscan_cases as hc
from contrastive_lift_amd import inference
from contrastive_lift_amd.hdbscan import DeviceHDBSCAN

PROB_TOL = 1e-12


def check(i, allow_single_cluster=True, mst=None):
    X, mcs, prim = hc.case(i)
    a, b, w = mst or prim
    assert len(np.unique(prim[2])) == len(prim[2]), "precondition: the MST weights of the case are pairwise distinct"
    got = DeviceHDBSCAN(mcs, allow_single_cluster=allow_single_cluster, mst_fn=lambda _: (a, b, w)).fit(X)
    labels, prob = hc.sklearn_fit(i, allow_single_cluster)
    assert got.labels_.dtype.kind == "i" and got.probabilities_.dtype == np.float64
    assert np.array_equal(got.labels_, labels), (i, int((got.labels_ != labels).sum()))
    worst = float(np.abs(got.probabilities_ - prob).max())
    assert worst <= PROB_TOL, (i, worst)
    return got


@pytest.mark.parametrize("i", range(12))
def test_labels_and_probabilities_equal_sklearn(i):
    got = check(i)
    assert got.n_rounds_ is None and len(got.mst_) == 3
    k = int(got.labels_.max()) + 1
    assert 3 <= k <= 6 and 4 <= round(100 * float((got.labels_ == -1).mean())) <= 13   # what the case table says of itself (whole per cent)


@pytest.mark.parametrize("i", [1, 6])
def test_no_single_cluster(i):
    check(i, allow_single_cluster=False)


@pytest.mark.parametrize("i", [0, 5])
def test_edge_order_and_endpoint_order_do_not_matter(i):
    a, b, w = hc.case(i)[2]
    rng = np.random.default_rng(7)
    p = rng.permutation(len(w))
    flip = rng.random(len(w)) < 0.5
    a2, b2 = np.where(flip, b, a)[p], np.where(flip, a, b)[p]
    check(i, mst=(a2, b2, w[p]))


def test_relabel_equals_a_fresh_fit():
    X, mcs, mst = hc.case(2)
    swept = DeviceHDBSCAN(mcs, mst_fn=lambda _: mst).fit(X)
    for m in (5, 60, 200):
        fresh = DeviceHDBSCAN(m, mst_fn=lambda _: mst).fit(X)
        swept.relabel(m)
        assert swept.min_cluster_size == m
        assert np.array_equal(swept.labels_, fresh.labels_) and np.array_equal(swept.probabilities_, fresh.probabilities_)
    assert len(np.unique(swept.labels_)) != len(np.unique(swept.relabel(5).labels_))          # the sweep does change the clustering


def test_refused_settings():
    with pytest.raises(ValueError, match="min_samples"):
        DeviceHDBSCAN(10, min_samples=2)
    with pytest.raises(ValueError, match="min_cluster_size"):
        DeviceHDBSCAN(1)


class _AllNoise(DeviceHDBSCAN):
    """The tree pass on Prim's tree, never a single cluster: with min_cluster_size above n / 2 nothing can split and all is noise."""

    def __init__(self, min_cluster_size, **kw):
        kw.update(allow_single_cluster=False, mst_fn=hc.prim_mst)
        super().__init__(min_cluster_size, **kw)


def test_all_noise(monkeypatch):
    X = (0.5 + 0.05 * np.random.default_rng(3).standard_normal((200, 3))).astype(np.float32)
    got = _AllNoise(120).fit(X)
    assert np.all(got.labels_ == -1) and np.all(got.probabilities_ == 0.0)
    from sklearn.cluster import HDBSCAN
    assert np.all(HDBSCAN(min_cluster_size=120, min_samples=1, allow_single_cluster=False, copy=True).fit(X).labels_ == -1)
    monkeypatch.setattr(inference, "DeviceHDBSCAN", _AllNoise)
    labels, cents = inference._hdbscan_fit(X, 120, hdbscan="device")
    assert np.all(labels == -1) and cents is None


def test_hdbscan_fit_device_backend_centroids(monkeypatch):
    monkeypatch.setattr(inference, "DeviceHDBSCAN", functools.partial(DeviceHDBSCAN, mst_fn=hc.prim_mst))
    X, mcs, _ = hc.case(4)
    pts = np.array(X)
    lab_d, cen_d = inference._hdbscan_fit(pts, mcs, hdbscan="device")
    lab_s, cen_s = inference._hdbscan_fit(pts, mcs, hdbscan="sklearn")
    assert np.array_equal(lab_d, lab_s) and cen_d.shape == cen_s.shape and cen_d.shape[0] >= 3
    assert float(np.abs(cen_d - cen_s).max()) <= 1e-9
    assert inference._hdbscan_fit(pts, mcs)[1].shape == cen_s.shape                     # the default backend is sklearn's
    with pytest.raises(ValueError, match="hdbscan"):
        inference._hdbscan_fit(pts, mcs, hdbscan="gpu")


def test_unknown_backend_is_refused_before_any_work():
    feats = np.concatenate([np.full((400, 1), -np.inf, dtype=np.float32), hc.blobs(1, 400, 3)], axis=1)
    sem = [torch.nn.functional.one_hot(torch.zeros(400, dtype=torch.long), 3).float()]
    with pytest.raises(ValueError, match="hdbscan"):
        inference.cluster(feats, 0.15, "cpu", 1, use_dbscan=True, cluster_size=10, hdbscan="cuda")
    with pytest.raises(ValueError, match="hdbscan"):
        inference.cluster_segmentwise(feats, sem, 0.15, "cpu", 1, use_dbscan=True, cluster_size=10, hdbscan="cuda")
    with pytest.raises(ValueError, match="hdbscan"):
        inference.cluster(feats, 0.15, "cpu", 1, hdbscan="cuda")                          # also when the MeanShift branch would run
