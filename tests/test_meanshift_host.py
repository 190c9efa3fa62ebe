"""Host side of DeviceMeanShift (contrastive_lift_amd/inference.py) against sklearn's MeanShift, no GPU: bin seeding, the merge of equal
centres, the (count, centre) ordering and the radius de-duplication, with the device climb replaced by a NumPy restatement of the kernel's
arithmetic (fp64 neighbour test and sum, fp32 mean, fp32 step norm)."""
import numpy as np
import pytest

from meanshift_cases import blobs, numpy_shift


def test_bin_seeds_match_sklearn():
    from sklearn.cluster import get_bin_seeds
    from contrastive_lift_amd.inference import bin_seeds
    X = blobs(3, 500, 3)
    for bw, freq in ((0.05, 10), (0.02, 1), (0.1, 3)):
        a, b = bin_seeds(X, bw, freq), get_bin_seeds(X, bw, freq)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert sorted(map(tuple, a)) == sorted(map(tuple, b))
    tiny = np.arange(12, dtype=np.float32).reshape(4, 3)                  # every point its own bin -> the points themselves
    assert bin_seeds(tiny, 0.01, 1) is tiny and get_bin_seeds(tiny, 0.01, 1) is tiny


@pytest.mark.parametrize("d,bw,max_iter", [(3, 0.06, 300), (3, 0.15, 300), (5, 0.2, 300), (3, 0.06, 2)])
def test_host_logic_matches_sklearn(d, bw, max_iter):
    from sklearn.cluster import MeanShift
    from contrastive_lift_amd.inference import DeviceMeanShift
    X = blobs(11 + d, 400, d)
    ref = MeanShift(bandwidth=bw, bin_seeding=True, min_bin_freq=10, cluster_all=False, max_iter=max_iter).fit(X)
    got = DeviceMeanShift(bw, min_bin_freq=10, max_iter=max_iter, device="cpu", shift_fn=numpy_shift).fit(X)
    assert got.cluster_centers_.shape == ref.cluster_centers_.shape
    assert got.cluster_centers_.dtype == np.float32
    np.testing.assert_allclose(got.cluster_centers_, ref.cluster_centers_, atol=1e-5 * bw)
    assert got.n_iter_ == ref.n_iter_
    assert np.array_equal(got.predict(X), ref.predict(X))


def test_merge_order_and_dedup():
    """Exactly equal centres merge, count-0 seeds drop, the ranking is (count, centre) descending, and a centre within the bandwidth of a
    better-ranked one goes."""
    from contrastive_lift_amd.inference import DeviceMeanShift
    X = blobs(5, 50, 2)

    def fake(X_, seeds, bw, it):
        c = np.array([[0.5, 0.5], [0.5, 0.5], [0.2, 0.2], [0.21, 0.2], [0.9, 0.9], [0.1, 0.9]], np.float32)
        return c, np.array([7, 7, 5, 9, 0, 5]), np.array([3, 3, 1, 4, 0, 2])
    ms = DeviceMeanShift(0.05, min_bin_freq=1, device="cpu", shift_fn=fake).fit(X)
    # ranked: (9, .21 .2), (7, .5 .5), (5, .2 .2) <- within 0.05 of the first: removed, (5, .1 .9); (0.9, 0.9) had no neighbour
    np.testing.assert_array_equal(ms.cluster_centers_, np.array([[0.21, 0.2], [0.5, 0.5], [0.1, 0.9]], np.float32))
    assert ms.n_iter_ == 4
    with pytest.raises(ValueError, match="bandwidth"):
        DeviceMeanShift(0.05, device="cpu", shift_fn=lambda X_, s, b, i: (np.zeros((2, 2), np.float32), np.zeros(2), np.zeros(2))).fit(X)


def test_cluster_rejects_unknown_meanshift_and_cpu_device():
    from contrastive_lift_amd import _lib
    from contrastive_lift_amd.inference import DeviceMeanShift, cluster
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from make_fake_predictions import fake_thing_features
    import torch
    feats, n_img = fake_thing_features(171, n_img=2, per=600)
    with pytest.raises(ValueError, match="meanshift"):
        cluster(feats, 0.15, torch.device("cpu"), num_images=n_img, meanshift="gpu")
    with pytest.raises(_lib.CliftError, match="GPU"):
        DeviceMeanShift(0.15, device="cpu").fit(blobs(1, 50, 3))


def test_segmentwise_return_dict_matches_g17_centroids():
    """cluster_segmentwise(return_dict=True): the reference's {thing class: centroids} cache; concatenated in key order it is the golden's
    centroid list (incl. the stale entry of the class under the 100-point minimum), with the reference's key / value dtypes."""
    import os, sys
    import torch
    from conftest import load_golden, REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_fake_predictions import fake_thing_features, fake_semantics_for
    from contrastive_lift_amd.inference import cluster_segmentwise
    g = load_golden("g17_meanshift_clustering")
    all_thing, n_img = fake_thing_features(int(g["seed"]))
    sems = fake_semantics_for(all_thing, n_img)
    np.random.seed(4321)
    onehot, cents = cluster_segmentwise(all_thing.copy(), sems, 0.15, torch.device("cpu"), num_images=n_img, meanshift="sklearn", return_dict=True)
    assert isinstance(cents, dict) and list(cents) == sorted(cents) and len(cents) == 3
    assert all(isinstance(k, np.int64) for k in cents) and all(v.dtype == np.float32 for v in cents.values())
    np.testing.assert_allclose(np.concatenate([cents[k] for k in cents], 0), g["seg.centroids"], rtol=1e-6, atol=1e-7)
    assert np.array_equal(onehot.argmax(-1).reshape(-1).numpy().astype(np.int16), g["seg.labels"])


def test_extract_requires_segmentwise():
    import importlib.util, os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("clift_extract_cli", os.path.join(REPO, "inference", "extract_train_centroids.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match="segmentwise"):
        mod.extract_train_centroids(None, "trajectory_blender", segmentwise=False)
    fb = importlib.util.spec_from_file_location("clift_fb_cli", os.path.join(REPO, "inference", "find_bandwidth.py"))
    fbm = importlib.util.module_from_spec(fb)
    fb.loader.exec_module(fbm)
    r = fbm.sweep_range(3, True, False)                      # the reference's MOS range: np.arange from sqrt(3)/3.5/50 (50 values)
    assert len(r) == 50 and abs(r[0] - np.sqrt(3) / 3.5 / 50) < 1e-15
    assert len(fbm.sweep_range(25, False, False)) == 24 and len(fbm.sweep_range(3, True, True)) == 19
