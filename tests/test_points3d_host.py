"""contrastive_lift_amd.points3d on the host (backend="sklearn") against golden G24, recorded from the reference's own
inference/visualize_bboxes.py (filter_pointcloud, get_tight_bbox "simple" / "pca") by tests/golden/make_points3d_golden.py, and the
fit_bboxes.py CLI round trip.  No GPU."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_golden


def g24():
    return load_golden("g24_points3d"), json.load(open(os.path.join(GOLDEN, "g24_points3d.json")))


def check_boxes_against_g24(boxes, g, rec, method):
    """Centre, extents and (pca) axes up to sign within the tolerances the generator wrote: 10x the reference-vs-fp64 difference it
    measured, floor 1e-6 of the cloud's diameter (1e-6 for the dimensionless 1 - |<a_port, a_ref>|)."""
    tol = rec[method]["tol"]
    ids = g[f"{method}.ids"].tolist()
    assert sorted(boxes) == ids
    worst = {"centre": 0.0, "extent": 0.0, "axis": 0.0}
    for j, i in enumerate(ids):
        b = boxes[i]
        assert np.asarray(b["bbox"][0]).shape == (3,) and np.asarray(b["bbox"][1]).shape == (3,)
        assert b["orientation"].shape == (3, 3) and b["position"].shape == (3,)
        worst["centre"] = max(worst["centre"], float(np.abs(b["position"] - g[f"{method}.position"][j]).max()))
        dots = np.sum(b["orientation"] * g[f"{method}.orientation"][j], -1)
        worst["axis"] = max(worst["axis"], float(np.max(1.0 - np.abs(dots))))
        mn, mx = np.asarray(b["bbox"][0]), np.asarray(b["bbox"][1])
        flip = dots < 0
        mn, mx = np.where(flip, -mx, mn), np.where(flip, -mn, mx)
        worst["extent"] = max(worst["extent"], float(np.abs(np.stack([mn, mx]) - g[f"{method}.bbox"][j]).max()))
    print(f"G24 {method}: worst differences {worst}, tolerances {tol}")
    for what in worst:
        assert worst[what] <= tol[what], (method, what, worst[what], tol[what])


def check_keep_against_g24(keep, g, rec):
    """At most the number of differing points per instance that the generator found between the reference (float32 statistics) and fp64
    statistics -- itself asserted there to be within max(2, 0.1 % of the instance)."""
    for i, allowed in rec["differing_points"].items():
        rows = g["labels"] == int(i)
        differ = int((keep[rows] != g["keep_ref"][rows]).sum())
        assert allowed <= max(2, int(0.001 * rec["sizes"][i]))
        assert differ <= allowed, (i, differ, allowed)
    assert not keep[np.isin(g["labels"], [0] + rec["skipped"])].any()


def inside_box(points, box, method, eps):
    """The reference's own check (visualize_bboxes.py:312-315) maps into the box frame with ``matmul(orientation.T, local.T).T``: that
    treats the COLUMNS of ``orientation`` as axes, which holds for "simple" (identity) only -- ``get_tight_bbox(..., "pca")`` stores
    ``pca.components_``, whose ROWS are the axes (its boxes are min / max of ``pca.transform``).  "simple" is checked with the reference's
    mapping as written, "pca" with the mapping its boxes were made with."""
    local = points.astype(np.float64) - box["position"]
    local = np.matmul(box["orientation"].T, local.T).T if method == "simple" else np.matmul(box["orientation"], local.T).T
    return bool(np.all((local >= np.asarray(box["bbox"][0]) - eps) & (local <= np.asarray(box["bbox"][1]) + eps)))


def test_sklearn_backend_reproduces_g24_distances_and_stage1():
    from contrastive_lift_amd import points3d
    g, rec = g24()
    keep, st = points3d.filter_pointcloud(g["points"], g["labels"], backend="sklearn", return_stages=True)
    d = st["kth_dist"].numpy()
    assert d.dtype == np.float64 and np.isinf(d[np.isin(g["labels"], [0] + rec["skipped"])]).all()
    assert np.array_equal(d, g["kth_dist"]), int((d != g["kth_dist"]).sum())              # both are the fp64 KD-tree: to the last bit
    assert (d[g["labels"] == 17] == 0).sum() >= 240                                        # the exact duplicates
    assert np.array_equal(st["stage1"].numpy(), g["stage1"])
    check_keep_against_g24(keep.numpy(), g, rec)
    assert np.array_equal(keep.numpy(), g["keep_fp64"])


@pytest.mark.parametrize("method", ["simple", "pca"])
def test_sklearn_backend_boxes_vs_g24(method):
    from contrastive_lift_amd import points3d
    g, rec = g24()
    boxes, info = points3d.fit_instance_boxes(g["points"], g["labels"], method=method, backend="sklearn", return_info=True)
    check_boxes_against_g24(boxes, g, rec, method)
    assert 0 not in boxes and 40 not in boxes and info["total"][40] == 9 and info["kept"][40] == 0
    assert info["kept"][31] == 7 and info["total"][31] == 10                               # exactly k points: 70 % strictly below the percentile
    if method == "pca":
        for b in boxes.values():
            o = b["orientation"]
            assert np.allclose(o @ o.T, np.eye(3), atol=1e-12)
            assert (o[np.arange(3), np.abs(o).argmax(1)] > 0).all()                        # the stated sign rule
            ext = b["bbox"][1] - b["bbox"][0]
            assert ext[0] >= ext[2]


@pytest.mark.parametrize("method", ["simple", "pca"])
def test_fit_bboxes_cli_round_trip(tmp_path, method):
    from contrastive_lift_amd import points3d
    g, rec = g24()
    with open(tmp_path / "pointcloud.pkl", "wb") as f:
        pickle.dump({"points": g["points"], "instances": g["labels"].astype(np.uint16)}, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "inference", "fit_bboxes.py"), "--pointcloud", str(tmp_path / "pointcloud.pkl"),
                        "--backend", "sklearn", "--method", method], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "filter + fit" in r.stdout and r.stdout.count("instance ") == 12
    boxes = pickle.load(open(tmp_path / "bboxes.pkl", "rb"))
    check_boxes_against_g24(boxes, g, rec, method)
    keep = points3d.filter_pointcloud(g["points"], g["labels"], backend="sklearn").numpy()
    for i, b in boxes.items():
        assert set(b) == {"bbox", "orientation", "position"} and len(b["bbox"]) == 2
        kept = g["points"][(g["labels"] == i) & keep]
        # 1e-9 of the diameter: the box and this check round a three-term fp64 dot product in different orders (a few ulp of ~10)
        assert kept.shape[0] > 0 and inside_box(kept, b, method, 1e-9 * rec["diameter"]), i


def test_rejected_methods_empty_labels_and_subsample():
    from contrastive_lift_amd import points3d
    g, _ = g24()
    for method in ("ellipsoid", "oriented"):
        with pytest.raises(ValueError, match="pca.*simple"):
            points3d.fit_instance_boxes(g["points"], g["labels"], method=method, backend="sklearn")
    with pytest.raises(ValueError, match="backend"):
        points3d.fit_instance_boxes(g["points"], g["labels"], backend="numpy")
    assert points3d.fit_instance_boxes(g["points"], np.zeros_like(g["labels"]), backend="sklearn") == {}
    assert not points3d.filter_pointcloud(g["points"], np.zeros_like(g["labels"]), backend="sklearn").any()
    runs = []
    for seed in (5, 5, 6):
        gen = torch.Generator().manual_seed(seed)
        boxes, info = points3d.fit_instance_boxes(g["points"], g["labels"], method="pca", max_points=1000, generator=gen, backend="sklearn",
                                                  return_info=True)
        runs.append((boxes, info["keep"].numpy()))
        for i, n in info["total"].items():
            assert info["kept"][i] <= min(n, 1000)
        assert info["kept"][3] <= 700 and info["total"][3] == 6000                         # 70 % of the 1000 drawn, at most
        assert not runs[-1][1][g["labels"] == 0].any()
    (b0, k0), (b1, k1), (b2, k2) = runs
    assert np.array_equal(k0, k1) and not np.array_equal(k0, k2)
    for i in b0:
        for key in ("orientation", "position"):
            assert np.array_equal(b0[i][key], b1[i][key])
        assert np.array_equal(np.stack(b0[i]["bbox"]), np.stack(b1[i]["bbox"]))
    small = g["labels"] == 13                                                              # 1000 points: not subsampled, same rows as without a cap
    full = points3d.fit_instance_boxes(g["points"], g["labels"], method="pca", backend="sklearn", return_info=True)[1]["keep"].numpy()
    assert np.array_equal(k0[small], full[small])


def test_backproject_and_percentile_match_numpy():
    from contrastive_lift_amd import points3d
    rng = np.random.default_rng(0)
    rays = torch.from_numpy(rng.standard_normal((50, 8)).astype(np.float32))
    dist = torch.from_numpy(rng.uniform(0, 3, 50).astype(np.float32))
    assert torch.equal(points3d.backproject(rays, dist), rays[:, :3] + dist[:, None] * rays[:, 3:6])
    counts = [1, 2, 3, 10, 11, 101, 1000, 4, 7]
    d = torch.from_numpy(rng.uniform(0, 1, sum(counts)))
    seg = torch.tensor(np.concatenate([[0], np.cumsum(counts)]))
    inst, c = points3d._instance_of_rows(seg)
    for pct in (70, 50, 0, 100, 33.3):
        got = points3d._segment_percentile(d, seg, inst, c, pct).numpy()
        want = np.array([np.percentile(d.numpy()[lo:hi], pct) for lo, hi in zip(seg[:-1].tolist(), seg[1:].tolist())])
        assert np.array_equal(got, want), (pct, got - want)
