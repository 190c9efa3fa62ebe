"""contrastive_lift_amd.points3d.fit_instance_ellipsoids on the host (backend="sklearn") against golden G26, recorded from the reference's
own getMinVolEllipse / get_tight_bbox(method="ellipsoid") by tests/golden/make_ellipsoid_golden.py on the cloud of G24; the fit_bboxes.py
CLI; the hand-made cases of tests/ellipsoid_cases.py.  No GPU."""
import functools
import importlib.util
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ellipsoid_cases as ec
from conftest import GOLDEN, REPO, load_golden


@functools.lru_cache(maxsize=None)
def g26():
    return load_golden("g24_points3d"), load_golden("g26_ellipsoid"), json.load(open(os.path.join(GOLDEN, "g26_ellipsoid.json")))


@functools.lru_cache(maxsize=None)
def host_fit():
    from contrastive_lift_amd import points3d
    g, _, _ = g26()
    return points3d.fit_instance_ellipsoids(g["points"], g["labels"], backend="sklearn", return_info=True)


def check_boxes_against_g26(boxes, iters, g, e, rec):
    """ids, iteration counts, centre / radii / axes (up to sign) within the json's tolerances, and the worst (p - c)^T A (p - c) over the
    kept rows no larger than the reference's own (x (1 + 1e-9))."""
    ids = e["ids"].tolist()
    assert sorted(boxes) == ids and 40 not in boxes and 0 not in boxes
    worst = {"centre": 0.0, "radii": 0.0, "axis": 0.0}
    for j, i in enumerate(ids):
        b = boxes[i]
        lo, hi = np.asarray(b["bbox"][0]), np.asarray(b["bbox"][1])
        assert lo.shape == hi.shape == (3,) and np.array_equal(lo, -hi) and b["orientation"].shape == (3, 3) and b["position"].shape == (3,)
        assert iters[i] == int(e["iters"][j]) == rec["iters"][str(i)], (i, iters[i], int(e["iters"][j]))
        worst["centre"] = max(worst["centre"], float(np.abs(b["position"] - e["centre"][j]).max()))
        worst["radii"] = max(worst["radii"], float(np.abs(hi - e["radii"][j]).max()))
        worst["axis"] = max(worst["axis"], ec.axis_gap(b["orientation"], e["rotation"][j]))
        kept = g["points"][(g["labels"] == i) & g["keep_fp64"]]
        w = ec.worst_norm(kept, b["position"], hi, b["orientation"])
        assert w <= float(e["worst_norm"][j]) * (1 + 1e-9), (i, w, float(e["worst_norm"][j]))
    print(f"G26: worst differences {worst}, tolerances {rec['tol']}")
    for what in worst:
        assert worst[what] <= rec["tol"][what], (what, worst[what], rec["tol"][what])


def test_fixture_is_consistent():
    """The generator's three assertions again, from the stored files, and the path of the test helper: a stale fixture fails here."""
    g, e, rec = g26()
    assert rec["same_path"] is True and rec["bbox_vs_ellipse"] <= 1e-12
    assert np.abs(e["bbox.position"] - e["centre"]).max() <= 1e-12 and np.abs(e["bbox.radii"] - e["radii"]).max() <= 1e-12
    assert np.abs(e["bbox.orientation"] - e["rotation"]).max() <= 1e-12
    assert rec["margin_floor"] == 1e-9 and min(rec["margin"].values()) > 1e-9 and float(e["margin"].min()) > 1e-9
    assert rec["tol"]["centre"] == max(10 * rec["ref_vs_restated"]["centre"], 1e-9 * rec["diameter"])
    assert rec["tol"]["radii"] == max(10 * rec["ref_vs_restated"]["radii"], 1e-9 * rec["diameter"])
    assert rec["tol"]["axis"] == max(10 * rec["ref_vs_restated"]["axis"], 1e-9)
    assert np.abs(e["restated.centre"] - e["centre"]).max() == rec["ref_vs_restated"]["centre"]
    assert e["kept"].tolist() == [4200, 2800, 2100, 1400, 1050, 700, 420, 210, 105, 28, 7]
    for j, i in enumerate(e["ids"].tolist()):
        rows = (g["labels"] == i) & g["keep_fp64"]
        assert int(rows.sum()) == int(e["kept"][j])
        picked = e["picked"][e["picked_off"][j]:e["picked_off"][j + 1]]
        assert len(picked) == int(e["iters"][j])
        r = ec.khachiyan(g["points"][rows])
        assert r["js"] == picked.tolist(), i                                               # the helper walks the reference's path
        assert r["margin"] > 1e-9
        assert 1.0 < float(e["worst_norm"][j]) < 1.1                                       # the reference's ellipsoid does not strictly enclose


def test_sklearn_backend_vs_g26():
    g, e, rec = g26()
    boxes, info = host_fit()
    check_boxes_against_g26(boxes, info["iters"], g, e, rec)
    assert info["not_converged"] == [] and info["kept"][40] == 0 and info["total"][40] == 9 and info["iters"][40] == 0
    assert {i: info["kept"][i] for i in boxes} == {int(i): n for i, n in rec["kept"].items()}
    assert np.array_equal(info["keep"].numpy(), g["keep_fp64"])
    for i, b in boxes.items():
        o = b["orientation"]
        assert np.allclose(o @ o.T, np.eye(3), atol=1e-12) and b["bbox"][1][0] <= b["bbox"][1][1] <= b["bbox"][1][2]
        assert 0 < info["err"][i] <= 0.01


def test_fit_bboxes_cli_ellipsoid(tmp_path):
    g, e, rec = g26()
    with open(tmp_path / "pointcloud.pkl", "wb") as f:
        pickle.dump({"points": g["points"], "instances": g["labels"].astype(np.uint16)}, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "inference", "fit_bboxes.py"), "--pointcloud", str(tmp_path / "pointcloud.pkl"),
                        "--backend", "sklearn", "--method", "ellipsoid"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "filter + fit" in r.stdout and r.stdout.count("instance ") == 12 and r.stdout.count(" iterations") == 11
    assert "instance 3: kept 4200 / 6000 points" in r.stdout and f"{rec['iters']['3']} iterations" in r.stdout
    boxes = pickle.load(open(tmp_path / "bboxes.pkl", "rb"))
    want, info = host_fit()
    check_boxes_against_g26(boxes, info["iters"], g, e, rec)
    for i in want:
        assert set(boxes[i]) == {"bbox", "orientation", "position"}
        for key in ("orientation", "position"):
            assert np.array_equal(boxes[i][key], want[i][key])
        assert np.array_equal(np.stack(boxes[i]["bbox"]), np.stack(want[i]["bbox"]))
    # a looser threshold is passed on: fewer iterations
    spec = importlib.util.spec_from_file_location("clift_fit_bboxes_ell", os.path.join(REPO, "inference", "fit_bboxes.py"))
    fb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fb)
    fb.fit_bboxes(str(tmp_path / "pointcloud.pkl"), "ellipsoid", "sklearn", out=str(tmp_path / "loose.pkl"), tolerance=0.05)
    loose = pickle.load(open(tmp_path / "loose.pkl", "rb"))
    assert sorted(loose) == sorted(want) and loose[3]["bbox"][1][2] < want[3]["bbox"][1][2]


def test_records_pass_through_resolve_edit():
    spec = importlib.util.spec_from_file_location("clift_edit_scene_ell", os.path.join(REPO, "inference", "edit_scene.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    g, _, _ = g26()
    boxes, _ = host_fit()
    for i, b in boxes.items():
        assert es.resolve_edit(boxes, i, "delete") is not None
        from contrastive_lift_amd import edit as ed
        box = ed.EditBox.from_fitted(b)
        kept = g["points"][(g["labels"] == i) & g["keep_fp64"]]
        # the box circumscribes the ellipsoid, and the ellipsoid holds the rows up to the reference's slack (norm <= 1.06)
        assert (np.abs(box.local(kept)) <= np.asarray(b["bbox"][1]) * np.sqrt(1.06)).all()


def fit_cases(parts, tolerance=0.01, max_iter=10000):
    """The host loop on hand-made instances as they are (the filter of fit_instance_ellipsoids would thin them out first)."""
    from contrastive_lift_amd import points3d
    return [points3d._mvee_host(np.asarray(p, np.float64).reshape(-1, 3), tolerance, max_iter) for p in parts]


def test_tetrahedron_and_repeated_centroid():
    (row, u), (row2, u2) = fit_cases([ec.TETRAHEDRON, ec.tetra_plus_centroid()])
    assert row[0] == 4 and row[1] == 1 and row[3] == 0                                     # the uniform weights are optimal: M = 4, step = 0
    radii, _ = ec.ellipsoid_of(ec.second_moment(row[7:13]))
    assert np.abs(row[4:7]).max() <= 1e-12 and np.abs(radii - np.sqrt(3.0)).max() <= 1e-12
    assert np.abs(u - 0.25).max() <= 1e-15
    # the four vertices tie in every iteration (a symmetry of the input), so which one rounding picks is free and only quantities that the
    # tetrahedron's symmetries leave alone are compared: the sorted radii and the length of the centre, against what the helper itself reaches
    ref = ec.khachiyan(ec.tetra_plus_centroid())
    r_ref, _ = ec.ellipsoid_of(ref["C"])
    reached = max(float(np.abs(r_ref - np.sqrt(3.0)).max()), float(np.linalg.norm(ref["centre"])))
    print(f"tetrahedron + 20 x centroid: the helper ends {reached:.3e} from the sphere after {ref['iters']} iterations")
    assert ref["status"] == 0 and reached < 0.05
    radii2, _ = ec.ellipsoid_of(ec.second_moment(row2[7:13]))
    assert row2[0] == 24 and row2[3] == 0
    assert np.abs(radii2 - np.sqrt(3.0)).max() <= reached + 1e-9 and np.linalg.norm(row2[4:7]) <= reached + 1e-9
    assert abs(u2.sum() - 1) <= 1e-12 and (u2 >= 0).all()


def test_degenerate_and_empty():
    from contrastive_lift_amd import points3d
    for P in (ec.COPLANAR4, ec.THREE, np.zeros((0, 3)), ec.TETRAHEDRON[:1]):
        row, u = fit_cases([P])[0]
        assert row[3] == 2 and row[0] == len(P) and (row[4:] == 0).all() and (u == 0).all() and np.isfinite(row).all()
        assert ec.khachiyan(P)["status"] == 2
    # through the public function: a good blob beside a coplanar and a 3-point instance (k = 3 lets the small ones reach the ellipsoid)
    rng = np.random.default_rng(5)
    flat = rng.integers(-64, 65, (40, 2)) / 64.0
    flat = np.concatenate([flat, flat.sum(1, keepdims=True)], 1)                           # z = x + y, exact in float32
    pts = np.concatenate([ec.blob(200, 3), flat, ec.THREE]).astype(np.float32)
    lab = np.concatenate([np.full(200, 4), np.full(40, 6), np.full(3, 9)])
    boxes, info = points3d.fit_instance_ellipsoids(pts, lab, backend="sklearn", k=3, return_info=True)
    assert sorted(boxes) == [4] and info["kept"][6] >= 4 and info["kept"][9] < 4 and info["not_converged"] == []
    assert points3d.fit_instance_ellipsoids(pts, np.zeros_like(lab), backend="sklearn") == {}
    g, _, _ = g26()
    assert points3d.fit_instance_ellipsoids(g["points"], np.zeros_like(g["labels"]), backend="sklearn") == {}
    with pytest.raises(ValueError, match="backend"):
        points3d.fit_instance_ellipsoids(pts, lab, backend="numpy")
    with pytest.raises(ValueError, match="max_iter"):
        points3d.fit_instance_ellipsoids(pts, lab, backend="sklearn", max_iter=0)
    with pytest.raises(ValueError, match="tolerance"):
        points3d.fit_instance_ellipsoids(pts, lab, backend="sklearn", tolerance=0.0)
    with pytest.raises(ValueError, match="pca.*simple.*fit_instance_ellipsoids"):
        points3d.fit_instance_boxes(pts, lab, method="ellipsoid", backend="sklearn")


def test_max_iter_stops_instance_8():
    from contrastive_lift_amd import points3d
    g, _, _ = g26()
    lab = np.where(g["labels"] == 8, 8, 0)
    boxes, info = points3d.fit_instance_ellipsoids(g["points"], lab, tolerance=1e-7, max_iter=50, backend="sklearn", return_info=True)
    assert sorted(boxes) == [8] and info["not_converged"] == [8] and info["iters"][8] == 50 and info["err"][8] > 1e-7
    ref = ec.khachiyan(g["points"][(g["labels"] == 8) & g["keep_fp64"]], tolerance=1e-7, max_iter=50)
    assert ref["status"] == 1 and ref["iters"] == 50 and ref["margin"] > 1e-9
    radii, rot = ec.ellipsoid_of(ref["C"])
    assert np.abs(boxes[8]["position"] - ref["centre"]).max() <= 1e-9 and np.abs(boxes[8]["bbox"][1] - radii).max() <= 1e-9
    assert ec.axis_gap(boxes[8]["orientation"], rot) <= 1e-9
