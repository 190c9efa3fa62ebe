"""clift_segment_mvee (csrc/points3d.hip) on the GPU: golden G26 (the reference's getMinVolEllipse on the cloud of G24) through the kernel,
run-to-run bits, skipping against removing rows, the edge layout and the large layout of tests/ellipsoid_cases.py against the numpy helper,
the max_iter stop, the device backend of fit_instance_ellipsoids against the host backend, and render_panopli.py --save_pointcloud ->
fit_bboxes.py --method ellipsoid -> an edit_scene delete end to end on a tiny trained MOS run."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import ellipsoid_cases as ec
from conftest import REPO
from test_ellipsoid_host import check_boxes_against_g26, g26, host_fit
from test_gpu_points3d import _load, sorted_cloud

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(REPO, "tools"))


def mvee(pts, seg, keep=None, **kw):
    from contrastive_lift_amd import points3d
    out, u = points3d.segment_mvee(torch.as_tensor(pts, device="cuda"), torch.as_tensor(seg, device="cuda"),
                                   None if keep is None else torch.as_tensor(keep, device="cuda"), **kw)
    return out, u


@functools.lru_cache(maxsize=None)
def g26_run():
    """G24 sorted by instance with keep_fp64 as the keep mask, through the kernel once: (ps, seg, keep, order, ids, out, u)."""
    g, _, _ = g26()
    ps, seg, order, ids = sorted_cloud(g["points"], g["labels"])
    keep = torch.as_tensor(g["keep_fp64"][order], device="cuda")
    out, u = mvee(ps, seg, keep)
    return ps, seg, keep, order, ids, out, u


@functools.lru_cache(maxsize=None)
def helper_on(which):
    pts, seg = ec.edge_layout() if which == "edge" else ec.large_layout()
    return pts, seg, [ec.khachiyan(pts[lo:hi]) for lo, hi in zip(seg[:-1], seg[1:])]


def assert_rows_equal_helper(out, refs, which, rel=1e-9):
    """Same iteration count, and centre / second moment / err within ``rel`` of the instance's scale (the largest |coordinate| for the
    centre, the largest entry of C for C)."""
    for gi, r in enumerate(refs):
        if r["status"] == 2:
            continue
        row = out[gi]
        assert row[3] == r["status"] and row[1] == r["iters"], (which, gi, row[:4], r["iters"])
        scale = max(1.0, float(np.abs(r["centre"]).max()))
        assert np.abs(row[4:7] - r["centre"]).max() <= rel * scale, (which, gi, row[4:7] - r["centre"])
        C = ec.second_moment(row[7:13])
        assert np.abs(C - r["C"]).max() <= rel * np.abs(r["C"]).max(), (which, gi, np.abs(C - r["C"]).max())
        assert abs(row[2] - r["err"]) <= rel * max(r["err"], 1e-3), (which, gi, row[2], r["err"])


def test_g26_through_the_kernel():
    g, e, rec = g26()
    ps, seg, keep, order, ids, out_t, u_t = g26_run()
    out, u = out_t.cpu().numpy(), u_t.cpu().numpy()
    edges, keep_np = seg.cpu().numpy(), keep.cpu().numpy()
    assert out.shape == (12, 14) and np.isfinite(out).all() and np.isfinite(u).all()
    assert (u >= 0).all() and (u[~keep_np] == 0).all()
    boxes, iters = {}, {}
    for gi, i in enumerate(ids.tolist()):
        lo, hi = edges[gi], edges[gi + 1]
        if i == 40:                                                                        # nine rows, none kept
            assert out[gi, 0] == 0 and out[gi, 3] == 2 and (out[gi, 4:] == 0).all() and (u[lo:hi] == 0).all()
            continue
        assert out[gi, 3] == 0 and out[gi, 0] == rec["kept"][str(i)] and 0 < out[gi, 2] <= 0.01 and out[gi, 13] == 0
        assert abs(u[lo:hi].sum() - 1.0) <= 1e-12, (i, u[lo:hi].sum() - 1.0)
        radii, rotation = ec.ellipsoid_of(ec.second_moment(out[gi, 7:13]))
        boxes[i] = {"bbox": (-radii, radii), "orientation": rotation, "position": out[gi, 4:7]}
        iters[i] = int(out[gi, 1])
    assert sorted(rec["kept"].values()) == [7, 28, 105, 210, 420, 700, 1050, 1400, 2100, 2800, 4200]
    check_boxes_against_g26(boxes, iters, g, e, rec)


def test_two_runs_give_the_same_bits():
    ps, seg, keep, _, _, out, u = g26_run()
    out2, u2 = mvee(ps, seg, keep)
    assert torch.equal(out, out2) and torch.equal(u, u2)


def test_skipping_rows_equals_removing_them():
    """keep = None on a compacted copy of the kept rows against keep on all rows.  The path is the same (m, iters, status are compared
    exactly), but not every bit: the sums of the kernel (mean, first V, centre, second moment) run over the fixed split "row lo + t + 256 j
    on thread t" of clift_segment_moments, which is a split of the instance's ROWS, kept or not, so removing rows regroups the terms and the
    sums differ in their last bits.  Hence 1e-13 (of max(1, |value|)) for centre, C and err, and for u."""
    ps, seg, keep, _, _, out, u = g26_run()
    inst = torch.repeat_interleave(torch.arange(seg.numel() - 1, device="cuda"), seg[1:] - seg[:-1])
    seg_c = torch.zeros_like(seg)
    seg_c[1:] = torch.cumsum(torch.bincount(inst[keep], minlength=seg.numel() - 1), 0)
    out_c, u_c = mvee(ps[keep].contiguous(), seg_c)
    a, b = out.cpu().numpy(), out_c.cpu().numpy()
    assert np.array_equal(a[:, [0, 1, 3, 13]], b[:, [0, 1, 3, 13]])
    assert (np.abs(a - b) <= 1e-13 * np.maximum(1.0, np.abs(a))).all(), np.abs(a - b).max()
    assert (u[keep] - u_c).abs().max().item() <= 1e-13


def test_edge_layout_in_one_call():
    from contrastive_lift_amd import _lib, points3d
    pts, seg, refs = helper_on("edge")
    assert [r["status"] for r in refs] == ec.EDGE_STATUS and all(r["margin"] > 1e-9 for r in refs if r["status"] == 0 and r["iters"] > 1)
    out_t, u_t = mvee(pts, seg)
    out, u = out_t.cpu().numpy(), u_t.cpu().numpy()
    assert out.shape == (7, 14) and np.isfinite(out).all() and np.isfinite(u).all()
    assert out[:, 3].tolist() == ec.EDGE_STATUS and out[:, 0].tolist() == np.diff(seg).tolist()
    assert out[0, 1] == 1 and np.abs(out[0, 4:7]).max() <= 1e-12                           # the tetrahedron: one iteration, the sphere of radius sqrt(3)
    assert np.abs(ec.ellipsoid_of(ec.second_moment(out[0, 7:13]))[0] - np.sqrt(3.0)).max() <= 1e-12
    assert_rows_equal_helper(out, refs, "edge")
    for gi, st in enumerate(ec.EDGE_STATUS):
        rows = u[seg[gi]:seg[gi + 1]]
        if st == 2:
            assert (out[gi, 4:] == 0).all() and out[gi, 2] == 0 and (rows == 0).all()
        else:
            assert abs(rows.sum() - 1.0) <= 1e-12 and (rows >= 0).all()
            assert np.abs(rows - refs[gi]["u"]).max() <= 1e-9
    # the host backend's loop gives the same rows
    for gi in (0, 4, 6):
        row, _ = points3d._mvee_host(pts[seg[gi]:seg[gi + 1]].astype(np.float64), 0.01, 10000)
        assert row[1] == out[gi, 1] and np.abs(row - out[gi]).max() <= 1e-9
    # nothing to do, and refused arguments
    ps, sg = torch.as_tensor(pts, device="cuda"), torch.as_tensor(seg, device="cuda")
    o0, u0 = points3d.segment_mvee(ps[:0].contiguous(), torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert o0.shape == (2, 14) and (o0.cpu().numpy()[:, 3] == 2).all() and u0.numel() == 0
    o0, u0 = points3d.segment_mvee(ps, sg[:1].contiguous())
    assert o0.shape == (0, 14) and (u0 == 0).all()
    lib = _lib.load()
    assert lib.clift_segment_mvee(None, 0, None, 0, None, 0.01, 10, None, None, _lib.stream()) == 0
    o1 = torch.full((1, 14), -1.0, dtype=torch.float64, device="cuda")
    assert lib.clift_segment_mvee(None, 0, _lib.ptr(sg), 1, None, 0.01, 10, None, _lib.ptr(o1), _lib.stream()) == 0
    assert o1.cpu().numpy().tolist() == [[0, 0, 0, 2] + [0] * 10]
    for kw in ({"max_iter": 0}, {"tolerance": 0.0}, {"max_iter": 1000001}, {"tolerance": float("nan")}):
        with pytest.raises(_lib.CliftError, match="max_iter|tolerance"):
            points3d.segment_mvee(ps, sg, **kw)


def test_one_large_instance_beside_300_small_ones():
    pts, seg, refs = helper_on("large")
    assert pts.shape[0] == 20000 + 300 * 30 and len(refs) == 301
    margin = min(r["margin"] for r in refs)
    assert all(r["status"] == 0 for r in refs) and margin > 1e-9, \
        f"seed {ec.LARGE_SEED} of ellipsoid_cases.large_layout leaves an argmax margin of {margin:.3e}: choose another seed, the kernel was not run"
    out_t, u_t = mvee(pts, seg)
    out, u = out_t.cpu().numpy(), u_t.cpu().numpy()
    print(f"large layout: {int(out[0, 1])} iterations on 20000 rows, {int(out[1:, 1].min())} .. {int(out[1:, 1].max())} on the small ones, margin {margin:.3e}")
    assert np.isfinite(out).all() and (out[:, 3] == 0).all()
    assert_rows_equal_helper(out, refs, "large")
    assert np.abs(u - np.concatenate([r["u"] for r in refs])).max() <= 1e-9
    out2, u2 = mvee(pts, seg)
    assert torch.equal(out_t, out2) and torch.equal(u_t, u2)


def test_max_iter_stops_with_the_last_iterate():
    g, _, _ = g26()
    ps, seg, keep, _, ids, _, _ = g26_run()
    out = mvee(ps, seg, keep, tolerance=1e-7, max_iter=50)[0].cpu().numpy()
    gi = ids.tolist().index(8)
    ref = ec.khachiyan(g["points"][(g["labels"] == 8) & g["keep_fp64"]], tolerance=1e-7, max_iter=50)
    assert ref["status"] == 1 and ref["iters"] == 50 and ref["margin"] > 1e-9
    assert out[gi, 3] == 1 and out[gi, 1] == 50 and out[gi, 2] > 1e-7
    assert_rows_equal_helper(out[gi:gi + 1], [ref], "max_iter")
    live = out[:, 0] >= 4
    assert (out[live, 3] == 1).all() and (out[live, 1] == 50).all() and (out[~live, 3] == 2).all()


def test_device_backend_equals_host_backend_on_g24():
    from contrastive_lift_amd import points3d
    g, e, rec = g26()
    boxes, info = points3d.fit_instance_ellipsoids(torch.as_tensor(g["points"], device="cuda"), torch.as_tensor(g["labels"].astype(np.int64), device="cuda"),
                                                   backend="device", return_info=True)
    host, hinfo = host_fit()
    assert sorted(boxes) == sorted(host) and info["iters"] == hinfo["iters"] and info["kept"] == hinfo["kept"] and info["not_converged"] == []
    assert np.array_equal(info["keep"].cpu().numpy(), hinfo["keep"].numpy())
    for i in host:
        assert np.abs(boxes[i]["position"] - host[i]["position"]).max() <= 1e-9 * rec["diameter"]
        assert np.abs(np.stack(boxes[i]["bbox"]) - np.stack(host[i]["bbox"])).max() <= 1e-9 * rec["diameter"]
        assert ec.axis_gap(boxes[i]["orientation"], host[i]["orientation"]) <= 1e-9
        assert abs(info["err"][i] - hinfo["err"][i]) <= 1e-9
    check_boxes_against_g26(boxes, info["iters"], g, e, rec)
    assert points3d.fit_instance_ellipsoids(g["points"], np.zeros_like(g["labels"]), backend="device") == {}


def test_render_save_pointcloud_fit_ellipsoids_then_delete(tmp_path, monkeypatch):
    """The tiny synthetic MOS run of test_render_save_pointcloud_then_fit_bboxes: render --save_pointcloud, fit_bboxes.py --method ellipsoid,
    then an edit_scene delete of one fitted instance renders."""
    import make_synthetic_mos as gen
    from contrastive_lift_amd.config import load_run_config
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_scene"), n_frames=40, size=64, trajectory_frames=3)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "e2e_ellipsoid")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_ell")
    run_dir = train.main(["+experiment=contrastive_lift_MOS", f"dataset_root={scene_dir}", "image_dim=64", "min_grid_dim=32",
                          "max_grid_dim=64", "max_epoch=6", "steps_per_epoch=400", "batch_size=2048", "chunk=0", "max_depth=3",
                          "seed=3", "max_rays_instances=512", "decay_step=[4,5]"])
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.subsample_frames, cfg.image_dim = ckpt, 2, [64, 64]
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_ell")
    np.random.seed(0)
    out = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, meanshift="device", save_pointcloud=True)
    r = subprocess.run([sys.executable, os.path.join(REPO, "inference", "fit_bboxes.py"), "--pointcloud", str(out / "pointcloud.pkl"),
                        "--method", "ellipsoid", "--max_points", "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout[-1500:])
    assert " iterations" in r.stdout and "(ellipsoid, backend device)" in r.stdout
    boxes = pickle.load(open(out / "bboxes.pkl", "rb"))
    assert len(boxes) >= 1
    for i, b in boxes.items():
        assert i != 0 and set(b) == {"bbox", "orientation", "position"}
        assert np.isfinite(b["position"]).all() and (np.asarray(b["bbox"][1]) > 0).all() and np.array_equal(b["bbox"][0], -np.asarray(b["bbox"][1]))
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_scene_ell_gpu")
    inst = sorted(boxes)[0]
    edited = es.edit_scene_checkpoint(cfg, es.resolve_edit(boxes, inst, "delete"), f"delete_{inst}")
    assert len(os.listdir(edited / "rgb")) >= 1 and len(os.listdir(edited / "rgb")) == len(os.listdir(edited / "depth"))
