"""csrc/points3d.hip on the GPU: clift_knn_kth_dist against golden G24 (the reference's KD-tree column) and sklearn's KDTree in the test
process, clift_segment_moments / clift_segment_extent against numpy fp64, the device backend of contrastive_lift_amd.points3d against the
host backend and G24, and render_panopli.py --save_pointcloud -> fit_bboxes.py end to end on a tiny trained MOS run."""
import importlib.util
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO
from test_points3d_host import check_boxes_against_g24, check_keep_against_g24, g24, inside_box

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(REPO, "tools"))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sorted_cloud(points, labels):
    from contrastive_lift_amd import points3d
    lab = torch.as_tensor(labels.astype(np.int64), device="cuda")
    order, ids, seg = points3d.group_by_instance(lab, 0)
    ps = torch.as_tensor(points, device="cuda")[order].contiguous()
    return ps, seg, order.cpu().numpy(), ids.cpu().numpy()


def test_knn_kth_dist_g24_bit_exact():
    from contrastive_lift_amd import _lib, points3d
    g, rec = g24()
    ps, seg, order, ids = sorted_cloud(g["points"], g["labels"])
    a = points3d.knn_kth_dist2(ps, seg, 10)
    b = points3d.knn_kth_dist2(ps, seg, 10)
    assert torch.equal(a, b)                                                               # two runs, the same bits
    d = np.sqrt(a.cpu().numpy())                                                           # fp64 sqrt: correctly rounded, as in the KD-tree
    want = g["kth_dist"][order]
    assert np.array_equal(d, want), (int((d != want).sum()), float(np.abs(d - want)[np.isfinite(want)].max()))
    short = g["labels"][order] == 40
    assert short.sum() == 9 and np.isinf(d[short]).all() and np.isfinite(d[~short]).all()
    assert (d[g["labels"][order] == 17] == 0).sum() >= 240
    for k in (1, 4, 5, 16):                                                                # every register-array width of the kernel
        from sklearn.neighbors import KDTree
        got = np.sqrt(points3d.knn_kth_dist2(ps, seg, k).cpu().numpy())
        e = seg.cpu().numpy()
        for lo, hi in zip(e[:-1], e[1:]):
            P = ps[lo:hi].cpu().numpy()
            ref = KDTree(P).query(P, k=k)[0][:, -1] if hi - lo >= k else np.full(hi - lo, np.inf)
            assert np.array_equal(got[lo:hi], ref), (k, lo, hi)
    with pytest.raises(_lib.CliftError, match="16"):
        points3d.knn_kth_dist2(ps, seg, 17)
    with pytest.raises(_lib.CliftError, match="k"):
        points3d.knn_kth_dist2(ps, seg, 0)


def test_knn_one_large_instance_beside_300_small_ones():
    from sklearn.neighbors import KDTree
    from contrastive_lift_amd import points3d
    rng = np.random.default_rng(50)
    sizes = [50000] + rng.integers(100, 400, 300).tolist()
    pts = np.concatenate([rng.uniform(-2, 2, 3) + rng.standard_normal((n, 3)) * rng.uniform(0.02, 0.3, 3) for n in sizes]).astype(np.float32)
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), device="cuda")
    ps = torch.as_tensor(pts, device="cuda")
    points3d.knn_kth_dist2(ps, seg, 10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d2 = points3d.knn_kth_dist2(ps, seg, 10)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = np.sqrt(d2.cpu().numpy())
    e = seg.cpu().numpy()
    t2 = time.perf_counter()
    want = np.concatenate([KDTree(pts[lo:hi]).query(pts[lo:hi], k=10)[0][:, -1] for lo, hi in zip(e[:-1], e[1:])])
    t3 = time.perf_counter()
    print(f"{pts.shape[0]} points, 1 x 50000 + 300 small: device {1e3 * (t1 - t0):.2f} ms, KDTree loop {t3 - t2:.2f} s")
    assert np.array_equal(got, want), int((got != want).sum())
    assert torch.equal(d2, points3d.knn_kth_dist2(ps, seg, 10))


def test_segment_moments_and_extent_vs_numpy():
    """Against numpy fp64 on G24, relative 1e-12: a sum is compared relative to the sum of the magnitudes of its terms (the scale that
    bounds the rounding error of any summation order: <= n eps = 7e-13 for the largest instance, far less in practice), an extent relative
    to the largest projected magnitude of the instance."""
    from contrastive_lift_amd import points3d
    g, _ = g24()
    ps, seg, order, ids = sorted_cloud(g["points"], g["labels"])
    G = ids.shape[0]
    rng = np.random.default_rng(1)
    keep_np = rng.uniform(size=ps.shape[0]) < 0.7
    centre_np = rng.uniform(-1, 1, (G, 3))
    axes_np = np.linalg.qr(rng.standard_normal((G, 3, 3)))[0]
    P = ps.cpu().numpy().astype(np.float64)
    e = seg.cpu().numpy()
    for keep, centre in ((None, None), (keep_np, None), (keep_np, centre_np)):
        kt = None if keep is None else torch.as_tensor(keep, device="cuda")
        ct = None if centre is None else torch.as_tensor(centre, device="cuda")
        a = points3d.segment_moments(ps, seg, kt, ct)
        assert torch.equal(a, points3d.segment_moments(ps, seg, kt, ct))                   # fixed split: the same bits
        a = a.cpu().numpy()
        frame = torch.as_tensor(np.concatenate([axes_np.reshape(G, 9), np.zeros((G, 3)) if centre is None else centre], 1), device="cuda")
        x = points3d.segment_extent(ps, seg, frame, kt)
        assert torch.equal(x, points3d.segment_extent(ps, seg, frame, kt))
        x = x.cpu().numpy()
        for gi in range(G):
            S = P[e[gi]:e[gi + 1]]
            if keep is not None:
                S = S[keep[e[gi]:e[gi + 1]]]
            q = S - (0.0 if centre is None else centre[gi])
            terms = np.stack([np.ones(len(q)), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                              q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], 1)
            want, scale = terms.sum(0), np.abs(terms).sum(0)
            assert a[gi, 0] == len(q)
            assert (np.abs(a[gi] - want) <= 1e-12 * scale).all(), (gi, a[gi] - want)
            if len(q):
                proj = q @ axes_np[gi].T
                wx = np.concatenate([proj.min(0), proj.max(0)])
                assert (np.abs(x[gi] - wx) <= 1e-12 * np.abs(proj).max()).all(), (gi, x[gi] - wx)
    # an instance without kept rows: zeros / +-inf
    none = torch.zeros(ps.shape[0], dtype=torch.bool, device="cuda")
    assert (points3d.segment_moments(ps, seg, none) == 0).all()
    x = points3d.segment_extent(ps, seg, frame, none).cpu().numpy()
    assert np.isposinf(x[:, :3]).all() and np.isneginf(x[:, 3:]).all()


def test_device_backend_equals_host_backend_and_g24():
    from contrastive_lift_amd import points3d
    g, rec = g24()
    kd, sd = points3d.filter_pointcloud(g["points"], g["labels"], backend="device", return_stages=True)
    kh, sh = points3d.filter_pointcloud(g["points"], g["labels"], backend="sklearn", return_stages=True)
    assert kd.is_cuda
    assert np.array_equal(sd["kth_dist"].cpu().numpy(), sh["kth_dist"].numpy())            # the device sqrt too is correctly rounded
    assert np.array_equal(sd["stage1"].cpu().numpy(), sh["stage1"].numpy())
    assert np.array_equal(kd.cpu().numpy(), kh.numpy())
    check_keep_against_g24(kd.cpu().numpy(), g, rec)
    for method in ("simple", "pca"):
        boxes, info = points3d.fit_instance_boxes(torch.as_tensor(g["points"], device="cuda"), torch.as_tensor(g["labels"].astype(np.int64), device="cuda"),
                                                  method=method, backend="device", return_info=True)
        check_boxes_against_g24(boxes, g, rec, method)
        assert np.array_equal(info["keep"].cpu().numpy(), kh.numpy())
        host = points3d.fit_instance_boxes(g["points"], g["labels"], method=method, backend="sklearn")
        for i in host:
            for key in ("orientation", "position"):
                assert np.abs(boxes[i][key] - host[i][key]).max() <= 1e-9, (method, i, key)
            assert np.abs(np.stack(boxes[i]["bbox"]) - np.stack(host[i]["bbox"])).max() <= 1e-9 * rec["diameter"]
    # the subsample branch on the device: seeded, a subset
    runs = [points3d.fit_instance_boxes(g["points"], g["labels"], max_points=1000, generator=torch.Generator().manual_seed(5), backend="device",
                                        return_info=True) for _ in range(2)]
    assert torch.equal(runs[0][1]["keep"], runs[1][1]["keep"]) and runs[0][1]["kept"][3] <= 700
    assert points3d.fit_instance_boxes(g["points"], np.zeros_like(g["labels"]), backend="device") == {}


def test_render_save_pointcloud_then_fit_bboxes(tmp_path, monkeypatch):
    """A tiny synthetic MOS run (the recipe of the mean-shift end-to-end test), render_panopli --save_pointcloud, fit_bboxes.py."""
    import make_synthetic_mos as gen
    from contrastive_lift_amd import points3d
    from contrastive_lift_amd.config import load_run_config
    from contrastive_lift_amd.data import get_scene
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_scene"), n_frames=40, size=64, trajectory_frames=3)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "e2e_points3d")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_p3")
    run_dir = train.main(["+experiment=contrastive_lift_MOS", f"dataset_root={scene_dir}", "image_dim=64", "min_grid_dim=32",
                          "max_grid_dim=64", "max_epoch=6", "steps_per_epoch=400", "batch_size=2048", "chunk=0", "max_depth=3",
                          "seed=3", "max_rays_instances=512", "decay_step=[4,5]"])
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.subsample_frames, cfg.image_dim = ckpt, 2, [64, 64]
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_p3")
    np.random.seed(0)
    out_plain = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, meanshift="device")
    assert not (out_plain / "pointcloud.pkl").exists()                                     # opt-in: off unless asked for
    np.random.seed(0)
    out = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, meanshift="device", save_pointcloud=True)
    cloud = pickle.load(open(out / "pointcloud.pkl", "rb"))
    scene = get_scene(cfg, "test", torch.device("cuda:0"))
    names = [scene.all_frame_names[i] for i in scene.val_indices]
    H, W = scene.image_dim
    P = len(names) * H * W
    assert cloud["points"].shape == (P, 3) and cloud["points"].dtype == np.float32 and np.isfinite(cloud["points"]).all()
    assert cloud["instances"].shape == (P,) and cloud["semantics"].shape == (P,) and cloud["semantics"].dtype == np.uint8
    assert cloud["rgb"].shape == (P, 3) and cloud["rgb"].dtype == np.uint8
    png = np.concatenate([np.asarray(Image.open(out / "pred_surrogateid" / f"{n}.png")).reshape(-1) for n in names])
    assert np.array_equal(cloud["instances"].astype(np.int64), png.astype(np.int64))
    sem = np.concatenate([np.asarray(Image.open(out / "pred_semantics" / f"{n}.png")).reshape(-1) for n in names])
    assert np.array_equal(cloud["semantics"], sem)
    assert (cloud["instances"] > 0).any()
    bounds = scene.scene_bounds.cpu().numpy().astype(np.float64)
    for method in ("pca", "simple"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "inference", "fit_bboxes.py"), "--pointcloud", str(out / "pointcloud.pkl"),
                            "--method", method, "--max_points", "200000"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        print(r.stdout[-1500:])
        boxes = pickle.load(open(out / "bboxes.pkl", "rb"))
        assert len(boxes) >= 1
        keep = points3d.filter_pointcloud(cloud["points"], cloud["instances"].astype(np.int64), backend="device").cpu().numpy()
        diam = float(np.linalg.norm(bounds[1] - bounds[0]))
        for i, b in boxes.items():
            assert i != 0 and set(b) == {"bbox", "orientation", "position"}
            kept = cloud["points"][(cloud["instances"] == i) & keep]
            assert kept.shape[0] > 0 and inside_box(kept, b, method, 1e-9 * diam), (method, i)
            assert (b["position"] >= bounds[0]).all() and (b["position"] <= bounds[1]).all(), (method, i, b["position"])
