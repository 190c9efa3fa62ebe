"""tests/points3d_cases.py on the host (CPU only): the layouts have the geometry they are there for, the references agree with each other
to their derived bound, every deliberately wrong variant is caught by some case, the argmax margin of the ellipsoid helper leaves at most
one instance per layout out of the comparison, ``group_by_instance`` and the host backend of ``filter_pointcloud`` behave on the
``degenerate`` cloud as designed, and the four entry points of csrc/points3d.hip refuse bad arguments before anything is launched."""
import os

import numpy as np
import pytest
import torch

import points3d_cases as pc


# ----------------------------------------------------------------------------- the layouts
def test_layout_table():
    pts, seg = pc.case("edges")
    assert pts.shape == (5552, 3) and pts.shape[0] % 256 != 0 and seg.shape[0] - 1 == 17 and seg[0] == 7 and seg[-1] == 5552 - 5
    assert np.diff(seg).tolist() == pc.EDGE_SIZES
    ptc, sc = pc.case("clamped")
    assert np.array_equal(ptc, pts) and sc[0] == -3 and sc[-1] == 5552 + 5 and np.array_equal(sc[1:-1], seg[1:-1])
    lo, hi = pc.bounds(sc, 5552)
    assert lo[0] == 0 and hi[0] == 7 and lo[-1] == seg[-2] and hi[-1] == 5552                      # the ends grow to the ends of the array
    assert [(pc.case(c)[0].shape[0], pc.case(c)[1].shape[0] - 1) for c in pc.CASES if c.startswith("tiny")] == [(1, 1), (3, 1), (64, 2), (5, 0)]
    pt, st = pc.case("ties")
    assert st.tolist() == [0, 40, 296, 596] and pt.shape[0] == 598
    assert (pt[:40] == pt[0]).all() and np.array_equal(np.unique(pt[40:296], axis=0).shape, (256, 3)) and (pt[40:296] == np.round(pt[40:296])).all()
    assert np.unique(pt[296:596], axis=0).shape[0] == 240
    pd, sd = pc.case("degenerate")
    assert np.diff(sd).tolist() == [40, 9, 10, 11, 300, 700]
    for name in pc.CASES:
        p, s = pc.case(name)
        assert p.dtype == np.float32 and s.dtype == np.int64 and (np.diff(s) >= 0).all()
    # the offset does what it is there for: one float32 ulp at x = 1000 is 2^-14, far above fp64 rounding
    assert abs(float(pts[:, 0].mean()) - 1000.0) < 0.1 and np.spacing(np.float32(1000.0)) == 2.0 ** -14


def test_the_geometry_holds():
    """What the cuts of the kernels meet.  The one-block-per-instance kernels (moments, extent, ellipsoid) cut an instance at t + 256 j and
    fold 64 lanes: the sizes end 0 and +-1 from a multiple of 64 and of 256, and one past 1024.  k_knn_kth cuts the ROW axis in 256-row
    blocks and 64-row waves whatever the instances are (with seg[0] = 7 every boundary of `edges` falls 7 to 43 rows past a wave cut: inside
    a wave, never on its edge; `windows` has the boundary ON the cut), stages the union of the block's instances in tiles of 1024 counted
    from the union's first row, and lets a wave skip the tiles its own instances miss."""
    for name in ("edges", "clamped"):
        pts, seg = pc.case(name)
        n = pts.shape[0]
        sizes = np.subtract(*pc.bounds(seg, n)[::-1]).tolist()
        for cut in (64, 256):
            offs = {((s + cut // 2) % cut) - cut // 2 for s in sizes if s > 0}
            assert {-1, 0, 1} <= offs, (name, cut, sorted(offs))
        assert 1025 in sizes and max(sizes) > 2 * pc.TILE                             # two and three tiles
        assert all(b % 64 not in (0, 1, 63) for b in seg[1:-1].tolist())                          # kNN: every boundary strictly inside a wave
        blocks = pc.knn_windows(seg, n)
        assert len(blocks) == 22 and blocks[-1]["rows"] == (5376, 5552)
        crowded = [b for b in blocks if len(b["instances"]) >= 3]
        assert len(crowded) >= 2
        big = [b for b in crowded if b["union"][1] - b["union"][0] > pc.TILE]
        assert len(big) >= 1 and len(big[0]["tiles"]) >= 3, [b["union"] for b in crowded]
        assert big[0]["rows"] == (2816, 3072) and len(big[0]["instances"]) == 5 and big[0]["union"] == (1992, 5547 if name == "edges" else 5552)
        # in that block some wave walks every tile and some wave skips the later ones
        walked = [[t for t in big[0]["tiles"] if w is not None and max(w[0], t[0]) < min(w[1], t[1])] for w in big[0]["waves"]]
        assert any(len(w) == len(big[0]["tiles"]) for w in walked) and any(0 < len(w) < len(big[0]["tiles"]) for w in walked)
        # empty instances between two others, and side by side
        e = np.diff(seg)
        assert e[11] == 0 and e[12] == 0 and e[10] > 0 and e[13] > 0
        # rows that belong to nobody, on both sides (edges) or on neither (clamped)
        inst = pc.instance_of_rows(seg, n)
        assert (inst == -1).sum() == (12 if name == "edges" else 0)
    pts, seg = pc.case("windows")
    blocks = pc.knn_windows(seg, pts.shape[0])
    b = blocks[4]
    assert seg[1] % 64 == 0 and seg[1] % 256 != 0 and b["rows"] == (1024, 1261) and b["union"] == (0, 1258) and len(b["tiles"]) == 2
    assert b["waves"][0] == (0, 1088) and b["waves"][1] == (1088, 1158)                           # wave 1 misses the first tile altogether
    assert not max(b["waves"][1][0], b["tiles"][0][0]) < min(b["waves"][1][1], b["tiles"][0][1])


def test_both_ends_of_every_kernel_width_and_both_kinds_of_result():
    assert pc.KS == (1, 4, 5, 8, 9, 12, 13, 16)
    for kt in (4, 8, 12, 16):                                                                      # k_knn_kth<KT> serves kt - 3 .. kt
        assert kt in pc.KS and kt - 3 in pc.KS
    seen = {}
    for name in pc.CASES:
        table, size = pc.knn_case_table(name)
        for k in pc.KS:
            d = pc.knn_from_table(table, size, k)
            fin, inf = seen.setdefault(pc.LAYOUT_OF[name], [False, False])
            seen[pc.LAYOUT_OF[name]] = [fin or bool(np.isfinite(d).any()), inf or bool(np.isposinf(d).any())]
            assert not np.isnan(d).any() and (d[np.isfinite(d)] >= 0).all()
    assert set(seen) == {"edges", "clamped", "windows", "tiny", "ties", "degenerate"} and all(all(v) for v in seen.values()), seen
    t, s = pc.knn_case_table("ties")
    assert (t[:40, :16] == 0).all()                                                                # 40 identical points: 0 for every k <= 16
    t, s = pc.knn_case_table("tiny_5_0")
    assert np.isposinf(t).all() and (s == 0).all()


# ----------------------------------------------------------------------------- the mistakes
KNN_ORDER = ("tiny_1_1", "tiny_64_2", "ties", "windows", "degenerate", "edges", "clamped")


def test_every_knn_mistake_is_caught():
    caught = {}
    for mistake in pc.KNN_MISTAKES:
        for name in KNN_ORDER:
            pts, seg = pc.case(name)
            table, size = pc.knn_case_table(name)
            wt, ws = pc.knn_table(pts, seg, mistake)
            ks = [k for k in pc.KS if not np.array_equal(pc.knn_from_table(table, size, k), pc.knn_from_table(wt, ws, k, mistake))]
            if ks:
                caught[mistake] = (name, ks)
                break
    print(caught)
    assert set(caught) == set(pc.KNN_MISTAKES), sorted(set(pc.KNN_MISTAKES) - set(caught))
    assert caught["more_than_k"] == ("tiny_1_1", [1])
    assert caught["no_self"][0] == "tiny_1_1" and caught["k_plus_1"][0] == "tiny_1_1"
    assert caught["no_boundary"][0] == "tiny_64_2" and caught["fp32"][0] == "tiny_64_2"
    assert caught["outside_finite"][0] == "ties"
    assert caught["first_tile_only"][0] == "windows"                                               # the first instance above 1024 rows
    assert caught["unclamped"][0] == "clamped"                                                     # the only layout with an entry outside [0, n]


def test_every_moment_mistake_is_caught():
    where = {"keep_eq_1": ("tiny_64_2", "bytes", "none"), "centre_fp32": ("tiny_64_2", "none", "mean"), "drop_last_row": ("tiny_3_1", "none", "none"),
             "drop_wave_partial": ("edges", "random70", "mean"), "np_sum": ("edges", "random70", "none")}
    assert set(where) == set(pc.MOMENT_MISTAKES)
    for mistake, (name, keep, centre) in where.items():
        pts, seg = pc.case(name)
        k, c = pc.keep_mask(name, keep), pc.centre_of(name, centre)
        good, bad = pc.moments_ordered(pts, seg, k, c), pc.moments_ordered(pts, seg, k, c, mistake)
        assert not np.array_equal(good, bad), (mistake, name)
        exact, scale, bound = pc.moments_exact(pts, seg, k, c)
        inside = (np.abs(bad - exact) <= bound[:, None] * scale).all()
        assert inside == (mistake == "np_sum"), (mistake, name)                                    # in bits only: numpy's order is a correct sum too


# ----------------------------------------------------------------------------- the references against each other
def test_ordered_restatement_is_accurate_and_sharp():
    worst, differ, nontrivial = 0.0, 0, 0
    for name in pc.CASES:
        pts, seg = pc.case(name)
        for keep in pc.KEEPS:
            for centre in pc.CENTRES:
                k, c = pc.keep_mask(name, keep), pc.centre_of(name, centre)
                got = pc.moments_ordered(pts, seg, k, c)
                exact, scale, bound = pc.moments_exact(pts, seg, k, c)
                assert np.array_equal(got[:, 0], exact[:, 0])                                      # the count is an integer
                err = np.abs(got - exact)
                assert (err <= bound[:, None] * scale).all(), (name, keep, centre, (err / np.maximum(bound[:, None] * scale, 1e-300)).max())
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(scale > 0, err / (bound[:, None] * scale), 0.0)
                worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
                assert (got[exact[:, 0] == 0] == 0).all()
                if keep == "none" and centre == "none":
                    plain = pc.moments_ordered(pts, seg, k, c, "np_sum")
                    # non-trivial: at least three rows whose sums are not exact anyway (identical or lattice points add exactly in any order)
                    for g in range(len(seg) - 1):
                        if exact[g, 0] >= 3 and not np.array_equal(plain[g], exact[g]):
                            nontrivial += 1
                            differ += int(not np.array_equal(plain[g], got[g]))
    print(f"moments_ordered against math.fsum: worst error {worst:.3f} of the bound; differs in bits from numpy's order on {differ} of {nontrivial} instances")
    assert nontrivial >= 20 and 2 * differ >= nontrivial, (differ, nontrivial)
    # the figure of the issue, on `edges` without keep and centre: units of 2^-53 * scale
    pts, seg = pc.case("edges")
    exact, scale, _ = pc.moments_exact(pts, seg)
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(scale > 0, np.abs(pc.moments_ordered(pts, seg) - exact) / (2.0 ** -53 * scale), 0.0)
    print(f"edges: worst error {units.max():.2f} x 2^-53 x scale")
    assert units.max() <= 11


def test_extent_reference_against_a_matrix_product():
    """The separate products of extent_reference against proj = q @ A.T (a different rounding: 1e-12 of the largest projection)."""
    for name in ("edges", "ties", "tiny_5_0"):
        pts, seg = pc.case(name)
        frame, keep = pc.frame_of(name, "mean"), pc.keep_mask(name, "random70")
        ref = pc.extent_reference(pts, seg, frame, keep)
        for g, (lo, hi) in enumerate(zip(*pc.bounds(seg, pts.shape[0]))):
            S = pts[lo:hi][keep[lo:hi] != 0].astype(np.float64)
            if len(S) == 0:
                assert np.isposinf(ref[g, :3]).all() and np.isneginf(ref[g, 3:]).all()
                continue
            proj = (S - frame[g, 9:]) @ frame[g, :9].reshape(3, 3).T
            assert np.abs(ref[g] - np.concatenate([proj.min(0), proj.max(0)])).max() <= 1e-12 * np.abs(proj).max()
        assert ref.shape == (len(seg) - 1, 6)
    A = pc.frame_of("edges", "none")[:, :9].reshape(-1, 3, 3)
    gap = np.abs(A @ A.transpose(0, 2, 1) - np.eye(3)).reshape(len(A), -1).max(1)
    assert (gap > 0.1).sum() == 1 and gap[3] > 0.1 and np.delete(gap, 3).max() < 1e-12             # one frame that is not orthonormal


def test_at_most_one_instance_per_layout_under_the_argmax_margin():
    for name in pc.MVEE_CASES:
        for kind in pc.MVEE_KEEPS:
            refs = pc.mvee_references(name, kind)
            low = pc.under_margin(refs)
            status = [r["status"] for r in refs]
            print(name, kind, "status", status, "under the margin", low, "iterations", [r["iters"] for r in refs])
            assert len(low) <= 1, f"{name}/{kind}: instances {low} under the margin of {pc.MVEE_MARGIN}: choose another seed"
            sizes = np.diff(np.clip(pc.case(name)[1], 0, 5552))
            if kind == "none":
                assert status == [0 if s >= 4 else 2 for s in sizes]
            else:
                keep = pc.mvee_keep(name, kind)
                lo, hi = pc.bounds(pc.case(name)[1], 5552)
                assert keep[lo[pc.THREE_ROWS]:hi[pc.THREE_ROWS]].sum() == 3 and keep[lo[pc.FOUR_ROWS]:hi[pc.FOUR_ROWS]].sum() == 4
                assert status[pc.THREE_ROWS] == 2 and status[pc.FOUR_ROWS] == 0 and refs[pc.FOUR_ROWS]["iters"] == 1
                # four non-coplanar rows: the simplex, every M_i = 4 up to rounding, so this is the instance the margin rule leaves out
                assert low in ([], [pc.FOUR_ROWS])
                other = pc.mvee_keep(name, kind, (0, 2, 255))
                assert np.array_equal(other != 0, keep != 0) and set(np.unique(other).tolist()) == {0, 2, 255} and set(np.unique(keep).tolist()) == {0, 1}


# ----------------------------------------------------------------------------- contrastive_lift_amd.points3d on the host
def test_group_by_instance_on_cpu_tensors():
    from contrastive_lift_amd import points3d
    lab = torch.tensor([5, -2, 0, 5, 3, -2, 0, 5, 3, -7])
    order, ids, seg = points3d.group_by_instance(lab, 0)
    assert ids.tolist() == [-7, -2, 3, 5] and seg.tolist() == [0, 1, 3, 5, 8]
    assert order.tolist() == [9, 1, 5, 4, 8, 0, 3, 7]                                              # stable: ascending row inside an instance
    assert order.dtype == torch.int64 and seg.dtype == torch.int64 and not seg.is_cuda
    order, ids, seg = points3d.group_by_instance(lab, None)
    assert ids.tolist() == [-7, -2, 0, 3, 5] and seg.tolist() == [0, 1, 3, 5, 7, 10] and order.tolist() == [9, 1, 5, 2, 6, 4, 8, 0, 3, 7]
    order, ids, seg = points3d.group_by_instance(lab, 5)
    assert ids.tolist() == [-7, -2, 0, 3] and seg.tolist() == [0, 1, 3, 5, 7]
    order, ids, seg = points3d.group_by_instance(torch.zeros(6, dtype=torch.int64), 0)             # every row ignored
    assert order.numel() == 0 and ids.numel() == 0 and seg.tolist() == [0]
    order, ids, seg = points3d.group_by_instance(torch.zeros(0, dtype=torch.int64), 0)
    assert order.numel() == 0 and seg.tolist() == [0]
    pts, labels, _ = pc.degenerate_cloud()
    order, ids, seg = points3d.group_by_instance(torch.as_tensor(labels), 0)
    ps, sg = pc.case("degenerate")
    assert ids.tolist() == [-2, 3, 5, 6, 11, 12] and np.array_equal(seg.numpy(), sg) and np.array_equal(pts[order.numpy()], ps)


def test_degenerate_cloud_through_the_host_filter():
    from contrastive_lift_amd import points3d
    pts, labels, what = pc.degenerate_cloud()
    ids = {v: k for k, v in what.items()}
    keep, st = points3d.filter_pointcloud(pts, labels, k=pc.FILTER_K, backend="sklearn", return_stages=True)
    keep, s1, d = keep.numpy(), st["stage1"].numpy(), st["kth_dist"].numpy()
    rows = {w: labels == i for w, i in ids.items()}
    assert [int(rows[w].sum()) for w in ("k-1", "k", "k+1", "identical", "planar", "blob")] == [9, 10, 11, 40, 300, 700]
    assert np.isposinf(d[rows["k-1"]]).all() and not s1[rows["k-1"]].any() and not keep[rows["k-1"]].any()
    assert np.isposinf(d[labels == 0]).all() and not keep[labels == 0].any()
    for w in ("k", "k+1", "identical", "planar", "blob"):
        assert np.isfinite(d[rows[w]]).all(), w
    assert s1[rows["k"]].sum() == 7 and s1[rows["k+1"]].sum() == 7                                 # strictly below the 70th percentile
    assert (d[rows["identical"]] == 0).all() and not s1[rows["identical"]].any() and not keep[rows["identical"]].any()
    assert s1[rows["planar"]].sum() == 210 and not keep[rows["planar"]].any()                      # 70 % at stage 1; std 0 on z: nothing at stage 2
    assert s1[rows["blob"]].sum() == 490 and 400 <= keep[rows["blob"]].sum() <= 490
    # the dyadic instances: sums and means are exact, whatever the order
    for w in ("identical", "planar"):
        P = pts[rows[w]].astype(np.float64)
        assert (P * 1024 == np.round(P * 1024)).all() and np.array_equal(P.sum(0), P[::-1].sum(0))
        assert np.array_equal(P[:, 2].mean(keepdims=True), P[:1, 2])
    # the k-th distances are the reference's, bit for bit
    ps, seg = pc.case("degenerate")
    order = np.nonzero(labels != 0)[0][np.argsort(labels[labels != 0], kind="stable")]
    assert np.array_equal(d[order], np.sqrt(pc.knn_reference(ps, seg, pc.FILTER_K)))


# ----------------------------------------------------------------------------- refusals
def test_refusals_return_before_anything_is_launched():
    """Argument checks of the four entry points: non-zero, the entry point's name in clift_last_error(), nothing touches a device (the
    pointers handed over are NULL or host memory that a launch would fault on, and this runs on machines without a GPU)."""
    import ctypes as C
    from contrastive_lift_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libclift.so is not built")
    lib = _lib.load()
    host = (C.c_double * 64)()
    p = C.cast(host, C.c_void_p)
    big = 2 ** 31 - 1024
    calls = {
        "clift_knn_kth_dist": {
            "n": lambda: lib.clift_knn_kth_dist(p, big, p, 1, 10, p, None), "n<0": lambda: lib.clift_knn_kth_dist(p, -1, p, 1, 10, p, None),
            "G": lambda: lib.clift_knn_kth_dist(p, 8, p, -1, 10, p, None), "k=0": lambda: lib.clift_knn_kth_dist(p, 8, p, 1, 0, p, None),
            "k=17": lambda: lib.clift_knn_kth_dist(p, 8, p, 1, 17, p, None), "seg": lambda: lib.clift_knn_kth_dist(p, 8, None, 1, 10, p, None)},
        "clift_segment_moments": {
            "n": lambda: lib.clift_segment_moments(p, big + 768, p, 1, None, None, p, None),
            "G": lambda: lib.clift_segment_moments(p, 8, p, -1, None, None, p, None),
            "seg": lambda: lib.clift_segment_moments(p, 8, None, 1, None, None, p, None)},
        "clift_segment_extent": {
            "n": lambda: lib.clift_segment_extent(p, big + 768, p, 1, None, p, p, None),
            "G": lambda: lib.clift_segment_extent(p, 8, p, -1, None, p, p, None),
            "seg": lambda: lib.clift_segment_extent(p, 8, None, 1, None, p, p, None),
            "frame": lambda: lib.clift_segment_extent(p, 8, p, 1, None, None, p, None)},
        "clift_segment_mvee": {
            "n": lambda: lib.clift_segment_mvee(p, big + 768, p, 1, None, 0.01, 10, p, p, None),
            "G": lambda: lib.clift_segment_mvee(p, 8, p, -1, None, 0.01, 10, p, p, None),
            "seg": lambda: lib.clift_segment_mvee(p, 8, None, 1, None, 0.01, 10, p, p, None),
            "max_iter=0": lambda: lib.clift_segment_mvee(p, 8, p, 1, None, 0.01, 0, p, p, None),
            "max_iter=1000001": lambda: lib.clift_segment_mvee(p, 8, p, 1, None, 0.01, 1000001, p, p, None),
            "tolerance=0": lambda: lib.clift_segment_mvee(p, 8, p, 1, None, 0.0, 10, p, p, None),
            "tolerance=nan": lambda: lib.clift_segment_mvee(p, 8, p, 1, None, float("nan"), 10, p, p, None)},
    }
    for name, bad in calls.items():
        for what, fn in bad.items():
            assert fn() != 0, (name, what)
            msg = lib.clift_last_error().decode()
            assert msg.startswith(name + ":"), (name, what, msg)
            key = what.split("=")[0].split("<")[0]
            assert {"n": " n ", "G": "G >= 0", "k": " k ", "seg": "NULL", "frame": "NULL", "max_iter": "max_iter", "tolerance": "tolerance"}[key] in msg, (name, what, msg)
    # the limits themselves are not refused for their size: the largest n the header allows, with nothing to do (G = 0), returns 0
    assert lib.clift_segment_moments(None, big - 1 + 768, None, 0, None, None, None, None) == 0
    assert lib.clift_knn_kth_dist(None, 0, None, 0, 10, None, None) == 0
