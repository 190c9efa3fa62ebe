"""The four entry points of csrc/points3d.hip on the GPU against the references of tests/points3d_cases.py, layout by layout: seg[0] > 0,
seg[G] < n, empty instances, entries of seg outside [0, n], instance boundaries inside waves and on a wave cut, instances of two and three
LDS tiles, both ends of every register width of the kNN.  clift_knn_kth_dist and clift_segment_extent are held to exact equality,
clift_segment_moments to the bits of the documented split AND to the derived bound against math.fsum, clift_segment_mvee to the numpy
Khachiyan of ellipsoid_cases.py by the rule of test_gpu_ellipsoid.py; the filter runs end to end on the ``degenerate`` cloud."""
import numpy as np
import pytest
import torch

import points3d_cases as pc

pytestmark = pytest.mark.gpu
SENTINEL = -7.5


def dev(x):
    return None if x is None else torch.tensor(np.asarray(x), device="cuda")                   # (a copy: the cases are read-only arrays)


def raw(name, *args):
    from contrastive_lift_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[_lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _lib.stream())
    assert rc == 0, (name, lib.clift_last_error().decode())


# ----------------------------------------------------------------------------- clift_knn_kth_dist
@pytest.mark.parametrize("name", pc.CASES)
def test_knn_equals_the_reference_bit_for_bit(name):
    from contrastive_lift_amd import points3d
    pts, seg = pc.case(name)
    table, size = pc.knn_case_table(name)
    ps, sg = dev(pts), dev(seg)
    for k in pc.KS:
        a = points3d.knn_kth_dist2(ps, sg, k)
        b = points3d.knn_kth_dist2(ps, sg, k)
        assert a.dtype == torch.float64 and a.shape == (pts.shape[0],) and torch.equal(a, b)       # two runs, the same bits
        got, want = a.cpu().numpy(), pc.knn_from_table(table, size, k)
        bad = np.nonzero(~((got == want) & (np.signbit(got) == np.signbit(want))))[0]              # bits: every value here is >= +0 or +inf
        assert bad.size == 0, (name, k, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert np.array_equal(np.isposinf(got), size < k)                                          # short instances and rows of nobody, only they
        if name == "ties":
            assert (got[:40] == 0).all()                                                           # 40 identical points: 0 for every k <= 16


def test_knn_n_zero_touches_nothing():
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    seg = torch.zeros(3, dtype=torch.int64, device="cuda")
    raw("clift_knn_kth_dist", None, 0, seg, 2, 10, out)
    raw("clift_knn_kth_dist", None, 0, None, 0, 1, None)
    assert (out.cpu().numpy() == SENTINEL).all()


# ----------------------------------------------------------------------------- clift_segment_moments
@pytest.mark.parametrize("name", pc.CASES)
def test_moments_equal_the_documented_split_and_keep_the_exact_bound(name):
    from contrastive_lift_amd import points3d
    pts, seg = pc.case(name)
    ps, sg = dev(pts), dev(seg)
    worst = 0.0
    for keep in pc.KEEPS:
        for centre in pc.CENTRES:
            k, c = pc.keep_mask(name, keep), pc.centre_of(name, centre)
            a = points3d.segment_moments(ps, sg, dev(k), dev(c))
            assert torch.equal(a, points3d.segment_moments(ps, sg, dev(k), dev(c)))
            got = a.cpu().numpy()
            want = pc.moments_ordered(pts, seg, k, c)
            exact, scale, bound = pc.moments_exact(pts, seg, k, c)
            assert got.shape == want.shape == (len(seg) - 1, 10)
            assert np.array_equal(got[:, 0].astype(np.int64), exact[:, 0].astype(np.int64)) and np.array_equal(got[:, 0], np.round(got[:, 0]))
            same = (got == want) & (np.signbit(got) == np.signbit(want))
            assert same.all(), (name, keep, centre, np.argwhere(~same)[:5].tolist(), (got - want)[~same][:5].tolist())
            err = np.abs(got - exact)
            assert (err <= bound[:, None] * scale).all(), (name, keep, centre)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(scale > 0, err / (bound[:, None] * scale), 0.0)
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            empty = exact[:, 0] == 0
            assert (got[empty] == 0).all() and not np.signbit(got[empty]).any()                    # exact zeros where nothing is kept
    print(f"{name}: worst moments error {worst:.3f} of the bound")


def test_moments_and_extent_n_zero():
    seg = torch.zeros(3, dtype=torch.int64, device="cuda")
    out = torch.full((2, 10), SENTINEL, dtype=torch.float64, device="cuda")
    raw("clift_segment_moments", None, 0, seg, 2, None, None, out)
    assert (out.cpu().numpy() == 0).all()
    frame = dev(np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (2, 1)))
    ext = torch.full((2, 6), SENTINEL, dtype=torch.float64, device="cuda")
    raw("clift_segment_extent", None, 0, seg, 2, None, frame, ext)
    x = ext.cpu().numpy()
    assert np.isposinf(x[:, :3]).all() and np.isneginf(x[:, 3:]).all()
    raw("clift_segment_moments", None, 0, None, 0, None, None, None)                               # G = 0: nothing to do
    raw("clift_segment_extent", None, 0, None, 0, None, None, None)


# ----------------------------------------------------------------------------- clift_segment_extent
@pytest.mark.parametrize("name", pc.CASES)
def test_extent_equals_the_reference(name):
    from contrastive_lift_amd import points3d
    pts, seg = pc.case(name)
    ps, sg = dev(pts), dev(seg)
    for keep in pc.KEEPS:
        for centre in pc.CENTRES:
            k, frame = pc.keep_mask(name, keep), pc.frame_of(name, centre)
            a = points3d.segment_extent(ps, sg, dev(frame), dev(k))
            assert torch.equal(a, points3d.segment_extent(ps, sg, dev(frame), dev(k)))
            got, want = a.cpu().numpy(), pc.extent_reference(pts, seg, frame, k)
            assert got.shape == want.shape and (got == want).all(), (name, keep, centre, np.argwhere(got != want)[:5].tolist())
            if keep == "zeros":
                assert np.isposinf(got[:, :3]).all() and np.isneginf(got[:, 3:]).all()


# ----------------------------------------------------------------------------- clift_segment_mvee
@pytest.mark.parametrize("name", pc.MVEE_CASES)
def test_mvee_through_a_raw_call(name):
    pts, seg = pc.case(name)
    n, G = pts.shape[0], len(seg) - 1
    ps, sg = dev(pts), dev(seg)
    lo, hi = pc.bounds(seg, n)
    inst = pc.instance_of_rows(seg, n)
    assert (inst == -1).sum() == (12 if name == "edges" else 0)

    def run(keep):
        u = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        out = torch.full((G, 14), SENTINEL, dtype=torch.float64, device="cuda")
        raw("clift_segment_mvee", ps, n, sg, G, dev(keep), 0.01, 10000, u, out)
        return out, u

    for kind in pc.MVEE_KEEPS:
        keep = pc.mvee_keep(name, kind)
        refs = pc.mvee_references(name, kind)
        out_t, u_t = run(keep)
        out2, u2 = run(keep)
        assert torch.equal(out_t, out2) and torch.equal(u_t, u2)
        out, u = out_t.cpu().numpy(), u_t.cpu().numpy()
        kept = np.ones(n, bool) if keep is None else keep != 0
        assert (u[inst == -1] == SENTINEL).all()                                                   # rows outside [seg[0], seg[G]) are not written
        assert (u[(inst >= 0) & ~kept] == 0).all() and (u[inst >= 0] >= 0).all() and np.isfinite(out).all()
        assert out[:, 3].tolist() == [r["status"] for r in refs] and (out[:, 13] == 0).all()
        assert out[:, 0].tolist() == [int(kept[a:b].sum()) for a, b in zip(lo, hi)]
        for g, r in enumerate(refs):
            if r["status"] == 2:
                assert (out[g, 4:] == 0).all() and out[g, 2] == 0 and (u[lo[g]:hi[g]] == 0).all(), (kind, g)
        u_rows = [u[a:b][kept[a:b]] for a, b in zip(lo, hi)]
        low = pc.under_margin(refs)
        assert len(low) <= 1
        done = pc.assert_mvee_rows(out, u_rows, refs, f"{name}/{kind}")
        assert done == sum(r["status"] != 2 for r in refs) - len(low)
        if kind == "masked":
            assert out[pc.THREE_ROWS, :4].tolist() == [3, 0, 0, 2] and (out[pc.THREE_ROWS, 4:] == 0).all()      # exactly three rows: degenerate
            assert out[pc.FOUR_ROWS, 0] == 4 and out[pc.FOUR_ROWS, 3] == 0 and out[pc.FOUR_ROWS, 1] == 1       # four non-coplanar rows: the simplex
            other = pc.mvee_keep(name, kind, (0, 2, 255))
            out3, u3 = run(other)
            assert torch.equal(out_t, out3) and torch.equal(u_t, u3)                               # keep != 0, whatever the byte


# ----------------------------------------------------------------------------- the filter end to end
def test_filter_device_equals_host_on_the_degenerate_cloud():
    from contrastive_lift_amd import points3d
    pts, labels, what = pc.degenerate_cloud()
    kd, sd = points3d.filter_pointcloud(pts, labels, k=pc.FILTER_K, backend="device", return_stages=True)
    kh, sh = points3d.filter_pointcloud(pts, labels, k=pc.FILTER_K, backend="sklearn", return_stages=True)
    assert kd.is_cuda
    d, h = sd["kth_dist"].cpu().numpy(), sh["kth_dist"].numpy()
    assert np.array_equal(d, h) and np.isposinf(d).sum() == 9 + 25
    assert np.array_equal(sd["stage1"].cpu().numpy(), sh["stage1"].numpy())
    assert np.array_equal(kd.cpu().numpy(), kh.numpy())
    ids = {v: k for k, v in what.items()}
    s1, keep = sd["stage1"].cpu().numpy(), kd.cpu().numpy()
    assert not s1[labels == ids["identical"]].any() and not s1[labels == ids["k-1"]].any()
    assert s1[labels == ids["planar"]].sum() == 210 and not keep[labels == ids["planar"]].any()
    assert keep[labels == ids["blob"]].sum() >= 400
