"""Instances in 3-D: the labelled point cloud of the rendered frames and per-instance boxes (reference inference/visualize_bboxes.py:
``filter_pointcloud`` :52-74, ``get_tight_bbox`` :78-131; the points are the pixels back-projected along their rays, render_panopli.py:124).

The reference handles one instance at a time on the host (boolean mask, KD-tree, 10-NN query, percentile, 3-sigma cut, PCA).  Here the
rows are sorted by instance once and every step runs for all instances of a scene at once: the k-th neighbour distances, the moments and
the extents in libclift.so (csrc/points3d.hip: clift_knn_kth_dist, clift_segment_moments, clift_segment_extent), the percentile selection,
the 3 x 3 eigen-decomposition and the sorting in torch / numpy.  The reference's default method, the minimum-volume enclosing ellipsoid
(``getMinVolEllipse`` :135-189), is ``fit_instance_ellipsoids``: Khachiyan's loop for all instances in one launch (clift_segment_mvee).  ``backend="sklearn"`` is the same function on the host with
``sklearn.neighbors.KDTree`` and numpy, for machines without a GPU; both backends take their statistics in fp64 (the reference takes mean and
std of a float32 array in float32, so a point lying on the 3-sigma face can fall either way there).
"""
import numpy as np
import torch

from . import _lib

METHODS = ("pca", "simple")
BACKENDS = ("device", "sklearn")


def backproject(rays, dist):
    """Points (P, 3) = origin + dist * direction of rays (P, >= 6) = [origin, direction, ...] (RP:124), on the tensors' device."""
    return rays[..., 0:3] + dist[..., None] * rays[..., 3:6]


# ----------------------------------------------------------------------------------------------------------------- kernel wrappers
def _check_sorted_input(pts, seg):
    if not pts.is_cuda or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3 or not pts.is_contiguous():
        raise _lib.CliftError(f"points3d: pts must be a contiguous CUDA float32 (n, 3) tensor, got {pts.dtype} {tuple(pts.shape)} on {pts.device}")
    if seg.device != pts.device or seg.dtype != torch.int64 or seg.dim() != 1 or seg.numel() < 1 or not seg.is_contiguous():
        raise _lib.CliftError("points3d: seg must be a contiguous int64 (G + 1,) tensor on the points' device")
    return pts.shape[0], seg.numel() - 1


def _keep_arg(keep, n, dev):
    if keep is None:
        return None
    if keep.device != dev or keep.numel() != n or keep.dtype not in (torch.bool, torch.uint8) or not keep.is_contiguous():
        raise _lib.CliftError("points3d: keep must be a contiguous bool / uint8 (n,) tensor on the points' device")
    return keep.view(torch.uint8)


def knn_kth_dist2(pts, seg, k):
    """clift_knn_kth_dist: (n,) fp64 squared distance of every row to its k-th nearest row of the same instance (itself included)."""
    n, G = _check_sorted_input(pts, seg)
    out = torch.empty((n,), dtype=torch.float64, device=pts.device)
    _lib.call("clift_knn_kth_dist", _lib.ptr(pts), n, _lib.ptr(seg), G, int(k), _lib.ptr(out), _lib.stream())
    return out


def segment_moments(pts, seg, keep=None, centre=None):
    """clift_segment_moments: (G, 10) fp64 = count, sums of x y z, sums of xx xy xz yy yz zz of (p - centre) over the kept rows."""
    n, G = _check_sorted_input(pts, seg)
    keep = _keep_arg(keep, n, pts.device)
    if centre is not None and (centre.device != pts.device or centre.dtype != torch.float64 or tuple(centre.shape) != (G, 3) or not centre.is_contiguous()):
        raise _lib.CliftError("points3d: centre must be a contiguous fp64 (G, 3) tensor on the points' device")
    out = torch.empty((G, 10), dtype=torch.float64, device=pts.device)
    _lib.call("clift_segment_moments", _lib.ptr(pts), n, _lib.ptr(seg), G, _lib.ptr(keep), _lib.ptr(centre), _lib.ptr(out), _lib.stream())
    return out


def segment_extent(pts, seg, frame, keep=None):
    """clift_segment_extent: (G, 6) fp64 = min (3) and max (3) of axes @ (p - centre) over the kept rows; frame (G, 12) = axes, centre."""
    n, G = _check_sorted_input(pts, seg)
    keep = _keep_arg(keep, n, pts.device)
    if frame.device != pts.device or frame.dtype != torch.float64 or tuple(frame.shape) != (G, 12) or not frame.is_contiguous():
        raise _lib.CliftError("points3d: frame must be a contiguous fp64 (G, 12) tensor on the points' device")
    out = torch.empty((G, 6), dtype=torch.float64, device=pts.device)
    _lib.call("clift_segment_extent", _lib.ptr(pts), n, _lib.ptr(seg), G, _lib.ptr(keep), _lib.ptr(frame), _lib.ptr(out), _lib.stream())
    return out


MVEE_COLUMNS = 14                                  # m, iters, err, status, c (3), Cxx Cxy Cxz Cyy Cyz Czz, 0
MVEE_PIVOT_REL = 1e-12                             # csrc/points3d.hip: a Cholesky pivot not above this share of its diagonal entry = not positive definite


def segment_mvee(pts, seg, keep=None, tolerance=0.01, max_iter=10000):
    """clift_segment_mvee: Khachiyan's minimum-volume enclosing ellipsoid of every instance's kept rows, the whole loop in one launch.
    Returns (out (G, 14) fp64 = m, iters, err, status, centre (3), Cxx Cxy Cxz Cyy Cyz Czz, 0; u (n,) fp64 weights).  status 0 converged,
    1 stopped at max_iter, 2 degenerate (fewer than 4 kept rows, coplanar / collinear rows: centre, C and the instance's u are 0)."""
    n, G = _check_sorted_input(pts, seg)
    keep = _keep_arg(keep, n, pts.device)
    out = torch.empty((G, MVEE_COLUMNS), dtype=torch.float64, device=pts.device)
    u = torch.zeros((n,), dtype=torch.float64, device=pts.device)
    _lib.call("clift_segment_mvee", _lib.ptr(pts), n, _lib.ptr(seg), G, _lib.ptr(keep), float(tolerance), int(max_iter), _lib.ptr(u), _lib.ptr(out),
              _lib.stream())
    return out, u


# ----------------------------------------------------------------------------------------------------------------- grouping
def _as_inputs(points, labels, backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    pts = torch.as_tensor(points)
    lab = torch.as_tensor(np.asarray(labels).astype(np.int64) if isinstance(labels, np.ndarray) else labels).reshape(-1).to(torch.int64)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] != lab.shape[0]:
        raise ValueError(f"points (P, 3) and labels (P,) expected, got {tuple(pts.shape)} and {tuple(lab.shape)}")
    if backend == "device":
        dev = pts.device if pts.is_cuda else torch.device("cuda")
        if not torch.cuda.is_available():
            raise _lib.CliftError('points3d: backend="device" runs on a GPU (there is no host fallback; backend="sklearn" is the host function)')
    else:
        dev = torch.device("cpu")
    return pts.to(dev, torch.float32), lab.to(dev)


def group_by_instance(labels, ignore_label=0):
    """Rows sorted by label (stable), the rows of ``ignore_label`` left out: (order (n,), ids (G,), seg (G + 1,)), all int64 on labels' device."""
    rows = torch.arange(labels.shape[0], device=labels.device) if ignore_label is None else torch.nonzero(labels != ignore_label).reshape(-1)
    order = rows[torch.argsort(labels[rows], stable=True)]
    ids, counts = torch.unique_consecutive(labels[order], return_counts=True)
    seg = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=labels.device)
    seg[1:] = torch.cumsum(counts, 0)
    return order, ids, seg


def _instance_of_rows(seg):
    counts = seg[1:] - seg[:-1]
    return torch.repeat_interleave(torch.arange(counts.numel(), device=seg.device), counts), counts


def _segment_percentile(d, seg, inst, counts, percentile):
    """np.percentile(d[seg[g]:seg[g+1]], percentile) for every g (method "linear"), with numpy's own arithmetic step by step
    (numpy/lib/_function_base_impl.py: virtual index (n - 1) * q, _get_indexes, _get_gamma, _lerp), so the value has numpy's bits.
    Empty instances get nan."""
    i1 = torch.argsort(d, stable=True)
    ds = d[i1[torch.argsort(inst[i1], stable=True)]]                   # ascending inside every instance, instances in order
    q = float(np.true_divide(percentile, 100))
    m = counts.to(torch.float64)
    virt = (m - 1) * q
    prev = torch.floor(virt)
    nxt = prev + 1
    above = virt >= m - 1
    prev = torch.where(above, m - 1, prev)
    nxt = torch.where(above, m - 1, nxt)
    below = virt < 0
    prev = torch.where(below, torch.zeros_like(prev), prev)
    nxt = torch.where(below, torch.zeros_like(nxt), nxt)
    gamma = virt - prev
    empty = counts == 0
    last = max(int(ds.numel()) - 1, 0)
    if ds.numel() == 0:
        return torch.full_like(m, float("nan"))
    a = ds[(seg[:-1] + prev.to(torch.int64)).clamp(0, last)]
    b = ds[(seg[:-1] + nxt.to(torch.int64)).clamp(0, last)]
    diff = b - a
    out = a + diff * gamma
    out = torch.where(gamma >= 0.5, b - diff * (1 - gamma), out)
    return torch.where(empty, torch.full_like(out, float("nan")), out)


# ----------------------------------------------------------------------------------------------------------------- the filter
def _filter_sorted(ps, seg, k, keep_percentile, n_sigma, backend):
    """Both stages of filter_pointcloud on rows sorted by instance.  Returns (dist (n,) fp64 k-th neighbour distance, +inf in instances
    with fewer than k rows; keep1 (n,) bool after the percentile stage; keep (n,) bool after the 3-sigma stage)."""
    n = ps.shape[0]
    if backend == "device":
        inst, counts = _instance_of_rows(seg)
        dist = torch.sqrt(knn_kth_dist2(ps, seg, k))
        valid = counts >= k
        thr = _segment_percentile(torch.where(valid[inst], dist, torch.zeros_like(dist)), seg, inst, counts, keep_percentile)
        keep1 = (dist < thr[inst]) & valid[inst]
        m = segment_moments(ps, seg, keep1)
        mean = (m[:, 1:4] / m[:, 0:1]).contiguous()                                   # nan where nothing survived: nothing is kept there
        m = segment_moments(ps, seg, keep1, mean)
        std = torch.sqrt(m[:, [4, 7, 9]] / m[:, 0:1])
        keep = keep1 & ((ps.to(torch.float64) - mean[inst]).abs() < n_sigma * std[inst]).all(1)
        return dist, keep1, keep
    from sklearn.neighbors import KDTree
    P_all = ps.cpu().numpy()
    edges = seg.cpu().numpy()
    dist = np.full(n, np.inf)
    keep1 = np.zeros(n, bool)
    keep = np.zeros(n, bool)
    for lo, hi in zip(edges[:-1], edges[1:]):
        P = P_all[lo:hi]
        if P.shape[0] < k:                                                            # KDTree.query raises here; the caller drops the instance
            continue
        d = KDTree(P).query(P, k=k)[0][:, -1]
        dist[lo:hi] = d
        k1 = d < np.percentile(d, keep_percentile)
        keep1[lo:hi] = k1
        S = P[k1].astype(np.float64)
        if S.shape[0] == 0:
            continue
        k2 = np.all(np.abs(S - S.mean(0)) < n_sigma * S.std(0), axis=-1)
        keep[lo:hi][k1] = k2
    return torch.from_numpy(dist), torch.from_numpy(keep1), torch.from_numpy(keep)


def filter_pointcloud(points, labels, k=10, keep_percentile=70, n_sigma=3, backend="device", ignore_label=0, return_stages=False):
    """Keep mask (P,) bool over the input rows: the reference's ``filter_pointcloud`` (visualize_bboxes.py:52-74) applied to every
    instance (distinct label) on its own.  Stage 1 keeps the points whose distance to their k-th nearest neighbour (the point itself
    counts, as in ``KDTree.query(points, k)``) is strictly below ``np.percentile(dist, keep_percentile)`` of that instance; stage 2 takes
    mean and population std (fp64) of the survivors and keeps those with ``|p - mean| < n_sigma * std`` on all three axes.  Rows labelled
    ``ignore_label`` (0 = stuff; None = no such label) and instances with fewer than k rows are not kept.

    ``backend="device"``: all instances at once on the GPU (``points`` may be a CUDA tensor already).  ``backend="sklearn"``: the same
    function on the host, one KD-tree per instance.  The mask comes back on the device the work ran on.  ``return_stages=True`` returns
    ``(keep, {"kth_dist": (P,) fp64, +inf where not computed, "stage1": (P,) bool})``."""
    pts, lab = _as_inputs(points, labels, backend)
    order, _, seg = group_by_instance(lab, ignore_label)
    ps = pts[order].contiguous()
    dist, keep1, keep = _filter_sorted(ps, seg, int(k), keep_percentile, n_sigma, backend)
    P = pts.shape[0]
    out = torch.zeros(P, dtype=torch.bool, device=pts.device)
    out[order] = keep.to(pts.device)
    if not return_stages:
        return out
    d_all = torch.full((P,), float("inf"), dtype=torch.float64, device=pts.device)
    d_all[order] = dist.to(pts.device)
    s1 = torch.zeros(P, dtype=torch.bool, device=pts.device)
    s1[order] = keep1.to(pts.device)
    return out, {"kth_dist": d_all, "stage1": s1}


# ----------------------------------------------------------------------------------------------------------------- boxes
def _subsample(order, seg, max_points, generator):
    counts = (seg[1:] - seg[:-1]).cpu().numpy()
    if not (counts > max_points).any():
        return order, seg
    edges = seg.cpu().numpy()
    parts = []
    for g, c in enumerate(counts):
        rows = order[edges[g]:edges[g + 1]]
        if c > max_points:
            pick = torch.sort(torch.randperm(int(c), generator=generator)[:max_points])[0]
            rows = rows[pick.to(rows.device)]
        parts.append(rows)
    new_seg = torch.zeros_like(seg)
    new_seg[1:] = torch.cumsum(torch.as_tensor(np.minimum(counts, max_points), device=seg.device), 0)
    return torch.cat(parts), new_seg


def _pca_axes(cov):
    """Rows = eigenvectors of the (G, 3, 3) covariances by descending eigenvalue; sign: the component of largest magnitude of every axis is
    positive (what sklearn's PCA leaves after ``svd_flip(u_based_decision=False)``)."""
    w, v = np.linalg.eigh(cov)
    axes = np.transpose(v, (0, 2, 1))[:, ::-1, :].copy()
    big = np.take_along_axis(axes, np.abs(axes).argmax(-1)[..., None], -1)
    return axes * np.where(big < 0, -1.0, 1.0)


def fit_instance_boxes(points, labels, method="pca", max_points=50000, generator=None, backend="device", k=10, keep_percentile=70,
                       n_sigma=3, return_info=False):
    """The reference's ``get_tight_bbox`` (visualize_bboxes.py:78-131) for the methods "pca" and "simple":
    ``{instance_id: {"bbox": (min (3,), max (3,)), "orientation": (3, 3), "position": (3,)}}`` with numpy fp64 values, in the box frame
    ``orientation @ (p - position)`` (rows of ``orientation`` are the axes, like ``PCA.components_``).  Label 0 (stuff) is skipped, and so
    are instances with fewer than k points or with no point left after ``filter_pointcloud``.

    Instances above ``max_points`` are subsampled without replacement first, with ``torch.randperm(count, generator=generator)`` on the host
    (``generator=None`` is torch's global CPU generator).  The reference draws from numpy's GLOBAL random state there
    (``np.random.choice``), so its boxes of large instances are reproducible only through ``np.random.seed``.

    "simple": centre = mean of the kept points, box = their min / max minus the centre, identity orientation.  "pca": centre = mean,
    axes = eigenvectors of the covariance by descending eigenvalue, each signed so that its largest component is positive, box = extent of
    the kept points along the axes.  "ellipsoid" and "oriented" of the reference are not built HERE: ValueError.  The ellipsoid is
    ``fit_instance_ellipsoids`` (the reference's Khachiyan loop forms an N x N matrix; that function does not); "oriented" stays refused:
    the reference's ``getMinVolBox`` returns from inside its loop after the first hull face.

    ``return_info=True`` returns ``(boxes, {"kept": {id: n}, "total": {id: n}, "keep": (P,) bool mask of the rows the boxes were fitted to})``."""
    if method not in METHODS:
        raise ValueError(f"method {method!r} is not built: choose one of {METHODS} (\"pca\" or \"simple\")"
                         + ("; the ellipsoid is fit_instance_ellipsoids" if method == "ellipsoid" else ""))
    pts, lab = _as_inputs(points, labels, backend)
    order, ids, seg = group_by_instance(lab, 0)
    total = (seg[1:] - seg[:-1]).cpu().numpy()
    order, seg = _subsample(order, seg, int(max_points), generator)
    ps = pts[order].contiguous()
    G = ids.numel()
    _, _, keep = _filter_sorted(ps, seg, int(k), keep_percentile, n_sigma, backend)
    keep = keep.to(pts.device).contiguous()
    if backend == "device":
        m = segment_moments(ps, seg, keep)
        cnt = m[:, 0].cpu().numpy()
        mean_t = (m[:, 1:4] / m[:, 0:1]).contiguous()
        mean = mean_t.cpu().numpy()
        if method == "pca":
            c = segment_moments(ps, seg, keep, mean_t).cpu().numpy()
            with np.errstate(invalid="ignore", divide="ignore"):
                cov = c[:, [4, 5, 6, 5, 7, 8, 6, 8, 9]].reshape(G, 3, 3) / c[:, 0].reshape(G, 1, 1)
            axes = _pca_axes(np.where(np.isfinite(cov), cov, 0.0))
        else:
            axes = np.broadcast_to(np.eye(3), (G, 3, 3)).copy()
        frame = torch.as_tensor(np.concatenate([axes.reshape(G, 9), np.where(np.isfinite(mean), mean, 0.0)], 1), device=pts.device).contiguous()
        ext = segment_extent(ps, seg, frame, keep).cpu().numpy()
    else:
        P_all, keep_np, edges = ps.numpy(), keep.numpy(), seg.numpy()
        cnt, mean, axes, ext = np.zeros(G), np.zeros((G, 3)), np.broadcast_to(np.eye(3), (G, 3, 3)).copy(), np.zeros((G, 6))
        for g in range(G):
            S = P_all[edges[g]:edges[g + 1]][keep_np[edges[g]:edges[g + 1]]].astype(np.float64)
            cnt[g] = S.shape[0]
            if S.shape[0] == 0:
                continue
            mean[g] = S.mean(0)
            q = S - mean[g]
            if method == "pca":
                axes[g] = _pca_axes((q.T @ q / S.shape[0])[None])[0]
            proj = q @ axes[g].T
            ext[g] = np.concatenate([proj.min(0), proj.max(0)])
    boxes, kept = {}, {}
    for g, inst_id in enumerate(ids.cpu().numpy().tolist()):
        kept[inst_id] = int(cnt[g])
        if cnt[g] > 0:
            boxes[inst_id] = {"bbox": (ext[g, 0:3].copy(), ext[g, 3:6].copy()), "orientation": axes[g].copy(), "position": mean[g].copy()}
    if not return_info:
        return boxes
    mask = torch.zeros(pts.shape[0], dtype=torch.bool, device=pts.device)
    mask[order] = keep
    return boxes, {"kept": kept, "total": {i: int(t) for i, t in zip(ids.cpu().numpy().tolist(), total)}, "keep": mask}


# ----------------------------------------------------------------------------------------------------------------- ellipsoids
def _mvee_factor(V):
    """L^-1 of V = L L^T (4 x 4, lower) with the kernel's rule: None when a pivot is not above MVEE_PIVOT_REL of its diagonal entry."""
    L = np.zeros((4, 4))
    for j in range(4):
        d = V[j, j] - L[j, :j] @ L[j, :j]
        if not (d > MVEE_PIVOT_REL * V[j, j] and d < np.inf):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 4):
            L[i, j] = (V[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return np.linalg.solve(L, np.eye(4))


def _mvee_host(S, tolerance, max_iter):
    """One instance of clift_segment_mvee on the host, with the kernel's choices (rows centred on their mean, rank-1 update of V, Cholesky
    factor, closed-form err): O(rows) per iteration, never the reference's N x N products.  S (m, 3) fp64.  Returns (row of MVEE_COLUMNS
    numbers, u (m,))."""
    m = S.shape[0]
    row = np.zeros(MVEE_COLUMNS)
    row[0], row[3] = m, 2
    if m < 4:
        return row, np.zeros(m)
    o = S.sum(0) / m
    q = np.concatenate([S - o, np.ones((m, 1))], 1)
    u = np.full(m, 1.0 / m)
    V = (q.T @ q) / m
    V[3, 3] = 1.0
    nsq, iters, err, status = 1.0 / m, 0, 0.0, 2
    with np.errstate(all="ignore"):
        while True:
            Li = _mvee_factor(V)
            if Li is None:
                break
            y = q @ Li.T
            M = (y * y).sum(1)
            j = int(np.argmax(M))                                                  # the lowest row on equal values
            Mj = M[j]
            if not np.isfinite(Mj):
                break
            step = (Mj - 4.0) / (4.0 * (Mj - 1.0))
            uj = u[j]
            err = abs(step) * np.sqrt(nsq - 2.0 * uj + 1.0)
            iters += 1
            if not np.isfinite(err):
                break
            k1 = 1.0 - step
            nsq = (k1 * k1) * nsq + 2.0 * (step * k1) * uj + step * step
            u = k1 * u
            u[j] += step
            if not err > tolerance:
                status = 0
                break
            if iters >= max_iter:
                status = 1
                break
            V = k1 * V + step * np.outer(q[j], q[j])
    row[1] = iters
    if status == 2:
        return row, np.zeros(m)
    p = q[:, :3]
    c = u @ p
    C = (p * u[:, None]).T @ p - np.outer(c, c)
    row[2], row[3], row[4:7] = err, status, o + c
    row[7:13] = C[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return row, u


def fit_instance_ellipsoids(points, labels, tolerance=0.01, max_iter=10000, max_points=50000, generator=None, backend="device", k=10,
                            keep_percentile=70, n_sigma=3, return_info=False):
    """The reference's ``get_tight_bbox(..., method="ellipsoid")`` (visualize_bboxes.py:101-107, its default): per instance the
    minimum-volume enclosing ellipsoid of the filtered points by Khachiyan's algorithm (``getMinVolEllipse`` :135-189) and the box that
    circumscribes it, ``{instance_id: {"bbox": ((-r0, -r1, -r2), (r0, r1, r2)), "orientation": rotation (3, 3), "position": centre (3,)}}``
    with numpy fp64 values.  Rows of ``rotation`` are the ellipsoid's axes (ascending radius, from ``svd(inv(C) / 3)`` as :180-187), so the
    record is in the box frame ``orientation @ (p - position)`` like the boxes of ``fit_instance_boxes``.

    Grouping, subsample (``max_points``, ``generator``) and filter (``k``, ``keep_percentile``, ``n_sigma``) are those of
    ``fit_instance_boxes``.  The loop needs a 4 x 4 moment matrix, its Cholesky factor, one quadratic form per point and an argmax per
    iteration -- the reference builds ``np.diag(u)`` and ``QT V^-1 Q``, N x N each (10 GB at its own cap of 50 000 points).  As in the
    reference the loop ends when the weights move by no more than ``tolerance`` (at least one iteration), so the ellipsoid need not strictly
    enclose: at 0.01 the worst point lies at about 1.05 in the ellipsoid's norm.  ``max_iter`` bounds the loop, which the reference does not.

    ``backend="device"``: all instances in one launch of clift_segment_mvee.  ``backend="sklearn"``: the same loop in numpy per instance.
    Label 0, instances with fewer than k points and DEGENERATE instances (fewer than 4 kept points, or coplanar / collinear kept points: the
    moment matrix is not positive definite) are left out; the reference raises ``numpy.linalg.LinAlgError`` for singular ones or returns
    what the inverse of a near-singular matrix gives.  Instances stopped at ``max_iter`` are returned and listed in
    ``info["not_converged"]``.

    ``return_info=True`` returns ``(boxes, {"iters": {id: n}, "err": {id: x}, "kept": {id: n}, "total": {id: n}, "not_converged": [ids],
    "keep": (P,) bool mask of the rows the ellipsoids were fitted to})``."""
    pts, lab = _as_inputs(points, labels, backend)
    order, ids, seg = group_by_instance(lab, 0)
    total = (seg[1:] - seg[:-1]).cpu().numpy()
    order, seg = _subsample(order, seg, int(max_points), generator)
    ps = pts[order].contiguous()
    G = ids.numel()
    _, _, keep = _filter_sorted(ps, seg, int(k), keep_percentile, n_sigma, backend)
    keep = keep.to(pts.device).contiguous()
    if backend == "device":
        rows = segment_mvee(ps, seg, keep, tolerance, max_iter)[0].cpu().numpy()
    else:
        if not (tolerance > 0 and 1 <= int(max_iter) <= 1000000):
            raise ValueError(f"need tolerance > 0 and 1 <= max_iter <= 1000000, got {tolerance} and {max_iter}")
        P_all, keep_np, edges = ps.numpy(), keep.numpy(), seg.numpy()
        rows = np.zeros((G, MVEE_COLUMNS))
        for g in range(G):
            S = P_all[edges[g]:edges[g + 1]][keep_np[edges[g]:edges[g + 1]]].astype(np.float64)
            rows[g] = _mvee_host(S, float(tolerance), int(max_iter))[0]
    boxes, kept, iters, err, not_converged = {}, {}, {}, {}, []
    for g, inst_id in enumerate(ids.cpu().numpy().tolist()):
        kept[inst_id], iters[inst_id], err[inst_id] = int(rows[g, 0]), int(rows[g, 1]), float(rows[g, 2])
        if rows[g, 3] == 2:
            continue
        if rows[g, 3] == 1:
            not_converged.append(inst_id)
        A = np.linalg.inv(rows[g, [7, 8, 9, 8, 10, 11, 9, 11, 12]].reshape(3, 3)) / 3.0
        _, sv, rotation = np.linalg.svd(A)
        radii = 1.0 / np.sqrt(sv)
        boxes[inst_id] = {"bbox": (-radii, radii.copy()), "orientation": rotation, "position": rows[g, 4:7].copy()}
    if not return_info:
        return boxes
    mask = torch.zeros(pts.shape[0], dtype=torch.bool, device=pts.device)
    mask[order] = keep
    return boxes, {"iters": iters, "err": err, "kept": kept, "total": {i: int(t) for i, t in zip(ids.cpu().numpy().tolist(), total)},
                   "not_converged": not_converged, "keep": mask}
