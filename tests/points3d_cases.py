"""Shared inputs of the per-instance 3-D kernel tests (test_points3d_cases_host.py on the CPU, test_gpu_points3d_cases.py on the GPU): seeded
LAYOUTS for the four entry points of csrc/points3d.hip and plain NumPy references of what include/clift.h promises for them.  Test
infrastructure: nothing under contrastive_lift_amd/ imports it, and nothing here touches the GPU.

The goldens G24 / G26 and the timing layouts all come out of ``points3d.group_by_instance``: seg[0] == 0, seg[G] == n, no empty instance, no
entry outside [0, n].  The layouts here are what that function never produces and the header allows all the same:

  edges       seg[0] = 7, sizes EDGE_SIZES (empty ones in front, in the middle and side by side; sizes on and one either side of 64 and 256, one
              either side of 512 and one past 1024, which is where the one-block-per-instance kernels cut an instance; 1025 and 2500 rows = two and three LDS tiles of the kNN),
              five rows behind seg[G] that belong to nobody.  n = 5552 (not a multiple of 256), G = 17.
  clamped     the same rows with seg[0] = -3 and seg[G] = n + 5: "clamped, never followed" -- the first and the last instance grow to the
              ends of the array.
  windows     one 1088-row instance that ends ON a wave cut inside a block, three small ones behind it: the next wave's window
              [wlo, whi) misses the first LDS tile of its block's union altogether, the waves before it miss nothing.
  tiny_*      (n, G) = (1, 1), (3, 1), (64, 2) and (5, 0).
  ties        40 identical points, an 8 x 8 x 4 integer lattice in permuted order, 300 points of which 60 are exact duplicates; two rows
              behind seg[G].
  degenerate  for the filter at k = 10: instances of 9, 10 and 11 rows, the 40 identical points, a planar instance of 300 points, a
              700-point blob.  The planar and the identical instance have coordinates that are multiples of 2^-10, so that their sums and
              means are exact in any order (with a non-dyadic constant coordinate the host backend's |p - mean| < 3 std on the axis without
              spread is decided by the rounding error of its own mean, and the two backends may then legitimately disagree).

Points are an anisotropic Gaussian, sigma (0.4, 0.2, 0.1), turned off the axes and offset by (1000, -3, 0.25): at x = 1000 one float32 ulp is
6e-5, so any fp32 distance arithmetic differs visibly from the fp64 contract.  Everything is float32.

References: ``knn_reference`` (the full fp64 matrix per clamped instance), ``moments_ordered`` (the documented split of
clift_segment_moments, rounding for rounding: a device result equals it bit for bit), ``moments_exact`` (math.fsum of the same terms and the
scale of the bound), ``extent_reference``; the ellipsoid is held against ``ellipsoid_cases.khachiyan`` by ``assert_mvee_rows``, the rule of
test_gpu_ellipsoid.py.  ``KNN_MISTAKES`` / ``MOMENT_MISTAKES`` name deliberately wrong variants (the ``mistake=`` argument); the host test
proves that each of them is caught on some case."""
import functools
import math

import numpy as np

import ellipsoid_cases as ec

f32, f64 = np.float32, np.float64
BLOCK, WAVE, TILE = 256, 64, 1024                 # rows of a kNN block = threads of every kernel's block, lanes of a wave, candidates of an LDS tile
KS = (1, 4, 5, 8, 9, 12, 13, 16)                  # both ends of every register width KT = 4, 8, 12, 16 of k_knn_kth
K_MAX = 16
SIGMA = np.array([0.4, 0.2, 0.1])
OFFSET = np.array([1000.0, -3.0, 0.25])
FAR_CENTRE = np.array([-2048.5, 511.25, 1.0e6 / 3.0])
EDGE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 0, 0, 9, 10, 11, 2500]
EDGE_SEED, TIES_SEED, DEGENERATE_SEED, WINDOWS_SEED, TINY_SEED, MVEE_KEEP_SEED = 3, 4, 5, 6, 7, 3001
FILTER_K = 10
MVEE_MARGIN = 1e-9

KNN_MISTAKES = {
    "no_self": "the row itself left out of its own neighbours",
    "k_plus_1": "the (k+1)-th smallest instead of the k-th",
    "no_boundary": "the instance boundary ignored: the rows next to the instance are candidates too",
    "fp32": "differences, products and sums in fp32",
    "first_tile_only": "candidates past the first 1024 of an instance dropped",
    "unclamped": "seg not clamped: an entry below 0 is followed from the end of the array",
    "outside_finite": "rows outside [seg[0], seg[G]) given a finite value",
    "more_than_k": "'at least k rows' read as 'more than k rows'",
}
MOMENT_MISTAKES = {
    "keep_eq_1": "keep == 1 instead of keep != 0",
    "centre_fp32": "the centre subtracted from the fp32 value in fp32",
    "drop_last_row": "the last row of an instance dropped",
    "drop_wave_partial": "the fourth wave's partial dropped",
    "np_sum": "numpy's own (pairwise) order, one contiguous column at a time (differs in bits only; still inside the exact bound)",
}
KEEPS = ("none", "zeros", "random70", "bytes", "lane255")
CENTRES = ("none", "mean", "far")


# ---------------------------------------------------------------------------------------------------------------- layouts
def cloud(n, seed):
    """(n, 3) float32: the anisotropic Gaussian, turned off the axes, at OFFSET."""
    rng = np.random.default_rng(seed)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return np.ascontiguousarray(((rng.standard_normal((n, 3)) * SIGMA) @ R.T + OFFSET).astype(f32))


def dyadic(P):
    """Coordinates rounded to multiples of 2^-10 (exact in float32 at these magnitudes; sums of a few hundred are exact in fp64)."""
    return (np.round(np.asarray(P, f64) * 1024.0) / 1024.0).astype(f32)


def identical40():
    return np.repeat(dyadic(OFFSET[None] + np.array([[0.123, -0.456, 0.789]])), 40, 0)


def _seg(first, sizes):
    return (first + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)


def _edges():
    n = 7 + sum(EDGE_SIZES) + 5
    return cloud(n, EDGE_SEED), _seg(7, EDGE_SIZES)


def _clamped():
    pts, seg = _edges()
    seg = seg.copy()
    seg[0], seg[-1] = -3, pts.shape[0] + 5
    return pts, seg


def _windows():
    sizes = [1088, 30, 40, 100]
    return cloud(sum(sizes) + 3, WINDOWS_SEED), _seg(0, sizes)


def _ties():
    rng = np.random.default_rng(TIES_SEED)
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    lattice = lattice[rng.permutation(lattice.shape[0])]
    base = cloud(240, TIES_SEED + 100)
    dup = np.concatenate([base, base[rng.choice(240, 60, replace=False)]])[rng.permutation(300)]
    parts = [identical40(), lattice, dup, cloud(2, TIES_SEED + 200)]
    return np.ascontiguousarray(np.concatenate(parts).astype(f32)), _seg(0, [40, 256, 300])


def degenerate_cloud():
    """(points (P, 3) float32, labels (P,) int64, {label: what}) in SHUFFLED row order; label 0 (stuff) on 25 rows."""
    rng = np.random.default_rng(DEGENERATE_SEED)
    planar = dyadic(cloud(300, DEGENERATE_SEED + 10))
    planar[:, 2] = f32(0.25)
    parts = {3: cloud(FILTER_K - 1, DEGENERATE_SEED + 1), 5: cloud(FILTER_K, DEGENERATE_SEED + 2), 6: cloud(FILTER_K + 1, DEGENERATE_SEED + 3),
             -2: identical40(), 11: planar, 12: cloud(700, DEGENERATE_SEED + 4), 0: cloud(25, DEGENERATE_SEED + 5)}
    what = {3: "k-1", 5: "k", 6: "k+1", -2: "identical", 11: "planar", 12: "blob"}
    pts = np.concatenate(list(parts.values()))
    lab = np.concatenate([np.full(p.shape[0], i, np.int64) for i, p in parts.items()])
    perm = rng.permutation(pts.shape[0])
    return np.ascontiguousarray(pts[perm]), lab[perm], what


def _degenerate():
    """The degenerate cloud sorted by label as group_by_instance sorts it (label 0 left out): ids -2, 3, 5, 6, 11, 12."""
    pts, lab, _ = degenerate_cloud()
    rows = np.nonzero(lab != 0)[0]
    order = rows[np.argsort(lab[rows], kind="stable")]
    return np.ascontiguousarray(pts[order]), _seg(0, np.unique(lab[order], return_counts=True)[1])


def _tiny(n, G):
    pts = cloud(n, TINY_SEED + n)
    return pts, {(1, 1): _seg(0, [1]), (3, 1): _seg(0, [3]), (64, 2): _seg(0, [30, 34]), (5, 0): _seg(0, [])}[(n, G)]


_BUILDERS = {"edges": _edges, "clamped": _clamped, "windows": _windows, "tiny_1_1": lambda: _tiny(1, 1), "tiny_3_1": lambda: _tiny(3, 1),
             "tiny_64_2": lambda: _tiny(64, 2), "tiny_5_0": lambda: _tiny(5, 0), "ties": _ties, "degenerate": _degenerate}
CASES = tuple(_BUILDERS)
LAYOUT_OF = {c: c.split("_")[0] for c in CASES}   # tiny_* are the members of one layout
MVEE_CASES = ("edges", "clamped")


@functools.lru_cache(maxsize=None)
def case(name):
    """(pts (n, 3) float32, seg (G + 1,) int64), read-only."""
    pts, seg = _BUILDERS[name]()
    assert pts.dtype == f32 and seg.dtype == np.int64
    pts.setflags(write=False)
    seg.setflags(write=False)
    return pts, seg


def bounds(seg, n):
    """(lo (G,), hi (G,)): instance g owns rows lo[g] .. hi[g], entries of seg clamped to [0, n]."""
    c = np.clip(np.asarray(seg, np.int64), 0, n)
    return c[:-1], c[1:]


def instance_of_rows(seg, n):
    """(n,) instance of every row, -1 for a row outside [seg[0], seg[G])."""
    inst = np.full(n, -1, np.int64)
    for g, (lo, hi) in enumerate(zip(*bounds(seg, n))):
        inst[lo:hi] = g
    return inst


def knn_windows(seg, n):
    """What k_knn_kth stages and walks, per 256-row block: [{"rows": (r0, r1), "instances": [g], "union": (blo, bhi), "tiles": [(t0, t1)],
    "waves": [(wlo, whi) or None]}].  A dead lane (row >= n) takes row n - 1, as in the kernel."""
    inst = instance_of_rows(seg, n)
    lo, hi = bounds(seg, n)
    blocks = []
    for r0 in range(0, n, BLOCK):
        rows = np.minimum(np.arange(r0, r0 + BLOCK), n - 1)
        g = inst[rows]
        has = (g >= 0) & (hi[np.maximum(g, 0)] > lo[np.maximum(g, 0)]) if len(lo) else np.zeros(BLOCK, bool)
        waves = []
        for w in range(BLOCK // WAVE):
            gw = g[w * WAVE:(w + 1) * WAVE][has[w * WAVE:(w + 1) * WAVE]]
            waves.append((int(lo[gw].min()), int(hi[gw].max())) if gw.size else None)
        live = [w for w in waves if w is not None]
        union = (min(w[0] for w in live), max(w[1] for w in live)) if live else (0, 0)
        tiles = [(t0, min(t0 + TILE, union[1])) for t0 in range(union[0], union[1], TILE)]
        blocks.append({"rows": (r0, min(r0 + BLOCK, n)), "instances": sorted(set(g[has].tolist())), "union": union, "tiles": tiles, "waves": waves})
    return blocks


# ---------------------------------------------------------------------------------------------------------------- kNN
def knn_table(pts, seg, mistake=None):
    """(sorted (n, K_MAX + 1) fp64: per row the K_MAX + 1 smallest squared distances to the rows of its clamped instance, itself included,
    ascending, +inf where the instance has fewer; rows (n,) = the size of the row's instance, 0 outside [seg[0], seg[G])).  The distance is
    the header's ((dx*dx + dy*dy) + dz*dz) in fp64, every operation a separate NumPy operation."""
    assert mistake is None or mistake in KNN_MISTAKES
    n = pts.shape[0]
    dt = f32 if mistake == "fp32" else f64
    P = np.asarray(pts, f32).astype(dt)
    table, size = np.full((n, K_MAX + 1), np.inf), np.zeros(n, np.int64)
    edges = np.asarray(seg, np.int64) if mistake == "unclamped" else np.clip(np.asarray(seg, np.int64), 0, n)
    for a, b in zip(edges[:-1], edges[1:]):
        lo, hi = int(max(a, 0)), int(min(b, n))                    # the rows that are written
        if hi <= lo:
            continue
        cand = np.arange(a, b)
        if mistake == "unclamped":
            cand = cand % n
        if mistake == "no_boundary":
            cand = np.arange(max(a - 16, 0), min(b + 16, n))
        if mistake == "first_tile_only":
            cand = cand[:TILE]
        Q, C = P[lo:hi], P[cand]
        dx, dy, dz = Q[:, None, 0] - C[None, :, 0], Q[:, None, 1] - C[None, :, 1], Q[:, None, 2] - C[None, :, 2]
        xx, yy, zz = dx * dx, dy * dy, dz * dz
        D = ((xx + yy) + zz).astype(f64)
        if mistake == "no_self":
            D[np.arange(lo, hi)[:, None] == cand[None, :]] = np.inf
        m = min(D.shape[1], K_MAX + 1)
        table[lo:hi, :m] = np.sort(D, axis=1)[:, :m]
        size[lo:hi] = hi - lo
    return table, size


def knn_from_table(table, size, k, mistake=None):
    col = table[:, k] if mistake == "k_plus_1" else table[:, k - 1]
    enough = size > k if mistake == "more_than_k" else size >= k
    out = np.where(enough, col, np.inf)
    if mistake == "outside_finite":
        out = np.where(size == 0, 0.0, out)
    return out


def knn_reference(pts, seg, k, mistake=None):
    """(n,) fp64: the squared distance of every row to its k-th nearest row of the same instance, itself included; +inf in instances with
    fewer than k rows and on rows in no instance."""
    return knn_from_table(*knn_table(pts, seg, mistake), k, mistake)


@functools.lru_cache(maxsize=None)
def knn_case_table(name):
    return knn_table(*case(name))


# ---------------------------------------------------------------------------------------------------------------- keep masks, centres, frames
@functools.lru_cache(maxsize=None)
def keep_mask(name, kind):
    """None or (n,) uint8."""
    pts, seg = case(name)
    n = pts.shape[0]
    rng = np.random.default_rng(1000 + CASES.index(name) * 10 + KEEPS.index(kind))
    if kind == "none":
        return None
    if kind == "zeros":
        k = np.zeros(n, np.uint8)
    elif kind == "random70":
        k = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    elif kind == "bytes":
        k = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
    else:
        k = np.ones(n, np.uint8)                                   # (rows in no instance: whatever stands there is never read)
        for lo, hi in zip(*bounds(seg, n)):
            k[lo:hi] = (np.arange(hi - lo) % BLOCK) == BLOCK - 1
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def centre_of(name, kind):
    """None or (G, 3) fp64."""
    pts, seg = case(name)
    G = seg.shape[0] - 1
    if kind == "none":
        return None
    c = np.tile(FAR_CENTRE, (G, 1))
    if kind == "mean":
        for g, (lo, hi) in enumerate(zip(*bounds(seg, pts.shape[0]))):
            c[g] = pts[lo:hi].astype(f64).mean(0) if hi > lo else 0.0
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def frame_of(name, kind):
    """(G, 12) fp64: random orthonormal axes per instance, ONE frame (instance min(3, G - 1)) that is not orthonormal; then the centre."""
    pts, seg = case(name)
    G = seg.shape[0] - 1
    rng = np.random.default_rng(2000 + CASES.index(name))
    A = np.linalg.qr(rng.standard_normal((G, 3, 3)))[0] if G else np.zeros((0, 3, 3))
    if G:
        A[min(3, G - 1)] = rng.standard_normal((3, 3)) * np.array([[2.0], [0.5], [1e-3]])
    c = centre_of(name, kind)
    out = np.ascontiguousarray(np.concatenate([A.reshape(G, 9), np.zeros((G, 3)) if c is None else c], 1))
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- moments and extents
def moment_terms(P, c, mistake=None):
    """(rows, 10) fp64: 1, qx, qy, qz, qx*qx, qx*qy, qx*qz, qy*qy, qy*qz, qz*qz with q = double(p) - c, every operation on its own."""
    if mistake == "centre_fp32":
        q = (np.asarray(P, f32) - np.asarray(c, f64).astype(f32)).astype(f64)
    else:
        q = np.asarray(P, f32).astype(f64) - np.asarray(c, f64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([np.ones(len(q)), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], 1)


def ordered_sum(terms, kept, mistake=None):
    """The fixed split: row t + 256 j of the instance goes to accumulator t in order of j (a row that is not kept adds nothing; + 0.0 on an
    accumulator that started at + 0.0 leaves the same bits); per group of 64 accumulators v = v + v[lane ^ off] for off = 32 .. 1; then
    ((p0 + p1) + p2) + p3."""
    rows, nv = terms.shape
    rounds = -(-rows // BLOCK)
    padded = np.zeros((max(rounds, 1) * BLOCK, nv))
    padded[:rows] = np.where(kept[:, None], terms, 0.0)
    acc = np.zeros((BLOCK, nv))
    for j in range(rounds):
        acc = acc + padded[j * BLOCK:(j + 1) * BLOCK]
    v = acc.reshape(BLOCK // WAVE, WAVE, nv)
    lane = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    p = v[:, 0]
    return (p[0] + p[1]) + p[2] if mistake == "drop_wave_partial" else ((p[0] + p[1]) + p[2]) + p[3]


def _kept_rows(keep, lo, hi, mistake=None):
    if keep is None:
        kept = np.ones(hi - lo, bool)
    else:
        kept = keep[lo:hi] == 1 if mistake == "keep_eq_1" else keep[lo:hi] != 0
    if mistake == "drop_last_row" and hi > lo:
        kept = kept.copy()
        kept[-1] = False
    return kept


def moments_ordered(pts, seg, keep=None, centre=None, mistake=None):
    """(G, 10) fp64: clift_segment_moments restated rounding for rounding."""
    assert mistake is None or mistake in MOMENT_MISTAKES
    n, G = pts.shape[0], len(seg) - 1
    out = np.zeros((G, 10))
    for g, (lo, hi) in enumerate(zip(*bounds(seg, n))):
        terms = moment_terms(pts[lo:hi], np.zeros(3) if centre is None else centre[g], mistake)
        kept = _kept_rows(keep, lo, hi, mistake)
        out[g] = np.ascontiguousarray(terms[kept].T).sum(1) if mistake == "np_sum" else ordered_sum(terms, kept, mistake)
    return out


def moments_exact(pts, seg, keep=None, centre=None):
    """(exact (G, 10): math.fsum of the same fp64 terms, correctly rounded; scale (G, 10): the sum of their magnitudes;
    bound (G,): (ceil(rows_g / 256) + 10) * 2^-53 -- a result of the split passes through at most ceil(rows_g / 256) additions on its
    accumulator, six in the butterfly and three over the partials, and the standard bound of a summation tree of that depth is
    depth * 2^-53 * sum |term| to first order; the + 10 instead of + 9 pays for the second order.)"""
    n, G = pts.shape[0], len(seg) - 1
    exact, scale, bound = np.zeros((G, 10)), np.zeros((G, 10)), np.zeros(G)
    for g, (lo, hi) in enumerate(zip(*bounds(seg, n))):
        terms = moment_terms(pts[lo:hi], np.zeros(3) if centre is None else centre[g])[_kept_rows(keep, lo, hi)]
        exact[g] = [math.fsum(terms[:, j]) for j in range(10)]
        scale[g] = [math.fsum(np.abs(terms[:, j])) for j in range(10)]
        bound[g] = (-(-(hi - lo) // BLOCK) + 10) * 2.0 ** -53
    return exact, scale, bound


def extent_reference(pts, seg, frame, keep=None):
    """(G, 6) fp64: min (3) and max (3) over the kept rows of v_r = ((A[r][0]*qx + A[r][1]*qy) + A[r][2]*qz), q = double(p) - c; +inf / -inf
    where nothing is kept."""
    n, G = pts.shape[0], len(seg) - 1
    out = np.concatenate([np.full((G, 3), np.inf), np.full((G, 3), -np.inf)], 1)
    for g, (lo, hi) in enumerate(zip(*bounds(seg, n))):
        kept = _kept_rows(keep, lo, hi)
        if not kept.any():
            continue
        A, c = frame[g, :9].reshape(3, 3), frame[g, 9:12]
        q = pts[lo:hi][kept].astype(f64) - c
        for r in range(3):
            ax, ay, az = A[r, 0] * q[:, 0], A[r, 1] * q[:, 1], A[r, 2] * q[:, 2]
            v = (ax + ay) + az
            out[g, r], out[g, 3 + r] = v.min(), v.max()
    return out


# ---------------------------------------------------------------------------------------------------------------- the ellipsoid
MVEE_KEEPS = ("none", "masked")
THREE_ROWS, FOUR_ROWS = 5, 6                      # instances of `edges` (255 and 256 rows) that the "masked" keep cuts down to 3 and to 4 rows


@functools.lru_cache(maxsize=None)
def mvee_keep(name, kind, alphabet=(0, 1)):
    """None, or (n,) uint8: a random 70 % of the rows, exactly three rows of instance THREE_ROWS and exactly four of instance FOUR_ROWS.
    ``alphabet`` = (0, 1) writes the mask with those bytes; (0, 2, 255) is the SAME mask with 2 or 255 wherever a row is kept."""
    if kind == "none":
        return None
    pts, seg = case(name)
    n = pts.shape[0]
    rng = np.random.default_rng(MVEE_KEEP_SEED + CASES.index(name))
    k = rng.uniform(size=n) < 0.7
    lo, hi = bounds(seg, n)
    for g, m in ((THREE_ROWS, 3), (FOUR_ROWS, 4)):
        k[lo[g]:hi[g]] = False
        k[lo[g] + rng.choice(hi[g] - lo[g], m, replace=False)] = True
    other = rng.choice(np.array(alphabet[1:], np.uint8), n)
    out = np.where(k, other, np.uint8(0)).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mvee_references(name, kind):
    """ellipsoid_cases.khachiyan on the kept rows of every clamped instance."""
    pts, seg = case(name)
    keep = mvee_keep(name, kind)
    refs = []
    for lo, hi in zip(*bounds(seg, pts.shape[0])):
        kept = _kept_rows(keep, lo, hi)
        refs.append(ec.khachiyan(pts[lo:hi][kept]))
    return refs


def under_margin(refs):
    """Instances whose argmax the helper cannot vouch for: not degenerate, and the smallest margin over their iterations <= MVEE_MARGIN."""
    return [g for g, r in enumerate(refs) if r["status"] != 2 and not r["margin"] > MVEE_MARGIN]


def assert_mvee_rows(out, u_rows, refs, which, rel=1e-9):
    """The rule of test_gpu_ellipsoid.py: same status and iteration count, centre within ``rel`` of max(1, largest |coordinate|), C within
    ``rel`` of its largest entry, err within ``rel`` of max(err, 1e-3), u within ``rel`` -- on the instances that converged in the helper
    with an argmax margin above MVEE_MARGIN.  ``u_rows[g]`` = the kernel's u on the KEPT rows of instance g.  Returns how many were compared."""
    done = 0
    for gi, r in enumerate(refs):
        if r["status"] == 2 or not r["margin"] > MVEE_MARGIN:
            continue
        row = out[gi]
        assert row[3] == r["status"] and row[1] == r["iters"], (which, gi, row[:4], r["iters"])
        scale = max(1.0, float(np.abs(r["centre"]).max()))
        assert np.abs(row[4:7] - r["centre"]).max() <= rel * scale, (which, gi, row[4:7] - r["centre"])
        C = ec.second_moment(row[7:13])
        assert np.abs(C - r["C"]).max() <= rel * np.abs(r["C"]).max(), (which, gi, np.abs(C - r["C"]).max())
        assert abs(row[2] - r["err"]) <= rel * max(r["err"], 1e-3), (which, gi, row[2], r["err"])
        assert np.abs(u_rows[gi] - r["u"]).max() <= rel, (which, gi, np.abs(u_rows[gi] - r["u"]).max())
        done += 1
    return done
