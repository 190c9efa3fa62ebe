"""Shared inputs of the mean-shift tests (test_meanshift_cases_host.py and test_meanshift_host.py on the CPU, test_gpu_meanshift_cases.py on the
GPU): seeded cases for clift_meanshift (csrc/cluster.hip) and two NumPy restatements of its per-seed climb.

``numpy_shift`` is the arithmetic that clift.h pins -- fp64 neighbour test and sum, fp32 mean, fp32 step norm -- with NumPy's own summation
order.  ``ordered_shift`` is the same climb with EVERY rounding of the kernel, the order of the neighbour sum included (the library is built
without contraction and cluster.hip documents the split), so a device result has to equal it bit for bit:

  d2     fp64, summed in dimension order from double(x_k) - double(m_k); neighbour when d2 <= bandwidth^2
  sum    point i goes to partial i % 256 and is added in ascending i; inside each group of 64 partials the xor butterfly at offsets
         32, 16, ..., 1 (a = a + a[lane ^ off]); then ((w0 + w1) + w2) + w3
  mean   float32(sum / count)
  norm   fp32 sum of fp32 squares in dimension order, fp32 sqrt
  stop   double(norm) <= 1e-3 * bandwidth or it == max_iter, checked BEFORE it += 1
  empty  a step without neighbour leaves the centre at the last mean, with count 0

``MISTAKES`` names deliberately wrong variants of ``ordered_shift`` (the ``mistake=`` argument); the host test proves that every one of them
changes a centre bit, a count or an iteration number on at least one case.  Nothing here touches the GPU."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
BLOCK, WAVE = 256, 64                             # threads of a block (one block per seed), lanes of a wave
MAX_D = 32

MISTAKES = {
    "d2_fp32": "the squared distance formed and summed in fp32",
    "sum_fp32": "the neighbour sum carried in fp32",
    "ball_exclusive": "d2 < bandwidth^2 instead of <=",
    "stop_exclusive": "norm < stop instead of <=",
    "it_first": "it incremented before it is compared with max_iter",
    "mean_fp64": "the fp64 mean, not its fp32 rounding, is the centre of the next step's ball",
    "stop_bw2": "stop = 1e-3 * bandwidth^2",
    "pad_read": "the first padding column read as one more coordinate",
}


# ---------------------------------------------------------------------------------------------------------------- references
def numpy_shift(X, seeds, bandwidth, max_iter):
    """What clift_meanshift computes, one seed at a time."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    bw2, stop = bandwidth * bandwidth, 1e-3 * bandwidth
    S, d = np.asarray(seeds).shape
    centers, counts, iters = np.zeros((S, d), np.float32), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for s, seed in enumerate(np.asarray(seeds, dtype=np.float32)):
        m, it = seed.copy(), 0
        while True:
            nb = ((X64 - m.astype(np.float64)) ** 2).sum(1) <= bw2
            c = int(nb.sum())
            if c == 0:
                break
            nm = (X64[nb].sum(0) / c).astype(np.float32)
            step = float(np.linalg.norm(nm - m))
            m = nm
            if step <= stop or it == max_iter:
                break
            it += 1
        centers[s], counts[s], iters[s] = m, c, it
    return centers, counts, iters


def blobs(seed, n_per, d, spread=0.05, k=4):
    rng = np.random.default_rng(seed)
    cent = rng.uniform(0.1, 0.9, (k, d))
    return np.concatenate([c + spread * rng.standard_normal((n_per, d)) for c in cent]).astype(np.float32)


def ordered_sum(rows, nb):
    """The kernel's neighbour sum of ``rows`` (n, d) over the mask ``nb``, in the dtype of ``rows``: 256 partials filled in ascending point
    index, an xor butterfly inside each group of 64, the four groups added in order.  (A thread adds nothing for a point outside the ball;
    adding +0 to a partial that started at +0 leaves the same bits.)"""
    n, d = rows.shape
    rounds = -(-n // BLOCK)
    padded = np.zeros((rounds * BLOCK, d), rows.dtype)
    padded[:n] = np.where(nb[:, None], rows, rows.dtype.type(0))
    part = np.zeros((BLOCK, d), rows.dtype)
    for r in range(rounds):
        part = part + padded[r * BLOCK:(r + 1) * BLOCK]
    a = part.reshape(BLOCK // WAVE, WAVE, d)
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off >= 1:
        a = a + a[:, lane ^ off]
        off //= 2
    w = a[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def ordered_shift(X, seeds, bandwidth, max_iter, mistake=None, trace=None):
    """clift_meanshift restated rounding for rounding: (centers (S, d) fp32, counts (S,) int64, iters (S,) int64).  ``X`` is (n, ldx) with
    ldx >= d = seeds.shape[1]; the columns from d on are padding.  ``mistake`` selects a wrong variant (``MISTAKES``).  ``trace``, a list,
    receives one record per seed: the neighbour count and the fp32 norm of every step, the last neighbour mask, and why the climb ended
    ("norm", "max_iter" or "empty"; "norm" when both hold)."""
    assert mistake is None or mistake in MISTAKES, mistake
    X = np.asarray(X, dtype=f32)
    seeds = np.asarray(seeds, dtype=f32)
    S, d = seeds.shape
    n = X.shape[0]
    X32 = np.ascontiguousarray(X[:, :d])
    X64 = X32.astype(f64)
    pad = X[:, d].astype(f64) if mistake == "pad_read" and X.shape[1] > d else None
    bw2 = bandwidth * bandwidth
    stop = 1e-3 * bw2 if mistake == "stop_bw2" else 1e-3 * bandwidth
    centers, counts, iters = np.zeros((S, d), f32), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for s in range(S):
        m = seeds[s].copy()
        centre64 = m.astype(f64)                             # centre of the ball: double(m), except under "mean_fp64"
        it, c, steps = 0, 0, 0
        rec = dict(counts=[], norms=[], nb=np.zeros(n, bool), end=None)
        while True:
            with np.errstate(invalid="ignore", over="ignore"):
                if mistake == "d2_fp32":
                    d2 = np.zeros(n, f32)
                    for k in range(d):
                        t = X32[:, k] - m[k]
                        d2 = d2 + t * t
                    d2 = d2.astype(f64)
                else:
                    d2 = np.zeros(n, f64)
                    for k in range(d):
                        t = X64[:, k] - centre64[k]
                        d2 = d2 + t * t
                if pad is not None:
                    d2 = d2 + pad * pad
                nb = d2 < bw2 if mistake == "ball_exclusive" else d2 <= bw2
            c = int(nb.sum())
            rec["counts"].append(c)
            if c == 0:
                rec["end"] = "empty"
                break
            rec["nb"] = nb
            total = ordered_sum(X32, nb).astype(f64) if mistake == "sum_fp32" else ordered_sum(X64, nb)
            mean64 = total / f64(c)
            nm = mean64.astype(f32)
            t = nm - m
            s2 = f32(0)
            for k in range(d):
                s2 = s2 + t[k] * t[k]
            norm = np.sqrt(s2)
            assert norm.dtype == f32 and s2.dtype == f32
            rec["norms"].append(norm)
            m = nm
            centre64 = mean64 if mistake == "mean_fp64" else m.astype(f64)
            small = f64(norm) < stop if mistake == "stop_exclusive" else f64(norm) <= stop
            steps += 1
            if mistake == "it_first":
                if small:
                    rec["end"] = "norm"
                    break
                it += 1
                if it == max_iter or steps > max_iter + 2000:
                    rec["end"] = "max_iter"
                    break
                continue
            if small or it == max_iter:
                rec["end"] = "norm" if small else "max_iter"
                break
            it += 1
        centers[s], counts[s], iters[s] = m, c, it
        if trace is not None:
            trace.append(rec)
    return centers, counts, iters


def fsum_mean(X, nb):
    """float32 of the exactly summed mean of the rows ``nb`` of X (n, d)."""
    rows = np.asarray(X, dtype=f32).astype(f64)[nb]
    return np.array([math.fsum(rows[:, k]) / len(rows) for k in range(rows.shape[1])], f64).astype(f32)


def ulps_apart(a, b):
    """Largest distance of two fp32 arrays in units of the last place (finite values of one sign per element, or equal)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.size == 0:
        return 0
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One clift_meanshift call: X (n, ldx) fp32 whose columns from d on are NaN, seeds (S, d) fp32, bandwidth, max_iter, and what the case
    is there for.  ``climb`` marks the cases that have to contain a real climb, ``shared`` those with two seeds that end on one neighbour set."""

    def __init__(self, name, X, d, seeds, bandwidth, max_iter, why, climb=False, shared=True):
        self.name, self.d, self.bandwidth, self.max_iter, self.why, self.climb, self.shared = name, d, float(bandwidth), int(max_iter), why, climb, shared
        self.X = np.ascontiguousarray(X, dtype=f32)
        self.seeds = np.ascontiguousarray(seeds, dtype=f32).reshape(-1, d)
        self.n, self.ldx = self.X.shape
        self.S = self.seeds.shape[0]
        assert 1 <= d <= MAX_D and self.ldx >= d and np.isnan(self.X[:, d:]).all() and np.isfinite(self.X[:, :d]).all()
        assert np.isfinite(self.seeds).all()

    @property
    def points(self):
        return self.X[:, :self.d]

    def __repr__(self):
        return f"Case({self.name}: n={self.n} d={self.d} ldx={self.ldx} S={self.S} bw={self.bandwidth:g} max_iter={self.max_iter})"


def width_group(d):
    """The k_meanshift instantiation that serves a width: <3, true>, else the smallest of <4>, <8>, <16>, <32> that holds it."""
    return 3 if d == 3 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def widen(P, ldx):
    """(n, ldx) copy of the points P (n, d) with NaN in the padding columns: they must not be read."""
    X = np.full((P.shape[0], ldx), np.nan, f32)
    X[:, :P.shape[1]] = P
    return X


FAR, LONE, KNOT = 50.0, -2.0, 3.0


def ramp_case(name, seed, n, d, ldx, bandwidth, max_iter, why, climb=True, length=0.6, noise=0.004, scale=1.0):
    """Points along a random direction whose density rises towards one end (Beta(2, 1) along the segment), with isotropic noise well under
    the bandwidth: a seed at the thin end climbs for many steps and its neighbour count grows on the way.  Three points are set aside: a
    lone one at LONE and, when there is room, a knot of points within 1e-3 of KNOT.  The seeds: climbers from the thin end and the middle,
    two starts beside the dense end, two starts beside the knot (they end on the same neighbour set), the lone point itself (count 1,
    iters 0) and a seed at FAR that never has a neighbour.  ``scale`` multiplies points, seeds and bandwidth: above 1 the stop value
    1e-3 * bandwidth is below 1e-3 * bandwidth^2, and steps of a size between the two occur."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    t = np.sort(rng.beta(2.0, 1.0, n))
    P = 0.5 + length * (t[:, None] - 0.5) * u + noise * rng.standard_normal((n, d))
    P = P[rng.permutation(n)]
    at = lambda tau: 0.5 + length * (tau - 0.5) * u
    seeds = []
    knot = min(5, max(0, n - 40))
    body = n - 1 - knot if n > 1 else n
    if n > 1:
        P[body] = LONE
        P[body + 1:] = KNOT + 1e-3 * rng.standard_normal((knot, d))
        seeds.append(P[body])
    lowest = int(np.argmin((P[:body] - 0.5) @ u))
    seeds += [P[lowest], at(0.3), at(0.55), at(0.93), at(0.97)]
    if knot:
        seeds += [np.full(d, KNOT) + 0.2 * bandwidth / math.sqrt(d), np.full(d, KNOT) - 0.3 * bandwidth / math.sqrt(d)]
    seeds.append(np.full(d, FAR))
    return Case(name, widen(scale * P, ldx), d, scale * np.array(seeds), scale * bandwidth, max_iter, why, climb=climb)


def single_point_case(name, d, ldx, why):
    """n = 1: 255 idle threads, three idle waves.  Seeds: the point, two starts beside it (the same set), one out of reach."""
    P = np.linspace(0.25, 0.75, d, dtype=f64)[None]
    seeds = np.concatenate([P, P + 0.01 / math.sqrt(d), P - 0.02 / math.sqrt(d), np.full((1, d), FAR)])
    return Case(name, widen(P, ldx), d, seeds, 0.05, 300, why)


def boundary_case():
    """Coordinates on the 2^-6 lattice, bandwidth 5 * 2^-6.  The seed (32, 32, 32) sits on a data point; (+-3, +-4, 0) and (0, 0, +-5) around
    it are at d2 == bandwidth^2 exactly (inside: <=), (+-3, +-4, +-1) just outside, (+-1, 0, 0) inside.  Every sum is exact and symmetric:
    the mean is the seed, the first step stops, count 7.  A second copy of the arrangement at (96, 32, 32) has a seed one lattice step off
    its centre."""
    ring = [(0, 0, 0), (3, 4, 0), (-3, -4, 0), (0, 0, 5), (0, 0, -5), (1, 0, 0), (-1, 0, 0), (3, 4, 1), (-3, -4, -1)]
    pts = [(cx + a, 32 + b, 32 + c) for cx in (32, 96) for a, b, c in ring]
    P = np.array(pts, f64) / 64.0
    seeds = np.array([(32, 32, 32), (97, 32, 32), (32, 32, 31), (3200, 3200, 3200)], f64) / 64.0
    return Case("boundary_lattice_d3", widen(P, 3), 3, seeds, 5.0 / 64.0, 300, "d2 == bandwidth^2 exactly: the ball is inclusive", shared=False)


def rounding_pairs():
    """A seed at 0.5^3 with mirrored pairs 0.5 +- t, t a multiple of 2^-22, all exactly representable, so the mean stays on the seed.  The
    bandwidths^2 of the two variants lie strictly between the exact d2 of a pair (which fp64 forms without error) and its fp32 value: one
    pair is inside in fp64 and outside in fp32, the other the opposite way.  Returns {fp32 value above the exact one: (q, exact, fp32)}."""
    rng = np.random.default_rng(71)
    found = {}
    while len(found) < 2:
        q = rng.integers(100000, 240000, 3)
        t32 = (q * 2.0 ** -22).astype(f32)
        exact = float(np.sum(q.astype(object) ** 2)) * 2.0 ** -44
        s = f32(0)
        for k in range(3):
            s = s + t32[k] * t32[k]
        if abs(float(s) - exact) > 2e-8 * exact:
            found.setdefault(float(s) > exact, (q, exact, float(s)))
    return found


def ball_rounding_cases():
    out = []
    for above, (q, exact, rounded) in sorted(rounding_pairs().items()):
        t = q * 2.0 ** -22
        P = np.array([[0.5, 0.5, 0.5], 0.5 + t, 0.5 - t, 0.5 + 2 * t, 0.5 - 2 * t])
        bw = math.sqrt(0.5 * (exact + rounded))
        lo, hi = min(exact, rounded), max(exact, rounded)
        assert lo < bw * bw < hi
        name = "ball_fp64_inside_fp32_outside_d3" if above else "ball_fp64_outside_fp32_inside_d3"
        out.append(Case(name, widen(P, 3), 3, np.array([[0.5, 0.5, 0.5], [FAR] * 3]), bw, 300,
                        "bandwidth^2 between the fp64 and the fp32 value of a pair's d2", shared=False))
    return out


def offset_cloud_case():
    """100 + 0.01 * noise, stretched along x: one fp32 ulp of a coordinate is 7.6e-6, a 2600th of the bandwidth.  An fp32 neighbour sum or a
    centre carried in fp64 lands elsewhere.  (x - m is exact in fp32 here, both being near 100: an fp32 d2 errs by 1e-7 relative only, and
    it is the ball_* cases that catch it.)"""
    rng = np.random.default_rng(83)
    noise = rng.standard_normal((1000, 3)) * np.array([3.0, 1.0, 1.0])
    P = (100.0 + 0.01 * noise).astype(f32)
    seeds = np.array([P[np.argmin(P[:, 0])], P[np.argmax(P[:, 0])], [100.02, 100.0, 100.0], [100.0, 100.0, 100.0], [100.001, 100.001, 100.0],
                      [FAR] * 3])
    return Case("offset_cloud_d3_n1000", widen(P, 3), 3, seeds, 0.02, 300, "coordinates near 100: fp64 distance and sum", climb=True)


def zero_stop_case():
    """A subnormal bandwidth: bandwidth^2 and 1e-3 * bandwidth both underflow to 0.  The ball holds the copies of the centre alone and the
    first step has norm 0 == stop: <= stops at once (iters 0), < goes on to max_iter."""
    P = np.array([[0.25, 0.5, 0.75]] * 3 + [[0.5, 0.5, 0.5]] * 2 + [[0.1, 0.2, 0.3]])
    seeds = np.array([[0.25, 0.5, 0.75], [0.5, 0.5, 0.5], [0.1, 0.2, 0.3], [0.3, 0.3, 0.3]])
    return Case("zero_stop_d3", widen(P, 6), 3, seeds, 2.0 ** -1070, 2, "norm == stop == 0: the stop test is inclusive", shared=False)


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        # <4, false>
        ramp_case("d1_n1000", 101, 1000, 1, 1, 0.05, 300, "<4>: d = 1, four points per thread", noise=0.0),
        ramp_case("d2_n257_ldx5", 102, 257, 2, 5, 0.08, 300, "<4>: d = 2, one thread holds two points, padded rows"),
        ramp_case("d4_n64_max2", 103, 64, 4, 4, 0.12, 2, "<4>: d = DM, exactly one wave, stopped by max_iter = 2", climb=False),
        single_point_case("d1_n1_ldx4", 1, 4, "<4>: one point, padded row"),
        # <3, true>
        ramp_case("d3_n1000_ldx6", 104, 1000, 3, 6, 0.06, 300, "<3>: padded rows"),
        ramp_case("d3_n63_max1", 105, 63, 3, 3, 0.12, 1, "<3>: less than one wave, stopped by max_iter = 1", climb=False),
        # <8, false>
        ramp_case("d5_n255_ldx8", 106, 255, 5, 8, 0.08, 300, "<8>: d < DM, one thread idle, padded rows"),
        ramp_case("d8_n1000", 107, 1000, 8, 8, 0.06, 300, "<8>: d = DM"),
        ramp_case("d8_n256_max0", 108, 256, 8, 8, 0.1, 0, "<8>: every thread one point, max_iter = 0: one step", climb=False),
        # <16, false>
        ramp_case("d9_n1000_x200", 109, 1000, 9, 9, 0.06, 300, "<16>: d < DM; bandwidth 12, steps between 1e-3 bw and 1e-3 bw^2", scale=200.0),
        ramp_case("d16_n257_ldx19", 110, 257, 16, 19, 0.09, 300, "<16>: d = DM, padded rows"),
        # <32, false>
        ramp_case("d17_n1000_ldx20", 111, 1000, 17, 20, 0.07, 300, "<32>: d < DM, padded rows"),
        ramp_case("d32_n1000", 112, 1000, 32, 32, 0.08, 300, "<32>: d = DM, the largest input"),
        single_point_case("d32_n1", 32, 32, "<32>: one point"),
        boundary_case(),
        offset_cloud_case(),
        zero_stop_case(),
    ] + ball_rounding_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def case_names():
    return [c.name for c in cases()]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``ordered_shift`` of a case, computed once: (centers, counts, iters, trace).  The arrays are read-only."""
    c = case(name)
    trace = []
    out = ordered_shift(c.X, c.seeds, c.bandwidth, c.max_iter, trace=trace)
    for a in out:
        a.setflags(write=False)
    return out + (trace,)


def shared_sets(name):
    """Groups (lists of seed indices, two or more) whose last step had the same non-empty neighbour set."""
    trace = reference(name)[3]
    groups = {}
    for s, rec in enumerate(trace):
        if rec["counts"][-1] > 0:
            groups.setdefault(rec["nb"].tobytes(), []).append(s)
    return [g for g in groups.values() if len(g) >= 2]
