"""Seeded inputs for the minimum-volume-ellipsoid tests (host and GPU) and a small numpy Khachiyan to hold the product against.  Test
infrastructure: nothing under contrastive_lift_amd/ imports it.

``khachiyan`` is written independently of the product's choices: rows centred on their mean, but V summed afresh every iteration,
``np.linalg.inv`` instead of a Cholesky factor and the norm of ``new_u - u`` taken directly.  It also returns, per iteration, the MARGIN of
the argmax: (largest M - second-largest DISTINCT M) / largest M.  While that stays far above fp64 rounding (1e-9 is asked for), two correct
implementations with different summation orders pick the same row in every iteration, so iteration counts can be compared exactly."""
import numpy as np

TETRAHEDRON = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
COPLANAR4 = np.array([[0, 0, 0], [1, 0, 1], [0, 1, 1], [1, 1, 2]], np.float64)          # z = x + y
THREE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float64)
EDGE_STATUS = [0, 2, 2, 2, 0, 2, 0]
LARGE_SEED = 7


def tetra_plus_centroid(repeats=20):
    return np.concatenate([TETRAHEDRON, np.repeat(TETRAHEDRON.mean(0, keepdims=True), repeats, 0)])


def blob(n, seed):
    """An anisotropic Gaussian blob off the world axes, float32-representable."""
    rng = np.random.default_rng(seed)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    P = (rng.standard_normal((n, 3)) * np.array([0.4, 0.2, 0.1])) @ R.T + rng.uniform(-2, 2, 3)
    return P.astype(np.float32).astype(np.float64)


def layout(parts):
    pts = np.concatenate([p.reshape(-1, 3) for p in parts]).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum([p.reshape(-1, 3).shape[0] for p in parts])]).astype(np.int64)
    return np.ascontiguousarray(pts), seg


def edge_layout():
    """G = 7: tetrahedron, empty, coplanar four, three points, 257-point blob, one point, 1 025-point blob (statuses EDGE_STATUS)."""
    return layout([TETRAHEDRON, np.zeros((0, 3)), COPLANAR4, THREE, blob(257, 11), np.array([[0.5, -0.25, 2.0]]), blob(1025, 12)])


def large_layout(seed=LARGE_SEED):
    """One instance of 20 000 points beside 300 instances of 30 points."""
    return layout([blob(20000, 1000 * seed)] + [blob(30, 1000 * seed + 1 + i) for i in range(300)])


def khachiyan(P, tolerance=0.01, max_iter=10000):
    """{"status", "iters", "err", "centre", "C", "js" (argmax row per iteration), "margin" (the smallest over the iterations), "u"}."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    m = P.shape[0]
    res = {"status": 2, "iters": 0, "err": 0.0, "centre": np.zeros(3), "C": np.zeros((3, 3)), "js": [], "margin": np.inf, "u": np.zeros(m)}
    if m < 4 or np.linalg.matrix_rank(P - P.mean(0)) < 3:
        return res
    o = P.mean(0)
    Q = np.concatenate([P - o, np.ones((m, 1))], 1)
    u = np.full(m, 1.0 / m)
    while True:
        V = (Q * u[:, None]).T @ Q
        M = np.einsum("ij,jk,ik->i", Q, np.linalg.inv(V), Q)
        j = int(np.argmax(M))
        others = M[M != M[j]]
        if others.size:
            res["margin"] = min(res["margin"], float((M[j] - others.max()) / M[j]))
        step = (M[j] - 4.0) / (4.0 * (M[j] - 1.0))
        new_u = (1.0 - step) * u
        new_u[j] += step
        res["err"] = float(np.linalg.norm(new_u - u))
        u = new_u
        res["js"].append(j)
        res["iters"] += 1
        if not res["err"] > tolerance:
            res["status"] = 0
            break
        if res["iters"] >= max_iter:
            res["status"] = 1
            break
    c = u @ Q[:, :3]
    res["centre"], res["C"], res["u"] = o + c, (Q[:, :3] * u[:, None]).T @ Q[:, :3] - np.outer(c, c), u
    return res


def second_moment(row6):
    """(3, 3) from Cxx Cxy Cxz Cyy Cyz Czz."""
    return np.asarray(row6, np.float64)[[0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(3, 3)


def ellipsoid_of(C):
    """(radii (3,), rotation (3, 3)) as the reference derives them (visualize_bboxes.py:180-187)."""
    _, s, rotation = np.linalg.svd(np.linalg.inv(C) / 3.0)
    return 1.0 / np.sqrt(s), rotation


def worst_norm(P, centre, radii, rotation):
    """max over the points of (p - c)^T A (p - c), A = rotation^T diag(1 / radii^2) rotation: 1 on the ellipsoid's surface."""
    local = (np.asarray(P, np.float64) - centre) @ rotation.T / radii
    return float((local * local).sum(1).max())


def axis_gap(a, b):
    return float(np.max(1.0 - np.abs(np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64), axis=-1))))
