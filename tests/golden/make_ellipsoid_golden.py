#!/usr/bin/env python3
"""Generate golden G26 (minimum-volume enclosing ellipsoids) by running the REFERENCE's own functions (build container only, CPU).

    CL_REFERENCE=<reference checkout> python tests/golden/make_ellipsoid_golden.py        # read-only, never copied

Input: the cloud of golden G24 (g24_points3d.npz: points, labels, keep_fp64), read from there -- no second copy of the points is stored.

Recorded from inference/visualize_bboxes.py, per fitted instance: centre, radii and rotation of ``getMinVolEllipse`` (:135-189) on the
instance's kept rows (the fp64-statistics keep set of G24, float32 rows as ``get_tight_bbox`` passes them), the number of iterations of its
Khachiyan loop and the row it picks in every iteration (``np.argmax`` is wrapped inside the imported module while it runs; rows are counted
among the instance's kept rows in input order), the reference's own worst (p - c)^T A (p - c) over those rows (about 1.05 at its tolerance
0.01: its ellipsoid does not strictly enclose), and ``get_tight_bbox(points, labels, method="ellipsoid")`` for all instances at once.

The same quantities come from a plain numpy restatement written here that needs O(N) work and memory per iteration (a 4 x 4 moment matrix,
its inverse, one quadratic form per row, an argmax) where the reference forms ``np.diag(u)`` and ``QT V^-1 Q``, N x N each; the differences
of the two are stored.  The generator ASSERTS: get_tight_bbox gives the numbers of getMinVolEllipse on the fp64 keep set (the keep sets are
identical on G24); the restatement picks the identical rows; and in every iteration of every instance the largest M exceeds the
second-largest DISTINCT M by more than 1e-9 of itself, so rounding cannot change the path.  A failure is a fixture problem: take another
cloud, not a wider tolerance.

Tolerances written to the json: max(10 x reference-vs-restatement difference, 1e-9 x cloud diameter) for centre and radii,
max(10 x difference, 1e-9) for 1 - |<axis, axis_ref>| (axes compared up to sign).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CL_REFERENCE")
TOLERANCE = 0.01
MARGIN_FLOOR = 1e-9


class RecordingNumpy:
    """numpy with an argmax that remembers what it returned."""

    def __init__(self):
        self.picked = []

    def __getattr__(self, name):
        return getattr(np, name)

    def argmax(self, a, *args, **kw):
        j = np.argmax(a, *args, **kw)
        self.picked.append(int(j))
        return j


def restatement(P, tolerance=TOLERANCE):
    """Khachiyan's loop in O(N) per iteration.  Returns (centre, radii, rotation, picked rows, smallest argmax margin)."""
    P = P.astype(np.float64)
    N = P.shape[0]
    o = P.mean(0)                                                              # M is affine invariant; centring keeps V well conditioned
    Q = np.concatenate([P - o, np.ones((N, 1))], 1)
    u = np.full(N, 1.0 / N)
    err, picked, margin = 1.0 + tolerance, [], np.inf
    while err > tolerance:
        V = (Q * u[:, None]).T @ Q
        M = np.einsum("ij,jk,ik->i", Q, np.linalg.inv(V), Q)
        j = int(np.argmax(M))
        others = M[M != M[j]]
        margin = min(margin, float((M[j] - others.max()) / M[j]))
        step = (M[j] - 4.0) / (4.0 * (M[j] - 1.0))
        new_u = (1.0 - step) * u
        new_u[j] += step
        err = np.linalg.norm(new_u - u)
        u = new_u
        picked.append(j)
    c = u @ Q[:, :3]
    C = (Q[:, :3] * u[:, None]).T @ Q[:, :3] - np.outer(c, c)
    _, s, rotation = np.linalg.svd(np.linalg.inv(C) / 3.0)
    return o + c, 1.0 / np.sqrt(s), rotation, picked, margin


def worst_norm(P, centre, radii, rotation):
    local = (P.astype(np.float64) - centre) @ rotation.T / radii
    return float((local * local).sum(1).max())


def axis_gap(a, b):
    return float(np.max(1.0 - np.abs(np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64), axis=-1))))


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set CL_REFERENCE to a checkout of the reference (yashbhalgat/Contrastive-Lift)")
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    from inference import visualize_bboxes as vb                               # the reference, imported only when this script runs
    g = np.load(os.path.join(HERE, "g24_points3d.npz"))
    g24 = json.load(open(os.path.join(HERE, "g24_points3d.json")))
    pts, lab, keep = g["points"], g["labels"], g["keep_fp64"]
    assert all(n == 0 for n in g24["differing_points"].values()), "the reference's float32 filter and the fp64 filter must agree on this cloud"
    ids = [int(i) for i in g["pca.ids"]]
    feed = ~np.isin(lab, g24["skipped"])
    boxes = vb.get_tight_bbox(pts[feed], lab[feed], method="ellipsoid")
    assert sorted(boxes) == ids
    out = {k: [] for k in ("centre", "radii", "rotation", "iters", "kept", "worst_norm", "bbox.position", "bbox.radii", "bbox.orientation",
                           "restated.centre", "restated.radii", "restated.rotation", "restated.worst_norm", "margin")}
    picked_all, d_centre, d_radii, d_axis, d_bbox = [], 0.0, 0.0, 0.0, 0.0
    real_np = vb.np
    for i in ids:
        S = pts[(lab == i) & keep]
        rec = RecordingNumpy()
        vb.np = rec
        try:
            centre, radii, rotation = vb.getMinVolEllipse(S)
        finally:
            vb.np = real_np
        c2, r2, R2, picked, margin = restatement(S)
        assert picked == rec.picked, (i, "the restatement takes another path than the reference")
        assert margin > MARGIN_FLOOR, (i, margin, "an argmax is decided by rounding on this cloud")
        b = boxes[i]
        d_bbox = max(d_bbox, float(np.abs(np.asarray(b["position"]) - centre).max()), float(np.abs(np.asarray(b["bbox"][1]) - radii).max()),
                     float(np.abs(np.asarray(b["orientation"]) - rotation).max()))
        assert np.allclose(-np.asarray(b["bbox"][0]), np.asarray(b["bbox"][1]), rtol=0, atol=0)
        d_centre = max(d_centre, float(np.abs(c2 - centre).max()))
        d_radii = max(d_radii, float(np.abs(r2 - radii).max()))
        d_axis = max(d_axis, axis_gap(R2, rotation))
        for key, v in (("centre", centre), ("radii", radii), ("rotation", rotation), ("iters", len(rec.picked)), ("kept", S.shape[0]),
                       ("worst_norm", worst_norm(S, centre, radii, rotation)), ("bbox.position", b["position"]), ("bbox.radii", b["bbox"][1]),
                       ("bbox.orientation", b["orientation"]), ("restated.centre", c2), ("restated.radii", r2), ("restated.rotation", R2),
                       ("restated.worst_norm", worst_norm(S, c2, r2, R2)), ("margin", margin)):
            out[key].append(np.asarray(v, np.float64))
        picked_all.append(np.asarray(rec.picked, np.int32))
        print(f"instance {i}: {S.shape[0]} kept rows, {len(rec.picked)} iterations, margin {margin:.3e}, worst norm {out['worst_norm'][-1]:.6f}")
    # the keep sets are identical, so get_tight_bbox ran getMinVolEllipse on the same rows: the same numbers (BLAS may still split a sum otherwise
    # for another call, hence not bit equality)
    assert d_bbox <= 1e-12, d_bbox
    arrays = {k: np.stack(v) for k, v in out.items()}
    arrays["ids"] = np.asarray(ids, np.int32)
    arrays["iters"] = arrays["iters"].astype(np.int32)
    arrays["kept"] = arrays["kept"].astype(np.int32)
    arrays["picked"] = np.concatenate(picked_all)
    arrays["picked_off"] = np.concatenate([[0], np.cumsum([len(p) for p in picked_all])]).astype(np.int32)
    diam = float(g24["diameter"])
    rec = {"source": "g24_points3d.npz (points, labels, keep_fp64)", "tolerance": TOLERANCE, "diameter": diam, "ids": ids,
           "iters": {str(i): int(n) for i, n in zip(ids, arrays["iters"])}, "kept": {str(i): int(n) for i, n in zip(ids, arrays["kept"])},
           "worst_norm": {str(i): float(x) for i, x in zip(ids, arrays["worst_norm"])},
           "margin": {str(i): float(x) for i, x in zip(ids, arrays["margin"])}, "margin_floor": MARGIN_FLOOR,
           "bbox_vs_ellipse": d_bbox, "same_path": True,
           "ref_vs_restated": {"centre": d_centre, "radii": d_radii, "axis": d_axis},
           "tol": {"centre": max(10 * d_centre, 1e-9 * diam), "radii": max(10 * d_radii, 1e-9 * diam), "axis": max(10 * d_axis, 1e-9)}}
    np.savez_compressed(os.path.join(HERE, "g26_ellipsoid.npz"), **arrays)
    with open(os.path.join(HERE, "g26_ellipsoid.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
