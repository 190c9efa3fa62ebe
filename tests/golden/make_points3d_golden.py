#!/usr/bin/env python3
"""Generate golden G24 (instances in 3-D) by running the REFERENCE's own functions (build container only, CPU).

    CL_REFERENCE=<reference checkout> python tests/golden/make_points3d_golden.py        # read-only, never copied

Input: a seeded synthetic labelled cloud, float32, ~20 k points: label 0 (stuff) present; 12 instances from 6 000 down to 9 points with
non-contiguous ids; anisotropic Gaussian blobs (std ratio 2 between successive axes, so the PCA axes are well defined) rotated off the
world axes; 5 % uniform outliers per instance; one instance with exact duplicate points (k-th distance 0 for those); one instance with
exactly k - 1 = 9 points (the reference raises there: recorded as skipped) and one with exactly k = 10.  Rows are shuffled.

Recorded from inference/visualize_bboxes.py: per instance the 10-NN distance column of its KD-tree query (:59-63) and the stage-1 set of
:65, the surviving rows of ``filter_pointcloud`` (turned into a keep set by matching rows -- exact duplicates share their distances and
their fate) and ``get_tight_bbox(..., "simple")`` / ``(..., "pca")``.  The reference takes mean / std of a float32 array in float32; the
generator recomputes keep set and boxes with fp64 statistics (plain numpy, written here, independent of the port) and stores how many
points differ per instance and the largest difference of any box number: the tests' tolerances are 10x those differences (floor 1e-6 of the
cloud's diameter), and the generator asserts that the differing points stay within max(2, 0.1 % of the instance) for the chosen seed.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CL_REFERENCE")
K = 10
SIZES = {3: 6000, 5: 4000, 7: 3000, 8: 2000, 12: 1500, 13: 1000, 17: 600, 21: 300, 22: 150, 30: 40, 31: K, 40: K - 1}
DUPLICATES_IN = 17
N_STUFF = 1500


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_cloud(seed):
    rng = np.random.default_rng(seed)
    pts, lab = [rng.uniform(-3.0, 3.0, (N_STUFF, 3))], [np.zeros(N_STUFF, np.int32)]
    for inst, n in SIZES.items():
        centre = rng.uniform(-2.0, 2.0, 3)
        s0 = rng.uniform(0.2, 0.4)
        std = np.array([s0, s0 / 2, s0 / 4])
        R = random_rotation(rng)
        n_out = int(round(0.05 * n)) if n >= 20 else 0
        core = (rng.standard_normal((n - n_out, 3)) * std) @ R.T + centre
        if inst == DUPLICATES_IN:
            core[:240] = np.repeat(core[:20], 12, axis=0)
        out = centre + rng.uniform(-6 * s0, 6 * s0, (n_out, 3))
        pts.append(np.concatenate([core, out]))
        lab.append(np.full(n, inst, np.int32))
    pts, lab = np.concatenate(pts).astype(np.float32), np.concatenate(lab)
    perm = rng.permutation(pts.shape[0])
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(lab[perm])


def rows_in(rows, kept):
    have = {r.tobytes() for r in kept}
    return np.array([r.tobytes() in have for r in rows], bool)


def fp64_filter(P, d):
    """The reference's two stages with fp64 statistics."""
    k1 = d < np.percentile(d, 70)
    S = P[k1].astype(np.float64)
    keep = np.zeros(P.shape[0], bool)
    keep[k1] = np.all(np.abs(S - S.mean(0)) < 3 * S.std(0), axis=-1)
    return keep


def fp64_box(S, method):
    S = S.astype(np.float64)
    mean = S.mean(0)
    q = S - mean
    axes = np.eye(3)
    if method == "pca":
        w, v = np.linalg.eigh(q.T @ q / S.shape[0])
        axes = v.T[::-1]
    proj = q @ axes.T
    return proj.min(0), proj.max(0), axes, mean


def axis_gap(a, b):
    return float(np.max(1.0 - np.abs(np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64), axis=-1))))


def build(seed, vb):
    from sklearn.neighbors import KDTree
    pts, lab = make_cloud(seed)
    P = pts.shape[0]
    kth = np.full(P, np.inf)
    stage1, keep_ref, keep64 = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool)
    skipped, differ = [], {}
    for inst in sorted(SIZES):
        rows = np.nonzero(lab == inst)[0]
        ip = pts[rows]
        assert ip.shape[0] <= 50000                                            # the reference's unseeded subsample branch is never taken
        try:
            kept = vb.filter_pointcloud(ip)
        except ValueError:
            skipped.append(inst)
            continue
        d = KDTree(ip).query(ip, k=K)[0][..., -1]                              # visualize_bboxes.py:59-63
        kth[rows] = d
        stage1[rows] = d < np.percentile(d, 70)                               # :65
        keep_ref[rows] = rows_in(ip, kept)
        assert int(keep_ref[rows].sum()) == kept.shape[0], (inst, int(keep_ref[rows].sum()), kept.shape[0])
        keep64[rows] = fp64_filter(ip, d)
        differ[inst] = int((keep_ref[rows] != keep64[rows]).sum())
    assert skipped == [40], skipped
    feed = ~np.isin(lab, skipped)
    out = {"points": pts, "labels": lab, "kth_dist": kth, "stage1": stage1, "keep_ref": keep_ref, "keep_fp64": keep64,
           "skipped": np.array(skipped, np.int32)}
    diam = float(np.linalg.norm(pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)))
    rec = {"seed": seed, "k": K, "diameter": diam, "differing_points": {str(i): n for i, n in differ.items()},
           "sizes": {str(i): n for i, n in SIZES.items()}, "skipped": skipped}
    for method in ("simple", "pca"):
        boxes = vb.get_tight_bbox(pts[feed], lab[feed], method=method)
        ids = sorted(boxes)
        assert ids == [i for i in sorted(SIZES) if i not in skipped]
        out[f"{method}.ids"] = np.array(ids, np.int32)
        out[f"{method}.bbox"] = np.array([[np.asarray(boxes[i]["bbox"][0]), np.asarray(boxes[i]["bbox"][1])] for i in ids], np.float64)
        out[f"{method}.orientation"] = np.array([boxes[i]["orientation"] for i in ids], np.float64)
        out[f"{method}.position"] = np.array([boxes[i]["position"] for i in ids], np.float64)
        d_centre = d_extent = d_axis = 0.0
        for j, i in enumerate(ids):
            mn, mx, axes, mean = fp64_box(pts[(lab == i) & keep64], method)
            d_centre = max(d_centre, float(np.abs(mean - out[f"{method}.position"][j]).max()))
            if method == "pca":                                                # extents up to the sign of each axis
                flip = np.sum(axes * out["pca.orientation"][j], -1) < 0
                mn, mx = np.where(flip, -mx, mn), np.where(flip, -mn, mx)
                d_axis = max(d_axis, axis_gap(axes, out["pca.orientation"][j]))
            d_extent = max(d_extent, float(np.abs(np.stack([mn, mx]) - out[f"{method}.bbox"][j]).max()))
        floor = 1e-6 * diam
        rec[method] = {"ref_vs_fp64": {"centre": d_centre, "extent": d_extent, "axis": d_axis},
                       "tol": {"centre": max(10 * d_centre, floor), "extent": max(10 * d_extent, floor), "axis": max(10 * d_axis, 1e-6)}}
    cap_ok = all(n <= max(2, int(0.001 * SIZES[i])) for i, n in differ.items())
    return out, rec, cap_ok


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set CL_REFERENCE to a checkout of the reference (yashbhalgat/Contrastive-Lift)")
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    from inference import visualize_bboxes as vb                               # the reference, imported only when this script runs
    for seed in range(24, 64):
        out, rec, cap_ok = build(seed, vb)
        if cap_ok:
            break
        print(f"seed {seed}: reference-vs-fp64 keep sets differ beyond the cap ({rec['differing_points']}), trying the next seed")
    else:
        raise SystemExit("no seed within the cap")
    np.savez_compressed(os.path.join(HERE, "g24_points3d.npz"), **out)
    with open(os.path.join(HERE, "g24_points3d.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
    print("points", out["points"].shape, "kept by the reference", int(out["keep_ref"].sum()))


if __name__ == "__main__":
    main()
