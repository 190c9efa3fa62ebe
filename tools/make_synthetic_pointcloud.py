#!/usr/bin/env python3
"""A seeded synthetic pointcloud.pkl for timing inference/fit_bboxes.py at scale: rotated anisotropic Gaussian blobs of unequal size with
5 % uniform outliers each, plus 10 % stuff (label 0), rows shuffled.

    python tools/make_synthetic_pointcloud.py --points 5900000 --instances 300 --seed 0 --out /tmp/cloud/pointcloud.pkl
"""
import argparse
import os
import pickle

import numpy as np


def make_pointcloud(n_points, n_instances, seed=0):
    rng = np.random.default_rng(seed)
    n_stuff = n_points // 10
    share = rng.uniform(0.2, 1.8, n_instances)
    sizes = np.maximum(20, (share / share.sum() * (n_points - n_stuff)).astype(np.int64))
    pts, lab = [rng.uniform(-4, 4, (n_stuff, 3)).astype(np.float32)], [np.zeros(n_stuff, np.uint16)]
    for g, n in enumerate(sizes.tolist()):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        s0 = rng.uniform(0.1, 0.3)
        n_out = n // 20
        core = (rng.standard_normal((n - n_out, 3)) * np.array([s0, s0 / 2, s0 / 4])) @ q.T
        p = np.concatenate([core, rng.uniform(-6 * s0, 6 * s0, (n_out, 3))]) + rng.uniform(-3, 3, 3)
        pts.append(p.astype(np.float32))
        lab.append(np.full(n, g + 1, np.uint16))
    pts, lab = np.concatenate(pts), np.concatenate(lab)
    perm = rng.permutation(pts.shape[0])
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(lab[perm])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5900000)
    ap.add_argument("--instances", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, required=True)
    a = ap.parse_args()
    points, instances = make_pointcloud(a.points, a.instances, a.seed)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "wb") as f:
        pickle.dump({"points": points, "instances": instances}, f)
    print(f"{a.out}: {points.shape[0]} points, {a.instances} instances, largest {int(np.bincount(instances)[1:].max())}")
