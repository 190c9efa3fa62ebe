#!/usr/bin/env python3
"""Per-instance 3-D boxes of a labelled point cloud (the step the reference keeps in inference/visualize_bboxes.py: filter_pointcloud
:52-74 + get_tight_bbox :78-131).

    python inference/fit_bboxes.py --pointcloud runs/<...>/pointcloud.pkl [--method pca|simple|ellipsoid] [--backend device|sklearn]
                                   [--tolerance 0.01] [--max_points 50000] [--seed 0] [--out <pkl>]

``--method ellipsoid`` (the reference's default) fits the minimum-volume enclosing ellipsoid of every instance by Khachiyan's algorithm
(``--tolerance``: its stopping threshold) and writes the box that circumscribes it.

Reads ``pointcloud.pkl`` (``{"points": (P, 3), "instances": (P,)}``, written by ``render_panopli.py --save_pointcloud``) and writes
``bboxes.pkl`` beside it: ``{instance_id: {"bbox": (min, max), "orientation": 3x3, "position": 3}}``, the file the reference's
``visualize_bboxes.py --bboxes`` loads.  Prints one line per instance and the seconds spent in filter + fit.
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import points3d                            # noqa: E402


def load_pointcloud(path):
    with open(path, "rb") as f:
        data = pickle.load(f)
    points = data["points"]
    if isinstance(points, list):                                     # visualize_bboxes.py:273-274
        points = torch.cat(points, dim=0).cpu().numpy()
    return np.ascontiguousarray(np.asarray(points), dtype=np.float32), np.asarray(data["instances"]).reshape(-1).astype(np.int64)


def fit_bboxes(pointcloud, method="pca", backend="device", max_points=50000, seed=0, out=None, tolerance=0.01):
    points, instances = load_pointcloud(pointcloud)
    out = out or os.path.join(os.path.dirname(os.path.abspath(pointcloud)), "bboxes.pkl")
    gen = torch.Generator().manual_seed(int(seed))
    if backend == "device":
        from contrastive_lift_amd import _lib
        _lib.load()
        points_in, labels_in = torch.from_numpy(points).cuda(), torch.from_numpy(instances).cuda()
        torch.cuda.synchronize()
    else:
        points_in, labels_in = points, instances
    t0 = time.perf_counter()
    if method == "ellipsoid":
        boxes, info = points3d.fit_instance_ellipsoids(points_in, labels_in, tolerance=tolerance, max_points=max_points, generator=gen,
                                                       backend=backend, return_info=True)
    else:
        boxes, info = points3d.fit_instance_boxes(points_in, labels_in, method=method, max_points=max_points, generator=gen, backend=backend,
                                                  return_info=True)
    if backend == "device":
        torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    for inst in sorted(info["total"]):
        if inst in boxes:
            ext = boxes[inst]["bbox"][1] - boxes[inst]["bbox"][0]
            more = ""
            if method == "ellipsoid":
                more = f", {info['iters'][inst]} iterations" + (" (not converged)" if inst in info["not_converged"] else "")
            print(f"instance {inst}: kept {info['kept'][inst]} / {info['total'][inst]} points, extent {ext[0]:.4f} x {ext[1]:.4f} x {ext[2]:.4f}{more}")
        else:
            print(f"instance {inst}: kept {info['kept'][inst]} / {info['total'][inst]} points, no box")
    with open(out, "wb") as f:
        pickle.dump(boxes, f)
    print(f"{len(boxes)} boxes ({method}, backend {backend}) from {points.shape[0]} points: filter + fit {seconds:.3f} s -> {out}")
    return out, seconds


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pointcloud", type=str, required=True, help="pointcloud.pkl with points (P, 3) and instances (P,), 0 = stuff")
    ap.add_argument("--method", choices=points3d.METHODS + ("ellipsoid",), default="pca")
    ap.add_argument("--tolerance", type=float, default=0.01, help="ellipsoid: Khachiyan's loop ends when the weights move by no more than this")
    ap.add_argument("--backend", choices=points3d.BACKENDS, default="device",
                    help="device: all instances at once on the GPU; sklearn: the reference's per-instance KD-tree on the host")
    ap.add_argument("--max_points", type=int, default=50000, help="larger instances are subsampled first (reference: 50000)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the subsample's generator")
    ap.add_argument("--out", type=str, default=None, help="default: bboxes.pkl beside the point cloud")
    a = ap.parse_args()
    fit_bboxes(a.pointcloud, a.method, a.backend, a.max_points, a.seed, a.out, a.tolerance)
