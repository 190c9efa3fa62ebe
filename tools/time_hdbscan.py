#!/usr/bin/env python3
"""Time the HDBSCAN fit of the --use_dbscan branch on the G17 50 000-point subsample (the point set of tests/test_gpu_meanshift.py):
sklearn.cluster.HDBSCAN on the CPU against DeviceHDBSCAN (clift_emst on the GPU + the host tree pass), and a 19-value ``relabel`` sweep.

    python tools/time_hdbscan.py [--min_cluster_size 500] [--out profiles/hdbscan_timing.txt] [--skip_sklearn]

Kernel time: hipEvents around clift_emst alone (points and buffers already on the device), one warm-up call, then the median of 5.
Host times are wall clock, single runs.  Asserts nothing but equal labels; the numbers are recorded, not gated."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from contrastive_lift_amd import _lib                                  # noqa: E402
from contrastive_lift_amd import hdbscan as hd                         # noqa: E402


def g17_subsample(n=50000):
    """cluster()'s preprocessing of the G17 features: 3-sigma filter, rescale to the unit box, ``n`` rows drawn with the global generator."""
    from make_fake_predictions import fake_thing_features
    feats, _ = fake_thing_features(171)
    f = feats[feats[:, 0] == -np.inf][:, 1:]
    mu, sd = f.mean(0), f.std(0)
    cf = f[np.all(np.abs(f - mu) < 3 * sd, 1)]
    bias, factor = cf.min(0), 1 / (cf.max(0) - cf.min(0))
    cr = (cf - bias) * factor
    np.random.seed(1234)
    return np.ascontiguousarray(cr[np.random.choice(cr.shape[0], n, replace=False)], dtype=np.float32)


def kernel_ms(X, repeats=5):
    """Median of ``repeats`` event-bracketed clift_emst calls after one warm-up; also the rounds of the last call."""
    x = torch.as_tensor(X, device="cuda")
    n, d = x.shape
    a = torch.empty((n - 1,), dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    w = torch.empty((n - 1,), dtype=torch.float64, device="cuda")
    info = torch.zeros((4,), dtype=torch.int32, device="cuda")
    nbytes = int(_lib.load().clift_emst_work_bytes(n))
    work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device="cuda")
    times = []
    for it in range(repeats + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.call("clift_emst", _lib.ptr(x), n, x.stride(0), d, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), _lib.ptr(info), _lib.ptr(work), nbytes,
                  _lib.stream())
        t1.record()
        torch.cuda.synchronize()
        if it:
            times.append(t0.elapsed_time(t1))
    return statistics.median(times), times, info.cpu().numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_cluster_size", type=int, default=500)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--skip_sklearn", action="store_true")
    args = ap.parse_args()
    X = g17_subsample(args.points)
    lines = [f"point set: G17 subsample, n = {X.shape[0]}, d = {X.shape[1]}, min_cluster_size = {args.min_cluster_size}, "
             f"{torch.cuda.get_device_name(0)}"]
    med, times, info = kernel_ms(X)
    lines.append(f"clift_emst kernel time: median {med:.2f} ms of {['%.2f' % t for t in times]} after one warm-up; rounds {int(info[0])}, "
                 f"components left {int(info[1])}, fault {int(info[2])}")
    t0 = time.perf_counter()
    dev = hd.DeviceHDBSCAN(args.min_cluster_size, device="cuda").fit(X)
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    link = hd.single_linkage(X.shape[0], *dev.mst_)
    t_link = time.perf_counter() - t0
    t0 = time.perf_counter()
    hd.tree_labels(X.shape[0], link, args.min_cluster_size, True)
    t_tree = time.perf_counter() - t0
    lines.append(f"DeviceHDBSCAN.fit wall: {t_fit:.3f} s  (host stage alone: orient + single linkage {t_link:.3f} s, condensed tree + labels "
                 f"{t_tree:.3f} s; the rest is the kernel, allocation and copies); clusters {int(dev.labels_.max()) + 1}, "
                 f"noise {float((dev.labels_ == -1).mean()):.3f}")
    sweep = list(range(10, 200, 10))
    t0 = time.perf_counter()
    ks = [int(dev.relabel(m).labels_.max()) + 1 for m in sweep]
    t_sweep = time.perf_counter() - t0
    lines.append(f"relabel sweep, {len(sweep)} values of min_cluster_size (10..190): {t_sweep:.3f} s, clusters {ks}")
    if not args.skip_sklearn:
        from sklearn.cluster import HDBSCAN
        t0 = time.perf_counter()
        ref = HDBSCAN(min_cluster_size=args.min_cluster_size, min_samples=1, allow_single_cluster=True, copy=True).fit(X)
        t_ref = time.perf_counter() - t0
        dev.relabel(args.min_cluster_size)
        same = bool(np.array_equal(ref.labels_, dev.labels_))
        lines.append(f"sklearn.cluster.HDBSCAN.fit wall: {t_ref:.3f} s = {t_ref / t_fit:.1f} x the device fit; labels equal: {same}, "
                     f"max |probability difference| {float(np.abs(ref.probabilities_ - dev.probabilities_).max()):.3g}")
        assert same, "device labels differ from sklearn's"
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
