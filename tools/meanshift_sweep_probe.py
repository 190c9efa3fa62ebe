#!/usr/bin/env python3
"""Per-bandwidth cost of the MeanShift fit, sklearn (CPU, single process) against DeviceMeanShift (clift_meanshift on the GPU).

    rocprofv3 --kernel-trace --stats -d <dir> -o ms -- python tools/meanshift_sweep_probe.py [--n12] > table.txt
    python tools/meanshift_sweep_probe.py --trace <dir>/.../ms_results.db table.txt           # adds the kernel times per fit
    python tools/meanshift_sweep_probe.py --find-bandwidth                                 # one full inference/find_bandwidth.py run, both ways

Data: the 50 000-point G17 subsample (3-D, tools/make_fake_predictions.fake_thing_features(171), rescaled as cluster() does) over the
MOS sweep values sqrt(3)/3.5 * k/50 (the first 12 with --n12, else all of them), and a 25-D set (five Gaussian blobs, 20 000 points, ``blobs25``;
the width of config/template/panopli_paper.yaml) over sqrt(25)/3.5 * k/25, k = 1..8.  One clift_meanshift dispatch per device fit, in
the order of the printed rows, so the i-th k_meanshift row of the kernel trace belongs to the i-th row of the table.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def g17_points():
    from make_fake_predictions import fake_thing_features
    feats, _ = fake_thing_features(171)
    f = feats[feats[:, 0] == -np.inf][:, 1:]
    mu, sd = f.mean(0), f.std(0)
    cf = f[np.all(np.abs(f - mu) < 3 * sd, 1)]
    cr = (cf - cf.min(0)) / (cf.max(0) - cf.min(0))
    np.random.seed(1234)
    return cr[np.random.choice(cr.shape[0], 50000, replace=False)].astype(np.float32)


def blobs25():
    """Five blobs that spread over 3 of the 25 axes and sit within 0.002 of 0 on the other 22 (in 25-D a bin centre of generic data is
    ~1.4 bandwidths from its points and bin seeding finds nothing)."""
    rng = np.random.default_rng(25)
    cent = np.zeros((5, 25))
    cent[:, :3] = rng.uniform(0.1, 0.9, (5, 3))
    scale = np.r_[np.full(3, 0.08), np.full(22, 0.002)]
    return np.concatenate([c + scale * rng.standard_normal((4000, 25)) for c in cent]).astype(np.float32)


def run(n12):
    import torch
    from sklearn.cluster import MeanShift
    from contrastive_lift_amd.inference import DeviceMeanShift
    sets = [("g17_3d", g17_points(), [np.sqrt(3) / 3.5 * k / 50 for k in range(1, 13 if n12 else 50)]),
            ("blobs_25d", blobs25(), [np.sqrt(25) / 3.5 * k / 25 for k in range(1, 9)])]
    print("set bandwidth K_sklearn K_device sklearn_s device_wall_s n_iter")
    DeviceMeanShift(0.1, device="cuda").fit(sets[0][1][:2000])           # warm-up: context, module load (its dispatch is row -1)
    torch.cuda.synchronize()
    for name, X, bws in sets:
        for bw in bws:
            t0 = time.perf_counter()
            try:
                ref = MeanShift(bandwidth=bw, bin_seeding=True, min_bin_freq=10, cluster_all=False).fit(X)
                k_ref = ref.cluster_centers_.shape[0]
            except ValueError:
                k_ref = 0
            t1 = time.perf_counter()
            try:
                got = DeviceMeanShift(bw, device="cuda").fit(X)
                k_dev, it = got.cluster_centers_.shape[0], got.n_iter_
            except ValueError:
                k_dev, it = 0, -1
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(f"{name} {bw:.5f} {k_ref} {k_dev} {t1 - t0:.3f} {t2 - t1:.4f} {it}", flush=True)


def full_find_bandwidth():
    """Train the tiny synthetic MOS run of tests/test_gpu_end_to_end.py in a temporary directory, then run the whole bandwidth search (the
    reference's 50-value MOS sweep, --subsample 5 as the CLI default) with the sklearn and the device MeanShift; prints wall times and curves."""
    import importlib.util
    import tempfile
    import make_synthetic_mos as gen
    from contrastive_lift_amd.config import load_run_config

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    with tempfile.TemporaryDirectory() as tmp:
        scene = gen.make_scene(os.path.join(tmp, "data", "synth_scene"), n_frames=40, size=64, trajectory_frames=3)
        os.chdir(tmp)
        os.environ["experiment"] = "fb_probe"
        train = load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "probe_train")
        run_dir = train.main(["+experiment=contrastive_lift_MOS", f"dataset_root={scene}", "image_dim=64", "min_grid_dim=32", "max_grid_dim=64",
                              "max_epoch=6", "steps_per_epoch=400", "batch_size=2048", "chunk=0", "max_depth=3", "seed=3",
                              "max_rays_instances=512", "decay_step=[4,5]"])
        cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
        cfg.resume = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
        cfg.subsample_frames, cfg.image_dim = 5, [64, 64]
        fb = load(os.path.join(REPO, "inference", "find_bandwidth.py"), "probe_fb")
        for ms in ("sklearn", "device"):
            np.random.seed(0)
            t0 = time.perf_counter()
            res = fb.find_bandwidth(cfg, meanshift=ms)
            print(f"find_bandwidth --meanshift {ms}: {time.perf_counter() - t0:.2f} s for {len(res['values'])} values; best {res['best']:.5f} "
                  f"pq {res['best_pq']:.4f}")
            print("  curve", " ".join(f"{v:.4f}:{p:.4f}" for v, p in res["values"]))


def kernel_times_ms(trace):
    """k_meanshift dispatch durations (ms) in launch order, from a kernel-trace CSV or a rocprofv3 results database (.db)."""
    if trace.endswith(".db"):
        import sqlite3
        q = "select start, end from kernels where name like '%k_meanshift%' order by start"
        return [(e - s_) * 1e-6 for s_, e in sqlite3.connect(trace).execute(q).fetchall()]
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_meanshift" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]


def merge(trace, table):
    rows = kernel_times_ms(trace)[1:]                                     # (the warm-up fit)
    lines = [l.split() for l in open(table).read().splitlines() if l and not l.startswith(("set", "#"))]
    lines = [l for l in lines if len(l) == 7]
    print("set bandwidth K_sklearn K_device sklearn_s device_kernel_ms speedup n_iter")
    rows = iter(rows)
    for l in lines:
        if l[6] == "-1":                                                  # no seed: the fit raised before any dispatch
            print(f"{l[0]} {l[1]} {l[2]} {l[3]} {l[4]} - - {l[6]}")
            continue
        ms = next(rows)
        print(f"{l[0]} {l[1]} {l[2]} {l[3]} {l[4]} {ms:.3f} {float(l[4]) / (ms * 1e-3):.0f}x {l[6]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n12", action="store_true", help="only the first 12 MOS sweep values for the 3-D set")
    ap.add_argument("--find-bandwidth", action="store_true", help="one full find_bandwidth run on the synthetic MOS scene, both ways")
    ap.add_argument("--trace", nargs=2, metavar=("KERNEL_TRACE_CSV", "TABLE"), help="merge kernel times into a table written earlier")
    a = ap.parse_args()
    if a.trace:
        merge(*a.trace)
    elif a.find_bandwidth:
        full_find_bandwidth()
    else:
        run(a.n12)
