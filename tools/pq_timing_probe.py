#!/usr/bin/env python3
"""Cost of scoring panoptic quality: the host path (np.unique / np.add.at per frame) against the device path (clift_label_overlap, two
launches per call) of metrics.panoptic_quality_per_frame and metrics.panoptic_quality.

    python tools/pq_timing_probe.py [--frames 200] [--out profiles/pq_device_timing.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/pq_timing_probe.py --device-only --reps 1
    python tools/pq_timing_probe.py --kernel-stats <dir> --out profiles/pq_device_timing.txt      # appends the kernels' own times

Labels: the project's generators -- a synthetic MOS scene (tools/make_synthetic_mos.py) and the prediction folders
tools/make_fake_predictions.py writes for it (ground truth with 8 % of the pixels re-labelled, instance ids permuted).  Two shapes: the
bandwidth sweep's (``--frames`` frames of 256 x 384 scored frame by frame against the per-view pseudo-labels, one sweep value) and scene
level (all frames concatenated, one match against the scene-consistent ground truth), and between them one validation view (one frame: a
PQ match plus a confusion matrix, labels starting on the GPU as in HotPathTrainer.validation_step).  "device" is timed twice: from host arrays (upload
included) and from tensors already on the GPU, which is where a sweep's rendered labels are.  Every row is the median of
``--reps`` runs after one warm-up run, and every count / device result is compared with the host result for equality.
"""
import argparse
import glob
import csv
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

IS_THING = [False, True]          # the MOS layout: class 0 stuff, class 1 thing


def make_frames(F, H, W, seed=5):
    """Label images from the project's own generators: a synthetic MOS scene (tools/make_synthetic_mos.make_scene, rendered square at
    max(H, W) and cropped to H x W) and the prediction folders tools/make_fake_predictions.write_fake_predictions writes for it, read back.
    Returns int32 arrays (F, H, W): pred semantics, pred surrogate ids, the per-view pseudo-labels (detic_*: what the sweep scores against)
    and the scene-consistent ground truth (semantic / instance: what evaluate.py scores against)."""
    import tempfile
    from PIL import Image
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_mos as gen
    from make_fake_predictions import write_fake_predictions
    size = max(H, W)
    r0, c0 = (size - H) // 2, (size - W) // 2
    with tempfile.TemporaryDirectory() as tmp:
        root = gen.make_scene(os.path.join(tmp, "scene"), n_frames=F, size=size, seed=seed)
        names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(root, "semantic")))
        rd = lambda d: [np.load(os.path.join(root, d, n + ".npy")) for n in names]
        sem, inst = rd("semantic"), rd("instance")
        write_fake_predictions(os.path.join(tmp, "exp"), names, sem, inst, np.random.default_rng(seed + 1))
        png = lambda d: [np.array(Image.open(os.path.join(tmp, "exp", d, n + ".png"))) for n in names]
        sets = [png("pred_semantics"), png("pred_surrogateid"), rd("detic_semantic"), rd("detic_instance"), sem, inst]
    return [np.stack(x)[:, r0:r0 + H, c0:c0 + W].astype(np.int32) for x in sets]


def timed(fn, reps, sync=None):
    """Result and median seconds of ``reps`` runs after one warm-up run -- every row of the table is taken this way."""
    fn()
    ts = []
    for _ in range(reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        r = fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts))


def run(a):
    import torch
    from contrastive_lift_amd.metrics import panoptic_quality, panoptic_quality_per_frame
    if a.cache and os.path.exists(a.cache):
        sets = [x for x in np.load(a.cache)["sets"]]
    else:
        sets = make_frames(a.frames, a.height, a.width)
        if a.cache:
            np.savez_compressed(a.cache, sets=np.stack(sets))
    stacked, scene_t = sets[:4], sets[4:]
    F = stacked[0].shape[0]
    names = [f"{i}.png" for i in range(F)]
    dicts = [{n: x[i] for i, n in enumerate(names)} for x in stacked]
    segs = np.mean([len(np.unique(stacked[2][i].astype(np.int64) * 65536 + stacked[3][i])) for i in range(F)])
    psegs = np.mean([len(np.unique(stacked[0][i].astype(np.int64) * 65536 + stacked[1][i])) for i in range(F)])
    lines = [f"# {F} frames of {a.height} x {a.width} (synthetic MOS scene + fake predictions): {segs:.1f} target and {psegs:.1f} predicted (class, id) "
             f"segments per frame on average; seconds = median of {a.reps} runs after one warm-up run, wall clock with a device synchronise",
             "shape backend seconds equal_to_host"]
    sync = torch.cuda.synchronize
    dev = [torch.from_numpy(x).cuda() for x in stacked]
    # ---- the sweep's shape: per-frame PQ of all frames, one sweep value
    host = None
    if not a.device_only:
        host, t = timed(lambda: panoptic_quality_per_frame(*dicts, IS_THING, ()), a.reps)
        lines.append(f"per_frame host {t:.4f} -")
        r, t = timed(lambda: panoptic_quality_per_frame(*stacked, IS_THING, (), backend="counts"), a.reps)
        lines.append(f"per_frame counts {t:.4f} {r == host}")
    r, t = timed(lambda: panoptic_quality_per_frame(*stacked, IS_THING, (), backend="device"), a.reps, sync)
    lines.append(f"per_frame device_from_host_arrays {t:.4f} {'-' if host is None else r == host}")
    r, t = timed(lambda: panoptic_quality_per_frame(*dev, IS_THING, (), backend="device"), a.reps, sync)
    lines.append(f"per_frame device_resident {t:.4f} {'-' if host is None else r == host}")
    # ---- one validation view: what HotPathTrainer.validation_step scores per view -- one PQ match and one confusion matrix of H * W pixels
    from contrastive_lift_amd.inference import ConfusionMatrix
    v = lambda x: x[0].reshape(-1).astype(np.int64)
    vp, vq = np.stack([v(stacked[0]), v(stacked[1])], -1), np.stack([v(stacked[2]), v(stacked[3])], -1)
    vpd, vqd = torch.from_numpy(vp).cuda(), torch.from_numpy(vq).cuda()

    def view(p_, q_, backend):
        iou = ConfusionMatrix(2, ignore_class=[0], backend=backend).add_batch(q_[:, 0] if backend != "host" else q_[:, 0].cpu().numpy(),
                                                                               p_[:, 0] if backend != "host" else p_[:, 0].cpu().numpy(), return_miou=True)
        return (float(iou),) + tuple(float(x) for x in panoptic_quality(p_, q_, {1}, {0}, True, backend=backend))
    host = None
    if not a.device_only:
        host, t = timed(lambda: view(vpd, vqd, "host"), a.reps, sync)                  # (labels start on the device, as in validation_step)
        lines.append(f"view host {t:.4f} -")
    r, t = timed(lambda: view(vpd, vqd, "device"), a.reps, sync)
    lines.append(f"view device_resident {t:.4f} {'-' if host is None else r == host}")
    # ---- scene level: all frames concatenated, one match against the scene-consistent ground truth
    p = np.stack([stacked[0].reshape(-1), stacked[1].reshape(-1)], -1).astype(np.int64)
    q = np.stack([scene_t[0].reshape(-1), scene_t[1].reshape(-1)], -1).astype(np.int64)
    things, stuff = {1}, {0}
    host = None
    if not a.device_only:
        host, t = timed(lambda: tuple(float(x) for x in panoptic_quality(p, q, things, stuff, True)), a.reps)
        lines.append(f"scene host {t:.4f} -")
    pd, qd = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    r, t = timed(lambda: tuple(float(x) for x in panoptic_quality(p, q, things, stuff, True, backend="device")), a.reps, sync)
    lines.append(f"scene device_from_host_arrays {t:.4f} {'-' if host is None else r == host}")
    r, t = timed(lambda: tuple(float(x) for x in panoptic_quality(pd, qd, things, stuff, True, backend="device")), a.reps, sync)
    lines.append(f"scene device_resident {t:.4f} {'-' if host is None else r == host}")
    return lines


def kernel_stats(d):
    """The k_label_overlap rows of rocprofv3's kernel_stats.csv files under ``d``."""
    lines = ["# kernel times (rocprofv3 --kernel-trace --stats of a --device-only --reps 1 run: 4 scorings per shape, 2 launches each): name calls total_ns average_ns"]
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            if "k_label_overlap" in row.get("Name", ""):
                lines.append(f"{row['Name']} {row.get('Calls')} {row.get('TotalDurationNs')} {row.get('AverageNs')}")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--cache", help="npz of the generated label images: written when missing, read when present")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="skip the host rows (for a run under the profiler)")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run: append the kernel rows instead of timing")
    ap.add_argument("--out", help="append the table to this file (default: print only)")
    a = ap.parse_args()
    lines = kernel_stats(a.kernel_stats) if a.kernel_stats else run(a)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
