#!/usr/bin/env python3
"""Drop-in for reference inference/find_bandwidth.py (same flags; :34-244, CLI :376-400): pick the clustering bandwidth (or the HDBSCAN
min_cluster_size) of a trained scene by panoptic quality against the 2-D pseudo-labels of the training frames.

    python inference/find_bandwidth.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt [--segmentwise] [--use_dbscan]
                                       [--meanshift device|sklearn] [--hdbscan sklearn|device] [--sweep START STOP STEP] [--subsample 5] ...

As the reference: renders the ``train`` split, merges every thing class into the first thing class (the predicted semantics here, the
pseudo-label semantics in the scoring), sweeps sqrt(max_instances)/3.5 * (1..49)/50 for MOS scenes and (1..24)/25 otherwise (HDBSCAN:
10..190 step 10 for MOS, 250..2950 step 50 otherwise), clusters the rendered features with every value (``cluster`` or
``cluster_segmentwise``; a value whose clustering raises is skipped) and scores it with the per-frame PQ
(metrics.panoptic_quality_per_frame: MOS scenes against detic_semantic / detic_instance with is_thing = [False, True], PanopLi-layout
scenes against m2f_semantics / m2f_instance with the ``--things_csv`` list and class 0 void).  Ties go to the later value.
Writes ``runs/<experiment>/all_thing_features_train.npy``, ``bandwidth_vs_pq.png`` and ``bandwidth_vs_pq.json`` ((value, pq) pairs and
the best value).  The MeanShift fits run on the GPU (``--meanshift device``) unless ``--meanshift sklearn``; ``--sweep`` replaces the
reference's range (np.arange(START, STOP, STEP)).  With ``--use_dbscan`` the HDBSCAN fits (one per value, times the class count when
segmentwise) run in sklearn on the CPU unless ``--hdbscan device`` (DeviceHDBSCAN); the JSON records which under ``"hdbscan"``.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from contrastive_lift_amd import inference as inf                    # noqa: E402
from contrastive_lift_amd.config import load_run_config              # noqa: E402
from contrastive_lift_amd.data import get_scene                       # noqa: E402
from contrastive_lift_amd.metrics import panoptic_quality_per_frame   # noqa: E402
from extract_train_centroids import init_ranks, render_features, split_frames  # noqa: E402
from render_panopli import build_from_checkpoint                      # noqa: E402


def things_to_first_class_onehot(semantics, thing_classes):
    """modify_things_to_singleclass_onehot (:254-259): pixels predicted as a thing class become a one-hot of the first thing class."""
    thing = torch.isin(semantics.argmax(dim=1), torch.tensor(list(thing_classes), device=semantics.device))
    out = torch.zeros_like(semantics)
    out[~thing] = semantics[~thing]
    out[thing, thing_classes[0]] = 1
    return out


def sweep_range(max_instances, is_mos, use_dbscan):
    """:160-170."""
    if use_dbscan:
        return np.arange(10, 200, 10) if is_mos else np.arange(250, 3000, 50)
    r = np.sqrt(max_instances) / 3.5
    n = 50 if is_mos else 25
    return np.arange(r / n, r, r / n)


def _resize(img, H, W):
    """MY_read_and_resize_labels[_npy] (:269-287): NEAREST to (W, H) when the size differs."""
    im = Image.fromarray(img)
    if im.size != (W, H):
        im = im.resize((W, H), Image.NEAREST)
    return np.array(im)


def load_targets(root, names, is_mos, H, W):
    """load_all_target_images[_MOS] (:290-311): the pseudo-labels of the training frames among ``names`` (``<stem>.png``)."""
    root = Path(root)
    sem, inst = {}, {}
    if is_mos:
        stems = sorted([x.stem for x in (root / "detic_semantic").iterdir() if x.name.endswith(".npy")], key=lambda y: int(y) if y.isnumeric() else y)
        train = set(stems[:int(len(stems) * 0.8)])
        for n in names:
            s = Path(n).stem
            if s in train:
                sem[n] = _resize(np.load(root / "detic_semantic" / f"{s}.npy").astype(np.int16), H, W)
                inst[n] = _resize(np.load(root / "detic_instance" / f"{s}.npy").astype(np.int16), H, W)
    else:
        train = set(str(x) for x in json.loads((root / "splits.json").read_text())["train"])
        for n in names:
            if Path(n).stem in train:
                sem[n] = _resize(np.array(Image.open(root / "m2f_semantics" / n)), H, W)
                inst[n] = _resize(np.array(Image.open(root / "m2f_instance" / n)), H, W)
    return sem, inst


def read_is_thing(things_csv):
    rows = [line.split(",") for line in Path(things_csv).read_text().strip().splitlines()]
    return [False] + [bool(int(r[1])) for r in rows]                  # class 0 = void


def find_bandwidth(config, debug=False, segmentwise=False, use_dbscan=False, meanshift="device", sweep=None,
                   things_csv="resources/scannet_reduced_things.csv", device="cuda:0", hdbscan="sklearn"):
    out = Path("runs") / Path(config.experiment)
    out.mkdir(exist_ok=True, parents=True)
    rank, device = init_ranks(device)
    is_mos = config.dataset_class == "mos"
    scene = get_scene(config, "train", device)
    H, W = scene.image_dim
    model, renderer, _ = build_from_checkpoint(config, scene, device)
    renderer.update_step_ratio(renderer.step_ratio * 0.5)                                    # :89
    fg = list(scene.segmentation_data.fg_classes)
    names, _, sems, _, _, things = render_features(config, scene, model, renderer, split_frames(scene))
    if rank != 0:
        return None
    sems = [things_to_first_class_onehot(s, fg) for s in sems]
    all_thing = torch.cat(things, 0).cpu().numpy()
    np.save(out / "all_thing_features_train.npy", all_thing)
    names = [f"{n}.png" for n in names]
    sem_images = {n: s.argmax(dim=1).reshape(H, W).cpu().numpy().astype(np.uint8) for n, s in zip(names, sems)}
    tgt_sem, tgt_inst = load_targets(config.dataset_root, names, is_mos, H, W)
    is_thing, faulty = ([False, True], ()) if is_mos else (read_is_thing(things_csv), (0,))
    values = np.arange(*sweep) if sweep is not None else sweep_range(int(config.max_instances), is_mos, use_dbscan)
    best_pq, best_val, curve = 0.0, None, []
    for val in values:
        val = float(val) if not use_dbscan else int(val)
        try:
            kw = dict(bandwidth=0.15, cluster_size=val, use_dbscan=True, hdbscan=hdbscan) if use_dbscan else dict(bandwidth=val, meanshift=meanshift)
            if segmentwise:
                insts, _ = inf.cluster_segmentwise(all_thing, sems, device=device, num_images=len(names), **kw)
            else:
                insts, _ = inf.cluster(all_thing, device=device, num_images=len(names), **kw)
        except Exception as e:                                                           # :210-212
            print(f"Clustering failed for value {val}: {e}")
            continue
        inst_images = {n: insts[i].argmax(dim=1).reshape(H, W).cpu().numpy().astype(np.int32) for i, n in enumerate(names)}
        if debug:
            d = out / f"pred_surrogateid_bw_{val}"
            d.mkdir(exist_ok=True)
            for n, im in inst_images.items():
                Image.fromarray(im.astype(np.uint16)).save(d / n)
        pq, _, _ = panoptic_quality_per_frame({n: sem_images[n] for n in tgt_sem}, inst_images, tgt_sem, tgt_inst, is_thing, faulty)
        print(f"bw: {val}, pq: {pq}")
        curve.append((val, pq))
        if pq >= best_pq:
            best_pq, best_val = pq, val
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure()
    plt.plot([v for v, _ in curve], [p for _, p in curve])
    if best_val is not None:
        plt.scatter(best_val, best_pq, s=100, facecolors="none", edgecolors="r")
    plt.xlabel("min_cluster_size" if use_dbscan else "bandwidth")
    plt.ylabel("panoptic quality")
    plt.title(f"Best {'min_cluster_size' if use_dbscan else 'bandwidth'}: {best_val}, pq: {best_pq}")
    plt.savefig(out / "bandwidth_vs_pq.png")
    plt.close()
    result = {"values": [[v, p] for v, p in curve], "best": best_val, "best_pq": best_pq, "use_dbscan": bool(use_dbscan),
              "segmentwise": bool(segmentwise), "meanshift": None if use_dbscan else meanshift,
              "hdbscan": hdbscan if use_dbscan else None}
    (out / "bandwidth_vs_pq.json").write_text(json.dumps(result, indent=1))
    print(f"Best bandwidth: {best_val}, pq: {best_pq}")
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="bandwidth search")
    ap.add_argument("--ckpt_path", required=True, type=str, help="path of checkpoint to be used")
    ap.add_argument("--subsample", required=False, type=int, default=5)
    ap.add_argument("--debug", action="store_true", help="write the surrogate-id images of every value")
    ap.add_argument("--segmentwise", action="store_true", help="segmentwise clustering")
    ap.add_argument("--use_dbscan", action="store_true", help="HDBSCAN for clustering")
    ap.add_argument("--meanshift", choices=("device", "sklearn"), default="device", help="where the MeanShift fits run")
    ap.add_argument("--hdbscan", choices=("sklearn", "device"), default="sklearn",
                    help="where the HDBSCAN fits of --use_dbscan run: sklearn on the CPU (the reference) or the GPU "
                         "(DeviceHDBSCAN: clift_emst + the host tree pass, pinned to sklearn's estimator)")
    ap.add_argument("--sweep", type=float, nargs=3, metavar=("START", "STOP", "STEP"), help="values np.arange(START, STOP, STEP) instead of the reference's range")
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384], help="reference hard-codes [256, 384] (:390)")
    ap.add_argument("--things_csv", default="resources/scannet_reduced_things.csv", help="name,is_thing rows (non-MOS scenes)")
    args = ap.parse_args()
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.subsample_frames = args.subsample
    cfg.image_dim = list(args.image_dim)
    t0 = time.time()
    find_bandwidth(cfg, args.debug, segmentwise=args.segmentwise, use_dbscan=args.use_dbscan, meanshift=args.meanshift, sweep=args.sweep,
                   things_csv=args.things_csv, hdbscan=args.hdbscan)
    print("Total time for finding bandwidth: ", time.time() - t0)
