#!/usr/bin/env python3
"""Drop-in for reference inference/extract_train_centroids.py (same flags; :33-148, CLI :325-350): render a trained scene, cluster the
rendered instance features class by class and cache the per-class centroids that ``render_panopli.py --cached_centroids_path`` reads.

    python inference/extract_train_centroids.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt --segmentwise [--bandwidth 0.15]
                                                [--meanshift device|sklearn] [--split train|test] [--use_dbscan [--hdbscan sklearn|device]] [--subsample 1] ...

Which frames: like the reference, the ``train`` split of a PanopLi-layout scene but the ``test`` split of a MOS scene (the reference builds
its MOS dataset with "test", :44-54); ``--split`` overrides that, ``--render_trajectory`` renders trajectories/trajectory_blender.pkl
instead.  Writes ``instance_features.npy``, ``thing_features.npy``, ``slow_features.npy`` (slow-fast runs) and ``all_centroids.pkl``
({thing class: centroids in feature units}, the reference's mapping incl. its dtypes) under
``runs/<scene>_<trajectory|train>_<experiment>[_dbscan][_seg]_clust<cluster_size>/``.

The MeanShift fits run on the GPU (``--meanshift device``, contrastive_lift_amd.inference.DeviceMeanShift) unless ``--meanshift sklearn``.
With ``--use_dbscan`` the per-class HDBSCAN fits run in sklearn on the CPU unless ``--hdbscan device`` (contrastive_lift_amd.hdbscan.DeviceHDBSCAN).
``--segmentwise`` is required: the cache is per class, and without it the reference writes the features and then dies (:143-148).
Under torch.distributed.run every rank renders a row-tile of each frame (as render_panopli.py); rank 0 clusters and writes.
"""
import argparse
import os
import pickle
import sys
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from contrastive_lift_amd import inference as inf                    # noqa: E402
from contrastive_lift_amd.config import load_run_config              # noqa: E402
from contrastive_lift_amd.data import get_scene                       # noqa: E402
from render_panopli import build_from_checkpoint                      # noqa: E402


def default_split(config):
    """The split the reference renders (:44-54): train for PanopLi-layout scenes, test for MOS scenes."""
    return "test" if config.dataset_class == "mos" else "train"


def init_ranks(device):
    """render_panopli.py's process setup: under torch.distributed.run one process per GPU joins the group; returns (rank, device)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        device = f"cuda:{local}"
        dist.init_process_group(os.environ.get("CLIFT_DIST_BACKEND", "nccl"))
    return (dist.get_rank() if dist.is_initialized() else 0), torch.device(device)


def render_features(config, scene, model, renderer, frames):
    """Render every (name, rays, K) frame (chunked, row-tiled over the ranks); returns per-frame lists (names, rgb, semantics, fast
    instance features, slow features, thing features) -- the loop of the reference's scripts (:88-127)."""
    H, W = scene.image_dim
    names, rgbs, sems, insts, slows, things = [], [], [], [], [], []
    with torch.no_grad():
        for name, rays, K_frame in frames:
            p_rgb, p_sem, p_inst, p_dist = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg)
            if config.use_delta:
                p_inst = p_inst + (rays[:, 0:3] + p_dist[:, None] * rays[:, 3:6])
            if model.slow_fast_mode:
                slows.append(p_inst[:, config.max_instances:])
                p_inst = p_inst[:, :config.max_instances]
            names.append(name)
            rgbs.append(p_rgb)
            sems.append(p_sem)
            insts.append(p_inst)
            things.append(inf.create_instances_from_semantics(p_inst, p_sem, scene.segmentation_data.fg_classes))
    return names, rgbs, sems, insts, slows, things


def split_frames(scene):
    idx = scene.train_indices if scene.split == "train" else scene.val_indices
    return ((scene.all_frame_names[i], scene.rays_for(i), scene.intrinsics[i]) for i in idx)


def output_dirname(config, trajectory_name, test_only, use_dbscan, segmentwise, cluster_size):
    return Path("runs") / (f"{Path(config.dataset_root).stem}_{trajectory_name if not test_only else 'train'}_{Path(config.experiment)}"
                           f"{'_dbscan' if use_dbscan else ''}{'_seg' if segmentwise else ''}_clust{cluster_size}")


def extract_train_centroids(config, trajectory_name, test_only=True, bandwidth=0.15, use_dbscan=False, segmentwise=True, use_silverman=False,
                            cluster_size=500, meanshift="device", split=None, device="cuda:0", hdbscan="sklearn"):
    if not segmentwise:
        raise ValueError("extract_train_centroids: the centroid cache is per thing class and needs --segmentwise "
                         "(without it the reference script fails after writing the features)")
    out = output_dirname(config, trajectory_name, test_only, use_dbscan, segmentwise, cluster_size)
    out.mkdir(exist_ok=True, parents=True)
    rank, device = init_ranks(device)
    scene = get_scene(config, split or default_split(config), device)
    model, renderer, _ = build_from_checkpoint(config, scene, device)
    renderer.update_step_ratio(renderer.step_ratio * 0.5)                                    # :85
    if test_only:
        frames = split_frames(scene)
    else:
        frames = ((n, r, scene.intrinsics[0]) for n, r in scene.trajectory_set(trajectory_name))
    names, rgbs, sems, insts, slows, things = render_features(config, scene, model, renderer, frames)
    if rank != 0:
        return out
    np.save(out / "instance_features.npy", torch.cat(insts, 0).cpu().numpy())
    all_thing = torch.cat(things, 0).cpu().numpy()
    np.save(out / "thing_features.npy", all_thing)
    if model.slow_fast_mode:
        np.save(out / "slow_features.npy", torch.cat(slows, 0).cpu().numpy())
    _, cents = inf.cluster_segmentwise(all_thing, sems, bandwidth, device, num_images=len(rgbs), use_silverman=use_silverman,
                                       use_dbscan=use_dbscan, cluster_size=cluster_size, meanshift=meanshift, return_dict=True,
                                       hdbscan=hdbscan)
    with open(out / "all_centroids.pkl", "wb") as f:
        pickle.dump(cents, f)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--render_trajectory", action="store_true")
    ap.add_argument("--bandwidth", type=float, default=0.15, required=False)
    ap.add_argument("--cluster_size", type=int, default=500, required=False, help="min_cluster_size for HDBSCAN")
    ap.add_argument("--use_dbscan", action="store_true")
    ap.add_argument("--segmentwise", action="store_true", help="required: the centroid cache is per thing class")
    ap.add_argument("--subsample", type=int, default=1, required=False)
    ap.add_argument("--use_silverman", action="store_true")
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384], help="reference hard-codes [256, 384] (:338)")
    ap.add_argument("--meanshift", choices=("device", "sklearn"), default="device", help="where the MeanShift fits run")
    ap.add_argument("--hdbscan", choices=("sklearn", "device"), default="sklearn",
                    help="where the HDBSCAN fits of --use_dbscan run: sklearn on the CPU (the reference) or the GPU "
                         "(DeviceHDBSCAN: clift_emst + the host tree pass, pinned to sklearn's estimator)")
    ap.add_argument("--split", choices=("train", "test"), default=None, help="frames to render (default: train; test for MOS scenes, as the reference)")
    args = ap.parse_args()
    if not args.segmentwise:
        ap.error("--segmentwise is required: all_centroids.pkl holds per-class centroids (the reference fails without it)")
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.subsample_frames = args.subsample
    cfg.image_dim = list(args.image_dim)
    print(extract_train_centroids(cfg, "trajectory_blender", test_only=not args.render_trajectory, bandwidth=args.bandwidth,
                                  use_dbscan=args.use_dbscan, segmentwise=True, use_silverman=args.use_silverman,
                                  cluster_size=args.cluster_size, meanshift=args.meanshift, split=args.split, hdbscan=args.hdbscan))
