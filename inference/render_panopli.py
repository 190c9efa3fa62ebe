#!/usr/bin/env python3
"""Drop-in for reference inference/render_panopli.py (same flags, same inputs and outputs; RP:430-458 -> 31-188).

    python inference/render_panopli.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt [--cached_centroids_path P]
                                       [--bandwidth 0.15] [--subsample 1] [--render_trajectory] ...

Reads ``runs/<experiment>/config.yaml`` next to the checkpoint (RP:445), rebuilds the field at ``min_grid_dim``, restores the
renderer buffers, upsamples to the checkpoint's grid if it was saved after an upscale epoch (RP:91-98), loads the weights,
halves the step ratio (RP:104) and renders every test frame in chunks on the GPU.  Writes ``instance_features.npy``,
``thing_features.npy``, ``slow_features.npy``, ``pred_semantics/*.png`` (uint8), ``pred_surrogateid/*.png`` (uint16) and
``vis_semantics_and_surrogate/*.png`` under ``runs/<scene>_<test|trajectory>_<experiment>/`` (RP:142-193).  With ``--save_pointcloud``
also ``pointcloud.pkl``: every rendered pixel back-projected along its ray (RP:124) with its surrogate id, the input of
``inference/fit_bboxes.py`` and of the reference's ``inference/visualize_bboxes.py``.

Surface outputs of the ray route (two more launches per chunk, only when asked for): ``--save_surface`` writes per frame
``surface/<frame>.npz`` (depth_median, hit, normals) and ``vis_normals/<frame>.png``; ``--pointcloud_depth median`` back-projects to the
median-depth hit point instead of the expected distance, drops the pixels whose ray never loses half its transmittance and adds their
normals to ``pointcloud.pkl``.

Amodal instance layers (a pass of its own per frame, only when asked for): ``--save_layers [--layers_level 0.5]`` writes per
frame ``layers/<frame>.npz`` and ``.json`` -- what every instance covers also behind the things in front of it, what of it is visible and
where its first sample lies -- and ``vis_amodal/<frame>.png``; with ``--layers_colour [--layers_colour_rest]`` also the colour of every
instance behind its occluders: ``colour`` in the npz and ``vis_amodal_rgb/<frame>/slot_<k>.png``, one RGBA image per slot.  It needs ``--cached_centroids_path`` (the centroids are numbered once for the
scene) or a linear_assignment model.
"""
import argparse
import functools
import os
import pickle
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import contrastive_lift_amd as cl                                   # noqa: E402
from contrastive_lift_amd import inference as inf                    # noqa: E402
from contrastive_lift_amd import points3d                            # noqa: E402
from contrastive_lift_amd.config import load_run_config              # noqa: E402
from contrastive_lift_amd.data import get_scene                       # noqa: E402


def strip_prefix(state_dict, key):
    """util/misc.py:159-164."""
    return {k[len(key) + 1:]: v for k, v in state_dict.items() if k.startswith(key + ".")}


def build_from_checkpoint(config, scene, device):
    from contrastive_lift_amd import engine
    engine.set_mlp_precision(getattr(config, "mlp_dtype", None) or engine.DEFAULT_MLP_DTYPE)
    ckpt = torch.load(config.resume, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"]
    total_classes = len(scene.segmentation_data.bg_classes) + len(scene.segmentation_data.fg_classes)
    slow_fast = config.instance_loss_mode == "slow_fast"
    g = int(config.min_grid_dim)
    model = cl.TensorVMSplit([g, g, g], num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32),
                             num_semantic_classes=total_classes,
                             dim_feature_instance=2 * config.max_instances if slow_fast else config.max_instances,
                             output_mlp_semantics=torch.nn.Identity() if config.semantic_weight_mode != "softmax" else torch.nn.Softmax(dim=-1),
                             use_semantic_mlp=config.use_mlp_for_semantics, use_instance_mlp=config.use_mlp_for_instances,
                             use_distilled_features_semantic=config.use_distilled_features_semantic,
                             use_distilled_features_instance=config.use_distilled_features_instance,
                             pe_sem=config.pe_sem, pe_ins=config.pe_ins, slow_fast_mode=slow_fast, use_proj=config.use_proj, device=device)
    renderer = cl.TensoRFRenderer(scene.scene_bounds, [g, g, g], semantic_weight_mode=config.semantic_weight_mode).to(device)
    renderer.load_state_dict(strip_prefix(sd, "renderer"))
    for epoch in list(config.grid_upscale_epochs)[::-1]:
        if ckpt["epoch"] >= epoch:
            model.upsample_volume_grid(renderer.grid_dim.tolist())
            break
    renderer.update_step_size(renderer.grid_dim)            # refresh host scalars from the restored buffers
    msd = strip_prefix(sd, "model")
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    if tuple(msd["density_plane.0"].shape) != shapes["density_plane.0"]:
        # checkpoint written after a bbox shrink: adopt the checkpoint's table shapes (RP:91-98 relies on
        # renderer.grid_dim carrying them)
        p0, l0 = msd["density_plane.0"], msd["density_line.0"]
        model.upsample_volume_grid([p0.shape[3], p0.shape[2], l0.shape[2]])
    model.load_state_dict(msd)
    return model, renderer, ckpt


def output_dirname(config, trajectory_name, test_only, use_dbscan, segmentwise):
    return Path("runs") / (f"{Path(config.dataset_root).stem}_{trajectory_name if not test_only else 'test'}_{Path(config.experiment)}"
                           f"{'_dbscan' if use_dbscan else ''}{'_seg' if segmentwise else ''}")


def glasbey(n):
    rng = np.random.default_rng(7)
    c = rng.uniform(0.15, 1.0, size=(n, 3))
    c[0] = 0
    return c


def distributed_device(device):
    """Launched under torch.distributed.run: one process per GPU, every frame rendered as row-tiles (one per rank) and assembled with one
    all-gather (inference.render_rays_sharded); clustering and file output happen on rank 0.  Returns (this rank's device, rank)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        device = f"cuda:{local}"
        dist.init_process_group(os.environ.get("CLIFT_DIST_BACKEND", "nccl"))
    return torch.device(device), (dist.get_rank() if dist.is_initialized() else 0)


def load_for_inference(config, device):
    """The test scene, the field and the renderer of a checkpoint, the step ratio halved (RP:104)."""
    scene = get_scene(config, "test", device)
    model, renderer, _ = build_from_checkpoint(config, scene, device)
    renderer.update_step_ratio(renderer.step_ratio * 0.5)
    return scene, model, renderer


def scene_frames(scene, trajectory_name, test_only):
    """(name, rays, intrinsics) per frame -- RP:67-72: the test split, or the predefined trajectory trajectories/<trajectory_name>.pkl
    (frames named by index, all with the intrinsics of frame 0)."""
    if test_only:
        return ((scene.all_frame_names[i], scene.rays_for(i), scene.intrinsics[i]) for i in scene.val_indices)
    return ((n, r, scene.intrinsics[0]) for n, r in scene.trajectory_set(trajectory_name))


def write_surface_frame(out, frame_name, depth_median, hit, normals):
    """The files of ``--save_surface`` for one frame (also of inference/edit_scene.py): ``surface/<frame>.npz`` with depth_median (H, W)
    float32 (a z-depth, like depth/), hit (H, W) bool and normals (H, W, 3) float32 (the un-normalised sums of w n), and
    ``vis_normals/<frame>.png``: (n / |n| + 1) / 2 where the ray hit, black elsewhere.  Tensors on any device."""
    for d in ("surface", "vis_normals"):
        (out / d).mkdir(exist_ok=True)
    hit = hit.cpu().numpy()
    nrm = normals.cpu().numpy().astype(np.float32)
    np.savez(out / "surface" / f"{frame_name}.npz", depth_median=depth_median.cpu().numpy().astype(np.float32), hit=hit, normals=nrm)
    unit = nrm / np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-20)
    vis = np.where(hit[..., None], (unit + 1.0) * 0.5, 0.0)
    Image.fromarray((vis.clip(0, 1) * 255).astype(np.uint8)).save(out / "vis_normals" / f"{frame_name}.png")


def layers_table(config, scene, cached_centroids_path):
    """The slot table of ``--save_layers``: the cached centroids numbered once for the scene (layers.SlotTable.from_centroids), or, for a
    linear-assignment model, whose instance outputs are slot scores, one slot per output."""
    from contrastive_lift_amd.layers import SlotTable
    fg = scene.segmentation_data.fg_classes
    total_classes = len(scene.segmentation_data.bg_classes) + len(fg)
    if cached_centroids_path is not None:
        with open(cached_centroids_path, "rb") as f:
            return SlotTable.from_centroids(pickle.load(f), fg, total_classes)
    if config.instance_loss_mode == "linear_assignment":
        return SlotTable.from_scores(fg, total_classes, int(config.max_instances))
    raise ValueError("--save_layers needs --cached_centroids_path (or a linear_assignment model): the layers are kept per centroid")


def write_layers_frame(out, frame_name, layers, table, H, W, rgb, level=0.5, colour=None):
    """The files of ``--save_layers`` for one frame, from its layers (H W, K + 1, 4) and rendered colours (H W, 3), tensors on any device.
    ``layers/<frame>.npz``: slots (n,) the slots with an amodal pixel (A > level) in this frame, slot_class (n,), and amodal = A, visible = V,
    front = zf, the distance at which the slot's first sample lies, each (n, H, W) float16.  ``layers/<frame>.json``: level and per such slot
    its class, centroid index, amodal and visible pixel counts, occlusion rate and mean amodal distance (layers.summarise).
    ``vis_amodal/<frame>.png``: the outline of every amodal mask, in the slot's colour, over the rendered colours.
    With ``colour`` (H W, K + 1, 4), the premultiplied colour layers of ``--layers_colour``: the npz also holds colour
    (n, H, W, 4) uint8, un-premultiplied RGB plus A, and ``vis_amodal_rgb/<frame>/slot_<k>.png`` is that RGBA image of slot k -- the
    instance with nothing in front of it."""
    import json
    from contrastive_lift_amd import layers as ly
    for d in ("layers", "vis_amodal"):
        (out / d).mkdir(exist_ok=True)
    s = ly.summarise(layers, table, level)
    present = torch.nonzero(s["amodal_pixels"] > 0).reshape(-1)
    sel = layers[:, present].permute(1, 0, 2).reshape(present.shape[0], H, W, 4).cpu()
    slots = present.cpu().numpy().astype(np.int32)
    extra = {}
    if colour is not None:
        rgba = ly.unpremultiply(colour[:, present].permute(1, 0, 2).reshape(present.shape[0], H, W, 4)).clamp(0, 1)
        extra["colour"] = (rgba * 255).round().to(torch.uint8).cpu().numpy()
        (out / "vis_amodal_rgb" / str(frame_name)).mkdir(exist_ok=True, parents=True)
        for i, img in zip(slots, extra["colour"]):
            Image.fromarray(np.ascontiguousarray(img)).save(out / "vis_amodal_rgb" / str(frame_name) / f"slot_{int(i)}.png")
    np.savez(out / "layers" / f"{frame_name}.npz", slots=slots, slot_class=table.slot_class[slots].astype(np.int32),
             amodal=sel[..., 0].numpy().astype(np.float16), visible=sel[..., 1].numpy().astype(np.float16),
             front=sel[..., 3].numpy().astype(np.float16), **extra)
    col = {k: v.cpu().numpy() for k, v in s.items()}
    summary = dict(frame=str(frame_name), level=float(level), n_slots=int(table.K),
                   slots=[dict(slot=int(i), slot_class=int(col["slot_class"][i]), slot_index=int(col["slot_index"][i]),
                               amodal_pixels=int(col["amodal_pixels"][i]), visible_pixels=int(col["visible_pixels"][i]),
                               occlusion=float(col["occlusion"][i]), mean_distance=float(col["mean_distance"][i])) for i in slots])
    with open(out / "layers" / f"{frame_name}.json", "w") as f:
        json.dump(summary, f, indent=1)
    vis = rgb.reshape(H, W, 3).cpu().numpy().clip(0, 1).copy()
    pal = glasbey(table.K + 2)
    masks = sel[..., 0].numpy() > level
    for i, m in zip(slots, masks):
        inner = m.copy()                                     # 4-neighbour erosion: a mask pixel with a neighbour outside is outline
        inner[1:] &= m[:-1]; inner[:-1] &= m[1:]; inner[:, 1:] &= m[:, :-1]; inner[:, :-1] &= m[:, 1:]
        vis[m & ~inner] = pal[int(i) + 1]
    Image.fromarray((vis * 255).astype(np.uint8)).save(out / "vis_amodal" / f"{frame_name}.png")


def render_panopli_checkpoint(config, trajectory_name, test_only=True, bandwidth=0.15, use_dbscan=False, segmentwise=False,
                              cached_centroids_path=None, device="cuda:0", use_silverman=False, cluster_size=500,
                              meanshift="sklearn", save_pointcloud=False, hdbscan="sklearn", save_surface=False, pointcloud_depth="expected",
                              save_layers=False, layers_level=0.5, layers_colour=False, layers_colour_rest=False):
    if (layers_colour or layers_colour_rest) and not save_layers:
        raise ValueError("layers_colour needs save_layers")
    if pointcloud_depth not in ("expected", "median"):
        raise ValueError(f"pointcloud_depth must be 'expected' or 'median', got {pointcloud_depth!r}")
    median_cloud = bool(save_pointcloud) and pointcloud_depth == "median"
    surface = bool(save_surface) or median_cloud
    out = output_dirname(config, trajectory_name, test_only, use_dbscan, segmentwise)
    out.mkdir(exist_ok=True, parents=True)
    device, rank = distributed_device(device)
    scene, model, renderer = load_for_inference(config, device)
    H, W = scene.image_dim
    fg = scene.segmentation_data.fg_classes
    table = layers_table(config, scene, cached_centroids_path) if save_layers else None
    rgbs, sems, depths, inst_feats, thing_feats, slow_feats, points = [], [], [], [], [], [], []
    names = []
    hits, normals, depths_med = [], [], []
    with torch.no_grad():
        for name, rays, K_frame in scene_frames(scene, trajectory_name, test_only):
            names.append(name)
            if surface:
                p_rgb, p_sem, p_inst, p_dist, p_dmed, p_hit, p_nrm = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg,
                                                                                            render_fn=inf.render_rays_surface)
                hits.append(p_hit > 0.5)
                normals.append(p_nrm.cpu())
                depths_med.append(inf.distance_to_depth(K_frame, p_dmed.view(H, W)).cpu())
            else:
                p_rgb, p_sem, p_inst, p_dist = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg)
            depths.append(inf.distance_to_depth(K_frame, p_dist.view(H, W)))
            if save_layers:         # a pass of its own over the frame; written at once: a frame's layers are large
                fn = functools.partial(inf.render_rays_layers, table=table, use_delta=bool(config.use_delta), colour=bool(layers_colour),
                                       colour_rest=bool(layers_colour_rest))
                lay, _, _, *lay_colour = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg, render_fn=fn)
                if rank == 0:
                    write_layers_frame(out, name, lay, table, H, W, p_rgb, layers_level, colour=lay_colour[0] if lay_colour else None)
                del lay, lay_colour
            if save_pointcloud:
                # (use_delta below keeps the expected distance for the instance features: only the saved points change)
                points.append(points3d.backproject(rays, p_dmed if median_cloud else p_dist).float().cpu())
            if config.use_delta:
                p_inst = p_inst + (rays[:, 0:3] + p_dist[:, None] * rays[:, 3:6])
            if model.slow_fast_mode:
                slow_feats.append(p_inst[:, config.max_instances:])
                p_inst = p_inst[:, :config.max_instances]
            inst_feats.append(p_inst)
            rgbs.append(p_rgb)
            sems.append(p_sem)
            thing_feats.append(inf.create_instances_from_semantics(p_inst, p_sem, fg))
    if rank != 0:
        return out
    np.save(out / "instance_features.npy", torch.cat(inst_feats, 0).cpu().numpy())
    all_thing = torch.cat(thing_feats, 0).cpu().numpy()
    np.save(out / "thing_features.npy", all_thing)
    if model.slow_fast_mode:
        np.save(out / "slow_features.npy", torch.cat(slow_feats, 0).cpu().numpy())
    if cached_centroids_path is not None:
        with open(cached_centroids_path, "rb") as f:
            cents = pickle.load(f)
        insts = inf.assign_clusters(all_thing, sems, cents, device, num_images=len(rgbs))
    else:
        if not segmentwise:
            insts, _ = inf.cluster(all_thing, bandwidth, device, num_images=len(rgbs), use_silverman=use_silverman, use_dbscan=use_dbscan,
                                   cluster_size=cluster_size, meanshift=meanshift, hdbscan=hdbscan)
        else:
            insts, _ = inf.cluster_segmentwise(all_thing, sems, bandwidth, device, num_images=len(rgbs), use_silverman=use_silverman,
                                               use_dbscan=use_dbscan, cluster_size=cluster_size, meanshift=meanshift, hdbscan=hdbscan)
    for d in ("vis_semantics_and_surrogate", "pred_semantics", "pred_surrogateid"):
        (out / d).mkdir(exist_ok=True)
    for j, frame_name in enumerate(names):
        name = f"{frame_name}.png"
        sem_id = sems[j].argmax(dim=1).reshape(H, W).cpu().numpy()
        sur_id = insts[j].argmax(dim=1).reshape(H, W).cpu().numpy()
        Image.fromarray(sem_id.astype(np.uint8)).save(out / "pred_semantics" / name)
        Image.fromarray(sur_id.astype(np.uint16)).save(out / "pred_surrogateid" / name)
        pal = glasbey(int(max(sur_id.max(), sem_id.max())) + 2)
        d = depths[j].reshape(H, W).cpu().numpy()
        d = (d - d.min()) / max(float(np.ptp(d)), 1e-8)
        vis = np.concatenate([rgbs[j].reshape(H, W, 3).cpu().numpy(), pal[sem_id], pal[sur_id], np.repeat(d[..., None], 3, -1)], 1)
        Image.fromarray((vis.clip(0, 1) * 255).astype(np.uint8)).save(out / "vis_semantics_and_surrogate" / name)
    if save_surface:
        for j, frame_name in enumerate(names):
            write_surface_frame(out, frame_name, depths_med[j].reshape(H, W), hits[j].reshape(H, W), normals[j].reshape(H, W, 3))
    if save_pointcloud:
        # the layout visualize_bboxes.py:269-275 loads: points (P, 3), instances (P,) = the ids written to pred_surrogateid (0 = stuff)
        cloud = {"points": torch.cat(points, 0).numpy().astype(np.float32),
                 "instances": torch.cat([i.argmax(dim=1) for i in insts], 0).cpu().numpy().astype(np.uint16),
                 "semantics": torch.cat([s.argmax(dim=1) for s in sems], 0).cpu().numpy().astype(np.uint8),
                 "rgb": (torch.cat(rgbs, 0).cpu().numpy().clip(0, 1) * 255).astype(np.uint8)}
        if median_cloud:        # the hit points: rows whose ray has no hit leave every array alike, the normals come along
            keep = torch.cat(hits, 0).cpu().numpy()
            cloud = {k: v[keep] for k, v in cloud.items()}
            cloud["normals"] = torch.cat(normals, 0).numpy().astype(np.float32)[keep]
        with open(out / "pointcloud.pkl", "wb") as f:
            pickle.dump(cloud, f)
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--render_trajectory", action="store_true")
    ap.add_argument("--bandwidth", type=float, default=0.15, required=False)
    ap.add_argument("--cluster_size", type=int, default=500, required=False, help="min_cluster_size for HDBSCAN")
    ap.add_argument("--use_dbscan", action="store_true",
                    help="HDBSCAN clustering (reference RP:236-255): the hdbscan package when it is installed, otherwise "
                         "sklearn.cluster.HDBSCAN (the same algorithm; scikit-learn >= 1.3)")
    ap.add_argument("--segmentwise", action="store_true")
    ap.add_argument("--subsample", type=int, default=1, required=False)
    ap.add_argument("--use_silverman", action="store_true")
    ap.add_argument("--cached_centroids_path", type=str, required=False)
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384], help="reference hard-codes [256, 384] (RP:450)")
    ap.add_argument("--meanshift", choices=("sklearn", "device"), default="sklearn",
                    help="where the MeanShift fits run: sklearn on the CPU (the reference) or the GPU (DeviceMeanShift)")
    ap.add_argument("--hdbscan", choices=("sklearn", "device"), default="sklearn",
                    help="where the HDBSCAN fits of --use_dbscan run: sklearn on the CPU (the reference) or the GPU "
                         "(DeviceHDBSCAN: clift_emst + the host tree pass, pinned to sklearn's estimator)")
    ap.add_argument("--save_pointcloud", action="store_true",
                    help="also write pointcloud.pkl (points, instances, semantics, rgb of every rendered pixel) for inference/fit_bboxes.py")
    ap.add_argument("--save_surface", action="store_true",
                    help="also write surface/<frame>.npz (depth_median, hit, normals) and vis_normals/<frame>.png: the median-depth hit and the "
                         "composited field normal of every pixel's ray")
    ap.add_argument("--pointcloud_depth", choices=("expected", "median"), default="expected",
                    help="where --save_pointcloud puts a pixel's point: at the expected distance (the reference), or at the median-depth hit "
                         "(pixels without a hit are dropped, a normals key is added)")
    ap.add_argument("--save_layers", action="store_true",
                    help="also write layers/<frame>.npz and .json (amodal opacity, visible weight and front distance of every instance slot, and "
                         "their summary) and vis_amodal/<frame>.png; needs --cached_centroids_path or a linear_assignment model")
    ap.add_argument("--layers_level", type=float, default=0.5, help="the opacity above which --save_layers counts a pixel into a mask")
    add_layers_colour_arguments(ap)
    return ap


def add_layers_colour_arguments(ap):
    """The colour-layer flags of ``--save_layers`` (inference/edit_scene.py has them too)."""
    ap.add_argument("--layers_colour", action="store_true",
                    help="--save_layers: also the colour of every instance behind its occluders (one more appearance pass over the listed samples "
                         "that have a slot): layers/<frame>.npz gains colour (n, H, W, 4) uint8 and vis_amodal_rgb/<frame>/slot_<k>.png is written, "
                         "an RGBA image per slot")
    ap.add_argument("--layers_colour_rest", action="store_true",
                    help="--layers_colour: colour every listed sample, the rest column's (stuff, unassigned) too -- much more appearance work")


def check_layers_colour_arguments(ap, args):
    if args.layers_colour and not args.save_layers:
        ap.error("--layers_colour needs --save_layers")
    if args.layers_colour_rest and not args.layers_colour:
        ap.error("--layers_colour_rest needs --layers_colour")


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_layers_colour_arguments(ap, args)
    return args


if __name__ == "__main__":
    args = parse_args()
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.subsample_frames = args.subsample
    cfg.image_dim = list(args.image_dim)
    print(render_panopli_checkpoint(cfg, "trajectory_blender", test_only=not args.render_trajectory, bandwidth=args.bandwidth,
                                    use_dbscan=args.use_dbscan, segmentwise=args.segmentwise,
                                    cached_centroids_path=args.cached_centroids_path, use_silverman=args.use_silverman,
                                    cluster_size=args.cluster_size, meanshift=args.meanshift, hdbscan=args.hdbscan,
                                    save_pointcloud=args.save_pointcloud, save_surface=args.save_surface,
                                    pointcloud_depth=args.pointcloud_depth, save_layers=args.save_layers,
                                    layers_level=args.layers_level, layers_colour=args.layers_colour,
                                    layers_colour_rest=args.layers_colour_rest))
