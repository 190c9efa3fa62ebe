#!/usr/bin/env python3
"""Render a trained scene with one boxed instance deleted, extracted, copied or moved.

    python inference/edit_scene.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt --bboxes bboxes.pkl --instance ID
                                   --op delete|extract|copy|move [--translate x y z] [--rotate_deg rx ry rz] [--pad 0.0]
                                   [--render_trajectory] [--image_dim H W] [--weight_thres 0]

``bboxes.pkl`` comes from ``inference/fit_bboxes.py`` (one oriented box per instance id).  ``copy`` and ``move`` are rigid: the box content
undergoes x -> R (x - pos) + pos + t with R = Rz Ry Rx of ``--rotate_deg`` and t = ``--translate`` (contrastive_lift_amd/edit.py; the
reference's forward_duplicate / forward_manipulate arithmetic, which is not rigid for R != I, stays available as
``TensoRFRenderer.forward_duplicate`` / ``forward_manipulate``).  Fitted boxes hug the filtered points: ``--pad`` grows the box on every
side.  Checkpoint loading and the frame loop are those of ``inference/render_panopli.py``; under torch.distributed.run every frame is
rendered as row-tiles over the ranks.  Writes ``rgb/*.png``, ``pred_semantics/*.png`` (uint8) and ``depth/*.npy`` under
``runs/<scene>_<test|trajectory>_<experiment>_edit_<op>_<id>/``.
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

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import render_panopli as rp                                           # noqa: E402
from contrastive_lift_amd import edit as ed                           # noqa: E402
from contrastive_lift_amd import inference as inf                     # noqa: E402
from contrastive_lift_amd.config import load_run_config               # noqa: E402

OPS = ("delete", "extract", "copy", "move")


def resolve_edit(boxes, instance, op, translate=(0.0, 0.0, 0.0), rotate_deg=(0.0, 0.0, 0.0), pad=0.0):
    if instance not in boxes:
        raise SystemExit(f"instance {instance} has no box (boxes: {sorted(boxes)})")
    box = ed.EditBox.from_fitted(boxes[instance], pad=pad)
    if op == "delete":
        return ed.delete(box)
    if op == "extract":
        return ed.extract(box)
    R = ed.rotation_from_euler_deg(*rotate_deg)
    return (ed.copy if op == "copy" else ed.move)(box, np.asarray(translate, dtype=np.float64), R)


def edit_scene_checkpoint(config, edit, tag, trajectory_name="trajectory_blender", test_only=True, device="cuda:0", weight_thres=0.0):
    out = Path(f"{rp.output_dirname(config, trajectory_name, test_only, False, False)}_edit_{tag}")
    device, rank = rp.distributed_device(device)
    scene, model, renderer = rp.load_for_inference(config, device)
    H, W = scene.image_dim
    render_fn = functools.partial(inf.render_rays_edit, edit=edit, weight_thres=float(weight_thres))
    if rank == 0:
        for d in ("rgb", "pred_semantics", "depth"):
            (out / d).mkdir(exist_ok=True, parents=True)
    with torch.no_grad():
        for name, rays, K_frame in rp.scene_frames(scene, trajectory_name, test_only):
            p_rgb, p_sem, _, p_dist = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg, render_fn=render_fn)
            if rank != 0:
                continue
            rgb = (p_rgb.reshape(H, W, 3).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
            Image.fromarray(rgb).save(out / "rgb" / f"{name}.png")
            Image.fromarray(p_sem.argmax(dim=1).reshape(H, W).cpu().numpy().astype(np.uint8)).save(out / "pred_semantics" / f"{name}.png")
            np.save(out / "depth" / f"{name}.npy", inf.distance_to_depth(K_frame, p_dist.view(H, W)).reshape(H, W).cpu().numpy())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--bboxes", type=str, required=True, help="bboxes.pkl of inference/fit_bboxes.py")
    ap.add_argument("--instance", type=int, required=True, help="instance id (a key of bboxes.pkl)")
    ap.add_argument("--op", choices=OPS, required=True)
    ap.add_argument("--translate", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="copy / move: translation t")
    ap.add_argument("--rotate_deg", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("RX", "RY", "RZ"),
                    help="copy / move: rotation about the box centre, R = Rz Ry Rx (degrees)")
    ap.add_argument("--pad", type=float, default=0.0, help="grow the fitted box by this much on every side")
    ap.add_argument("--render_trajectory", action="store_true")
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384])
    ap.add_argument("--weight_thres", type=float, default=0.0,
                    help="evaluate the heads where w > this (0: every sample with weight, like the reference's edit renders; 1e-4: the plain render's threshold)")
    args = ap.parse_args()
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.subsample_frames = 1
    cfg.image_dim = list(args.image_dim)
    with open(args.bboxes, "rb") as f:
        the_edit = resolve_edit(pickle.load(f), args.instance, args.op, args.translate, args.rotate_deg, args.pad)
    print(edit_scene_checkpoint(cfg, the_edit, f"{args.op}_{args.instance}", test_only=not args.render_trajectory, weight_thres=args.weight_thres))
