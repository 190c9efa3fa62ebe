"""Torch restatement of a render under an edit PROGRAM (an ordered list of edits applied in one render), written from the definition and
composed from the CPU oracle like tests/edit_cases.py.  Test infrastructure only.

The definition: scene_0 is the trained field, scene_i is e_i applied to scene_{i-1}.  A sample (p, d) is evaluated in scene_n by walking
e_n ... e_1: edit i tests the CURRENT p against its source and destination box; a sample its kill rule names is empty and the walk stops;
a sample inside its destination box continues at the point (and with the view direction) the content there came from.  What is left after
e_1 is looked up in the field.  The in-aabb mask comes from the unedited samples, the heads are evaluated at every in-aabb sample and
sigma is zeroed for the killed ones -- as ``edit_cases.render_edit`` does for one edit.

``render_program`` takes the edits as ``edit_cases.Spec`` (plain callables): it does not go through ``contrastive_lift_amd.edit``.
"""
import numpy as np
import torch

import edit_cases as ec
from oracle import field as fld, render as orender


def box_spec(op, axes, centre, lo, hi):
    """delete / extract of the box {lo <= axes (p - centre) <= hi} (rows of ``axes`` are the box axes) as a ``Spec``."""
    axes, centre, lo, hi = (torch.as_tensor(np.asarray(x), dtype=torch.float32) for x in (axes, centre, lo, hi))

    def inside(p):
        q = (p - centre) @ axes.T
        return ((lo <= q) & (q <= hi)).all(-1)
    if op == "delete":
        return ec.Spec(inside, None, None, None, lambda s, d: s)
    if op == "extract":
        return ec.Spec(inside, None, None, None, lambda s, d: ~s)
    raise ValueError(op)


def moved_box(axes, centre, translation, rotation):
    """Where the box (axes, centre) stands after x -> R (x - centre) + centre + t: a point y is inside iff R^-1 (y - centre - t) + centre was,
    i.e. axes' = axes R^-1, centre' = centre + t (bounds unchanged).  fp64 numpy."""
    axes, centre, t, R = (np.asarray(x, dtype=np.float64) for x in (axes, centre, translation, rotation))
    return axes @ np.linalg.inv(R), centre + t


def walk(flat, dirs, specs):
    """The backward walk over flat fp32 points (n, 3) and directions (n, 3): returns (points looked up, their directions, killed (n,),
    number of remaps per point (n,))."""
    flat, dirs = flat.clone(), dirs.clone()
    n = flat.shape[0]
    dead = torch.zeros(n, dtype=torch.bool)
    hops = torch.zeros(n, dtype=torch.int64)
    for spec in reversed(list(specs)):
        src = spec.src(flat) if spec.src is not None else torch.zeros(n, dtype=torch.bool)
        dst = spec.dst(flat) if spec.dst is not None else torch.zeros(n, dtype=torch.bool)
        dead = dead | spec.kill(src, dst).bool()
        mov = dst & ~dead                                                    # a killed sample has stopped
        if bool(mov.any()):
            moved = spec.point(flat[mov])
            dirs[mov] = spec.direction(dirs[mov])
            flat[mov] = moved
            hops[mov] += 1
    return flat, dirs, dead, hops


def render_program(P, rays, cfg, specs, white_bg):
    """The render of ``edit_cases.render_edit`` with the list of ``Spec`` in the place of the one.  Returns (rgb, sem, inst, depth), the
    sigma array and the (N, S) number of remaps per sample."""
    pts, z, inbox = orender.sample_along_rays(rays, cfg, None)               # the mask: from the UNEDITED samples
    N, S = z.shape
    flat, dirs, dead, hops = walk(pts.reshape(-1, 3), rays[:, None, 3:6].expand(N, S, 3).reshape(-1, 3), specs)
    xn = orender.normalize(flat.reshape(N, S, 3), cfg)
    dirs = dirs.reshape(N, S, 3)
    Ccls = P[[k for k in P if k.startswith("render_semantic_mlp.mlp.") and k.endswith(".weight")][-1]].shape[0]
    D = fld.instance_width(P)
    sigma, rgb = torch.zeros(N, S), torch.zeros(N, S, 3)
    sem, inst = torch.zeros(N, S, Ccls), torch.zeros(N, S, D)
    if bool(inbox.any()):
        xa = xn[inbox]
        sigma[inbox] = fld.density(P, xa, cfg.density_shift)
        rgb[inbox] = fld.appearance_mlp(P, dirs[inbox], fld.appearance_feature(P, xa))
        sem[inbox] = fld.semantic_head(P, xa, softmax=(cfg.semantic_weight_mode == "softmax"))
        inst[inbox] = fld.instance_head(P, xa)
    sigma[dead.reshape(N, S)] = 0
    dists, _ = orender._deltas_midpoints(z)
    _, w, _ = orender.sigma_to_weights(sigma, dists * cfg.distance_scale)
    opacity = w.sum(-1)
    rgb_map = (w[..., None] * rgb).sum(-2)
    ws = w[..., None]
    if cfg.semantic_weight_mode == "argmax":
        ws = torch.nn.functional.one_hot(w.argmax(dim=1), num_classes=S).to(w.dtype)[..., None]
    sem_map = orender._softmax_log((ws * sem).sum(-2), cfg)
    inst_map = (ws * inst).sum(-2)
    if white_bg:
        rgb_map = rgb_map + (1.0 - opacity[..., None])
    return (rgb_map.clamp(0, 1), sem_map, inst_map, (w * z).sum(-1)), sigma, hops.reshape(N, S)


def rays_off_all_faces(rays, cfg, program):
    """(N,) bool, fp64: the criterion of test_gpu_scene_edit.rays_off_the_faces at every stage of the walk.  A ray is left out when one of
    its samples, at the position it has when edit i tests it (a killed sample is tested no further), lies within 1e-5 of a face plane of
    src_i or dst_i: there two fp32 classifications may disagree.  ``program``: an iterable of ``edit.Edit`` (fp64 boxes and maps).  At most
    4 rays may be left out."""
    N = rays.shape[0]
    p = orender.sample_along_rays(rays, cfg, None)[0].reshape(-1, 3).double().numpy().copy()
    near = np.zeros(p.shape[0], dtype=bool)
    dead = np.zeros(p.shape[0], dtype=bool)
    for e in reversed(list(program)):
        for box in (e.src, e.dst):
            q = box.local(p)
            near |= ~dead & ((np.abs(q - box.lo) < 1e-5) | (np.abs(q - box.hi) < 1e-5)).any(1)
        dead |= e.killed(p)
        if e.mode >= 2:                                                      # DUPLICATE, MANIPULATE: the remapping modes
            mov = ~dead & e.dst.contains(p)
            p[mov] = p[mov] @ e.M.T + e.t
    keep = torch.from_numpy(~near.reshape(N, -1).any(1))
    assert int((~keep).sum()) <= 4, "choose other boxes: samples of more than 4 rays sit on a face at some stage of the walk"
    return keep
