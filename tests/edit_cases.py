"""Torch restatement of the scene-editing renders, composed from the CPU oracle (oracle.render / oracle.field), and the scenes the edit tests
share.  Test infrastructure only.

``reference_edit(op, ...)`` restates the reference's forward_delete / forward_extract / forward_duplicate / forward_manipulate
(model/renderer/panopli_tensoRF_renderer.py:303-623) line by line, box test included (split_points_minimal, :785-797: the fp32 inverse of
the box's 4 x 4 pose).  ``rigid_edit(op, ...)`` states ``copy`` / ``move`` from the motion of the object, x -> R (x - pos) + pos + t,
without going through contrastive_lift_amd.edit's resolved record.  Both return a ``Spec`` that ``render_edit`` renders: every head is
evaluated at every in-box sample (no weight threshold), sigma is zeroed after the density lookup.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from oracle import field as fld, params as op_, render as orender

RES, C_CLS, E_INST, SHIFT = (9, 13, 17), 4, 3, -3.0
AABB = torch.tensor([[-0.9, -0.7, -0.5], [0.8, 0.7, 0.6]])


def yaw(a):
    c, s = np.cos(a), np.sin(a)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def rot_xyz(rx, ry, rz):
    """Rz Ry Rx (radians), fp32."""
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return torch.tensor(yaw(rz).double().numpy() @ Ry @ Rx, dtype=torch.float32)


def golden_params(g):
    res = tuple(int(x) for x in g["res"])
    return op_.add_blob(op_.make_params(int(g["seed"]), res, int(g["C"]), int(g["E"])), res, 2.5, 0.45)


def golden_bbox(g):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g[k]))
    return {"extent": T("extent"), "position": T("position"), "orientation": T("orientation")}


def scene130():
    """The second scene: G6's field with 130 rays (not a multiple of 64) -- 122 through the box from three sides, 8 that miss it."""
    rng = np.random.default_rng(2511)
    P = op_.add_blob(op_.make_params(61, RES, C_CLS, E_INST), RES, 2.5, 0.45)
    n_hit, n_miss = 122, 8
    eyes = rng.standard_normal((n_hit, 3))
    eyes = 0.95 * eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
    target = rng.uniform(-0.35, 0.35, (n_hit, 3))
    d = target - eyes
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_miss = np.tile(np.array([[0.0, 0.0, -0.95]]), (n_miss, 1)) + rng.uniform(-0.02, 0.02, (n_miss, 3))
    d_miss = rng.standard_normal((n_miss, 3)) * 0.1 + np.array([1.0, 0.0, -0.3])          # away from the box
    d_miss /= np.linalg.norm(d_miss, axis=1, keepdims=True)
    o, d = np.concatenate([eyes, o_miss]), np.concatenate([d, d_miss])
    far = -(o * d).sum(1) + np.sqrt(np.maximum((o * d).sum(1) ** 2 - ((o * o).sum(1) - 1.0), 0.0))     # exit of the unit sphere
    rays = np.concatenate([o, d, np.full((o.shape[0], 1), 0.01), far[:, None]], 1).astype(np.float32)
    rays = torch.from_numpy(rays[rng.permutation(rays.shape[0])])
    return P, rays


@dataclass
class Spec:
    src: Optional[Callable]          # flat fp32 points (n, 3) -> bool (n,)
    dst: Optional[Callable]
    point: Optional[Callable]        # points inside dst -> where they are looked up
    direction: Optional[Callable]    # their view directions -> the ones the appearance MLP sees
    kill: Callable                   # (src, dst) -> bool (n,)


def split_points_minimal(xyz, extent, position, orientation):
    """renderer.py:785-797 for one box: q = (inverse of [[orientation, position], [0, 1]]) applied to the points; inside iff
    -extent / 2 <= q <= extent / 2."""
    pose = torch.eye(4)
    pose[:3, :3], pose[:3, 3] = orientation, position
    inv = torch.linalg.inv(pose)
    q = (inv @ torch.cat([xyz, torch.ones(xyz.shape[0], 1)], 1).T).T[:, :3]
    return ((q <= extent / 2) & (q >= -extent / 2)).all(-1)


def reference_edit(op, bbox, translation=None, rotation=None):
    ext, pos, O = bbox["extent"], bbox["position"], bbox["orientation"]
    src = lambda p: split_points_minimal(p, ext, pos, O)
    if op == "delete":                                                       # :305,346
        return Spec(src, None, None, None, lambda s, d: s)
    if op == "extract":                                                      # :381-383,423
        return Spec(src, None, None, None, lambda s, d: ~s)
    t, R = translation, rotation
    Rinv = torch.linalg.inv(R)
    turn = lambda v: (Rinv @ v.T).T                                          # :472,558
    if op == "duplicate":                                                    # :458,462 -- nothing is killed
        dst = lambda p: split_points_minimal(p, ext, R @ pos + t, R @ O)
        return Spec(None, dst, lambda p: p - t, turn, lambda s, d: torch.zeros_like(d))
    if op == "manipulate":                                                   # :541,548,594
        dst = lambda p: split_points_minimal(p, ext, pos + t, R @ O)
        return Spec(src, dst, lambda p: (R @ (p - pos).T).T + pos - t, turn, lambda s, d: s & ~d)
    raise ValueError(op)


def rigid_edit(op, axes, centre, lo, hi, translation, rotation):
    """copy / move of the content of the box {lo <= axes (p - centre) <= hi} (rows of ``axes`` are the box axes) under
    x -> R (x - centre) + centre + t: a point p of the moved box shows the field at the point that was carried there."""
    axes, centre, lo, hi, t, R = (x.to(torch.float32) for x in (axes, centre, lo, hi, translation, rotation))
    Rinv = torch.linalg.inv(R)

    def inside(p):
        q = (p - centre) @ axes.T
        return ((lo <= q) & (q <= hi)).all(-1)
    back = lambda p: (p - centre - t) @ Rinv.T + centre                      # where the content at p came from
    if op not in ("copy", "move"):
        raise ValueError(op)
    kill = (lambda s, d: s & ~d) if op == "move" else (lambda s, d: torch.zeros_like(d))
    return Spec(inside, lambda p: inside(back(p)), back, lambda v: v @ Rinv.T, kill)


def render_edit(P, rays, cfg, spec, white_bg):
    """One of the reference's edit forwards with the edit given as a ``Spec``.  Returns (rgb, sem, inst, depth) and the sigma array."""
    pts, z, inbox = orender.sample_along_rays(rays, cfg, None)               # mask_xyz BEFORE the remap (:304)
    N, S = z.shape
    flat = pts.reshape(-1, 3).clone()
    dirs = rays[:, None, 3:6].expand(N, S, 3).reshape(-1, 3).clone()
    src = spec.src(flat) if spec.src is not None else torch.zeros(N * S, dtype=torch.bool)
    dst = spec.dst(flat) if spec.dst is not None else torch.zeros(N * S, dtype=torch.bool)
    if bool(dst.any()):
        moved = spec.point(flat[dst])
        dirs[dst] = spec.direction(dirs[dst])
        flat[dst] = moved
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
    sigma[spec.kill(src, dst).reshape(N, S)] = 0                             # after the lookup (:346,423,594)
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
    return (rgb_map.clamp(0, 1), sem_map, inst_map, (w * z).sum(-1)), sigma
