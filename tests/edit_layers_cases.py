"""What the tests of the layers of an edited scene share: the G27 blob scene with its boxes, programs and rays, the fp32
numpy restatement of the origin rule of clift_edit_list_active_origin (every operation rounded on its own, as in edit_program_cases.walk),
the retargeting rule, made-up alpha-lists and the CPU oracle's per-sample alphas and weights under a program.  Test infrastructure only,
not a test module.

The origin rule: walking the program backwards, i = n .. 1, the 1-based position of the FIRST edit met that remaps the sample and is a
DUPLICATE; 0 if the walk meets none; a killed sample has stopped.
"""
import numpy as np
import torch

import edit_surface_cases as esc
import surface_cases as sc
from contrastive_lift_amd import edit as ed
from oracle import field as fld, params as op, render as orender

F32 = np.float32
N_BLOB, N_FRONT = 130, 64
CORE_HALF = 0.16
COPY_T, MOVE_T, COPY2_T = (0.0, 0.45, 0.0), (0.0, -0.9, 0.0), (0.45, 0.0, 0.0)


# ----------------------------------------------------------------------------- the scene
def boxes():
    """core: the blob's core; cp: a copy of it at +0.45 y; mv: that copy moved to -0.45 y; cp2: a copy of the copy at +0.45 x; mv_only:
    the core itself moved to +0.45 y (a program without a copy)."""
    half = np.full(3, CORE_HALF)
    core = ed.EditBox(np.eye(3), esc.BLOB_CENTRE, -half, half)
    cp = ed.copy(core, COPY_T)
    at_copy = ed.EditBox(np.eye(3), cp.dst.centre, -half, half)
    return dict(core=core, cp=cp, mv=ed.move(at_copy, MOVE_T), cp2=ed.copy(at_copy, COPY2_T), mv_only=ed.move(core, COPY_T))


def programs():
    b = boxes()
    return {"cp": ed.EditProgram([b["cp"]]), "cp_mv": ed.EditProgram([b["cp"], b["mv"]]), "cp_cp2": ed.EditProgram([b["cp"], b["cp2"]]),
            "mv_only": ed.EditProgram([b["mv_only"]])}


def blob_rays():
    """The 130 rays of tests/test_gpu_layers.py: 120 from a sphere of radius 0.9 aimed near the blob, 10 that start below the box and point
    away from it."""
    rng = np.random.default_rng(27)
    eyes = rng.standard_normal((120, 3))
    eyes = 0.9 * eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
    target = np.array([[-0.05, 0.0, 0.05]]) + rng.uniform(-0.08, 0.08, (120, 3))
    d = target - eyes
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_miss = np.array([[0.0, 0.0, -0.95]]) + rng.uniform(-0.02, 0.02, (10, 3))
    d_miss = rng.standard_normal((10, 3)) * 0.1 + np.array([1.0, 0.0, -0.3])
    d_miss /= np.linalg.norm(d_miss, axis=1, keepdims=True)
    o, d = np.concatenate([eyes, o_miss]), np.concatenate([d, d_miss])
    return torch.from_numpy(np.concatenate([o, d, np.full((N_BLOB, 1), 0.01), np.full((N_BLOB, 1), 4.0)], 1).astype(F32))


def front_rays():
    """64 rays that look at the blob's core from +y, through the place of the copy."""
    rng = np.random.default_rng(5)
    tgt = esc.BLOB_CENTRE[None] + rng.uniform(-0.06, 0.06, (N_FRONT, 3))
    eye = np.clip(esc.BLOB_CENTRE[None] + 0.93 * np.array([[0.0, 1.0, 0.0]]) + rng.uniform(-0.03, 0.03, (N_FRONT, 3)), -0.98, 0.98)
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(np.concatenate([eye, d, np.full((N_FRONT, 1), 0.01), np.full((N_FRONT, 1), 4.0)], 1).astype(F32))


def side_rays():
    """16 rays that cross the place of the MOVED copy (mv.dst) along +x, clear of the blob: on them the copy is the only opaque thing."""
    rng = np.random.default_rng(9)
    c = boxes()["mv"].dst.centre
    n = 16
    tgt = c[None] + rng.uniform(-0.08, 0.08, (n, 3))
    eye = np.clip(c[None] + np.array([[-0.8, 0.0, 0.0]]) + rng.uniform(-0.03, 0.03, (n, 3)), -0.98, 0.98)
    eye[:, 0] = -0.88
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(np.concatenate([eye, d, np.full((n, 1), 0.01), np.full((n, 1), 4.0)], 1).astype(F32))


def scene_rays():
    return torch.cat([blob_rays(), front_rays()], 0)


def oracle_scene(g):
    """(P, cfg, res, C, E, shift, aabb) of the G27 golden ``g``: the blob field and the oracle's render settings at step ratio 0.25."""
    res = tuple(int(x) for x in g["res"])
    aabb, shift, C_, E = torch.from_numpy(np.asarray(g["aabb"])).float(), float(g["shift"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    return P, orender.RenderCfg(aabb, res, step_ratio=0.25, density_shift=shift), res, C_, E, shift, aabb


def host_walk(rays, cfg, prog):
    """The fp64 walk over every sample of the rays: dict(points (N S, 3) fp64 world, src, origin, state, inbox (N, S) bool, N, S)."""
    pts, z, inbox = orender.sample_along_rays(rays, cfg, None)
    N, S = z.shape
    flat = pts.reshape(-1, 3).double().numpy()
    src, origin, state = prog.origins(flat)
    return dict(points=flat, src=src, origin=origin, state=state, inbox=inbox.numpy(), z=z, N=N, S=S)


def untouched_rays(walk):
    """(N,) bool: no in-aabb sample of the ray is remapped or killed."""
    return ~((walk["state"].reshape(walk["N"], walk["S"]) != 0) & walk["inbox"]).any(1)


def oracle_weights(P, cfg, walk, lo, hi):
    """fp32 oracle: (alpha, w) (N, S) of the scene the walk describes -- the density at the looked-up point of every in-aabb sample, 0 where
    killed."""
    N, S = walk["N"], walk["S"]
    xn = torch.from_numpy(esc.normalise(walk["src"], lo, hi)).float()
    sig = torch.zeros(N * S)
    m = torch.from_numpy(walk["inbox"].reshape(-1))
    sig[m] = fld.density(P, xn[m], cfg.density_shift)
    sig[torch.from_numpy((walk["state"] & ed.STATE_KILLED) != 0)] = 0
    dists, _ = orender._deltas_midpoints(walk["z"])
    a, w, _ = orender.sigma_to_weights(sig.reshape(N, S), dists * cfg.distance_scale)
    return a.double().numpy(), w.double().numpy()


# ----------------------------------------------------------------------------- fp32 restatements
def world_samples_np(lo, hi, step, rays, act_idx, S):
    """(M, 3) fp32 world points of list entries, o + d z with the march's own z (surface_cases.sample_z) and separately rounded ops: the
    bits the kernels form (the helper of tests/test_gpu_edit_surface.py)."""
    rays = np.asarray(rays, F32)
    z = sc.sample_z(rays, lo, hi, step, S, None)
    sid = np.asarray(act_idx).astype(np.int64)
    r, k = sid // S, sid % S
    zz = z[r, k]
    return (rays[r, 0:3] + (rays[r, 3:6] * zz[:, None]).astype(F32)).astype(F32)


def _f(a):
    return np.asarray(a, np.float64).astype(F32)


def _row3(a, v):
    """(n,) = (a0 v0 + a1 v1) + a2 v2, every multiply and add rounded on its own."""
    return ((a[0] * v[:, 0]).astype(F32) + (a[1] * v[:, 1]).astype(F32)).astype(F32) + (a[2] * v[:, 2]).astype(F32)


def _in_box(box, p):
    A, c, lo, hi = _f(box.axes), _f(box.centre), _f(box.lo), _f(box.hi)
    d = (p - c[None]).astype(F32)
    inside = np.ones(p.shape[0], bool)
    for i in range(3):
        q = _row3(A[i], d).astype(F32)
        inside &= (lo[i] <= q) & (q <= hi[i])
    return inside


def origin_restatement(prog, world):
    """fp32: (looked-up points (n, 3), origin (n,) uint8, state (n,) uint8) of fp32 world points under the program's fp32 records."""
    p = np.array(world, F32)
    n = p.shape[0]
    dead, hops, origin = np.zeros(n, bool), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(len(prog), 0, -1):
        e = prog[i - 1]
        src = _in_box(e.src, p) if e.mode != ed.DUPLICATE else np.zeros(n, bool)
        mov = _in_box(e.dst, p) if e.mode >= ed.DUPLICATE else np.zeros(n, bool)
        kill = src if e.mode == ed.DELETE else ~src if e.mode == ed.EXTRACT else (src & ~mov) if e.mode == ed.MANIPULATE else np.zeros(n, bool)
        go = mov & ~dead
        if go.any():
            M, t = _f(e.M), _f(e.t)
            q = np.stack([(_row3(M[j], p[go]).astype(F32) + t[j]).astype(F32) for j in range(3)], 1)
            p[go] = q
            hops[go] += 1
            if e.mode == ed.DUPLICATE:
                origin[go & (origin == 0)] = i
        dead |= kill
    return p, origin, hops | np.where(dead, np.uint8(ed.STATE_KILLED), np.uint8(0))


def retarget_restatement(base_slots, origin, K, copy_edit):
    """The rule of ``layers.retarget`` row by row: origin i > 0 and a base slot in [0, K) -> K + (the rank of edit i among the copies)."""
    col = {int(e) + 1: K + j for j, e in enumerate(copy_edit)}
    out = np.asarray(base_slots, np.int32).copy()
    for r in range(out.shape[0]):
        if origin[r] > 0 and 0 <= out[r] < K:
            out[r] = col[int(origin[r])]
    return out


def made_up_list(M, N, S, seed):
    """M list entries of several rays, ascending: ids in [0, N S)."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(N * S, M, replace=False)).astype(np.int32)
