"""What the tests of the edited-scene surface outputs share: the fp64 reference of the gradient of the edited density, the
programs the kernel tests walk, the rows a comparison leaves out, and the G27 scene's boxes for the end-to-end tests.  Test infrastructure
only, not a test module.

The reference, as the issue fixes it: the walk of ``EditProgram.jacobians`` (fp64) gives, per world point p, the point p' = J p + b at which
the field is looked up, the chain J = M_{i_h} ... M_{i_1} and the state byte; ``surface_cases.grad_reference`` gives the gradient g_n of the
unedited raw density at the normalised p'; g' = g_n * 2 / extent is its world gradient and J^T g' the world gradient of the edited density.
A killed row is all zeros.
"""
import numpy as np

import surface_cases as sc
from contrastive_lift_amd import edit as ed
from oracle import field as fld

import torch


def normalise(p, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (np.asarray(p, np.float64) - lo) * (2.0 / (hi - lo)) - 1.0


def reference(P, prog, pts, lo, hi, shift):
    """fp64 -> dict(g (n, 3) world gradient of the edited raw density, raw (n,) the raw density at the looked-up point, bound (n, 3) =
    |J|^T |g'| (what a relative tolerance on g' becomes once a rotation mixes its components), xn (n, 3) looked-up normalised points,
    state (n,) uint8, killed (n,) bool, hops (n,) int).  Killed rows: g = raw = bound = 0."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    src, J, state = prog.jacobians(np.asarray(pts, np.float64))
    xn = normalise(src, lo, hi)
    g_n, raw = sc.grad_reference(P, xn, shift)
    gw = g_n * (2.0 / (hi - lo))[None]
    g = np.einsum("nji,nj->ni", J, gw)
    bound = np.einsum("nji,nj->ni", np.abs(J), np.abs(gw))
    killed = (state & ed.STATE_KILLED) != 0
    g[killed], bound[killed], raw = 0.0, 0.0, np.where(killed, 0.0, raw)
    return dict(g=g, raw=raw, bound=bound, xn=xn, state=state, killed=killed, hops=(state & ed.STATE_REMAPS).astype(np.int64))


def edited_density(P, prog, pts, lo, hi, shift):
    """fp64 raw density of the edited scene at world points: the field at the looked-up point, 0 where killed."""
    src, _, state = prog.jacobians(np.asarray(pts, np.float64))
    P64 = {k: v.double() for k, v in P.items() if k.startswith("density_")}
    raw = fld.density_raw(P64, torch.from_numpy(normalise(src, lo, hi)), float(shift), explicit=True).numpy()
    return np.where((state & ed.STATE_KILLED) != 0, 0.0, raw)


def face_distance(prog, pts):
    """(n,) fp64: the smallest distance of a point, at the position it has when edit i tests it (a killed point is tested no further), to a
    face plane of src_i or dst_i, over the whole walk -- within round-off of a face two classifications may disagree."""
    p = np.array(pts, dtype=np.float64)
    dist = np.full(p.shape[0], np.inf)
    dead = np.zeros(p.shape[0], dtype=bool)
    for e in reversed(list(prog)):
        for box in (e.src, e.dst):
            q = box.local(p)
            d = np.minimum(np.abs(q - box.lo), np.abs(q - box.hi)).min(1)
            dist = np.where(dead, dist, np.minimum(dist, d))
        dead |= e.killed(p)
        if e.mode >= ed.DUPLICATE:
            mov = ~dead & e.dst.contains(p)
            p[mov] = p[mov] @ e.M.T + e.t
    return dist


def left_out(ref, prog, pts, res):
    """(n,) bool: rows a device comparison leaves out -- within 1e-4 of a texel line at the looked-up position (rows that are looked up at
    all), or within 1e-5 of a box face at some stage of the walk."""
    return (~ref["killed"] & sc.near_texel_line(ref["xn"], res)) | (face_distance(prog, pts) < 1e-5)


# ----------------------------------------------------------------------------- the programs of the kernel tests
def _rot(rx, ry, rz):
    return ed.rotation_from_euler_deg(np.rad2deg(rx), np.rad2deg(ry), np.rad2deg(rz))


def programs(lo, hi):
    """name -> EditProgram, boxes placed in fractions of the box ``[lo, hi]``: the four modes alone, three mixed edits, the full eight with
    one object moved three times (rows with 0, 1, 2 and 3 remaps), a reference-faithful manipulate with a rotation (no rigid motion), a
    map that is no rotation at all (scale and shear) and a program that kills every point of 1.2 x the box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, u = (lo + hi) / 2, hi - lo

    def box(f, hs=0.14, R=None):
        return ed.EditBox(np.eye(3) if R is None else R, c + np.asarray(f) * u, -hs * u, hs * u)

    A, B = box((-0.35, -0.35, -0.3), R=_rot(0.0, 0.0, 0.3)), box((-0.3, 0.3, 0.3))
    out = {
        "delete": [ed.delete(box((-0.1, 0.1, 0.0), hs=0.3))],
        "extract": [ed.extract(box((0.05, -0.05, 0.0), hs=0.45, R=_rot(0.1, 0.0, 0.2)))],
        # (the source box reaches out of the aabb: some remapped points read padding)
        "copy": [ed.copy(box((-0.42, -0.15, 0.1), hs=0.2), np.array([0.55, 0.2, -0.15]) * u, _rot(0.2, -0.3, 0.5))],
        "move": [ed.move(box((-0.2, -0.15, 0.1), hs=0.2), np.array([0.4, 0.25, -0.1]) * u, _rot(0.0, 0.0, np.pi / 4))],
    }
    m = ed.move(box((-0.2, -0.2, 0.0), hs=0.2), np.array([0.45, 0.3, 0.1]) * u, _rot(0.3, 0.2, -0.6))
    out["mixed3"] = [ed.delete(box((0.3, -0.3, -0.2), hs=0.18)), m, ed.copy(m.dst, np.array([-0.1, 0.0, -0.3]) * u, _rot(0.0, 0.4, 0.0))]
    e1 = ed.move(A, np.array([0.35, 0.0, 0.0]) * u, _rot(0.0, 0.0, np.pi / 6))
    e2 = ed.copy(e1.dst, np.array([0.0, 0.0, 0.6]) * u, _rot(0.2, 0.1, -0.4))
    e3 = ed.move(e1.dst, np.array([0.35, 0.0, 0.0]) * u, None)
    e4 = ed.move(e3.dst, np.array([0.0, 0.4, 0.0]) * u, _rot(-0.3, 0.5, 0.2))
    e5 = ed.copy(B, np.array([0.4, 0.05, 0.0]) * u, _rot(0.0, 0.0, np.pi / 2))
    out["full8"] = [e1, e2, e3, e4, e5, ed.delete(box((-0.3, 0.3, -0.3))), ed.extract(box((0.0, 0.0, 0.0), hs=0.55)),
                    ed.delete(box((0.4, 0.4, 0.35), hs=0.12))]
    ref_box = {"extent": 0.5 * u, "position": c + np.array([-0.15, -0.1, 0.05]) * u, "orientation": _rot(0.0, 0.0, 0.25)}
    out["nonrigid"] = [ed.reference_manipulate(ref_box, np.array([0.3, 0.2, -0.1]) * u, _rot(0.2, -0.1, 0.6))]
    shear = np.array([[1.3, 0.4, 0.0], [-0.2, 0.8, 0.3], [0.1, 0.0, 1.1]])
    dst = box((0.2, 0.1, -0.1), hs=0.25, R=_rot(0.0, 0.3, 0.0))
    out["sheared"] = [ed.Edit(ed.MANIPULATE, box((-0.25, -0.2, 0.15), hs=0.2), dst, shear, c + np.array([-0.25, -0.2, 0.15]) * u - shear @ dst.centre)]
    # (the walk meets the copy first: some rows are remapped and then killed)
    out["kill_all"] = [ed.delete(box((0.0, 0.0, 0.0), hs=0.7)), ed.copy(box((0.0, 0.0, 0.2), hs=0.2), np.array([0.1, 0.1, -0.3]) * u, None)]
    return {k: ed.EditProgram(v) for k, v in out.items()}


POINT_SEED = 2024                                            # of the kernel tests' 4097 points (checked on the CPU: tests/test_edit_surface_host.py)


def world_points(n, lo, hi, seed):
    """(n, 3) fp32 world points uniform in 1.2 x the box: some points, and some remapped ones, read padding."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, u = (lo + hi) / 2, hi - lo
    return (c + 0.6 * u * np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))).astype(np.float32)


# ----------------------------------------------------------------------------- the G27 blob scene, end to end
# The blob of tests/test_gpu_surface.py's scene sits in the middle of the box, a Gaussian of width 0.3 in normalised units, over a floor
# softplus(-3) = 0.049 that the field has everywhere.  BLOB_HALF, the box of the copy and the move, is the blob's core out to 0.5 normalised
# units: as large as a box can be whose image under the move (a 45 degree yaw and MOVE_T) still lies inside the aabb.  DELETE_HALF is
# the blob out to 0.8 normalised units: what is left outside it (the floor and the Gaussian's tail) gathers an opacity of at most 0.41 along
# any of the scene's rays, so no ray loses half its transmittance.  EMPTY_BOX sits in a corner of the aabb that no sample comes near (0.12).
BLOB_CENTRE = np.array([-0.05, 0.0, 0.05])
BLOB_HALF = 0.5 * np.array([0.85, 0.7, 0.55])
DELETE_HALF = 0.8 * np.array([0.85, 0.7, 0.55])
EMPTY_CENTRE, EMPTY_HALF = np.array([0.71, 0.61, -0.41]), np.array([0.08, 0.08, 0.08])
MOVE_T = np.array([0.29, 0.12, 0.0])
MOVE_R = ed.rotation_from_euler_deg(0.0, 0.0, 45.0)


def blob_box(half=BLOB_HALF):
    return ed.EditBox(np.eye(3), BLOB_CENTRE, -half, half)


def empty_box():
    return ed.EditBox(np.eye(3), EMPTY_CENTRE, -EMPTY_HALF, EMPTY_HALF)


def moved_rays(rays):
    """The rays turned and shifted by the move x -> R (x - c) + c + t: aimed at the new position as they were at the old one."""
    r = np.asarray(rays, np.float64)
    o = (r[:, 0:3] - BLOB_CENTRE) @ MOVE_R.T + BLOB_CENTRE + MOVE_T
    d = r[:, 3:6] @ MOVE_R.T
    return np.concatenate([o, d, r[:, 6:8]], 1).astype(np.float32)


def sample_points(rays, lo, hi, step, S):
    """(N, S, 3) fp64 sample positions of the rays and (N, S) whether they lie inside the aabb (from the march's own fp32 distances)."""
    z = sc.sample_z(rays, lo, hi, step, S, None)[:, :S].astype(np.float64)
    r = np.asarray(rays, np.float64)
    p = r[:, None, 0:3] + z[..., None] * r[:, None, 3:6]
    return p, ((p >= np.asarray(lo, np.float64)) & (p <= np.asarray(hi, np.float64))).all(-1)
