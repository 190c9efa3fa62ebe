"""What the edited-mesh tests share: the two programs, the fp64 reference walk over the fp32 records, the face rule, the point sets.  Test
infrastructure only, not a test module.

The reference walk works on the records AS ROUNDED TO fp32 (``Edit.record()``), in fp64: the rounding of the record drops out of every
comparison with the device walk, what is left is the device's own fp32 arithmetic.

The face rule (that of ``edit_program_cases.rays_off_all_faces``): two fp32 classifications may disagree within 1e-5 of a box face, so a
row is left out when, at the position it has when edit i tests it (a killed row is tested no further), it lies within 1e-5 of a face
plane of src_i or dst_i.
"""
import numpy as np
import torch

import edit_cases as ec

FACE_EPS = 1e-5
KILLED = 0x80


def chain_program():
    """move A, delete B, copy of A's destination: up to 2 remaps."""
    from test_gpu_edit_program import chain_case
    return chain_case()[0]


def eight_program():
    """Eight edits over ``small_boxes()``: even i a turned move, i % 4 == 1 a turned copy, the rest deletes."""
    from contrastive_lift_amd import edit
    from test_gpu_edit_program import small_boxes
    out = []
    for i, b in enumerate(small_boxes()):
        if i % 2 == 0:
            out.append(edit.move(b, [0.05, 0.04, -0.03], ec.rot_xyz(0.1 * i, 0.2, -0.1 * i)))
        elif i % 4 == 1:
            out.append(edit.copy(b, [0.1, -0.05, 0.06], ec.rot_xyz(0.3, 0.1 * i, 0.0)))
        else:
            out.append(edit.delete(b))
    return edit.EditProgram(out)


def program(name):
    return {"chain": chain_program, "eight": eight_program}[name]()


def _box64(rec):
    f = lambda a, shape: np.asarray(list(a), dtype=np.float32).astype(np.float64).reshape(shape)
    return f(rec.axes, (3, 3)), f(rec.centre, (3,)), f(rec.lo, (3,)), f(rec.hi, (3,))


def _local(box, p):
    A, c, _, _ = box
    return (p - c) @ A.T


def _inside(box, p):
    q = _local(box, p)
    return np.all((box[2] <= q) & (q <= box[3]), axis=-1)


def _near(box, p):
    q = _local(box, p)
    return ((np.abs(q - box[2]) < FACE_EPS) | (np.abs(q - box[3]) < FACE_EPS)).any(1)


def ref_walk(prog, points, dirs=None):
    """fp64 walk over the fp32 records -> dict(p, d (None without dirs), hops (n) int, killed (n) bool, state (n) uint8, keep (n) bool: the
    rows the face rule does not leave out)."""
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    d = None if dirs is None else np.array(dirs, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    dead, near, hops = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, np.int64)
    f = lambda a, shape: np.asarray(list(a), dtype=np.float32).astype(np.float64).reshape(shape)
    for e in reversed(list(prog)):
        rec = e.record()
        src, dst = _box64(rec.src), _box64(rec.dst)
        M, t, Dinv = f(rec.map_m, (3, 3)), f(rec.map_t, (3,)), f(rec.dir_inv, (3, 3))
        near |= ~dead & (_near(src, p) | _near(dst, p))
        in_src = (rec.mode != 2) & _inside(src, p)
        in_dst = (rec.mode >= 2) & _inside(dst, p)
        kill = {0: in_src, 1: ~in_src, 2: np.zeros(n, bool), 3: in_src & ~in_dst}[rec.mode]
        mov = ~dead & in_dst
        p[mov] = p[mov] @ M.T + t
        if d is not None:
            d[mov] = d[mov] @ Dinv.T
        hops[mov] += 1
        dead |= kill
    state = (hops | np.where(dead, KILLED, 0)).astype(np.uint8)
    return dict(p=p, d=d, hops=hops, killed=dead, state=state, keep=~near)


def cloud_points(n=4096):
    """(points, unit directions) fp32: points uniform over the aabb grown by 0.1, directions uniform on the sphere."""
    lo, hi = ec.AABB[0].double().numpy(), ec.AABB[1].double().numpy()
    pts = np.random.default_rng(0).uniform(lo - 0.1, hi + 0.1, (n, 3)).astype(np.float32)
    d = np.random.default_rng(1).standard_normal((n, 3))
    return pts, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def lattice_points(upsample, aabb=None, res=None):
    """The lattice points of ``get_dense_sigma(m, upsample)`` as the kernel forms them: fp32, lo (1 - s) + hi s with s = torch.linspace(0, 1,
    n), x-major.  -> ((N, 3) fp32 numpy, (n0, n1, n2))."""
    aabb = ec.AABB if aabb is None else aabb
    n = [int(r) * int(upsample) for r in (ec.RES if res is None else res)]
    ticks = []
    for a in range(3):
        s = torch.linspace(0, 1, n[a])
        ticks.append(aabb[0][a] * (1 - s) + aabb[1][a] * s)
    g = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1).reshape(-1, 3)
    return g.numpy().astype(np.float32), tuple(n)


def normalise64(p, aabb=None):
    """fp64 normalised coordinates of world points in the aabb."""
    aabb = ec.AABB if aabb is None else aabb
    lo, hi = aabb[0].double().numpy(), aabb[1].double().numpy()
    return (np.asarray(p, np.float64) - lo) * (2.0 / (hi - lo)) - 1.0


def cell_diagonal(shape, aabb=None):
    aabb = ec.AABB if aabb is None else aabb
    ext = (aabb[1] - aabb[0]).double().numpy()
    return float(np.linalg.norm(ext / (np.asarray(shape, np.float64) - 1.0)))


def box_depth(box, p):
    """How deep world points lie inside an ``EditBox`` (fp64): the smallest distance to a face plane for a point inside, negative =
    that far outside along the worst axis (a lower bound of the Euclidean distance to the box: the axes are orthonormal)."""
    q = box.local(np.asarray(p, np.float64))
    return np.minimum(q - box.lo, box.hi - q).min(1)
