"""What the tests of shaped edits share: programs whose edits carry random bit lattices, point sets that fill the small boxes,
the fp32 numpy restatement of the shaped walk (every operation rounded on its own, as the kernels do), the fp64 reference walk over the
fp32 records with the face rule extended to cell faces, and a plain loop for the packing rule.  Test infrastructure only, not a test module.

The shaped rule, for an edit with a shape: src = mode != DUPLICATE and p in src and bit(p); mov = mode >= DUPLICATE and p in dst and
bit(M p + t), the bit read in the SOURCE frame with a clamped cell index.  An edit without a shape keeps the box rule.
"""
import numpy as np

from contrastive_lift_amd import edit as ed

F32 = np.float32
FACE_EPS = 1e-5
KILLED = 0x80


# ----------------------------------------------------------------------------- programs and points
def with_shapes(prog, shapes):
    """The program with ``shapes[i]`` (an ``EditShape`` or None) on edit i."""
    return ed.EditProgram([e.with_shape(s) for e, s in zip(prog, shapes)])


def bernoulli_shapes(n, dims, p=0.5, seed=11):
    """n shapes of ``dims`` with independent Bernoulli(p) bits, one generator for all of them."""
    rng = np.random.default_rng(seed)
    return [ed.EditShape.from_flags(rng.random(dims) < p, backend="host") for _ in range(n)]


def box_points(prog, per_box=256, seed=7):
    """(n, 3) fp32 world points: per edit ``per_box`` uniform in its source box and ``per_box`` in its destination box, both grown by 10 % of
    their extent on every side -- the small boxes of the programs get rows a uniform cloud over the aabb would not give them."""
    rng = np.random.default_rng(seed)
    out = []
    for e in prog:
        for box in (e.src, e.dst):
            ext = box.hi - box.lo
            q = rng.uniform(box.lo - 0.1 * ext, box.hi + 0.1 * ext, (per_box, 3))
            out.append(q @ box.axes + box.centre)                     # the rows of axes are orthonormal: A^-1 = A^T
    return np.concatenate(out).astype(F32)


def unit_dirs(n, seed=1):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


# ----------------------------------------------------------------------------- the packing rule, as a loop
def pack_loop(flags, grow):
    """uint32 words of (G0, G1, G2) flags: bit = 1 iff a flag within Chebyshev distance ``grow`` is set, clipped at the border; x-major, bit
    lin & 31 of word lin >> 5.  Plain Python loops."""
    f = np.asarray(flags) != 0
    G = f.shape
    words = [0] * ((f.size + 31) // 32)
    for i0 in range(G[0]):
        for i1 in range(G[1]):
            for i2 in range(G[2]):
                nb = f[max(i0 - grow, 0):i0 + grow + 1, max(i1 - grow, 0):i1 + grow + 1, max(i2 - grow, 0):i2 + grow + 1]
                if nb.any():
                    lin = (i0 * G[1] + i1) * G[2] + i2
                    words[lin >> 5] |= 1 << (lin & 31)
    return np.asarray(words, dtype=np.uint64).astype(np.uint32)


# ----------------------------------------------------------------------------- fp32 restatement
def _f(a):
    return np.asarray(a, np.float64).astype(F32)


def _row3(a, v):
    """(n,) = (a0 v0 + a1 v1) + a2 v2, every multiply and add rounded on its own."""
    return ((a[0] * v[:, 0]).astype(F32) + (a[1] * v[:, 1]).astype(F32)).astype(F32) + (a[2] * v[:, 2]).astype(F32)


def _local32(box, p):
    A, c = _f(box.axes), _f(box.centre)
    d = (p - c[None]).astype(F32)
    return np.stack([_row3(A[i], d).astype(F32) for i in range(3)], 1)


def _in_box32(box, p):
    q, lo, hi = _local32(box, p), _f(box.lo), _f(box.hi)
    return ((lo[None] <= q) & (q <= hi[None])).all(1)


def _bit32(shape, box, x):
    """The kernel's membership: u = (q - lo) * inv_cell, one subtraction and one product, floor, clamp, the bit."""
    q, lo, inv = _local32(box, x), _f(box.lo), shape.inv_cell(box)
    lin = np.zeros(x.shape[0], np.int64)
    for a in range(3):
        u = ((q[:, a] - lo[a]).astype(F32) * inv[a]).astype(F32)
        lin = lin * shape.dims[a] + np.clip(np.floor(u), 0, shape.dims[a] - 1).astype(np.int64)
    return ((shape.words[lin >> 5] >> (lin & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def _remap32(M, t, p):
    return np.stack([(_row3(M[j], p).astype(F32) + t[j]).astype(F32) for j in range(3)], 1)


def walk32(prog, points, dirs=None):
    """fp32, operation for operation: (looked-up points (n, 3), directions or None, state (n,) uint8) of fp32 world points under the
    program's fp32 records and shapes."""
    p = np.array(points, F32)
    d = None if dirs is None else np.array(dirs, F32)
    n = p.shape[0]
    dead, hops = np.zeros(n, bool), np.zeros(n, np.uint8)
    for e in reversed(list(prog)):
        M, t, Dinv = _f(e.M), _f(e.t), _f(e.dir_inv)
        src = _in_box32(e.src, p) if e.mode != ed.DUPLICATE else np.zeros(n, bool)
        mov = _in_box32(e.dst, p) if e.mode >= ed.DUPLICATE else np.zeros(n, bool)
        if e.shape is not None:
            src[src] = _bit32(e.shape, e.src, p[src])
            mov[mov] = _bit32(e.shape, e.src, _remap32(M, t, p[mov]))
        kill = src if e.mode == ed.DELETE else ~src if e.mode == ed.EXTRACT else (src & ~mov) if e.mode == ed.MANIPULATE else np.zeros(n, bool)
        go = mov & ~dead
        if go.any():
            if d is not None:
                d[go] = np.stack([_row3(Dinv[j], d[go]).astype(F32) for j in range(3)], 1)
            p[go] = _remap32(M, t, p[go])
            hops[go] += 1
        dead |= kill
    return p, d, hops | np.where(dead, np.uint8(KILLED), np.uint8(0))


# ----------------------------------------------------------------------------- fp64 reference over the fp32 records, with the face rule
def _box64(box):
    return _f(box.axes).astype(np.float64), _f(box.centre).astype(np.float64), _f(box.lo).astype(np.float64), _f(box.hi).astype(np.float64)


def _q64(box, p):
    return (p - box[1]) @ box[0].T


def _inside64(box, p):
    q = _q64(box, p)
    return np.all((box[2] <= q) & (q <= box[3]), axis=-1)


def _near_box(box, p):
    q = _q64(box, p)
    return ((np.abs(q - box[2]) < FACE_EPS) | (np.abs(q - box[3]) < FACE_EPS)).any(1)


def _cells64(shape, box, x):
    """(bit, near a cell face) of fp64 points in the lattice over the fp32 box, the scale G / (hi - lo) in fp64 (the kernel's fp32 scale is
    off by 2^-24 relative: that moves a cell face by less than 1e-7 of the box's extent, far inside the band)."""
    G = np.asarray(shape.dims, np.float64)
    u = (_q64(box, x) - box[2]) * (G / (box[3] - box[2]))
    h = (box[3] - box[2]) / G
    near = (np.abs(u - np.rint(u)) * h < FACE_EPS).any(1)
    i = np.clip(np.floor(u), 0, G - 1).astype(np.int64)
    lin = (i[:, 0] * shape.dims[1] + i[:, 1]) * shape.dims[2] + i[:, 2]
    return ((shape.words[lin >> 5] >> (lin & 31).astype(np.uint32)) & np.uint32(1)).astype(bool), near


def ref_walk(prog, points, dirs=None):
    """fp64 walk over the fp32 records and shapes -> dict(p, d, hops, killed, state, keep).  keep: the rows the face rule does not leave out --
    a row is left out if, at a stage where an edit tests it (a killed row is tested no further), it lies within 1e-5 of a face plane of the
    edit's source or destination box, or within 1e-5 of a cell face of a lattice that stage reads for it (the source lattice at p for a
    row inside the source box, at M p + t for a row inside the destination box)."""
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    d = None if dirs is None else np.array(dirs, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    dead, near, hops = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, np.int64)
    for e in reversed(list(prog)):
        src_b, dst_b = _box64(e.src), _box64(e.dst)
        M, t, Dinv = _f(e.M).astype(np.float64), _f(e.t).astype(np.float64), _f(e.dir_inv).astype(np.float64)
        near |= ~dead & (_near_box(src_b, p) | _near_box(dst_b, p))
        in_src = (e.mode != ed.DUPLICATE) & _inside64(src_b, p)
        in_dst = (e.mode >= ed.DUPLICATE) & _inside64(dst_b, p)
        if e.shape is not None:
            for mask, at in ((in_src, p), (in_dst, p @ M.T + t)):
                bit, close = _cells64(e.shape, src_b, at)
                near |= ~dead & mask & close
                mask &= bit
        kill = {0: in_src, 1: ~in_src, 2: np.zeros(n, bool), 3: in_src & ~in_dst}[e.mode]
        mov = ~dead & in_dst
        p[mov] = p[mov] @ M.T + t
        if d is not None:
            d[mov] = d[mov] @ Dinv.T
        hops[mov] += 1
        dead |= kill
    state = (hops | np.where(dead, KILLED, 0)).astype(np.uint8)
    return dict(p=p, d=d, hops=hops, killed=dead, state=state, keep=~near)


def brute_walk(prog, points):
    """The fp64 host rule point by point, in plain Python over ``Edit`` objects (fp64 boxes and maps): -> (points, state)."""
    out_p, out_s = [], []
    for x in np.asarray(points, np.float64):
        p, dead, hops = x.copy(), False, 0
        for e in reversed(list(prog)):
            def bit(y):
                if e.shape is None:
                    return True
                G = e.shape.dims
                u = (e.src.axes @ (y - e.src.centre) - e.src.lo) * (np.asarray(G, np.float64) / (e.src.hi - e.src.lo))
                i = [min(G[a] - 1, max(0, int(np.floor(u[a])))) for a in range(3)]
                lin = (i[0] * G[1] + i[1]) * G[2] + i[2]
                return bool((int(e.shape.words[lin >> 5]) >> (lin & 31)) & 1)
            src = e.mode != ed.DUPLICATE and bool(e.src.contains(p[None])[0]) and bit(p)
            mov = e.mode >= ed.DUPLICATE and bool(e.dst.contains(p[None])[0]) and bit(e.M @ p + e.t)
            kill = {ed.DELETE: src, ed.EXTRACT: not src, ed.DUPLICATE: False, ed.MANIPULATE: src and not mov}[e.mode]
            if not dead and mov:
                p, hops = e.M @ p + e.t, hops + 1
            dead = dead or kill
        out_p.append(p)
        out_s.append(hops | (KILLED if dead else 0))
    return np.asarray(out_p), np.asarray(out_s, np.uint8)


# ----------------------------------------------------------------------------- the render oracle's route
def shaped_spec(spec, e):
    """``spec`` (an ``edit_cases.Spec`` of the box edit) narrowed by the shape of ``e`` (an ``edit.Edit``): the source test also needs the
    bit of p, the destination test the bit of the point the content came from, both from the fp64 host rule (``EditShape.bit``)."""
    import torch
    import edit_cases as ec
    if e.shape is None:
        return spec
    bit = lambda p: torch.from_numpy(e.shape.bit(e.src, p.double().numpy()))
    src = None if spec.src is None else (lambda p: spec.src(p) & bit(p))
    dst = None if spec.dst is None else (lambda p: spec.dst(p) & bit(spec.point(p)))
    return ec.Spec(src, dst, spec.point, spec.direction, spec.kill)


def rays_off_all_faces(rays, cfg, prog, cap):
    """(N,) bool, fp64: ``edit_program_cases.rays_off_all_faces`` with the face rule of ``ref_walk`` (box faces and the cell faces of the
    lattices a stage reads): a ray is left out when one of its samples is.  At most ``cap`` rays may be left out -- asserted here, from
    the fp64 walk alone."""
    import torch
    from oracle import render as orender
    N = rays.shape[0]
    p = orender.sample_along_rays(rays, cfg, None)[0].reshape(-1, 3).double().numpy()
    keep = torch.from_numpy(ref_walk(prog, p)["keep"].reshape(N, -1).all(1))
    assert int((~keep).sum()) <= cap, f"choose other boxes or lattices: samples of {int((~keep).sum())} rays sit on a face (cap {cap})"
    return keep
