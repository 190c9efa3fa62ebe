"""CPU restatement of the device iso-surface extractor (csrc/isosurface.hip) in numpy, written from the rules of DESIGN.md 6d, plus the
scalar fields and the mesh invariants the tests use.  Not a test module.

Rules restated here (the kernels must agree with every one of them):
  * lattice (n0, n1, n2), x-major: linear_index(i, j, k) = (i * n1 + j) * n2 + k; "inside" is vol >= level, NaN is outside;
  * cell (i, j, k) splits into 6 tetrahedra, one per permutation (a, b, c) of the axes IN LEXICOGRAPHIC ORDER:
    v0 = c000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = c111 (the Kuhn split);
  * 7 edge classes per lattice point, offsets CLASS_OFFSETS in that order; an edge is owned by its lower endpoint, exists when both
    endpoints are lattice points, and carries one vertex when its endpoints classify differently;
  * vertex position p = pa + t (pb - pa), t = (level - va) / (vb - va) clamped to [0, 1] (fmax / fmin: a NaN t becomes 0), fp32, one
    rounding per operation, a = the owner;
  * vertex index = rank of the key 7 * linear_index(owner) + class among the active edges;
  * 1 or 3 inside corners: one triangle; 2: a quad, split along the diagonal through its smallest vertex index: with the quad's cycle
    rotated so that the smallest index comes first, (q0, q1, q2) then (q0, q2, q3);
  * winding: normal from inside to outside.  HERE it is decided geometrically on the unit cell from the MIDPOINTS of the crossed edges
    (never from the computed vertices), for every permutation and every case separately -- the kernels use one table for the identity
    permutation and reverse it for odd permutations, so the two derivations are independent;
  * faces in scan order (cell by linear index, tetrahedron, triangle).
"""
import itertools

import numpy as np

CLASS_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
CLASS_OF_OFFSET = {o: c for c, o in enumerate(CLASS_OFFSETS)}
PERMS = tuple(itertools.permutations(range(3)))            # lexicographic: the tetrahedron order inside a cell
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def tet_corners(perm):
    """Corner offsets (v0, v1, v2, v3) of the tetrahedron of one axis permutation."""
    a, b, _ = perm
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return (0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1)


def tet_polygon(perm, inside):
    """The crossed edges of one tetrahedron as a cycle of (lower corner, upper corner) local vertex pairs, wound so that the normal of
    the polygon through the edge MIDPOINTS points from the inside corners to the outside corners.  ``inside``: 4 bools.  [] when the
    tetrahedron is not crossed."""
    ins = [v for v in range(4) if inside[v]]
    outs = [v for v in range(4) if not inside[v]]
    if not ins or not outs:
        return []
    e = lambda u, v: (min(u, v), max(u, v))
    if len(ins) == 1:
        cyc = [e(ins[0], o) for o in outs]
    elif len(outs) == 1:
        cyc = [e(i, outs[0]) for i in ins]
    else:                                                   # consecutive edges share a corner: a proper quad, never a bow-tie
        (a, b), (c, d) = ins, outs
        cyc = [e(a, c), e(a, d), e(b, d), e(b, c)]
    P = np.array(tet_corners(perm), np.float64)
    mid = np.array([(P[u] + P[v]) / 2 for u, v in cyc])
    normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    if float(normal @ (P[outs].mean(0) - P[ins].mean(0))) < 0:
        cyc = cyc[::-1]
    return cyc


_POLYGONS = {}


def polygon_table():
    """(perm, case) -> tet_polygon, derived once."""
    if not _POLYGONS:
        _POLYGONS.update({(perm, case): tet_polygon(perm, [(case >> v) & 1 for v in range(4)]) for perm in PERMS for case in range(16)})
    return _POLYGONS


def _empty():
    return np.zeros(0, np.int64), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)


def marching_tetrahedra(vol, level, ticks):
    """-> (keys (V) int64 ascending, verts (V, 3) float32, faces (F, 3) int32) by the rules above.  ticks: three 1-D arrays of world
    coordinates."""
    vol = np.ascontiguousarray(vol, np.float32)
    level = np.float32(level)
    n0, n1, n2 = vol.shape
    if min(vol.shape) < 2:
        return _empty()
    ticks = [np.asarray(t, np.float32) for t in ticks]
    with np.errstate(invalid="ignore"):
        inside = vol >= level
    if inside.all() or not inside.any():
        return _empty()
    lin = np.arange(n0 * n1 * n2, dtype=np.int64).reshape(vol.shape)
    keys, pos = [], []
    for cls, (dx, dy, dz) in enumerate(CLASS_OFFSETS):
        lo = (slice(0, n0 - dx), slice(0, n1 - dy), slice(0, n2 - dz))
        hi = (slice(dx, n0), slice(dy, n1), slice(dz, n2))
        act = inside[lo] != inside[hi]
        idx = np.argwhere(act)
        if idx.shape[0] == 0:
            continue
        va, vb = vol[lo][act], vol[hi][act]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = ((level - va) / (vb - va)).astype(np.float32)
        t = np.fmin(np.fmax(t, np.float32(0)), np.float32(1))
        p = np.empty((idx.shape[0], 3), np.float32)
        for ax, d in enumerate((dx, dy, dz)):
            pa, pb = ticks[ax][idx[:, ax]], ticks[ax][idx[:, ax] + d]
            p[:, ax] = pa + (t * (pb - pa)).astype(np.float32)
        keys.append(7 * lin[lo][act] + cls)
        pos.append(p)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    keys, verts = keys[order], pos[order]
    index_of = {int(k): n for n, k in enumerate(keys)}
    polygons = polygon_table()
    faces = []
    n_in = sum(inside[dx:n0 - 1 + dx, dy:n1 - 1 + dy, dz:n2 - 1 + dz].astype(np.int32) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    for i, j, k in np.argwhere((n_in > 0) & (n_in < 8)):                  # argwhere walks in linear-index order
        for perm in PERMS:
            corners = tet_corners(perm)
            case = sum(int(inside[i + o[0], j + o[1], k + o[2]]) << v for v, o in enumerate(corners))
            cyc = polygons[(perm, case)]
            if not cyc:
                continue
            ids = []
            for u, v in cyc:
                ou, ov = corners[u], corners[v]
                cls = CLASS_OF_OFFSET[(ov[0] - ou[0], ov[1] - ou[1], ov[2] - ou[2])]
                ids.append(index_of[7 * int(lin[i + ou[0], j + ou[1], k + ou[2]]) + cls])
            if len(ids) == 3:
                faces.append(ids)
            else:
                m = ids.index(min(ids))
                q = ids[m:] + ids[:m]
                faces.append([q[0], q[1], q[2]])
                faces.append([q[0], q[2], q[3]])
    return keys, verts, np.asarray(faces, np.int32).reshape(-1, 3)


def vertex_normals(vol, level, ticks, keys):
    """Per-vertex normal of the extractor: minus the central-difference gradient of vol (one-sided at the border) at the two endpoints of
    the vertex's edge, interpolated with the vertex's t, normalised (zero where the length is zero or not finite).  fp32, one rounding
    per operation, in the kernel's order."""
    vol = np.ascontiguousarray(vol, np.float32)
    level = np.float32(level)
    shape = vol.shape
    ticks = [np.asarray(t, np.float32) for t in ticks]

    def grad(idx):
        g = np.empty((idx.shape[0], 3), np.float32)
        for ax in range(3):
            lo, hi = np.maximum(idx[:, ax] - 1, 0), np.minimum(idx[:, ax] + 1, shape[ax] - 1)
            a, b = idx.copy(), idx.copy()
            a[:, ax], b[:, ax] = lo, hi
            g[:, ax] = (vol[b[:, 0], b[:, 1], b[:, 2]] - vol[a[:, 0], a[:, 1], a[:, 2]]) / (ticks[ax][hi] - ticks[ax][lo])
        return g

    keys = np.asarray(keys, np.int64)
    owner = np.stack(np.unravel_index(keys // 7, shape), 1)
    other = owner + np.asarray(CLASS_OFFSETS, np.int64)[keys % 7]
    va, vb = vol[owner[:, 0], owner[:, 1], owner[:, 2]], vol[other[:, 0], other[:, 1], other[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = ((level - va) / (vb - va)).astype(np.float32)
        t = np.fmin(np.fmax(t, np.float32(0)), np.float32(1))[:, None]
        ga, gb = grad(owner), grad(other)
        g = ga + (t * (gb - ga)).astype(np.float32)
        length = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(np.float32))
        ok = np.isfinite(length) & (length > 0)
        n = np.where(ok[:, None], -g / np.where(ok, length, np.float32(1))[:, None], np.float32(0))
    return n.astype(np.float32)


# --------------------------------------------------------------------------- mesh invariants
def canonical_faces(faces):
    """Every face rotated so that its smallest index comes first (the winding is kept), the rows then sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    m = np.argmin(f, 1)
    r = np.stack([f[np.arange(f.shape[0]), (m + s) % 3] for s in range(3)], 1)
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


def closed_oriented(faces):
    """(every directed edge appears once, every undirected edge is in exactly two triangles)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed_once = np.unique(d, axis=0).shape[0] == d.shape[0]
    _, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    return bool(directed_once), bool((cnt == 2).all())


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return int(n_verts) - int(np.unique(np.sort(d, 1), axis=0).shape[0]) + int(f.shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def ulp_distance(a, b):
    """Largest distance in units in the last place between two float32 arrays of equal shape (finite values)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.abs(ordered(a) - ordered(b)).max()) if a.size else 0


# --------------------------------------------------------------------------- fields
def _ticks(shape, half):
    return [np.linspace(-h, h, n).astype(np.float32) for n, h in zip(shape, half)]


def _grid(ticks):
    return np.meshgrid(*[t.astype(np.float64) for t in ticks], indexing="ij")


def _grid64(shape, half):
    return np.meshgrid(*[np.linspace(-h, h, n) for n, h in zip(shape, half)], indexing="ij")


def _snap(vol64):
    return np.where(np.abs(vol64) < 1e-7, 0.0, vol64).astype(np.float32)


def sphere_case():
    """Radius 0.45 on (9, 13, 17) over +-(1, 0.8, 0.6): the signed distance vol = r - |x| in fp64 on the fp64 lattice, level 0.  The
    lattice points (0, 0, +-0.45) lie on the level: what fp64 leaves of them (below 1e-7) is snapped to exactly 0."""
    shape, half, r = (9, 13, 17), (1.0, 0.8, 0.6), 0.45
    ticks = _ticks(shape, half)
    X, Y, Z = _grid64(shape, half)
    vol = _snap(r - np.sqrt(X * X + Y * Y + Z * Z))
    return dict(name="sphere", vol=vol, level=0.0, ticks=ticks, chi=2, closed=True, analytic_volume=4.0 / 3.0 * np.pi * r ** 3)


def torus_case():
    """R 0.45, r 0.17 on (21, 21, 13) over +-(0.8, 0.8, 0.4): the signed distance vol = r - sqrt((sqrt(x^2 + y^2) - R)^2 + z^2), level 0."""
    shape, half, R, r = (21, 21, 13), (0.8, 0.8, 0.4), 0.45, 0.17
    ticks = _ticks(shape, half)
    X, Y, Z = _grid64(shape, half)
    vol = _snap(r - np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z))
    return dict(name="torus", vol=vol, level=0.0, ticks=ticks, chi=0, closed=True, analytic_volume=2.0 * np.pi ** 2 * R * r * r)


def _border(vol, value):
    vol[0], vol[-1], vol[:, 0], vol[:, -1], vol[:, :, 0], vol[:, :, -1] = (value,) * 6
    return vol


def random_case(seed):
    """standard_normal (8, 9, 10), border faces -1, level 0."""
    vol = _border(np.random.default_rng(seed).standard_normal((8, 9, 10)).astype(np.float32), -1.0)
    return dict(name=f"random{seed}", vol=vol, level=0.0, ticks=_ticks(vol.shape, (1.0, 1.0, 1.0)), chi=None, closed=True)


def tie_case():
    """Values from {-1, 0, 1} on (7, 7, 7), border -1, level 0: a third of the lattice points sit exactly on the level."""
    vol = _border(np.random.default_rng(7).integers(-1, 2, (7, 7, 7)).astype(np.float32), -1.0)
    return dict(name="tie", vol=vol, level=0.0, ticks=_ticks(vol.shape, (1.0, 1.0, 1.0)), chi=None, closed=True)


def open_case():
    """A Gaussian blob centred on a lattice corner, so that the lattice boundary cuts the surface: an open mesh."""
    shape = (7, 9, 8)
    ticks = _ticks(shape, (1.0, 1.0, 1.0))
    X, Y, Z = _grid(ticks)
    vol = np.exp(-((X - 1.0) ** 2 + (Y + 1.0) ** 2 + (Z - 0.2) ** 2) / 0.8).astype(np.float32)
    return dict(name="open", vol=vol, level=0.5, ticks=ticks, chi=None, closed=False)


def closed_cases():
    return [sphere_case(), torus_case(), random_case(0), random_case(1), random_case(2), tie_case()]


def single_cell_case(pattern):
    """One (2, 2, 2) cell whose corner (dx, dy, dz) is inside when bit dx + 2 dy + 4 dz of ``pattern`` is set; distinct magnitudes."""
    vol = np.empty((2, 2, 2), np.float32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                b = dx + 2 * dy + 4 * dz
                vol[dx, dy, dz] = (0.25 + 0.125 * b) * (1.0 if (pattern >> b) & 1 else -1.0)
    return dict(name=f"cell{pattern:03d}", vol=vol, level=0.0, ticks=_ticks((2, 2, 2), (0.5, 0.75, 1.0)), chi=None, closed=False)
