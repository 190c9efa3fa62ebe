"""The scene as a labelled surface mesh: iso-surface of the density lattice (csrc/isosurface.hip: marching tetrahedra on the Kuhn split,
DESIGN.md 6d), per-vertex colour / class / instance id from the field's own heads, binary PLY output.

    vol = renderer.get_dense_sigma(model, upsample)                      # clift_dense_sigma
    verts, faces, normals = extract_isosurface(vol, level, renderer.lattice_ticks(vol.shape))
    sem, inst, rgb = label_vertices(model, renderer, verts, normals, thing_classes, centroids)
    write_ply(path, verts, faces, normals, rgb, sem, inst)

Ordering contract of ``extract_isosurface`` (two runs give the same bits, order included): vertex v is the v-th active edge by the key
7 * linear_index(owner) + class; faces follow the scan (cell by linear index, tetrahedron by the lexicographic order of its axis
permutation, triangle; a quad is split along the diagonal through its smallest vertex index, that vertex first).
"""
import numpy as np
import torch

from . import _lib

ISO_LIMIT = 2 ** 31


def _empty(dev):
    z = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    return z, torch.zeros((0, 3), dtype=torch.int32, device=dev), z.clone()


@torch.no_grad()
def extract_isosurface(vol, level, ticks, want_normals=True, return_keys=False):
    """Iso-surface ``vol >= level`` of a device lattice vol (n0, n1, n2) fp32 whose lattice point (i, j, k) sits at the world position
    (ticks[0][i], ticks[1][j], ticks[2][k]).  -> (verts (V, 3) f32, faces (F, 3) i32, normals (V, 3) f32), all on the device; normals
    (minus the normalised gradient of vol: they point from inside to outside, like the faces' winding) are None with
    ``want_normals=False``.  Three launches and one host read of the two totals; the scans between are torch.cumsum in int64.
    Memory beside vol and the outputs: 25 bytes per lattice point (mask 1, two int32 counts, two int64 offsets) plus cumsum's result.
    ``return_keys=True`` appends the (V) int64 keys 7 * linear_index(owner) + class of the vertices, ascending (tests, debugging)."""
    vol = _lib.f32(vol, "vol")
    if vol.dim() != 3:
        raise ValueError(f"vol must be (n0, n1, n2), got {tuple(vol.shape)}")
    vol = vol.contiguous()
    dev = vol.device
    n0, n1, n2 = (int(x) for x in vol.shape)
    if n0 * n1 * n2 >= ISO_LIMIT:
        raise _lib.CliftError(f"extract_isosurface: {n0 * n1 * n2} lattice points, must be < 2^31")
    if len(ticks) != 3:
        raise ValueError("ticks: three per-axis coordinate arrays")
    ticks = [_lib.f32(t, f"ticks[{a}]").reshape(-1).contiguous() for a, t in enumerate(ticks)]
    for a, t in enumerate(ticks):
        if t.shape[0] != vol.shape[a] or t.device != dev:
            raise ValueError(f"ticks[{a}] holds {t.shape[0]} coordinates on {t.device}, the lattice has {vol.shape[a]} on {dev}")
    level = float(level)
    no_keys = (torch.zeros(0, dtype=torch.int64, device=dev),) if return_keys else ()
    if min(n0, n1, n2) < 2:
        return _empty(dev) + no_keys
    N = n0 * n1 * n2
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    n_vert = torch.empty(N, dtype=torch.int32, device=dev)
    n_tri = torch.empty(N, dtype=torch.int32, device=dev)
    _lib.call("clift_iso_classify", _lib.ptr(vol), n0, n1, n2, level, _lib.ptr(mask), _lib.ptr(n_vert), _lib.ptr(n_tri), _lib.stream())
    v_end = torch.cumsum(n_vert, 0, dtype=torch.int64)
    t_end = torch.cumsum(n_tri, 0, dtype=torch.int64)
    V, F = (int(x) for x in torch.stack([v_end[-1], t_end[-1]]).tolist())          # the one host read
    if V >= ISO_LIMIT or F >= ISO_LIMIT:
        raise _lib.CliftError(f"extract_isosurface: {V} vertices and {F} faces, each must be < 2^31 (raise the level or lower the upsampling)")
    if V == 0 or F == 0:
        return _empty(dev) + no_keys
    v_off, t_off = v_end - n_vert, t_end - n_tri
    del v_end, t_end
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev) if want_normals else None
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    _lib.call("clift_iso_vertices", _lib.ptr(vol), n0, n1, n2, level, _lib.ptr(ticks[0]), _lib.ptr(ticks[1]), _lib.ptr(ticks[2]), _lib.ptr(mask),
              _lib.ptr(v_off), V, _lib.ptr(verts), _lib.ptr(normals), _lib.stream())
    _lib.call("clift_iso_faces", _lib.ptr(vol), n0, n1, n2, level, _lib.ptr(mask), _lib.ptr(v_off), _lib.ptr(t_off), V, F, _lib.ptr(faces),
              _lib.stream())
    if return_keys:                               # row-major nonzero of the (N, 7) bit table: ascending in lattice point, then class
        at = ((mask.to(torch.int32)[:, None] >> torch.arange(7, device=dev, dtype=torch.int32)) & 1).nonzero()
        return verts, faces, normals, 7 * at[:, 0] + at[:, 1]
    return verts, faces, normals


@torch.no_grad()
def label_vertices(model, renderer, verts, normals, thing_classes, centroids=None, chunk=2 ** 20, use_delta=False, edit=None):
    """Per vertex (world positions ``verts`` (V, 3) on the device): semantic class (V) int64 = argmax of the semantic head; instance id (V)
    int64; rgb (V, 3) fp32 in [0, 1] from the appearance head seen along ``-normal``.  All through the field's own point-wise methods
    (xyz-MLP and VM-grid heads alike), ``chunk`` vertices at a time.

    Instance id without ``centroids``: the argmax of the fast half of the instance head -- the reference's per-voxel rule
    (get_instance_clusters), meaningful for ``linear_assignment`` models, whose outputs are slot scores.  With ``centroids`` (the dict of
    an ``all_centroids.pkl``: class -> (K, E)): vertices of stuff classes get 0, a vertex of thing class c gets the nearest centroid of c,
    numbered as ``inference.assign_clusters`` numbers ``pred_surrogateid`` -- over ALL vertices at once, since that numbering offsets
    every class by the labels seen before it.  ``use_delta``: the field predicts an offset, the feature is output + position
    (render_panopli.py, config.use_delta).

    ``edit`` (an ``edit.Edit``, an ``edit.EditProgram`` or a sequence of edits): the vertices are those of the EDITED scene.  Every chunk
    first goes through ``EditProgram.apply_to_points(verts, -normals)`` (clift_edit_list_points): the three heads are evaluated where the
    vertex's content came from, the appearance head along the turned view direction, and with ``use_delta`` the feature is
    fast(source) + source -- a moved object keeps its class, id and colour, a copy carries the original's id.  A killed vertex (the cap
    of a cut) is labelled at the position where its walk stopped.  Rows the program does not touch get the bits they get without it."""
    from . import edit as ed
    from . import inference as inf
    prog = None if edit is None else ed.as_program(edit)
    verts = _lib.f32(verts, "verts").reshape(-1, 3).contiguous()
    dev = verts.device
    V = verts.shape[0]
    sem = torch.empty(V, dtype=torch.int64, device=dev)
    rgb = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if model.render_instance_mlp is None:
        raise ValueError("label_vertices: the field has no instance head")
    E = model.dim_feature_instance // 2 if model.slow_fast_mode else model.dim_feature_instance
    feats = torch.empty((V, E), dtype=torch.float32, device=dev)
    normals = _lib.f32(normals, "normals").reshape(-1, 3)
    if normals.shape[0] != V:
        raise ValueError(f"label_vertices: {normals.shape[0]} normals for {V} vertices")
    for a in range(0, V, int(chunk)):
        b = min(V, a + int(chunk))
        xyz = verts[a:b]
        view = (-normals[a:b]).contiguous()
        if prog is not None:
            xyz, view, _ = prog.apply_to_points(xyz, view)
        xn = renderer.normalize_coordinates(xyz).contiguous()
        sem[a:b] = model.render_semantic_mlp(None, model.compute_semantic_feature(xn)).argmax(-1)
        fast = model.render_instance_mlp(None, model.compute_instance_feature(xn))[:, :E]
        feats[a:b] = fast + xyz if use_delta else fast
        rgb[a:b] = model.render_appearance_mlp(view, model.compute_appearance_feature(xn))
    if centroids is None:
        inst = feats.argmax(-1) if V else torch.zeros(0, dtype=torch.int64, device=dev)
    else:
        thing = torch.isin(sem, torch.tensor(sorted(int(c) for c in thing_classes), dtype=torch.int64, device=dev))
        inst = inf.assign_cluster_labels(feats, sem, thing, centroids) + 1
    return sem, inst, rgb


def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"),
                       ("blue", "u1"), ("semantic", "u1"), ("instance", "<u2")])
PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, verts, faces, normals, rgb, semantics, instances):
    """Binary little-endian PLY: vertex properties x y z nx ny nz (float) red green blue (uchar; ``rgb`` in [0, 1] fp or already uint8)
    semantic (uchar) instance (ushort); faces as ``list uchar int vertex_indices``."""
    verts, normals = _np(verts, np.float32).reshape(-1, 3), _np(normals, np.float32).reshape(-1, 3)
    faces = _np(faces, np.int32).reshape(-1, 3)
    rgb = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    if rgb.dtype != np.uint8:
        rgb = np.rint(np.clip(rgb.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    rgb = rgb.reshape(-1, 3)
    semantics, instances = _np(semantics, np.int64).reshape(-1), _np(instances, np.int64).reshape(-1)
    V = verts.shape[0]
    if not (normals.shape[0] == rgb.shape[0] == semantics.shape[0] == instances.shape[0] == V):
        raise ValueError("write_ply: per-vertex arrays of different lengths")
    if V and (semantics.min() < 0 or semantics.max() > 255 or instances.min() < 0 or instances.max() > 65535):
        raise ValueError("write_ply: semantic must fit uchar and instance ushort")
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("write_ply: a face names a vertex that does not exist")
    vrec = np.empty(V, PLY_VERTEX)
    for n, name in enumerate(("x", "y", "z")):
        vrec[name], vrec["n" + name] = verts[:, n], normals[:, n]
    vrec["red"], vrec["green"], vrec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    vrec["semantic"], vrec["instance"] = semantics, instances
    frec = np.empty(faces.shape[0], PLY_FACE)
    frec["n"], frec["v"] = 3, faces
    types = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<u2": "ushort"}
    head = ["ply", "format binary_little_endian 1.0", "comment contrastive_lift_amd mesh: semantic = class id, instance = surrogate id (0 = stuff)",
            f"element vertex {V}"]
    head += [f"property {types[PLY_VERTEX[name].str]} {name}" for name in PLY_VERTEX.names]
    head += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_ply(path):
    """Parse a PLY written by ``write_ply`` -> dict(verts, normals, rgb (uint8), semantics, instances, faces)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln.split()[-1] for ln in lines if ln.startswith("property ") and " list " not in ln]
    if tuple(props) != PLY_VERTEX.names:
        raise ValueError(f"{path}: vertex properties {props}")
    V, F = counts["vertex"], counts["face"]
    if len(data) != end + V * PLY_VERTEX.itemsize + F * PLY_FACE.itemsize:
        raise ValueError(f"{path}: {len(data)} bytes for {V} vertices and {F} faces")
    v = np.frombuffer(data, PLY_VERTEX, V, end)
    fr = np.frombuffer(data, PLY_FACE, F, end + V * PLY_VERTEX.itemsize)
    if F and not (fr["n"] == 3).all():
        raise ValueError(f"{path}: a face that is no triangle")
    return dict(verts=np.stack([v["x"], v["y"], v["z"]], 1), normals=np.stack([v["nx"], v["ny"], v["nz"]], 1),
                rgb=np.stack([v["red"], v["green"], v["blue"]], 1), semantics=v["semantic"].copy(), instances=v["instance"].copy(),
                faces=fr["v"].copy())
