"""Relations of a keyed 3-D lattice (csrc/relations.hip: clift_lattice_relations) and the scene graph made of them: what
rests on what, what touches what, how much of an object's surface is free.

    key, nodes = node_keys(sem, inst)                                    # (class, instance) pairs of the inside points -> keys 1..K
    rel = lattice_relations(key, n_keys=len(nodes) + 1, gap=1)           # count, isum, ibox, faces, near, rejected: integer tables
    graph = SceneGraph.from_counts(rel, nodes, ticks, up="+z")           # fp64 on the host; graph.to_json()

The tables (the rules in full: include/clift.h).  Key 0 is background, valid keys are 0 .. n_keys - 1.  ``count[k]`` points carry key k,
``isum[k][a]`` is the sum of their index along axis a, ``ibox[k]`` = min_0 min_1 min_2 max_0 max_1 max_2 of their indices (min_a = n_a,
max_a = -1 for a key nobody carries).  ``faces[u][v][a]`` counts the neighbours (p, p + e_a) with keys u != v, u the lower one; against key 0
these are free faces.  ``near[u][v][a]`` (``gap`` >= 1) counts the points of u != 0 whose +a neighbour is background and whose look along +a,
at most ``gap`` background points deep, ends at another key v: objects in a density field are usually separated by a thin empty gap at the
level set, so plain adjacency misses "cup on table".  A point with a key outside [0, n_keys) is counted in ``rejected`` and nowhere else.

``backend="device"`` is one kernel launch; ``backend="host"`` gives the same integers in vectorised numpy (shifted slices and np.add.at) for
machines and tests without a GPU.  What the lattice modules share is in ``lattice``.
"""
import numpy as np
import torch

from . import _lib, lattice
from .lattice import MAX_KEYS   # noqa: F401  (CLIFT_REL_MAX_KEYS; callers read it as relations.MAX_KEYS)

LDS_KEYS = 32                    # CLIFT_REL_LDS_KEYS: up to here the kernel counts pairs in a block-private LDS table
MAX_GAP = 4                      # CLIFT_REL_MAX_GAP
TILE = (8, 8, 32)                # the kernel's tile extents (csrc/relations.hip: REL_T0, REL_T1, REL_T2)
UP_AXES = lattice.DIRECTIONS     # "+x", "-x", "+y", "-y", "+z", "-z"
TABLES = ("count", "isum", "ibox", "faces", "near", "rejected")


def _tables_host(key, n_keys, gap):
    k = key.cpu().numpy().astype(np.int64)
    valid = (k >= 0) & (k < n_keys)
    kv = np.where(valid, k, -1)                                            # -1: rejected, and later: beyond the lattice
    count = np.bincount(kv[valid], minlength=n_keys).astype(np.int64)
    isum = np.zeros((n_keys, 3), np.int64)
    ibox = lattice.index_box(k, n_keys).astype(np.int32)
    at = np.nonzero(valid)
    for a in range(3):
        np.add.at(isum[:, a], kv[valid], at[a])
    faces = np.zeros((n_keys, n_keys, 3), np.int32)
    near = np.zeros((n_keys, n_keys, 3), np.int32) if gap > 0 else None
    for a in range(3):
        m = np.moveaxis(kv, a, 2)                                          # the axis of the pair last
        n = m.shape[2]
        lo, hi = m[:, :, :n - 1], m[:, :, 1:]
        pair = (lo >= 0) & (hi >= 0) & (lo != hi)
        np.add.at(faces[:, :, a], (lo[pair], hi[pair]), 1)
        if gap == 0 or n < 2:
            continue
        pad = np.concatenate([m, np.full(m.shape[:2] + (gap + 1,), -1, np.int64)], 2)
        u = pad[:, :, :n]
        looking = (u > 0) & (pad[:, :, 1:n + 1] == 0)
        for d in range(2, gap + 2):
            w = pad[:, :, d:n + d]
            hit = looking & (w > 0) & (w != u)
            np.add.at(near[:, :, a], (u[hit], w[hit]), 1)
            looking &= w == 0
    out = dict(count=count, isum=isum, ibox=ibox, faces=faces, near=near, rejected=np.asarray([int((~valid).sum())], np.int32))
    return {name: None if v is None else torch.from_numpy(v).to(key.device) for name, v in out.items()}


@torch.no_grad()
def relation_tables(key, n_keys=None, gap=0, backend="device"):
    """The tables of clift_lattice_relations as a dict of tensors on key's device -- count (n_keys) int64, isum (n_keys, 3) int64, ibox
    (n_keys, 6) int32, faces and near (n_keys, n_keys, 3) int32 (near is None when gap == 0), rejected (1) int32 -- whatever ``rejected``
    says (``lattice_relations`` raises on it).  ``n_keys=None``: max(key) + 1, one read of the lattice's maximum."""
    key, n_keys = lattice.prepare(key, n_keys, "lattice_relations")
    gap = int(gap)
    if not 0 <= gap <= MAX_GAP:
        raise ValueError(f"gap must be 0 .. {MAX_GAP} (got {gap})")
    if lattice.check_backend(backend) == "host":
        return _tables_host(key, n_keys, gap)
    lattice.require_device(key, "lattice_relations")
    dev, (n0, n1, n2) = key.device, key.shape
    out = dict(count=torch.empty(n_keys, dtype=torch.int64, device=dev), isum=torch.empty((n_keys, 3), dtype=torch.int64, device=dev),
               ibox=torch.empty((n_keys, 6), dtype=torch.int32, device=dev), faces=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev),
               near=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev) if gap > 0 else None,
               rejected=torch.empty(1, dtype=torch.int32, device=dev))
    _lib.call("clift_lattice_relations", _lib.ptr(key), n0, n1, n2, n_keys, gap, _lib.ptr(out["count"]), _lib.ptr(out["isum"]), _lib.ptr(out["ibox"]),
              _lib.ptr(out["faces"]), _lib.ptr(out["near"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


@torch.no_grad()
def lattice_relations(key, n_keys=None, gap=0, backend="device"):
    """``relation_tables`` of a key lattice (n0, n1, n2) bool or integer; raises CliftError when a point's key lies outside [0, n_keys)."""
    out = relation_tables(key, n_keys, gap, backend)
    lattice.raise_on_rejected(out, out["count"].shape[0], "lattice_relations")
    return out


@torch.no_grad()
def node_keys(sem, inst):
    """Two int lattices of one shape, ``sem < 0`` marking outside -> (key int32 like sem, nodes).  ``nodes`` is the sorted list of the distinct
    (class, instance) pairs among the inside points; pair number i (from 0) gets key i + 1, outside points key 0.  Instance 0 means a stuff
    class as one node."""
    if not torch.is_tensor(sem):
        sem = torch.from_numpy(np.ascontiguousarray(sem))
    if not torch.is_tensor(inst):
        inst = torch.from_numpy(np.ascontiguousarray(inst))
    for name, t in (("sem", sem), ("inst", inst)):
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer lattice, got {t.dtype}")
    if sem.shape != inst.shape:
        raise ValueError(f"sem and inst must have one shape, got {tuple(sem.shape)} and {tuple(inst.shape)}")
    inst = inst.to(sem.device)
    inside = sem >= 0
    key = torch.zeros(sem.shape, dtype=torch.int32, device=sem.device)
    if not bool(inside.any()):
        return key, []
    s, i = sem[inside].long(), inst[inside].long()
    if int(i.min()) < 0:
        raise ValueError(f"instance ids must be >= 0 (found {int(i.min())})")
    width = int(i.max()) + 1
    codes, inverse = torch.unique(s * width + i, sorted=True, return_inverse=True)
    key[inside] = (inverse + 1).int()
    codes = codes.cpu().numpy()
    return key, [(int(c // width), int(c % width)) for c in codes]


def _up_axis(up):
    if up not in UP_AXES:
        raise ValueError(f"up must be one of {', '.join(UP_AXES)} (got {up!r})")
    return "xyz".index(up[1]), up[0] == "+"


class SceneGraph(lattice.Summary):
    """The graph of ``SceneGraph.from_counts``: ``nodes`` (one dict per key 1..K), ``pairs`` (one dict per ordered pair of nodes with any
    contact, u the lower one along the axis of the contact) and ``relations`` (the named ones: "on" and "beside")."""

    def __init__(self, up, min_faces, nodes, pairs, relations):
        self.up, self.min_faces, self.nodes, self.pairs, self.relations = up, min_faces, nodes, pairs, relations

    @classmethod
    def from_counts(cls, rel, nodes, ticks, up="+z", min_faces=4):
        """``rel``: the tables of ``lattice_relations`` with n_keys = len(nodes) + 1; ``nodes``: the (class, instance) pairs of ``node_keys``;
        ``ticks``: the three uniform coordinate arrays of the lattice (``renderer.lattice_ticks``).  Everything in fp64 on the host.

        Per node: voxels, volume (voxels x the cell volume), centroid = tick(isum / count), index_box and box (the ticks at its corners), and
        free_area per direction: free faces x the area of a cell face.  Per ordered pair with any contact: faces and near per axis.
        Named relations, with a = the axis of ``up`` and contact = faces + near:
          on      "v on u" when contact[u][v][a] >= min_faces (for a negative ``up`` the roles swap: contact[v][u][a]); ``support`` is that
                  count divided by all faces of v that look against ``up``, background included.
          beside  u < v with at least min_faces contacts on the other two axes together, in either order, and none along ``up``."""
        axis, positive = _up_axis(up)
        min_faces = int(min_faces)
        host = lattice.to_host(rel, ("count", "isum", "ibox", "faces", "near"), np.int64)
        count, isum, ibox, faces = host["count"], host["isum"], host["ibox"], host["faces"]
        near = np.zeros_like(faces) if host["near"] is None else host["near"]
        K = lattice.node_count(count, nodes)
        ticks, step = lattice.host_ticks(ticks)
        first = np.asarray([t[0] for t in ticks])
        face_area = np.asarray([abs(step[1] * step[2]), abs(step[0] * step[2]), abs(step[0] * step[1])])
        cell = float(abs(step[0] * step[1] * step[2]))
        contact = faces + near
        out_nodes = []
        for k in range(1, K + 1):
            n = int(count[k])
            node = dict(key=k, semantic=int(nodes[k - 1][0]), instance=int(nodes[k - 1][1]), voxels=n, volume=n * cell)
            if n > 0:
                node["centroid"] = (first + step * (isum[k] / n)).tolist()
                node["index_box"] = [int(x) for x in ibox[k]]
                node["box"] = (first + step * ibox[k, :3]).tolist() + (first + step * ibox[k, 3:]).tolist()
            else:
                node["centroid"] = node["index_box"] = node["box"] = None
            node["free_area"] = {}
            for a in range(3):
                node["free_area"]["+" + "xyz"[a]] = float(faces[k, 0, a] * face_area[a])
                node["free_area"]["-" + "xyz"[a]] = float(faces[0, k, a] * face_area[a])
            out_nodes.append(node)
        pairs, relations = [], []
        for u in range(1, K + 1):
            for v in range(1, K + 1):
                if u != v and contact[u, v].any():
                    pairs.append(dict(u=u, v=v, faces=[int(x) for x in faces[u, v]], near=[int(x) for x in near[u, v]]))
        for u in range(1, K + 1):
            for v in range(1, K + 1):
                if u == v:
                    continue
                c = int(contact[u, v, axis] if positive else contact[v, u, axis])
                if c >= min_faces and c > 0:
                    below = int(faces[:, v, axis].sum() if positive else faces[v, :, axis].sum())      # all faces of v that look against up
                    relations.append(dict(relation="on", subject=v, object=u, contact=c, support=c / below if below else None))
        horizontal = [a for a in range(3) if a != axis]
        for u in range(1, K + 1):
            for v in range(u + 1, K + 1):
                side = int(sum(contact[u, v, a] + contact[v, u, a] for a in horizontal))
                if side >= min_faces and side > 0 and contact[u, v, axis] + contact[v, u, axis] == 0:
                    relations.append(dict(relation="beside", subject=u, object=v, contact=side, support=None))
        return cls(up, min_faces, out_nodes, pairs, relations)

    def on(self):
        """{key of v: [(key of u, support), ...]}: what every node rests on."""
        out = {}
        for r in self.relations:
            if r["relation"] == "on":
                out.setdefault(r["subject"], []).append((r["object"], r["support"]))
        return out

    def beside(self):
        """The set of (u, v), u < v, that stand beside one another."""
        return {(r["subject"], r["object"]) for r in self.relations if r["relation"] == "beside"}

    def to_dict(self):
        return dict(up=self.up, min_faces=self.min_faces, nodes=self.nodes, pairs=self.pairs, relations=self.relations)
