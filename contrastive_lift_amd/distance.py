"""Distance transform of a keyed 3-D lattice (csrc/distance.hip: clift_lattice_distance): per lattice point the exact squared
Euclidean distance to the nearest site and that site's linear index, per pair of instances their true gap -- diagonal neighbours included,
which the axis looks of ``relations`` and ``clearance`` cannot see --, and whether the object that an edit places collides.

    t = lattice_distance(key, n_keys, sites=None, key_min=True)         # packed (n0, n1, n2) int64, rejected, key_min (n_keys,)
    dist2, nearest = split(t["packed"])                                  # int32 each; NONE and -1 where there is no site
    owner = voronoi_keys(key, t["packed"], max_dist2=9)                  # the key of every point's nearest site
    tables = separation(key, n_keys)                                     # gap2, at, to (n_keys, n_keys) int32
    summary = Separation.from_tables(tables, nodes, ticks)               # fp64 on the host; summary.to_json()
    found = placement(model, renderer, edit.move(box, t, shape=sh))      # verdict, overlap, depth2, gap2, ...

The rules (in full: include/clift.h).  Valid keys are 0 .. n_keys - 1; a point is a site when its key is valid and ``sites`` names it (key 0
may be named: the transform of the complement).  ``packed[p] = (dist2 << 31) | nearest``: the minimum over all sites of the squared index
distance, the site with the smallest linear index ``lin = (i0 n1 + i1) n2 + i2`` among those at that distance; ``NONE_WORD`` without any site.
``key_min[u]`` = min over the points p of key u >= 1 of (dist2(p) << 31) | lin(p).  Distances are in index units; world distances are formed
afterwards from the lattice ticks of the two points that were chosen.

``backend="device"`` is one call (three passes: z, y, x); ``backend="host"`` gives the same integers in numpy -- the same three passes, one
offset of the axis at a time over the whole lattice (three lattices of int64 in memory), ending an axis once the offset squared exceeds every
distance found -- for machines and tests without a GPU.  What the lattice modules share is in ``lattice``.
"""
import math

import numpy as np
import torch

from . import _lib, lattice
from .lattice import INDEX_MASK, MAX_DIM, NONE_WORD   # (CLIFT_DT_MAX_DIM, CLIFT_DT_NONE: read as distance.MAX_DIM, distance.NONE_WORD too)
from .lattice import key_table as site_table, placement_key, scene_before   # noqa: F401  (still read as distance.site_table, ...)

NONE = 0x7fffffff                # the dist2 of ``split`` where there is no site; gap2 where there is no pair
MAX_SEPARATION_KEYS = 256        # ``separation`` runs one transform per key


def _axis_pass_host(cur, axis):
    """min over j of cur[j] + ((i - j)^2 << 31) along ``axis``, NONE_WORD tested and never added to."""
    m = np.moveaxis(cur, axis, 0)
    n = m.shape[0]
    best = m.copy()
    for d in range(1, n):
        # strictly: a candidate with d^2 == dist2 ties on distance and may win on the index
        if int(best.max()) != NONE_WORD and d * d > int(best.max() >> 31):
            break
        add = np.int64(d * d) << np.int64(31)
        for src, dst in ((m[:-d], best[d:]), (m[d:], best[:-d])):
            np.minimum(dst, np.where(src != NONE_WORD, src + add, NONE_WORD), out=dst)
    return np.moveaxis(best, 0, axis)


def _tables_host(key, n_keys, table, want_min):
    k = key.cpu().numpy().astype(np.int64)
    valid = (k >= 0) & (k < n_keys)
    is_site = valid & table[np.where(valid, k, 0)]
    lin = np.arange(k.size, dtype=np.int64).reshape(k.shape)
    cur = np.where(is_site, lin, np.int64(NONE_WORD))
    for axis in (2, 1, 0):
        cur = _axis_pass_host(cur, axis)
    out = dict(packed=np.ascontiguousarray(cur), rejected=np.asarray([int((~valid).sum())], np.int32))
    if want_min:
        km = np.full(n_keys, NONE_WORD, np.int64)
        mine = valid & (k >= 1) & (cur != NONE_WORD)
        np.minimum.at(km, k[mine], ((cur[mine] >> 31) << 31) | lin[mine])
        out["key_min"] = km
    return {name: torch.from_numpy(v).to(key.device) for name, v in out.items()}


def _run(key, n_keys, table, want_min, backend, work=None):
    """One transform of a prepared key.  ``work``: a scratch tensor (N,) int64 on the device to use again, or None."""
    if backend == "host":
        return _tables_host(key, n_keys, table, want_min)
    lattice.require_device(key, "lattice_distance")
    dev, (n0, n1, n2) = key.device, key.shape
    site = torch.from_numpy(table.astype(np.uint8)).to(dev)
    out = dict(packed=torch.empty((n0, n1, n2), dtype=torch.int64, device=dev), rejected=torch.empty(1, dtype=torch.int32, device=dev))
    if work is None:
        work = torch.empty(n0 * n1 * n2, dtype=torch.int64, device=dev)
    if want_min:
        out["key_min"] = torch.empty(n_keys, dtype=torch.int64, device=dev)
    _lib.call("clift_lattice_distance", _lib.ptr(key), n0, n1, n2, n_keys, _lib.ptr(site), _lib.ptr(out["packed"]), _lib.ptr(work),
              _lib.ptr(out["key_min"]) if want_min else None, _lib.ptr(out["rejected"]), _lib.stream())
    return out


@torch.no_grad()
def distance_tables(key, n_keys=None, sites=None, key_min=False, backend="device"):
    """The transform of a key lattice (n0, n1, n2) bool or integer as a dict of tensors on key's device -- ``packed`` (n0, n1, n2) int64,
    ``rejected`` (1,) int32 and, with ``key_min=True``, ``key_min`` (n_keys,) int64 -- whatever ``rejected`` says (``lattice_distance`` raises
    on it).  ``sites``: see ``lattice.key_table``.  ``n_keys=None``: max(key) + 1, one read of the lattice's maximum."""
    return _tables(key, n_keys, sites, key_min, backend)[0]


def _tables(key, n_keys, sites, key_min, backend):
    key, n_keys = lattice.prepare(key, n_keys, "lattice_distance", MAX_DIM)
    lattice.check_backend(backend)
    return _run(key, n_keys, lattice.key_table(sites, n_keys), bool(key_min), backend), n_keys


@torch.no_grad()
def lattice_distance(key, n_keys=None, sites=None, key_min=False, backend="device"):
    """``distance_tables``; raises CliftError when a point's key lies outside [0, n_keys)."""
    out, n_keys = _tables(key, n_keys, sites, key_min, backend)
    lattice.raise_on_rejected(out, n_keys, "lattice_distance")
    return out


def split(packed):
    """packed words (tensor or numpy array) -> (dist2, nearest), int32 each and of packed's kind: NONE and -1 where the word is NONE_WORD."""
    if torch.is_tensor(packed):
        empty = packed == NONE_WORD
        return (torch.where(empty, NONE, packed >> 31).to(torch.int32), torch.where(empty, -1, packed & INDEX_MASK).to(torch.int32))
    packed = np.asarray(packed, np.int64)
    empty = packed == NONE_WORD
    return np.where(empty, NONE, packed >> 31).astype(np.int32), np.where(empty, -1, packed & INDEX_MASK).astype(np.int32)


@torch.no_grad()
def voronoi_keys(key, packed, max_dist2=None):
    """Per point the key of its nearest site (int32, key's shape, on packed's device): the Voronoi labelling of the lattice by the sites of
    ``packed``.  0 where there is no site, or where dist2 > ``max_dist2``."""
    key = lattice.as_key(key)
    packed = packed if torch.is_tensor(packed) else torch.from_numpy(np.ascontiguousarray(packed))
    if tuple(packed.shape) != tuple(key.shape):
        raise ValueError(f"packed {tuple(packed.shape)} and key {tuple(key.shape)} are not one lattice")
    dist2, nearest = split(packed)
    keep = nearest >= 0
    if max_dist2 is not None:
        keep = keep & (dist2 <= int(max_dist2))
    owner = key.to(packed.device).reshape(-1)[nearest.clamp(min=0).long().reshape(-1)].view(key.shape)
    return torch.where(keep, owner, 0).to(torch.int32)


@torch.no_grad()
def separation(key, n_keys=None, backend="device"):
    """The true gaps between the keys of a lattice -> dict of int32 tensors on key's device: ``gap2[u][v]`` (n_keys, n_keys) the smallest
    squared index distance between a point of u and a point of v (NONE on the diagonal, for key 0 and for keys nobody carries; symmetric),
    ``at[u][v]`` the lin of the point of u that realises it (the smallest lin among those), ``to[u][v]`` that point's nearest point of v
    (-1 each where gap2 is NONE), and ``rejected``.  One transform per key v >= 1 that occurs, with sites = v and key_min: at most
    ``MAX_SEPARATION_KEYS`` keys.  Raises CliftError on a key outside [0, n_keys)."""
    key, n_keys = lattice.prepare(key, n_keys, "separation", MAX_DIM)
    lattice.check_backend(backend)
    if n_keys > MAX_SEPARATION_KEYS:
        raise ValueError(f"separation runs one transform per key and takes at most {MAX_SEPARATION_KEYS} keys (got n_keys = {n_keys}): drop the "
                         "small components first (--min_component)")
    dev = key.device
    gap2 = torch.full((n_keys, n_keys), NONE, dtype=torch.int64, device=dev)
    at = torch.full((n_keys, n_keys), -1, dtype=torch.int64, device=dev)
    to = torch.full((n_keys, n_keys), -1, dtype=torch.int64, device=dev)
    present = torch.unique(key[(key >= 1) & (key < n_keys)]).tolist()
    work = torch.empty(key.numel(), dtype=torch.int64, device=dev) if backend == "device" and key.is_cuda else None
    rejected = None
    for v in present:
        out = _run(key, n_keys, lattice.key_table(int(v), n_keys), True, backend, work)
        lattice.raise_on_rejected(out, n_keys, "separation")
        rejected = out["rejected"]
        km = out["key_min"].clone()
        km[v] = NONE_WORD                                                  # the diagonal
        found = km != NONE_WORD
        point = torch.where(found, km & INDEX_MASK, 0)
        gap2[:, v] = torch.where(found, km >> 31, NONE)
        at[:, v] = torch.where(found, point, -1)
        to[:, v] = torch.where(found, out["packed"].reshape(-1)[point] & INDEX_MASK, -1)
    if rejected is None:
        rejected = torch.tensor([int(((key < 0) | (key >= n_keys)).sum())], dtype=torch.int32, device=dev)
        lattice.raise_on_rejected(dict(rejected=rejected), n_keys, "separation")
    return dict(gap2=gap2.to(torch.int32), at=at.to(torch.int32), to=to.to(torch.int32), rejected=rejected)


def _world(lin, ticks):
    shape = [t.shape[0] for t in ticks]
    idx = np.unravel_index(int(lin), shape)
    return [float(ticks[a][idx[a]]) for a in range(3)]


class Separation(lattice.Summary):
    """The summary of ``Separation.from_tables``: ``nodes``, one dict per key 1..K with its nearest other node, and ``pairs``, one dict per
    unordered pair of nodes within ``max_cells``."""

    def __init__(self, max_cells, nodes, pairs):
        self.max_cells, self.nodes, self.pairs = max_cells, nodes, pairs

    @classmethod
    def from_tables(cls, tables, nodes, ticks, max_cells=None):
        """``tables``: the tables of ``separation`` with n_keys = len(nodes) + 1; ``nodes``: the (class, instance) pairs of
        ``relations.node_keys``; ``ticks``: the three coordinate arrays of the lattice (``renderer.lattice_ticks``).  fp64 on the host.

        Per node: ``nearest`` = dict(key, cells = sqrt(gap2), distance) of the other node with the smallest gap2 (the smaller key on a tie),
        None for a node alone.  Per unordered pair u < v with sqrt(gap2) <= ``max_cells`` (None: every pair that exists): ``gap2``,
        ``cells``, ``distance`` = the world distance between the two points, in fp64 from the ticks of at[u][v] and to[u][v], and those
        points as ``point_a`` (of u) and ``point_b`` (of v)."""
        host = lattice.to_host(tables, ("gap2", "at", "to"), np.int64)
        gap2, at, to = host["gap2"], host["at"], host["to"]
        K = lattice.node_count(gap2, nodes)
        if max_cells is not None and not float(max_cells) >= 0.0:
            raise ValueError(f"max_cells must be >= 0 (got {max_cells})")
        ticks, _ = lattice.host_ticks(ticks)

        def world_distance(u, v):
            a, b = _world(at[u, v], ticks), _world(to[u, v], ticks)
            return a, b, math.sqrt(sum((x - y) ** 2 for x, y in zip(a, b)))

        out_nodes, pairs = [], []
        for u in range(1, K + 1):
            node = dict(key=u, semantic=int(nodes[u - 1][0]), instance=int(nodes[u - 1][1]), nearest=None)
            row = gap2[u, 1:]
            if row.size and int(row.min()) != NONE:
                v = 1 + int(np.argmin(row))
                node["nearest"] = dict(key=v, cells=math.sqrt(int(gap2[u, v])), distance=world_distance(u, v)[2])
            out_nodes.append(node)
            for v in range(u + 1, K + 1):
                g = int(gap2[u, v])
                if g == NONE or (max_cells is not None and math.sqrt(g) > float(max_cells)):
                    continue
                a, b, dist = world_distance(u, v)
                pairs.append(dict(a=u, b=v, gap2=g, cells=math.sqrt(g), distance=dist, point_a=a, point_b=b))
        return cls(None if max_cells is None else float(max_cells), out_nodes, pairs)

    def to_dict(self):
        return dict(max_cells=self.max_cells, nodes=self.nodes, pairs=self.pairs)


def placement_from_keys(key, ticks, backend="device"):
    """``placement`` from its key lattice (0 .. 3: 1 = the rest of the scene, 2 = the moved content, 3 = both) and the lattice ticks."""
    key = lattice.as_key(key)
    n_moved, overlap = int((key >= 2).sum()), int((key == 3).sum())
    if n_moved == 0:
        lattice.refuse_empty_moved("placement")
    ticks, step = lattice.host_ticks(ticks)
    rest = lattice_distance(key, 4, sites=[1, 3], key_min=True, backend=backend)
    word = int(torch.minimum(rest["key_min"][2], rest["key_min"][3]))
    gap2 = moved_point = rest_point = None
    if word != NONE_WORD:
        gap2, at = word >> 31, word & INDEX_MASK
        moved_point, rest_point = _world(at, ticks), _world(int(rest["packed"].reshape(-1)[at]) & INDEX_MASK, ticks)
    depth2 = 0
    if overlap > 0:
        free = lattice_distance(key, 4, sites=[0, 2], backend=backend)
        depth2 = int(split(free["packed"])[0][key == 3].max())
    verdict = "collides" if overlap > 0 else "touches" if gap2 is not None and gap2 <= 3 else "clear"
    return dict(n_moved=n_moved, overlap=overlap, depth2=depth2, gap2=gap2, moved_point=moved_point, rest_point=rest_point,
                spacing=[float(abs(s)) for s in step], verdict=verdict)


@torch.no_grad()
def placement(model, renderer, edit, upsample=1, level=None):
    """Does the object that the LAST edit of ``edit`` (an ``Edit`` or an ``EditProgram``; a copy or a move, else ValueError) places collide
    with what was there?  Two transforms of ``lattice.placement_key``.  Sites {1, 3} with key_min: ``gap2`` = the smallest squared index distance
    from a point of the moved content to the rest of the scene (0 when they overlap; None when the scene holds nothing else) with the two
    world points ``moved_point`` and ``rest_point``.  Sites {0, 2}: ``depth2`` = the largest dist2 over the overlapping points, how deep
    the deepest of them lies in what was there (0 without overlap).  -> dict(n_moved, overlap = the points of key 3, depth2, gap2,
    moved_point, rest_point, spacing (3,), verdict): "collides" when overlap > 0, "touches" when gap2 <= 3 (a neighbour within the
    3 x 3 x 3 cube around a point), else "clear".  No density of the moved object on the lattice is a CliftError."""
    key, ticks = lattice.placement_key(model, renderer, edit, upsample, level)
    return placement_from_keys(key, ticks)
