"""Placement map of a keyed 3-D lattice (csrc/placement.hip: clift_lattice_placement): for EVERY translation of an object's voxel
shape over the lattice the number of cells that collide and the number of faces it would rest on, and the nearest translation at which it
fits and stands -- where ``clearance`` looks along one axis and ``distance.placement`` at a single position.

    t = lattice_placement(key, shape, n_keys, solid=None, direction="-z", target=(3, 4, 5))   # overlap, support (T), count, best, rejected
    dist2, where = split_best(int(t["best"][1]), t["overlap"].shape)         # the nearest free and supported translation, or None
    shape, origin = object_of(key, u)                                        # the cells of key u in its index box, and the box's low corner
    t = node_placement(key, n_keys, u)                                       # where else node u could stand
    summary = PlacementMap.from_tables(t, origin, ticks)                     # fp64 on the host; summary.to_json()
    snap = snap_offset(model, renderer, edit.move(box, t, shape=sh))         # found, steps (3,), offset (3,), support, ...

The rules (in full: include/clift.h).  A point is solid when its key is valid (0 .. n_keys - 1) and ``solid`` names it.  The object lies wholly
inside the lattice with the corner of its box at t: T = n - m + 1 translations per axis, ``lin_T(t) = (t0 T1 + t1) T2 + t2``.
``overlap[t]`` = the cells c of the shape with t + c solid; ``support[t]`` = the cells c whose neighbour c + e_d along ``direction`` is not a
cell of the shape (a neighbour outside the shape's box is not) and has t + c + e_d a solid lattice point -- the lattice border is not a floor.
``count`` = (the free translations, overlap == 0; those of them with support >= ``min_support``); ``best`` = of each kind the minimum of
``(|t - target|^2 << 31) | lin_T(t)``, ``NONE_WORD`` where there is none.  Distances are in index units.

``backend="device"`` is one call (three launches: the two masks of the shape, the bit-packed lattice, the correlation); ``backend="host"``
gives the same integers in numpy -- one shifted slice of the zero-padded solid lattice per mask cell, added into int32 -- for machines and
tests without a GPU.  What the lattice modules share is in ``lattice``.
"""
import numpy as np
import torch

from . import _lib, lattice
from .lattice import INDEX_MASK, NONE_WORD

def work_words(n, m):
    """CLIFT_PM_WORK_WORDS: the int64 words of scratch for a lattice ``n`` and a shape ``m``."""
    mw = (m[2] + 2 + 63) // 64
    wp = (n[2] - m[2] + 1 + 63) // 64 + mw
    return (n[0] + 2) * (n[1] + 2) * wp + 2 * (m[0] + 2) * (m[1] + 2) * mw


def _as_shape(shape, n):
    """-> the object's cells as a contiguous uint8 tensor (m0, m1, m2) of 0 and 1, on the caller's device."""
    if not torch.is_tensor(shape):
        shape = torch.from_numpy(np.ascontiguousarray(shape))
    if shape.dim() != 3:
        raise ValueError(f"shape must be (m0, m1, m2), got {tuple(shape.shape)}")
    if shape.dtype.is_floating_point or shape.dtype.is_complex:
        raise ValueError(f"shape must be bool or integer, got {shape.dtype}")
    m = tuple(int(x) for x in shape.shape)
    if min(m) < 1 or any(m[a] > n[a] for a in range(3)):
        raise ValueError(f"every shape dimension must be 1 .. the lattice's (got {m[0]} x {m[1]} x {m[2]} in {n[0]} x {n[1]} x {n[2]})")
    shape = (shape != 0).to(torch.uint8).contiguous()
    if not bool(shape.any()):
        raise ValueError("the shape holds no cell")
    return shape, m


def _correlate_host(pad, mask, T):
    out = np.zeros(T, np.int32)
    for s0, s1, s2 in np.argwhere(mask):
        out += pad[s0:s0 + T[0], s1:s1 + T[1], s2:s2 + T[2]]
    return out


def _best_host(mask, word):
    return int(word[mask].min()) if mask.any() else NONE_WORD


def _tables_host(key, n_keys, table, shape, d, min_support, target):
    k = key.cpu().numpy().astype(np.int64)
    valid = (k >= 0) & (k < n_keys)
    n, m = k.shape, tuple(shape.shape)
    T = tuple(n[a] - m[a] + 1 for a in range(3))
    pad = np.zeros(tuple(x + 2 for x in n), np.int32)                      # the lattice with one empty point around it: p' = p + 1
    pad[1:-1, 1:-1, 1:-1] = valid & table[np.where(valid, k, 0)]
    cells = np.zeros(tuple(x + 2 for x in m), bool)                        # the shape's box grown by one: c' = c + 1
    cells[1:-1, 1:-1, 1:-1] = shape.cpu().numpy() != 0
    shadow = np.roll(cells, 1 if d % 2 == 0 else -1, axis=d // 2) & ~cells  # (the grown border is empty: nothing wraps around)
    overlap, support = _correlate_host(pad, cells, T), _correlate_host(pad, shadow, T)
    idx = np.indices(T).astype(np.int64)
    dist2 = sum((idx[a] - target[a]) ** 2 for a in range(3))
    word = (dist2 << 31) | ((idx[0] * T[1] + idx[1]) * T[2] + idx[2])
    free = overlap == 0
    stands = free & (support >= min_support)
    out = dict(overlap=overlap, support=support, count=np.asarray([int(free.sum()), int(stands.sum())], np.int32),
               best=np.asarray([_best_host(free, word), _best_host(stands, word)], np.int64), rejected=np.asarray([int((~valid).sum())], np.int32))
    return {name: torch.from_numpy(v).to(key.device) for name, v in out.items()}


def _tables(key, shape, n_keys, solid, direction, target, min_support, backend):
    key, n_keys = lattice.prepare(key, n_keys, "lattice_placement", lattice.MAX_DIM)
    lattice.check_backend(backend)
    n = tuple(key.shape)
    shape, m = _as_shape(shape, n)
    d = lattice.direction_index(direction)
    min_support = int(min_support)
    if min_support < 1:
        raise ValueError(f"min_support must be >= 1 (got {min_support})")
    table = lattice.key_table(solid, n_keys)
    T = tuple(n[a] - m[a] + 1 for a in range(3))
    target = (0, 0, 0) if target is None else tuple(int(x) for x in target)
    if len(target) != 3:
        raise ValueError(f"target must be three indices, got {target}")
    target = tuple(min(max(target[a], 0), T[a] - 1) for a in range(3))
    if backend == "host":
        return _tables_host(key, n_keys, table, shape, d, min_support, target), n_keys
    lattice.require_device(key, "lattice_placement")
    dev = key.device
    shape = shape.to(dev)
    site = torch.from_numpy(table.astype(np.uint8)).to(dev)
    out = dict(overlap=torch.empty(T, dtype=torch.int32, device=dev), support=torch.empty(T, dtype=torch.int32, device=dev),
               count=torch.empty(2, dtype=torch.int32, device=dev), best=torch.empty(2, dtype=torch.int64, device=dev),
               rejected=torch.empty(1, dtype=torch.int32, device=dev))
    work = torch.empty(work_words(n, m), dtype=torch.int64, device=dev)
    _lib.call("clift_lattice_placement", _lib.ptr(key), *n, n_keys, _lib.ptr(site), _lib.ptr(shape), *m, d, min_support, *target,
              _lib.ptr(out["overlap"]), _lib.ptr(out["support"]), _lib.ptr(out["count"]), _lib.ptr(out["best"]), _lib.ptr(out["rejected"]),
              _lib.ptr(work), _lib.stream())
    return out, n_keys


@torch.no_grad()
def placement_tables(key, shape, n_keys=None, solid=None, direction="-z", target=None, min_support=1, backend="device"):
    """The placement map of ``shape`` (m0, m1, m2) bool or integer, a non-zero entry is a cell, over a key lattice (n0, n1, n2) bool or
    integer, as a dict of tensors on key's device -- ``overlap`` and ``support`` (T) int32, ``count`` (2) int32, ``best`` (2) int64,
    ``rejected`` (1) int32 -- whatever ``rejected`` says (``lattice_placement`` raises on it).  ``solid``: the forms of
    ``lattice.key_table``, None = every key >= 1.  ``direction``: "+x" .. "-z".  ``target``: three indices, None = (0, 0, 0); one outside
    T is clamped.  ``n_keys=None``: max(key) + 1.  A shape without a cell is a ValueError."""
    return _tables(key, shape, n_keys, solid, direction, target, min_support, backend)[0]


@torch.no_grad()
def lattice_placement(key, shape, n_keys=None, solid=None, direction="-z", target=None, min_support=1, backend="device"):
    """``placement_tables``; raises CliftError when a point's key lies outside [0, n_keys)."""
    out, n_keys = _tables(key, shape, n_keys, solid, direction, target, min_support, backend)
    lattice.raise_on_rejected(out, n_keys, "lattice_placement")
    return out


def split_best(word, T):
    """A word of ``best`` and the translation counts T -> (dist2, (t0, t1, t2)), or None for ``NONE_WORD``."""
    word = int(word)
    if word == NONE_WORD:
        return None
    lin = word & INDEX_MASK
    return word >> 31, (lin // (int(T[1]) * int(T[2])), (lin // int(T[2])) % int(T[1]), lin % int(T[2]))


def object_of(key, u):
    """-> (shape, origin): the points of key ``u`` cropped to their index box (``lattice.index_box``) as a uint8 tensor on key's device,
    and the box's low corner (three ints).  A key that no point carries is a ValueError."""
    key = lattice.as_key(key)
    u = int(u)
    if u < 0:
        raise ValueError(f"the key of an object is >= 0 (got {u})")
    box = lattice.index_box(key, u + 1)[u]
    if box[3] < 0:
        raise ValueError(f"no lattice point carries key {u}")
    lo, hi = [int(x) for x in box[:3]], [int(x) + 1 for x in box[3:]]
    return (key[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == u).to(torch.uint8).contiguous(), tuple(lo)


@torch.no_grad()
def node_placement(key, n_keys, u, direction="-z", min_support=1, backend="device"):
    """Where else could node ``u`` stand?  ``lattice_placement`` of shape = ``object_of(key, u)`` over the lattice with every key >= 1
    except u solid, the target u's own origin -> (tables, origin)."""
    key, n_keys = lattice.prepare(key, n_keys, "node_placement", lattice.MAX_DIM)
    u = int(u)
    if not 1 <= u < n_keys:
        raise ValueError(f"node key {u} lies outside [1, {n_keys})")
    shape, origin = object_of(key, u)
    solid = np.zeros(n_keys, bool)
    solid[1:] = True
    solid[u] = False
    return lattice_placement(key, shape, n_keys, solid, direction, origin, min_support, backend), origin


class PlacementMap(lattice.Summary):
    """The summary of ``PlacementMap.from_tables``: ``n_translations``, ``n_free``, ``n_supported`` and, for ``best_free`` and
    ``best_supported``, a dict (None where there is none) of the translation, the step vector from the origin, the world offset, overlap
    and support there, and dist2."""

    def __init__(self, origin, n_translations, n_free, n_supported, best_free, best_supported):
        self.origin, self.n_translations, self.n_free, self.n_supported = origin, n_translations, n_free, n_supported
        self.best_free, self.best_supported = best_free, best_supported

    @classmethod
    def from_tables(cls, tables, origin, ticks):
        """``tables``: the tables of ``lattice_placement``; ``origin``: where the object stands now, three indices (``object_of``);
        ``ticks``: the three uniform coordinate arrays of the lattice (``renderer.lattice_ticks``).  fp64 on the host: ``offset`` = the
        steps times the tick spacing of each axis, signed."""
        host = lattice.to_host(tables, ("overlap", "support", "count", "best"))
        T = host["overlap"].shape
        origin = [int(x) for x in origin]
        _, step = lattice.host_ticks(ticks)

        def entry(word):
            found = split_best(word, T)
            if found is None:
                return None
            dist2, t = found
            steps = [t[a] - origin[a] for a in range(3)]
            return dict(translation=list(t), steps=steps, offset=[float(steps[a] * step[a]) for a in range(3)],
                        overlap=int(host["overlap"][t]), support=int(host["support"][t]), dist2=int(dist2))
        return cls(origin, int(np.prod(T)), int(host["count"][0]), int(host["count"][1]), entry(host["best"][0]), entry(host["best"][1]))

    def to_dict(self):
        return dict(origin=self.origin, n_translations=self.n_translations, n_free=self.n_free, n_supported=self.n_supported,
                    best_free=self.best_free, best_supported=self.best_supported)


def snap_from_keys(key, ticks, direction="-z", min_support=1, backend="device"):
    """``snap_offset`` from its key lattice (0 .. 3: 1 = the rest of the scene, 2 = the moved content, 3 = both) and the lattice ticks."""
    key = lattice.as_key(key)
    lattice.direction_index(direction)
    n_moved = int((key >= 2).sum())
    if n_moved == 0:
        lattice.refuse_empty_moved("snap_offset")
    shape, origin = object_of(key >= 2, 1)
    tables = lattice_placement(key, shape, 4, [1, 3], direction, origin, min_support, backend)
    T = tuple(tables["overlap"].shape)
    _, step = lattice.host_ticks(ticks)
    found = split_best(tables["best"][1], T)
    dist2, t = found if found is not None else (None, origin)
    steps = np.asarray([t[a] - origin[a] for a in range(3)], np.int64)
    return dict(found=found is not None, steps=steps, offset=steps * step, overlap_before=int(tables["overlap"][origin]),
                support_before=int(tables["support"][origin]), support=int(tables["support"][t]) if found is not None else None, dist2=dist2,
                n_free=int(tables["count"][0]), n_supported=int(tables["count"][1]), n_moved=n_moved, direction=direction,
                spacing=np.abs(step))


@torch.no_grad()
def snap_offset(model, renderer, edit, direction="-z", upsample=1, level=None, min_support=1):
    """The nearest place where the object that the LAST edit of ``edit`` (an ``Edit`` or an ``EditProgram``; a copy or a move, else
    ValueError) places fits and stands: the companion of ``clearance.settle_offset`` (one axis) and ``distance.placement`` (one position).
    The lattice is ``lattice.placement_key`` (R + 2 M); the shape and its origin are the moved content cropped to its index box, solid is
    what stood there before the paste (keys 1 and 3), the target is the origin.  -> dict(found, steps (3,) int, offset (3,) fp64 world
    translation, overlap_before = overlap[origin], support_before, support and dist2 at the chosen translation, n_free, n_supported,
    n_moved, direction, spacing (3,)); ``found`` is False, the steps and the offset zero and support and dist2 None when no free
    translation has ``min_support`` faces along ``direction``.  No density of the moved object on the lattice is a CliftError."""
    key, ticks = lattice.placement_key(model, renderer, edit, upsample, level)
    return snap_from_keys(key, ticks, direction, min_support)
