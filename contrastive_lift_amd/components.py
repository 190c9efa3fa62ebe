"""Connected components of a keyed 3-D lattice (csrc/components.hip: clift_cc_label) and what the surface export does with
them: drop the floaters of a density lattice before it is meshed, and give the separated pieces of one instance id ids of their own.

    vol, info = filter_components(sigma, level, min_voxels=64)           # then mesh.extract_isosurface(vol, level, ticks)
    labels, sizes = label_components(key)                                # 1..K by ascending first point, sizes[0] = 0
    new_key, table = split_disconnected(id_lattice)                      # the largest fragment keeps the id, the others get fresh ones

Two lattice points belong together iff they are neighbours under ``connectivity`` and carry the same non-zero key.  Connectivity 6 = faces,
26 = full, 14 = "kuhn" = +-d for the seven non-zero d in {0,1}^3: the seven edge classes of the mesher.  All vertex pairs of a Kuhn
tetrahedron are Kuhn edges, so with "kuhn" a face of the mesh belongs to one component of the inside set and to no second one -- dropping
a component removes whole closed pieces of the surface and touches nothing else.

``backend="device"`` is the kernel plus torch on the device; ``backend="host"`` gives the same integers through scipy.ndimage.label (one
call per distinct key) for machines and tests without a GPU.  What the lattice modules share is in ``lattice``.
"""
import numpy as np
import torch

from . import _lib, lattice

KUHN_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))       # the mesher's edge classes, in its order
_CONNECTIVITY = {6: 6, 14: 14, 26: 26, "6": 6, "14": 14, "26": 26, "kuhn": 14}


def connectivity_code(connectivity):
    """6 / 26 / 14 / "kuhn" (numbers also as strings) -> 6, 14 or 26."""
    try:
        return _CONNECTIVITY[connectivity]
    except (KeyError, TypeError):
        raise ValueError(f"connectivity must be 6, 26, 14 or 'kuhn' (got {connectivity!r})") from None


def structure(connectivity):
    """The (3, 3, 3) bool neighbourhood of a connectivity, as scipy.ndimage.label takes it."""
    code = connectivity_code(connectivity)
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for d in np.ndindex(3, 3, 3):
        o = tuple(x - 1 for x in d)
        n = sum(abs(x) for x in o)
        if n and (code == 26 or (code == 6 and n == 1) or (code == 14 and (o in KUHN_OFFSETS or tuple(-x for x in o) in KUHN_OFFSETS))):
            s[d] = True
    return s


def _roots_host(key, code):
    from scipy import ndimage
    k = key.cpu().numpy()
    root = np.full(k.size, -1, np.int64)
    st = structure(code)
    for v in np.unique(k):
        if v == 0:
            continue
        lab, n = ndimage.label(k == v, structure=st)
        lab = lab.reshape(-1)
        at = np.flatnonzero(lab)
        first = np.full(n + 1, k.size, np.int64)
        np.minimum.at(first, lab[at], at)
        root[at] = first[lab[at]]
    return torch.from_numpy(root.astype(np.int32)).reshape(k.shape).to(key.device)


def component_roots(key, connectivity="kuhn", backend="device"):
    """root (n0, n1, n2) int32: the smallest linear index of any point of the component, -1 where key == 0."""
    code, key = connectivity_code(connectivity), lattice.as_lattice(key, "component_roots")
    if key.numel() == 0:                                                     # (an empty lattice has no component: no error here)
        return torch.zeros_like(key)
    if lattice.check_backend(backend) == "host":
        return _roots_host(key, code)
    lattice.require_device(key, "component_roots")
    root = torch.empty_like(key)
    _lib.call("clift_cc_label", _lib.ptr(key), *key.shape, code, _lib.ptr(root), _lib.stream())
    return root


def _label(key, connectivity, backend):
    """-> (labels like key int32, sizes (K + 1) int64, first (K + 1) int64: the smallest linear index of every component, first[0] = -1)."""
    root = component_roots(key, connectivity, backend)
    dev, flat = root.device, root.reshape(-1)
    is_root = flat == torch.arange(flat.shape[0], dtype=torch.int32, device=dev)
    rank = torch.cumsum(is_root, 0, dtype=torch.int32)                      # number of the component whose first point is <= p
    labels = torch.where(flat >= 0, rank[flat.clamp(min=0).long()], torch.zeros_like(flat))
    first = torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), is_root.nonzero().reshape(-1)])
    # the counts by sorting (every label 1..K occurs): torch.bincount's atomic histogram serialises on the bin of a dominant component --
    # 7.7 against 0.16 ms on a 256^3 lattice with one component of 634 000 points among 278 000; the same integers
    counts = torch.unique(labels[flat >= 0], return_counts=True)[1]
    sizes = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts])
    return labels.reshape(root.shape), sizes, first


@torch.no_grad()
def label_components(key, connectivity="kuhn", backend="device"):
    """Components of ``key`` (n0, n1, n2) bool or integer, 0 = background -> (labels int32 of key's shape, 0 = background, the components
    numbered 1..K by ascending first (smallest linear index) point; sizes (K + 1) int64 with sizes[0] = 0), both on key's device."""
    labels, sizes, _ = _label(key, connectivity, backend)
    return labels, sizes


@torch.no_grad()
def filter_components(vol, level, min_voxels=0, keep_largest=None, connectivity="kuhn", backend="device"):
    """Drop small components of the inside set ``vol >= level`` (NaN is outside, as in the mesher) -> (vol_filtered, info).  A component is
    dropped if it has fewer than ``min_voxels`` points, and with ``keep_largest=k`` also if it is not among the k largest (ties go to the
    smaller first point).  Dropped points are set to the largest normal fp32 below ``level`` -- finite, outside, and the smallest change of
    the lattice that makes them so; everything else comes back bit for bit, in a new tensor.  info: K, sizes (K + 1), kept (the ids that
    stay, ascending), dropped (the number of points).  With both options off nothing is labelled and ``vol`` itself is returned (info: K
    None, dropped 0)."""
    min_voxels = int(min_voxels or 0)
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError(f"keep_largest must be >= 0 (got {keep_largest})")
    if min_voxels <= 0 and keep_largest is None:
        return vol, dict(K=None, sizes=None, kept=None, dropped=0)
    if not torch.is_tensor(vol) or vol.dtype != torch.float32 or vol.dim() != 3:
        raise ValueError("vol must be a float32 tensor (n0, n1, n2)")
    lvl = torch.tensor(float(level), dtype=torch.float32)
    fill = torch.nextafter(lvl, torch.tensor(-float("inf")))
    if abs(float(fill)) < torch.finfo(torch.float32).tiny:                   # no denormal: a comparison that flushes would read it as 0
        fill = torch.tensor(-torch.finfo(torch.float32).tiny)
    if not bool(torch.isfinite(lvl)) or not bool(torch.isfinite(fill)):
        raise ValueError(f"level must be finite with a finite fp32 below it (got {level})")
    labels, sizes, _ = _label(vol >= lvl.to(vol.device), connectivity, backend)
    K = sizes.shape[0] - 1
    keep = sizes >= min_voxels
    keep[0] = False
    if keep_largest is not None and int(keep_largest) < K:
        order = torch.sort(-sizes[1:], stable=True).indices + 1              # descending size, then ascending id = ascending first point
        top = torch.zeros_like(keep)
        top[order[:int(keep_largest)]] = True
        keep &= top
    drop = (labels > 0) & ~keep[labels.long()]
    out = torch.where(drop, fill.to(vol.device), vol)
    return out, dict(K=K, sizes=sizes, kept=keep.nonzero().reshape(-1), dropped=int(drop.sum()))


@torch.no_grad()
def split_disconnected(key, connectivity="kuhn", min_voxels=1, backend="device", first_fresh=None):
    """Give the separated pieces of one id ids of their own -> (new_key like key, bool as int32; table).  For every id the largest fragment
    (ties: the smaller first point) keeps the id; every other fragment with at least ``min_voxels`` points gets a fresh id max(key) + 1,
    + 2, ... in the order (ascending original id, descending size, ascending first point); smaller fragments keep the parent's id.
    table: {fresh id: the id it was split from}.  ``first_fresh``: the fresh ids start there if that is above max(key) + 1 (a caller that
    holds further ids which the lattice does not).  Ids are positive: a negative key is refused (max(key) + 1 could be the background)."""
    if not torch.is_tensor(key):
        key = torch.from_numpy(np.ascontiguousarray(key))
    out_dtype = torch.int32 if key.dtype == torch.bool else key.dtype
    labels, sizes, first = _label(key, connectivity, backend)
    K = sizes.shape[0] - 1
    if K == 0:
        return key.to(out_dtype, copy=True), {}
    flat = key.reshape(-1)
    comp_key = flat[first[1:]].cpu().numpy().astype(np.int64)               # K values: the table work is per component, on the host
    if comp_key.min() < 0:
        raise ValueError(f"split_disconnected: ids must be positive (found {int(comp_key.min())})")
    size = sizes[1:].cpu().numpy()
    ids = np.arange(1, K + 1)
    order = np.lexsort((ids, -size, comp_key))                              # id, then size descending, then first point
    ck, sz = comp_key[order], size[order]
    largest = np.ones(K, bool)
    largest[1:] = ck[1:] != ck[:-1]
    fresh = ~largest & (sz >= int(min_voxels))
    new_of = ck.copy()
    new_of[fresh] = max(int(comp_key.max()) + 1, int(first_fresh or 0)) + np.arange(int(fresh.sum()))
    table = {int(n): int(p) for n, p in zip(new_of[fresh], ck[fresh])}
    lut = np.zeros(K + 1, np.int64)
    lut[ids[order]] = new_of
    new_key = torch.from_numpy(lut).to(key.device)[labels.reshape(-1).long()].to(out_dtype)
    return new_key.reshape(key.shape), table


@torch.no_grad()
def vertex_owner_inside(keys, vol, level):
    """The linear index of the INSIDE endpoint of each vertex's edge.  ``keys``: the ``return_keys=True`` keys of
    ``mesh.extract_isosurface``, 7 * lin(owner) + class.  -> the owner if vol[owner] >= level, else the owner plus the class's offset."""
    if not torch.is_tensor(vol):
        vol = torch.from_numpy(np.ascontiguousarray(vol, np.float32))
    if not torch.is_tensor(keys):
        keys = torch.from_numpy(np.ascontiguousarray(keys, np.int64))
    keys = keys.to(vol.device).long()
    _, n1, n2 = (int(x) for x in vol.shape)
    step = torch.tensor([(d0 * n1 + d1) * n2 + d2 for d0, d1, d2 in KUHN_OFFSETS], dtype=torch.int64, device=vol.device)
    owner, cls = keys // 7, keys % 7
    inside = vol.reshape(-1)[owner] >= torch.tensor(float(level), dtype=torch.float32, device=vol.device)
    return torch.where(inside, owner, owner + step[cls])
