"""Shared inputs of the connected-component tests and the CPU restatement of the rule (contrastive_lift_amd/components.py):
two lattice points belong together iff they are neighbours under the connectivity and carry the same non-zero key; components are numbered
1..K by ascending first (smallest linear index) point; root = that first point, -1 for background.  Not a test module.

Two restatements, independent of the package: ``flood_fill`` (a breadth-first fill in scan order, plain Python) and ``scipy_labels`` (one
scipy.ndimage.label call per distinct key, renumbered by first point)."""
import collections
import itertools

import numpy as np

from mesh_cases import CLASS_OFFSETS

CONNECTIVITIES = (6, "kuhn", 26)
RANDOM_MASK_COUNTS = {6: 3248, "kuhn": 828, 26: 74}            # components of random_mask(), checked with scipy 1.15


def offsets(connectivity):
    """All neighbour offsets of a connectivity (both signs)."""
    if connectivity == 6:
        return [d for d in itertools.product((-1, 0, 1), repeat=3) if sum(abs(x) for x in d) == 1]
    if connectivity == 26:
        return [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    if connectivity in ("kuhn", 14):
        return [tuple(s * x for x in d) for d in CLASS_OFFSETS for s in (1, -1)]
    raise ValueError(connectivity)


def structure(connectivity):
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for d in offsets(connectivity):
        s[1 + d[0], 1 + d[1], 1 + d[2]] = True
    return s


def flood_fill(key, connectivity):
    """-> (labels int32, sizes (K + 1) int64, roots int32) by a breadth-first fill started at every unlabelled point in scan order."""
    key = np.asarray(key).astype(np.int64)
    shape = key.shape
    labels, roots = np.zeros(shape, np.int32), np.full(shape, -1, np.int32)
    offs, sizes = offsets(connectivity), [0]
    for start in zip(*np.nonzero(key)):                        # nonzero walks in linear-index order
        if labels[start]:
            continue
        k, lab, first = key[start], len(sizes), int(np.ravel_multi_index(start, shape))
        labels[start], roots[start] = lab, first
        queue, n = collections.deque([start]), 1
        while queue:
            p = queue.popleft()
            for d in offs:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if min(q) < 0 or q[0] >= shape[0] or q[1] >= shape[1] or q[2] >= shape[2] or labels[q] or key[q] != k:
                    continue
                labels[q], roots[q] = lab, first
                queue.append(q)
                n += 1
        sizes.append(n)
    return labels, np.asarray(sizes, np.int64), roots


def scipy_labels(key, connectivity):
    """-> (labels int32, sizes (K + 1) int64) through scipy.ndimage.label, one call per distinct key, renumbered by first point."""
    from scipy import ndimage
    key = np.asarray(key).astype(np.int64)
    prov, n_all = np.zeros(key.shape, np.int64), 0
    for v in np.unique(key[key != 0]):
        lab, n = ndimage.label(key == v, structure=structure(connectivity))
        prov[lab > 0] = lab[lab > 0] + n_all
        n_all += n
    flat = prov.reshape(-1)
    at = np.flatnonzero(flat)
    _, first_at = np.unique(flat[at], return_index=True)       # first occurrence of every provisional label, by label
    lut = np.zeros(n_all + 1, np.int64)
    lut[1:][np.argsort(at[first_at])] = np.arange(1, n_all + 1)
    labels = lut[prov].astype(np.int32)
    return labels, np.concatenate([[0], np.bincount(labels.reshape(-1), minlength=n_all + 1)[1:]]).astype(np.int64)


# --------------------------------------------------------------------------- key lattices
def random_mask():
    """(33, 17, 65): the sizes straddle any power-of-two tile in every axis."""
    return np.random.default_rng(1).random((33, 17, 65)) < 0.2


def thin_cases():
    rng = np.random.default_rng(4)
    return {f"thin{'x'.join(map(str, s))}": rng.random(s) < 0.55 for s in ((70, 5, 3), (3, 5, 70), (1, 1, 40), (2, 2, 2))}


def checkerboard():
    i, j, k = np.indices((10, 9, 34))
    return (i + j + k) % 2 == 0


def snake():
    """A one-point-wide boustrophedon path through 17^3: every even layer holds the same serpentine (its even rows, joined at alternating
    ends), consecutive layers are joined at alternating ends of it.  1457 points, one component under 6, a path: the longest root chains
    a lattice of this size can make."""
    m = np.zeros((17, 17, 17), bool)
    for i in range(0, 17, 2):
        m[i, 0::2, :] = True
        m[i, 1::4, 16] = True
        m[i, 3::4, 0] = True
    for n, i in enumerate(range(1, 17, 2)):
        m[(i, 16, 16) if n % 2 == 0 else (i, 0, 0)] = True
    return m


def keyed():
    return np.random.default_rng(2).integers(0, 4, (9, 10, 11)).astype(np.int32)


def key_cases():
    """name -> key lattice (bool or int32): every case the device is compared on."""
    cases = {"random": random_mask(), "empty": np.zeros((6, 11, 21), bool), "full": np.ones((6, 11, 21), bool), "checkerboard": checkerboard(),
             "snake": snake(), "keyed": keyed(), "split": split_lattice()}
    cases.update(thin_cases())
    with np.errstate(invalid="ignore"):
        cases["floater"] = floater_volume()["vol"] >= 0.0
    return cases


# --------------------------------------------------------------------------- the floater volume
FLOATER_BALLS = (((14, 15, 16), 9.5), ((32, 8, 8), 2.6), ((30, 30, 34), 3.2), ((8, 30, 36), 2.6))        # the two 2.6 balls tie in size
FLOATER_SPECKS = ((36, 20, 5), (3, 3, 38), (20, 35, 3))


def floater_volume():
    """(40, 38, 42) fp32, level 0: vol = max over the balls of (radius - distance), floor -1, plus three single-point specks of 0.7.  One
    large ball, three small ones (two of the same size) and the specks; no two touch under 26 and none touches the lattice boundary, so
    every component's surface is a closed sphere."""
    shape = (40, 38, 42)
    idx = np.indices(shape).astype(np.float64)
    vol = np.full(shape, -1.0)
    for c, r in FLOATER_BALLS:
        vol = np.maximum(vol, r - np.sqrt(sum((idx[a] - c[a]) ** 2 for a in range(3))))
    for s in FLOATER_SPECKS:
        vol[s] = 0.7
    ticks = [np.linspace(-1.0, 1.0, n).astype(np.float32) for n in shape]
    return dict(name="floater", vol=vol.astype(np.float32), level=0.0, ticks=ticks, n_components=len(FLOATER_BALLS) + len(FLOATER_SPECKS))


# --------------------------------------------------------------------------- id lattices for split_disconnected
def split_lattice():
    """(12, 20, 24) int32, three ids: 1 and 3 in one box each, 2 in two separated boxes (210 and 120 points) plus a 3-point crumb."""
    k = np.zeros((12, 20, 24), np.int32)
    k[1:5, 1:6, 1:7] = 1
    k[6:11, 2:8, 2:9] = 2                                      # 210 points: keeps the id
    k[2:6, 12:17, 14:20] = 2                                   # 120 points: a fresh id
    k[9, 16, 3:6] = 2                                          # the crumb
    k[7:11, 11:18, 10:22] = 3
    return k


def split_order_lattice():
    """(1, 1, 60) int32 of runs: id 1 in fragments of 5, 3, 3 points (a tie), id 2 in fragments of 4, 6, 2 -- in this order along the row."""
    k = np.zeros((1, 1, 60), np.int32)
    for start, n, v in ((1, 5, 1), (8, 4, 2), (14, 3, 1), (19, 6, 2), (27, 3, 1), (32, 2, 2)):
        k[0, 0, start:start + n] = v
    return k
