"""Shared by tests/test_distance_host.py and tests/test_gpu_distance.py (not collected by pytest): a brute force over all (point, site) pairs
and plain loops as a restatement of the contract of clift_lattice_distance (include/clift.h) that knows nothing of the package, and the key
lattices of the GPU parity test."""
import numpy as np

import clearance_cases as cc
import relations_cases as rc

NONE = 0x7fffffff                # no site: the dist2 of split, a gap2 without a pair
NONE_WORD = 0x7fffffffffffffff   # CLIFT_DT_NONE, restated
MASK = 0x7fffffff
MAX_DIM = 16384
MAX_KEYS = rc.MAX_KEYS
BRUTE_SHAPES = [(5, 6, 7), (1, 1, 9), (9, 1, 1), (1, 7, 1), (4, 4, 4), (3, 7, 13)]
DENSITIES = [0.0, 0.02, 0.1, 0.5, 1.0]
SCIPY_SHAPES = [(17, 9, 70), (33, 31, 95), (200, 3, 5)]


# ============================================================================ the contract, by brute force
def table_of(sites, n_keys):
    """None (every key >= 1), a key or a list of keys -> (n_keys,) bool."""
    t = np.zeros(n_keys, bool)
    if sites is None:
        t[1:] = True
    else:
        t[np.atleast_1d(np.asarray(sites, np.int64))] = True
    return t


def site_mask(key, n_keys, table):
    key = np.asarray(key).astype(np.int64)
    valid = (key >= 0) & (key < n_keys)
    return valid & np.asarray(table, bool)[np.where(valid, key, 0)]


def brute_packed(key, n_keys, table):
    """The packed words of the contract: for every point the minimum over ALL sites of (|p - s|^2 << 31) | lin(s)."""
    key = np.asarray(key)
    mask = site_mask(key, n_keys, table).reshape(-1)
    pts = np.stack(np.meshgrid(*[np.arange(n) for n in key.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    lin = np.flatnonzero(mask).astype(np.int64)
    if lin.size == 0:
        return np.full(key.shape, NONE_WORD, np.int64)
    out = np.empty(pts.shape[0], np.int64)
    for lo in range(0, pts.shape[0], 512):                                  # (rows of the pair matrix, 512 points at a time)
        d = ((pts[lo:lo + 512, None, :] - pts[None, lin, :]) ** 2).sum(-1)
        out[lo:lo + 512] = ((d << 31) | lin[None, :]).min(1)
    return out.reshape(key.shape)


def loop_key_min(key, n_keys, packed):
    """key_min of the contract, point by point."""
    km = [NONE_WORD] * n_keys
    for lin, (k, w) in enumerate(zip(np.asarray(key).reshape(-1).tolist(), np.asarray(packed).reshape(-1).tolist())):
        if 1 <= k < n_keys and w != NONE_WORD:
            km[k] = min(km[k], ((w >> 31) << 31) | lin)
    return np.asarray(km, np.int64)


def loop_separation(key, n_keys):
    """gap2, at, to of the contract: for every ordered pair of keys the pair matrix of their points."""
    key = np.asarray(key)
    flat = key.reshape(-1)
    pts = np.stack(np.meshgrid(*[np.arange(n) for n in key.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    gap2 = np.full((n_keys, n_keys), NONE, np.int32)
    at, to = np.full((n_keys, n_keys), -1, np.int32), np.full((n_keys, n_keys), -1, np.int32)
    where = {k: np.flatnonzero(flat == k) for k in range(1, n_keys)}
    for u in range(1, n_keys):
        for v in range(1, n_keys):
            if u == v or where[u].size == 0 or where[v].size == 0:
                continue
            d = ((pts[where[u], None, :] - pts[None, where[v], :]) ** 2).sum(-1)        # (points of u, points of v)
            word = ((d << 31) | where[v][None, :]).min(1)                               # each point of u: its packed word in transform v
            best = (((word >> 31) << 31) | where[u]).min()                              # key_min[u]
            gap2[u, v], at[u, v] = best >> 31, best & MASK
            to[u, v] = word[np.flatnonzero(where[u] == (best & MASK))[0]] & MASK
    return dict(gap2=gap2, at=at, to=to)


def check_nearest(key, n_keys, table, packed):
    """'' when every word names a site at exactly its dist2 (and sites name themselves), else what is wrong."""
    key = np.asarray(key)
    mask = site_mask(key, n_keys, table).reshape(-1)
    w = np.asarray(packed).reshape(-1)
    if not mask.any():
        return "" if (w == NONE_WORD).all() else "words without a site"
    if (w == NONE_WORD).any():
        return "an empty word beside sites"
    near, d2 = w & MASK, w >> 31
    if not mask[near].all():
        return "nearest is no site"
    p, s = np.stack(np.unravel_index(np.arange(w.size), key.shape), -1), np.stack(np.unravel_index(near, key.shape), -1)
    if not np.array_equal(((p - s) ** 2).sum(-1), d2):
        return "nearest is not at dist2"
    if not np.array_equal(near[mask], np.flatnonzero(mask)):
        return "a site does not name itself"
    return ""


def scipy_dist2(mask):
    """Squared distances to the nearest True point by scipy (its doubles, squared and rounded)."""
    from scipy import ndimage
    return np.rint(ndimage.distance_transform_edt(~mask) ** 2).astype(np.int64)


def to_numpy(tables):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in tables.items()}


def same(a, b, names):
    """'' when two dicts hold the same integers under ``names``, else the first name that differs."""
    for name in names:
        x, y = a[name], b[name]
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
            return name
    return ""


def identities(sep, clr, rel):
    """'' when the two identities hold between separation tables, clearance tables and relations tables (gap 0) of one lattice."""
    gap2 = sep["gap2"].astype(np.int64)
    pair = clr["pair"].astype(np.int64)
    bound = np.where(pair != cc.NONE, (pair + 1) ** 2, np.int64(NONE) ** 2).min(2)       # over the six directions
    if not (gap2[1:, 1:] <= np.minimum(bound, NONE)[1:, 1:]).all():
        return "gap2 <= (pair + 1)^2"
    faces = rel["faces"][1:, 1:].sum(2)
    if not np.array_equal(gap2[1:, 1:] == 1, (faces + faces.T) > 0):
        return "gap2 == 1 where there is a face"
    return ""


# ============================================================================ the cases
def random_sites(shape, density, seed):
    """A key lattice of 0 / 1 with ones at ``density``."""
    return (np.random.default_rng(seed).random(shape) < density).astype(np.int32)


def one_site(shape, at):
    key = np.zeros(shape, np.int32)
    key[at] = 1
    return key


def separation_lattices():
    """name -> (key, n_keys): lattices of tests/clearance_cases.py small enough for the pair matrices of ``loop_separation``."""
    return {"cup": (cc.cup_room(), 4), "C shape": (cc.c_shape(), 3), "slack steps": (cc.slack_steps(), 3),
            "(3, 4, 5) n_keys 33": (cc.random_key((3, 4, 5), 33, 0.3, 1), 33), "(9, 10, 67) n_keys 3": (cc.random_key((9, 10, 67), 3, 0.9, 2), 3),
            "(9, 10, 67) n_keys 33": (cc.random_key((9, 10, 67), 33, 0.9, 3), 33), "room": (rc.room(), 4)}


def identity_lattices():
    """name -> (key, n_keys): lattices of tests/clearance_cases.py for the identities with relations and clearance."""
    out = separation_lattices()
    out["(17, 9, 70) n_keys 33"] = (cc.random_key((17, 9, 70), 33, 0.9, 4), 33)
    out["skewed and sparse"] = cc.device_cases()["skewed and sparse"]
    return out


def device_cases():
    """name -> (key, n_keys, sites, key_min): the lattices of the GPU parity test."""
    out = {}
    for j, shape in enumerate(BRUTE_SHAPES + SCIPY_SHAPES):
        for density in DENSITIES if j < len(BRUTE_SHAPES) else (0.002, 0.1):
            out[f"{shape} density {density}"] = (random_sites(shape, density, 7 * j + int(100 * density)), 2, None, True)
    for n2 in (1, 63, 64, 65, 130):                                         # the chunks of a row
        out[f"(6, 5, {n2}) sparse"] = (random_sites((6, 5, n2), 0.03, n2), 2, None, True)
        out[f"(2, 3, {n2}) a site at each end of the row"] = (one_site((2, 3, n2), (slice(None), slice(None), [0, n2 - 1])), 2, None, True)
    for n in (1, 2, 65, 200):                                               # the search of unbounded length
        for a in (0, 1):
            shape = (n, 3, 70) if a == 0 else (3, n, 70)
            for end in (0, n - 1):
                at = [slice(None)] * 3
                at[a] = end
                out[f"columns of {n} along {a}, the only site at {end}"] = (one_site(shape, tuple(at)), 2, None, True)
    out["one site in a corner of (40, 40, 70)"] = (one_site((40, 40, 70), (0, 0, 0)), 2, None, True)
    out["one site in the far corner of (40, 40, 70)"] = (one_site((40, 40, 70), (39, 39, 69)), 2, None, True)
    out["all sites"] = (np.ones((7, 6, 70), np.int32), 2, None, True)
    out["all background"] = (np.zeros((7, 6, 70), np.int32), 3, None, True)
    out["background as the site"] = (random_sites((17, 9, 70), 0.7, 5), 2, [0], True)
    out["1024 keys, many in a wave"] = (cc.many_keys_in_a_wave(), MAX_KEYS, list(range(1, MAX_KEYS, 7)), True)
    out["1024 keys at random"] = (cc.random_key((9, 10, 67), MAX_KEYS, 0.5, 7), MAX_KEYS, [3, 500, 1023], True)
    out["33 keys, sites 1 .. 4"] = (cc.random_key((33, 31, 95), 33, 0.9, 9), 33, [1, 2, 3, 4], True)
    out["(200, 33, 70) one key of 8"] = (cc.random_key((200, 33, 70), 8, 0.98, 11), 8, [5], True)
    out["no key_min"] = (cc.random_key((17, 9, 70), 5, 0.8, 12), 5, [2], False)
    out["cup, all but the room"] = (cc.cup_room(), 4, [2, 3], True)
    out["rejected keys"] = (rc.cases()["rejected keys"][0], 5, None, True)
    return out
