"""Shared by tests/test_relations_host.py and tests/test_gpu_relations.py (not collected by pytest): the key lattices, a plain triple-loop
restatement of the contract of clift_lattice_relations (include/clift.h) that knows nothing of the package, and a hand-built room with the
numbers it must give."""
import numpy as np

TILE = (8, 8, 32)                # the kernel's tile extents, restated (relations.TILE is checked against it)
LDS_KEYS = 32                    # CLIFT_REL_LDS_KEYS, restated
MAX_KEYS = 1024
GAPS = (0, 1, 2, 4)


# ============================================================================ the contract, as loops
def loop_relations(key, n_keys, gap):
    """The tables of the contract, point by point.  -> dict of numpy arrays (near None when gap == 0)."""
    key = np.asarray(key)
    n = key.shape
    k = key.tolist()
    count = [0] * n_keys
    isum = [[0, 0, 0] for _ in range(n_keys)]
    ibox = [[n[0], n[1], n[2], -1, -1, -1] for _ in range(n_keys)]
    faces = np.zeros((n_keys, n_keys, 3), np.int32)
    near = np.zeros((n_keys, n_keys, 3), np.int32) if gap > 0 else None
    rejected = 0
    ok = lambda x: 0 <= x < n_keys
    for i0 in range(n[0]):
        for i1 in range(n[1]):
            for i2 in range(n[2]):
                u = k[i0][i1][i2]
                if not ok(u):
                    rejected += 1
                    continue
                p = (i0, i1, i2)
                count[u] += 1
                for a in range(3):
                    isum[u][a] += p[a]
                    ibox[u][a] = min(ibox[u][a], p[a])
                    ibox[u][3 + a] = max(ibox[u][3 + a], p[a])
                for a in range(3):
                    if p[a] + 1 >= n[a]:
                        continue
                    q = list(p)
                    q[a] += 1
                    v = k[q[0]][q[1]][q[2]]
                    if not ok(v):
                        continue
                    if v != u:
                        faces[u, v, a] += 1
                    if gap > 0 and u != 0 and v == 0:
                        for d in range(2, gap + 2):
                            if p[a] + d >= n[a]:
                                break
                            q = list(p)
                            q[a] += d
                            w = k[q[0]][q[1]][q[2]]
                            if not ok(w):
                                break
                            if w != 0:
                                if w != u:
                                    near[u, w, a] += 1
                                break
    return dict(count=np.asarray(count, np.int64), isum=np.asarray(isum, np.int64).reshape(n_keys, 3),
                ibox=np.asarray(ibox, np.int32).reshape(n_keys, 6), faces=faces, near=near, rejected=np.asarray([rejected], np.int32))


def same_tables(a, b):
    """'' when two table dicts (numpy) hold the same integers, else the name of the first that differs."""
    for name in ("count", "isum", "ibox", "faces", "near", "rejected"):
        x, y = a[name], b[name]
        if (x is None) != (y is None):
            return name
        if x is not None and (x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y)):
            return name
    return ""


def to_numpy(tables):
    return {k: None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in tables.items()}


# ============================================================================ the cases
def _random(shape, n_keys, density, seed):
    rng = np.random.default_rng(seed)
    key = rng.integers(1, max(n_keys, 2), shape).astype(np.int32) if n_keys > 1 else np.zeros(shape, np.int32)
    return np.where(rng.random(shape) < density, key, 0).astype(np.int32)


def looks(a):
    """Lines along axis ``a`` on a (19, 19, 70) lattice of background, each on coordinates of its own, three apart (a look along ``a`` stays
    on its line; along the other axes a look of depth >= 2 reaches the next line): a look-through that crosses a tile border at every depth
    1..5, runs into the lattice border, meets its own key (a hole) and meets a rejected key (9, with n_keys = 9)."""
    shape = (19, 19, 70)
    key = np.zeros(shape, np.int32)
    t, n = TILE[a], shape[a]
    lines = [[(t - 1, 1), (t - 1 + d, 2)] for d in range(1, 7)]                           # 1 0..0 2 across the tile border: d - 1 background points
    lines += [[(t - 2, 3), (t, 4)], [(t, 5), (t + 2, 6)]]                                  # the gap itself on either side of the border
    lines += [[(n - 2, 1)], [(n - 3, 2)], [(n - 1, 3)]]                                    # into the lattice border
    lines += [[(1, 4), (3, 4)], [(t - 1, 5), (t + 2, 5)], [(2, 6), (4, 6), (6, 7)]]        # holes; a hole and then another key
    lines += [[(1, 7), (3, 9)], [(t - 1, 8), (t + 1, 9), (t + 2, 1)], [(2, 9), (3, 1)], [(4, 2), (5, 9)]]      # rejected keys
    lines += [[(0, 1), (1, 2), (2, 0), (3, 2), (4, 1)]]                                    # plain faces beside a gap
    others = [b for b in range(3) if b != a]
    for j, line in enumerate(lines):
        at = [0, 0, 0]
        at[others[0]] = 1 + 3 * (j % 6)
        at[others[1]] = 1 + 3 * (j // 6) + (0 if others[1] != 2 else 28)                   # along axis 2: on either side of its tile border
        for pos, val in line:
            at[a] = pos
            key[tuple(at)] = val
    return key


def many_keys_in_a_wave():
    """256 distinct keys on (2, 8, 32): every wave of the kernel (two rows of 32 points) holds 64 distinct keys."""
    i = np.indices((2, 8, 32))
    return (1 + i[1] * 32 + i[2] + 300 * i[0]).astype(np.int32)


def skewed(shape, n_keys, seed):
    """Key 1 owns 99 % of the points; the rest is spread over all keys, background included."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.01, rng.integers(0, n_keys, shape), 1).astype(np.int32)


def room():
    """(12, 12, 10), up = +z: the floor (key 1) is all x, y at z 0..1; the table (2) x, y 2..9, z 2..5; the cup (3) x, y 4..6, z 7..8 -- one
    empty layer above the table."""
    key = np.zeros((12, 12, 10), np.int32)
    key[:, :, 0:2] = 1
    key[2:10, 2:10, 2:6] = 2
    key[4:7, 4:7, 7:9] = 3
    return key


ROOM_NODES = [(0, 0), (1, 1), (2, 1)]                          # floor: a stuff class; table and cup: things
ROOM_TICKS = [np.linspace(-1.0, 1.2, 12), np.linspace(0.0, 3.3, 12), np.linspace(0.5, 1.4, 10)]      # steps 0.2, 0.3, 0.1
# checked by hand: (table, u, v, axis) -> count
ROOM_FACES = {(1, 2, 2): 64, (1, 0, 2): 80, (2, 0, 2): 64, (0, 3, 2): 9, (0, 2, 0): 32, (2, 0, 0): 32, (0, 2, 1): 32, (2, 0, 1): 32,
              (3, 0, 2): 9, (0, 3, 0): 6, (3, 0, 0): 6, (2, 3, 2): 0, (1, 3, 2): 0}
ROOM_NEAR_GAP1 = {(2, 3, 2): 9, (1, 2, 2): 0, (1, 3, 2): 0}
ROOM_COUNT = [12 * 12 * 10 - 288 - 256 - 18, 288, 256, 18]


def cases():
    """name -> (key, n_keys, gap).  At most about 40 000 points each (the triple loop walks them all)."""
    out = {"one point": (np.ones((1, 1, 1), np.int32), 2, 1), "one row": (_random((1, 1, 7), 3, 0.7, 1), 3, 2),
           "one column": (_random((5, 1, 3), 3, 0.7, 2), 3, 4)}
    for j, shape in enumerate([(TILE[0] - 1, TILE[1] + 1, TILE[2] - 1), TILE, (TILE[0] + 1, TILE[1] - 1, TILE[2] + 1)]):
        out[f"tile extents {shape}"] = (_random(shape, 6, 0.5, 10 + j), 6, 2)
    for a in range(3):
        for gap in GAPS:
            out[f"looks along {a} gap {gap}"] = (looks(a), 9, gap)
    for n_keys in (1, 2, LDS_KEYS, LDS_KEYS + 1, MAX_KEYS):
        out[f"n_keys {n_keys}"] = (_random((9, 10, 35), n_keys, 0.6, 20 + n_keys), n_keys, 1)
    out["skewed, table in LDS"] = (skewed((16, 16, 64), 8, 3), 8, 1)
    out["64 keys in a wave"] = (many_keys_in_a_wave(), 600, 1)
    for j, (density, gap) in enumerate([(0.05, 4), (0.5, 1), (0.95, 2)]):
        out[f"random density {density}"] = (_random((17, 19, 37), 7, density, 30 + j), 7, gap)
    out["rejected keys"] = (np.where(np.random.default_rng(5).random((9, 9, 33)) < 0.1, np.random.default_rng(6).integers(-3, 12, (9, 9, 33)),
                                     _random((9, 9, 33), 5, 0.5, 7)).astype(np.int32), 5, 2)
    out["room gap 0"] = (room(), 4, 0)
    out["room gap 1"] = (room(), 4, 1)
    return out


def skew_case():
    """The one large case (262 144 points): key 1 owns 99 %, 40 keys, the kernel's table in memory."""
    return skewed((64, 64, 64), 40, 4), 40, 2


def long_cases():
    """name -> (key, n_keys, gap): thin lattices of more than 2048 tiles along one axis, so that every block of the kernel's fixed grid (at
    most 1024 blocks) walks several tiles and carries its folded moments and its table from one tile to the next -- a path that a compact
    lattice only reaches above two million points.  Runs of 37 equal keys with 3 % noise; tables in LDS (5 keys) and in memory (40 keys)."""
    out = {}
    for a, (n, n_keys) in enumerate([(8 * 2050, 5), (8 * 2050, 40), (32 * 2050, 5)]):
        shape = [2, 2, 2] if a < 2 else [1, 2, 2]
        shape[a] = n
        rng = np.random.default_rng(40 + a)
        runs = (np.indices(shape)[a] // 37) % n_keys
        out[f"long along {a}"] = (np.where(rng.random(shape) < 0.03, rng.integers(0, n_keys, shape), runs).astype(np.int32), n_keys, 2)
    return out
