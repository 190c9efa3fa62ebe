"""Shared by tests/test_clearance_host.py and tests/test_gpu_clearance.py (not collected by pytest): a plain per-column loop as a restatement of
the contract of clift_lattice_clearance (include/clift.h) that knows nothing of the package, the key lattices, hand-built cases with the
numbers they must give, and the two identities that tie the tables to those of clift_lattice_relations."""
import numpy as np

import relations_cases as rc

NONE = 0x7fffffff                # CLIFT_CLR_NONE, restated
MAX_SLACK = 4
LDS_KEYS = rc.LDS_KEYS
MAX_KEYS = rc.MAX_KEYS
NAMES = ("pair", "travel", "landing", "rejected")
PX, MX, PY, MY, PZ, MZ = range(6)


# ============================================================================ the contract, as loops
def column_events(column, n_keys):
    """The events of one column, a list of keys: [(u, v, g)] with u below v."""
    out, last, last_i = [], None, 0
    for j, k in enumerate(column):
        if not 0 <= k < n_keys:
            last = None                                                     # a rejected key ends the look from both sides
        elif k != 0:
            if last is not None and last != k:
                out.append((last, k, j - last_i - 1))
            last, last_i = k, j
    return out


def loop_clearance(key, n_keys, slack):
    """The tables of the contract, column by column.  -> dict of numpy arrays."""
    key = np.asarray(key)
    n = key.shape
    events = []                                                             # (u, v, d, g), both directions
    for a in range(3):
        cols = np.moveaxis(key, a, 2).reshape(-1, n[a]).tolist()
        for col in cols:
            for u, v, g in column_events(col, n_keys):
                events.append((u, v, 2 * a, g))
                events.append((v, u, 2 * a + 1, g))
    pair = np.full((n_keys, n_keys, 6), NONE, np.int32)
    for u, v, d, g in events:
        pair[u, v, d] = min(pair[u, v, d], g)
    travel = pair.min(axis=1)
    landing = np.zeros((n_keys, n_keys, 6), np.int32)
    for u, v, d, g in events:
        if g <= int(travel[u, d]) + slack:
            landing[u, v, d] += 1
    rejected = int(((key < 0) | (key >= n_keys)).sum())
    return dict(pair=pair, travel=travel, landing=landing, rejected=np.asarray([rejected], np.int32))


def same_tables(a, b):
    """'' when two table dicts (numpy) hold the same integers, else the name of the first that differs."""
    for name in NAMES:
        x, y = a[name], b[name]
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
            return name
    return ""


def to_numpy(tables):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in tables.items()}


def identities(clr, rel, gap):
    """'' when the two identities hold between clearance tables and relations tables of one lattice (``gap`` as given to relations)."""
    pair = clr["pair"][1:, 1:, 0::2]                                        # (u, v, a) for the + directions, keys >= 1
    faces = rel["faces"][1:, 1:]
    if not np.array_equal(pair == 0, faces > 0):
        return "faces"
    if gap >= 1 and not np.array_equal(pair <= gap, faces + rel["near"][1:, 1:] > 0):
        return "near"
    return ""


# ============================================================================ the cases
def random_key(shape, n_keys, background, seed):
    """Keys 1 .. n_keys - 1 at random, background with probability ``background``."""
    rng = np.random.default_rng(seed)
    key = rng.integers(1, max(n_keys, 2), shape).astype(np.int32)
    return np.where(rng.random(shape) < background, 0, key).astype(np.int32)


def cup_room():
    """(12, 12, 12) inside a room (key 1: floor z 0, walls and ceiling all around), the table (2) x, y 2..9, z 1..4, the cup (3) x, y 4..6,
    z 8..9: 3 empty points above the table."""
    key = np.zeros((12, 12, 12), np.int32)
    key[[0, -1], :, :] = 1
    key[:, [0, -1], :] = 1
    key[:, :, [0, -1]] = 1
    key[2:10, 2:10, 1:5] = 2
    key[4:7, 4:7, 8:10] = 3
    return key


CUP_NODES = [(0, 0), (1, 1), (2, 1)]
CUP_TICKS = [np.linspace(-1.0, 1.2, 12), np.linspace(0.0, 3.3, 12), np.linspace(0.5, 1.6, 12)]      # steps 0.2, 0.3, 0.1


def c_shape():
    """(1, 10, 5): one C-shaped object (key 1) -- a back along y 1..6 at z 0 and two arms along z at y 1 and y 6 that face each other across
    background -- and a point of key 2 at y 9, z 2: the column along y at z 2 reads 0 1 0 0 0 0 1 0 0 2, so the arms give no event and the
    only event of the lattice is (1, 2, +y, 2), counted from the second arm."""
    key = np.zeros((1, 10, 5), np.int32)
    key[0, 1:7, 0] = 1
    key[0, 1, 0:4] = key[0, 6, 0:4] = 1
    key[0, 9, 2] = 2
    return key


def rejected_between():
    """(1, 1, 9): 1 0 9 0 2 0 0 3 with n_keys = 4: the rejected key stands between 1 and 2; 2 and 3 are two points apart."""
    return np.asarray([1, 0, 9, 0, 2, 0, 0, 3, 0], np.int32).reshape(1, 1, 9)


def slack_steps():
    """(1, 2, 8), two columns along z: key 2 hovers 1 point over key 1 in the first and 2 points over it in the second."""
    key = np.zeros((1, 2, 8), np.int32)
    key[0, :, 0] = 1
    key[0, 0, 2] = 2
    key[0, 1, 3] = 2
    return key


def many_keys_in_a_wave():
    """Hundreds of distinct keys (up to 896) on (4, 4, 64), a third of the points background: the 64 points of a row (one wave along z) all
    carry different keys, and so do the 64 columns of a group."""
    i = np.indices((4, 4, 64))
    key = (1 + (i[2] // 2) + 32 * (i[1] // 2) + 64 * (i[0] // 2) + 256 * (i[2] % 2) + 512 * (i[1] % 2)) % 1024
    hole = ((i[0] + i[1] + i[2]) % 3) == 0
    return np.where(hole, 0, key).astype(np.int32)


def long_carries():
    """name -> key: two keys at index 1 and 200 along one axis and nothing between (the run spans several 64-point chunks of a row, or 199
    steps of a lane's walk), and columns that are non-zero only at their two ends."""
    out = {}
    for a, shape in enumerate([(300, 2, 2), (2, 300, 2), (2, 2, 256)]):
        key = np.zeros(shape, np.int32)
        at = [slice(None)] * 3
        at[a] = 1
        key[tuple(at)] = 1
        at[a] = 200
        key[tuple(at)] = 2
        out[f"two keys 199 apart along {a}"] = key
        ends = np.zeros(shape, np.int32)
        at[a] = 0
        ends[tuple(at)] = 1
        at[a] = shape[a] - 1
        ends[tuple(at)] = 2
        out[f"the two ends of a column along {a}"] = ends
    return out


def device_cases():
    """name -> (key, n_keys): the lattices of the GPU parity test, beside ``long_carries``."""
    out = {}
    shapes = [(1, 1, 1), (1, 1, 64), (1, 1, 65), (2, 3, 129), (17, 9, 70), (33, 31, 95)]
    for j, shape in enumerate(shapes):
        for n_keys in (2, 3, LDS_KEYS, LDS_KEYS + 1):
            out[f"{shape} n_keys {n_keys}"] = (random_key(shape, n_keys, (0.3, 0.9)[(j + n_keys) % 2], 100 + 10 * j + n_keys), n_keys)
    out["1024 keys, many in a wave"] = (many_keys_in_a_wave(), MAX_KEYS)
    out["1024 keys at random"] = (random_key((9, 10, 67), MAX_KEYS, 0.5, 7), MAX_KEYS)
    out["skewed, table in LDS"] = (rc.skewed((16, 16, 64), 8, 3), 8)
    out["skewed, table in memory"] = (rc.skewed((16, 16, 64), 40, 4), 40)
    sparse = np.where(np.random.default_rng(8).random((16, 16, 64)) < 0.9, 0, rc.skewed((16, 16, 64), 8, 5)).astype(np.int32)
    out["skewed and sparse"] = (sparse, 8)
    for name, key in long_carries().items():
        out[name] = (key, 3)
    out["all background"] = (np.zeros((5, 6, 70), np.int32), 3)
    out["one key"] = (np.ones((5, 6, 70), np.int32), 2)
    out["n_keys 1"] = (np.zeros((3, 3, 3), np.int32), 1)
    out["cup"] = (cup_room(), 4)
    out["C shape"] = (c_shape(), 3)
    out["rejected between"] = (rejected_between(), 4)
    out["rejected keys"] = (rc.cases()["rejected keys"][0], 5)
    return out
