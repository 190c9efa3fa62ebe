"""Cases and the brute force of the placement map, shared by tests/test_placement_host.py and tests/test_gpu_placement.py.
Not a test module.  The brute force is a loop over the translations, the cells and the neighbour rule, written from the rules of
include/clift.h and independent of the numpy backend of contrastive_lift_amd/placement.py."""
import functools
import itertools

import numpy as np

NONE_WORD = 0x7fffffffffffffff   # CLIFT_PM_NONE, restated
NAMES = ("overlap", "support", "count", "best", "rejected")
DIRECTIONS = ("+x", "-x", "+y", "-y", "+z", "-z")


def table_of(solid, n_keys):
    """``solid`` -> (n_keys,) bool, restated: None = every key >= 1, an int, an iterable of keys, a bool array."""
    table = np.zeros(n_keys, bool)
    if solid is None:
        table[1:] = True
    elif isinstance(solid, np.ndarray) and solid.dtype == np.bool_:
        table[:] = solid
    else:
        table[[solid] if isinstance(solid, (int, np.integer)) else list(solid)] = True
    return table


def brute(key, n_keys, solid, shape, direction, target=(0, 0, 0), min_support=1):
    """The five tables by loops.  ``target`` must lie inside T."""
    key, shape = np.asarray(key).astype(np.int64), np.asarray(shape)
    table = table_of(solid, n_keys)
    n, m = key.shape, shape.shape
    T = tuple(n[a] - m[a] + 1 for a in range(3))
    d = DIRECTIONS.index(direction)
    e = [0, 0, 0]
    e[d // 2] = 1 if d % 2 == 0 else -1

    def is_solid(p):
        if any(p[a] < 0 or p[a] >= n[a] for a in range(3)):
            return False                                                     # the lattice border is not a floor
        k = int(key[p])
        return 0 <= k < n_keys and bool(table[k])
    cells = [tuple(int(x) for x in c) for c in np.argwhere(shape != 0)]
    inside = set(cells)
    faces = [c for c in cells if tuple(c[a] + e[a] for a in range(3)) not in inside]
    overlap, support = np.zeros(T, np.int32), np.zeros(T, np.int32)
    count, best = [0, 0], [NONE_WORD, NONE_WORD]
    for lin, t in enumerate(itertools.product(*[range(x) for x in T])):
        overlap[t] = sum(is_solid(tuple(t[a] + c[a] for a in range(3))) for c in cells)
        support[t] = sum(is_solid(tuple(t[a] + c[a] + e[a] for a in range(3))) for c in faces)
        word = (sum((t[a] - target[a]) ** 2 for a in range(3)) << 31) | lin
        for which, yes in enumerate((overlap[t] == 0, overlap[t] == 0 and support[t] >= min_support)):
            if yes:
                count[which] += 1
                best[which] = min(best[which], word)
    rejected = int(((key < 0) | (key >= n_keys)).sum())
    return dict(overlap=overlap, support=support, count=np.asarray(count, np.int32), best=np.asarray(best, np.int64),
                rejected=np.asarray([rejected], np.int32))


def to_numpy(tables):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in tables.items()}


def same(a, b, names=NAMES):
    """'' when two table dicts (numpy) hold the same integers, else the name of the first that differs."""
    for name in names:
        x, y = a[name], b[name]
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
            return name
    return ""


# ============================================================================ the cases
def random_case(n, m, density, fill, seed, n_keys=4, solid=None, target=None, min_support=1):
    """A lattice ``n`` with keys 1 .. n_keys - 1 at ``density`` (else 0) and a shape ``m`` filled at ``fill`` whose two opposite corners are
    cells, so that its index box is the whole of m."""
    rng = np.random.default_rng(seed)
    key = np.where(rng.random(n) < density, rng.integers(1, max(n_keys, 2), n), 0).astype(np.int32)
    shape = (rng.random(m) < fill).astype(np.uint8)
    shape[0, 0, 0] = shape[-1, -1, -1] = 1
    T = tuple(n[a] - m[a] + 1 for a in range(3))
    return dict(key=key, n_keys=n_keys, solid=solid, shape=shape, target=tuple(x // 2 for x in T) if target is None else target, min_support=min_support)


# lattice, object, solid density, shape fill: words that straddle 64-bit borders along z (n2 and m2 at 63, 64, 65 and above 128), objects
# longer than 64 along x and y, sparse shapes with empty rows, more than one block
TABLE = [((5, 6, 7), (2, 3, 2), 0.3, 0.7), ((6, 5, 63), (2, 2, 1), 0.05, 1.0), ((6, 5, 64), (2, 2, 63), 0.01, 0.5), ((6, 5, 65), (2, 2, 64), 0.01, 0.5),
         ((3, 4, 130), (2, 2, 65), 0.01, 0.5), ((3, 4, 200), (2, 3, 129), 0.004, 0.3), ((70, 5, 6), (65, 2, 3), 0.01, 0.5),
         ((5, 70, 6), (2, 65, 3), 0.01, 0.5), ((40, 33, 70), (7, 9, 33), 0.002, 0.3)]
SMALL = "(5, 6, 7) object (2, 3, 2)"
NONE_CASES = ("a single translation", "all solid", "an empty lattice")


def _raw_cases():
    out = {}
    for j, (n, m, density, fill) in enumerate(TABLE):
        out[f"{n} object {m}"] = random_case(n, m, density, fill, 1000 + j, min_support=1 + j % 2)
    out["(9, 3, 5) object (9, 1, 1)"] = random_case((9, 3, 5), (9, 1, 1), 0.05, 0.6, 21)
    out["T2 = 1: (4, 5, 66) object (2, 2, 66)"] = random_case((4, 5, 66), (2, 2, 66), 0.004, 0.4, 22)
    mixed = np.random.default_rng(23).random(1024) < 0.5
    out["1024 keys, a mixed solid table"] = random_case((9, 10, 67), (2, 2, 3), 0.3, 0.8, 24, n_keys=1024, solid=mixed, target=(100, -4, 30))
    out["solid names key 0 too"] = random_case((6, 7, 9), (1, 2, 2), 0.8, 1.0, 25, n_keys=5, solid=[0, 2])
    rejected = random_case((7, 6, 70), (2, 2, 5), 0.1, 0.7, 26, n_keys=3)
    rejected["key"][::3, 1::2, ::5] = np.random.default_rng(27).choice([-1, 3, 9, -1000], rejected["key"][::3, 1::2, ::5].shape)
    out["rejected keys"] = rejected
    out["a single translation"] = random_case((6, 6, 6), (6, 6, 6), 0.1, 0.5, 28)
    solid = random_case((5, 4, 6), (2, 2, 2), 1.0, 0.8, 29)
    out["all solid"] = solid
    empty = random_case((5, 4, 70), (2, 3, 5), 0.0, 0.6, 30)
    out["an empty lattice"] = empty
    return out


def host_of(case, direction):
    from contrastive_lift_amd import placement
    return to_numpy(placement.placement_tables(case["key"], case["shape"], case["n_keys"], case["solid"], direction, case["target"],
                                               case["min_support"], backend="host"))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(key, n_keys, solid, shape, target, min_support).  Every case outside ``NONE_CASES`` has a free translation, and a free
    and supported one for at least one direction (asserted here with the numpy backend, which tests/test_placement_host.py holds to the
    brute force): a kernel that returns zeros cannot agree with it."""
    out = _raw_cases()
    for name, case in out.items():
        if name in NONE_CASES:
            continue
        counts = [host_of(case, d)["count"] for d in DIRECTIONS]
        assert all(c[0] >= 1 for c in counts) and any(c[1] >= 1 for c in counts), (name, [c.tolist() for c in counts])
    return out


@functools.lru_cache(maxsize=None)
def host_tables():
    """(name, direction) -> the tables of backend="host": computed once, left unchanged."""
    return {(name, d): host_of(case, d) for name, case in cases().items() for d in DIRECTIONS}


# ============================================================================ hand lattices
def hover_room():
    """(6, 6, 14), two keys: key 1 = a floor at z 0 and a block x, y 1..2, z 1..3 on it; key 2 = an object with a foot: a plate x, y 3..4 at
    z 8 and one foot cell (3, 3, 7) under it.  Along -z the foot travels 6 steps to the floor and lands on one face."""
    key = np.zeros((6, 6, 14), np.int32)
    key[:, :, 0] = 1
    key[1:3, 1:3, 1:4] = 1
    key[3:5, 3:5, 8] = 2
    key[3, 3, 7] = 2
    return key
