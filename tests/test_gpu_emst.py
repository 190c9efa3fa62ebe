"""clift_emst (csrc/emst.hip) on the GPU against a numpy Prim on the fp64 distance matrix (tests/hdbscan_cases.py).

The weight multiset of a minimum spanning tree is unique even under ties, and the kernel's d2 is the same fp64 arithmetic with a correctly
rounded sqrt: the sorted weights must be equal BIT FOR BIT.  The edges must form a spanning tree with a < b."""
import math

import numpy as np
import pytest
import torch

import hdbscan_cases as hc
from contrastive_lift_amd import _lib

pytestmark = pytest.mark.gpu


def emst(X, ldx=None, work_bytes=None):
    """Raw call: (a, b, w, info) numpy arrays.  ``ldx`` > d pads the rows with NaN columns (they must not be read)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    if ldx is not None:
        wide = np.full((n, ldx), np.nan, dtype=np.float32)
        wide[:, :d] = X
        X = wide
    x = torch.as_tensor(X, device="cuda")
    a = torch.full((n - 1,), -7, dtype=torch.int32, device="cuda")
    b = torch.full((n - 1,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((n - 1,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    nbytes = int(_lib.load().clift_emst_work_bytes(n)) if work_bytes is None else work_bytes
    work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device="cuda")
    _lib.call("clift_emst", _lib.ptr(x), n, x.stride(0), d, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), _lib.ptr(info), _lib.ptr(work), nbytes,
              _lib.stream())
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy(), info.cpu().numpy()


def lattice():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(5).permutation(len(g))].astype(np.float32)


def duplicated():
    X = hc.blobs(21, 300, 3)
    rng = np.random.default_rng(6)
    X[rng.choice(300, 40, replace=False)] = X[rng.choice(300, 40, replace=False)]
    return X


def two_far_blobs():
    rng = np.random.default_rng(8)
    X = 0.01 * rng.standard_normal((130, 3))
    X[65:, 0] += 100.0
    return X.astype(np.float32)


SETS = {
    "n2": lambda: (hc.blobs(30, 2, 3, k=1), None),
    "n3": lambda: (hc.blobs(31, 3, 3, k=1), None),
    "n257": lambda: (hc.blobs(32, 257, 3), None),
    "n1025": lambda: (hc.blobs(33, 1025, 3), None),
    "ldx": lambda: (hc.blobs(34, 300, 3), 6),
    "d8": lambda: (hc.blobs(35, 300, 8), None),
    "d32": lambda: (hc.blobs(36, 300, 32), None),
    "d5_ldx": lambda: (hc.blobs(37, 261, 5), 8),
    "d1": lambda: (hc.blobs(38, 300, 1), None),                 # d = 1, 2, 4: launch_nearest<4, false, 2>
    "d2_ldx": lambda: (hc.blobs(39, 261, 2), 5),
    "d4": lambda: (hc.blobs(40, 300, 4), None),
    "d9": lambda: (hc.blobs(41, 300, 9), None),                 # d = 9 - 16: launch_nearest<16, false, 1>
    "d16_ldx": lambda: (hc.blobs(42, 257, 16), 19),
    "d17": lambda: (hc.blobs(43, 300, 17), None),
    "same_point": lambda: (np.tile(np.float32([[0.25, 0.5, 0.75]]), (64, 1)), None),
    "duplicates": lambda: (duplicated(), None),
    "lattice": lambda: (lattice(), None),
    "two_far_blobs": lambda: (two_far_blobs(), None),
}


@pytest.mark.parametrize("name", list(SETS))
def test_weights_bit_equal_and_spanning(name):
    X, ldx = SETS[name]()
    n = X.shape[0]
    a, b, w, info = emst(X, ldx)
    ref = np.sort(hc.prim_mst(X)[2])
    print(name, "rounds", info[0], "max |dw|", float(np.abs(np.sort(w) - ref).max()))
    assert info[1] == 1 and info[2] == 0 and info[3] == 0 and 1 <= info[0] <= math.ceil(math.log2(n)), info
    assert hc.is_spanning_tree(n, a, b)
    assert np.array_equal(np.sort(w).view(np.int64), ref.view(np.int64))
    d2 = hc.dist2(X)
    assert np.array_equal(w.view(np.int64), np.sqrt(d2[a, b]).view(np.int64))            # every edge carries its own length
    again = emst(X, ldx)
    for u, v in zip((a, b, w, info), again):
        assert np.array_equal(u.view(np.int64) if u.dtype == np.float64 else u, v.view(np.int64) if v.dtype == np.float64 else v)
    if name == "two_far_blobs":
        assert np.sum(w > 50.0) == 1
    if name == "same_point":
        assert np.all(w == 0.0)


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    x = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    out = [torch.full((8,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    w = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    work = torch.zeros((lib.clift_emst_work_bytes(8) // 8 + 1,), dtype=torch.int64, device="cuda")
    P = _lib.ptr
    good = dict(X=P(x), n=8, ldx=3, d=3, a=P(out[0]), b=P(out[1]), w=P(w), info=P(info), work=P(work), bytes=work.numel() * 8)
    bad = [("n = 1", dict(n=1), "n >= 2"), ("n = 131073", dict(n=131073), "CLIFT_EMST_MAX_N"), ("d = 33", dict(d=33, ldx=33), "feature width"),
           ("d = 0", dict(d=0), "d >= 1"), ("ldx < d", dict(ldx=2), "ldx"), ("small work", dict(bytes=lib.clift_emst_work_bytes(8) - 1), "work_bytes"),
           ("NULL X", dict(X=None), "NULL"), ("NULL edge_a", dict(a=None), "NULL"), ("NULL edge_w", dict(w=None), "NULL"),
           ("NULL info", dict(info=None), "NULL"), ("NULL work", dict(work=None), "NULL")]
    for what, change, word in bad:
        k = dict(good, **change)
        rc = lib.clift_emst(k["X"], k["n"], k["ldx"], k["d"], k["a"], k["b"], k["w"], k["info"], k["work"], k["bytes"], _lib.stream())
        assert rc != 0, what
        assert word in lib.clift_last_error().decode(), (what, lib.clift_last_error().decode())
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out + [w, info]) and bool((work == 0).all())      # nothing was launched
    assert lib.clift_emst_work_bytes(131072) == 256 + 131072 * 236
    with pytest.raises(_lib.CliftError, match="clift_emst"):
        _lib.call("clift_emst", good["X"], 1, 3, 3, good["a"], good["b"], good["w"], good["info"], good["work"], good["bytes"], _lib.stream())
