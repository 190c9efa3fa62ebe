"""Shared inputs of the HDBSCAN tests (no tests here): the blob generator, the case table and a plain numpy Prim.

On these 12 cases the weights of the minimum spanning tree are pairwise distinct (asserted by the tests as a precondition), sklearn finds
3 - 6 clusters with 4 - 13 % noise points, and an MST from any algorithm -- distances in fp64 from the fp32 points, edges oriented parent ->
child from point 0 -- reproduces ``sklearn.cluster.HDBSCAN(...).fit(X).labels_`` exactly."""
import functools

import numpy as np


def blobs(seed, n, d, k=4, noise=0.15):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.1, 0.9, size=(k, d))
    per = (n - int(n * noise)) // k
    parts = [c + 0.03 * rng.standard_normal((per, d)) for c in centres]
    parts.append(rng.uniform(0.0, 1.0, size=(n - per * k, d)))
    X = np.concatenate(parts, axis=0)
    return X[rng.permutation(n)].astype(np.float32)


# (seed, n, d, min_cluster_size)
CASES = [(s, [300, 700, 1500, 2500][s % 4], 8 if s in (3, 7) else 3, [10, 15, 25, 400][s % 4]) for s in range(12)]


def dist2(X):
    """(n, n) fp64: sum_k (double(x_ik) - double(x_jk))^2 added in dimension order, every product and sum rounded separately."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    d2 = np.zeros((X.shape[0], X.shape[0]))
    for k in range(X.shape[1]):
        t = X[:, None, k] - X[None, :, k]
        d2 += t * t
    return d2


def prim_mst(X):
    """(a, b, w) of a minimum spanning tree: Prim from point 0 on the fp64 distance matrix (zero distances are ordinary edges)."""
    D = np.sqrt(dist2(X))
    n = D.shape[0]
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    best, src = D[0].copy(), np.zeros(n, dtype=np.int64)
    best[0] = np.inf
    a, b, w = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), np.zeros(n - 1)
    for e in range(n - 1):
        j = int(np.argmin(np.where(in_tree, np.inf, best)))
        a[e], b[e], w[e] = src[j], j, best[j]
        in_tree[j] = True
        closer = ~in_tree & (D[j] < best)
        best[closer], src[closer] = D[j][closer], j
    return a, b, w


@functools.lru_cache(maxsize=None)
def case(i):
    """(X, min_cluster_size, (a, b, w) of prim_mst(X)) of case i; computed once, shared, never modified by a test."""
    seed, n, d, mcs = CASES[i]
    X = blobs(seed, n, d)
    X.setflags(write=False)
    mst = prim_mst(X)
    for arr in mst:
        arr.setflags(write=False)
    return X, mcs, mst


@functools.lru_cache(maxsize=None)
def sklearn_fit(i, allow_single_cluster=True):
    """(labels_, probabilities_) of sklearn's estimator on case i."""
    from sklearn.cluster import HDBSCAN
    X, mcs, _ = case(i)
    cl = HDBSCAN(min_cluster_size=mcs, min_samples=1, allow_single_cluster=allow_single_cluster, copy=True).fit(np.array(X))
    return cl.labels_, cl.probabilities_


def is_spanning_tree(n, a, b):
    """n - 1 edges with a < b inside [0, n) that connect all n points."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != (n - 1,) or b.shape != (n - 1,) or not np.all((0 <= a) & (a < b) & (b < n)):
        return False
    root = list(range(n))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        root[find(x)] = find(y)
    return len({find(x) for x in range(n)}) == 1
