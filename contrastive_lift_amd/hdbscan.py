"""HDBSCAN(min_cluster_size, min_samples=1) with the minimum spanning tree on the GPU -- the reference's ``--use_dbscan`` clustering
(inference/render_panopli.py:236-241, 321-326) without the CPU fit.

With ``min_samples=1`` every core distance is 0, the mutual-reachability graph is the plain Euclidean graph, and the fit is the Euclidean
minimum spanning tree of the points (``clift_emst``: brute-force Boruvka, fp64 distances from the fp32 points) followed by a pass over its
n - 1 edges.  That pass is host code, restated here from the algorithm as scikit-learn's estimator runs it (``sklearn/cluster/_hdbscan``:
``_linkage.pyx`` for the single-linkage tree, ``_tree.pyx`` for the condensed tree, the stabilities, excess-of-mass selection, labels and
probabilities) -- none of sklearn's private modules is imported:

* the tree is rooted at point 0 and every edge made (parent, child): the edges sklearn's Prim from node 0 emits, which fixes left / right in
  the dendrogram and with it the cluster numbering;
* the edges sorted by weight are merged by union-find into the single-linkage tree (the only Python loop over n - 1 items);
* condensing is vectorised: a point leaves its cluster at the merge above the topmost ancestor smaller than ``min_cluster_size`` (pointer
  jumping), a cluster ends at the first merge of two parts that both reach ``min_cluster_size``, and those merges are numbered in the
  breadth-first order of the dendrogram (depth, then left to right);
* a cluster's stability is summed down its spine in the order sklearn adds the terms (same bits), selection and labelling loop over the
  clusters only.

``fit`` needs the weights of the tree to decide nothing twice: with pairwise distinct weights (any real feature cloud) the result equals
``sklearn.cluster.HDBSCAN(...).fit(X).labels_`` exactly and ``probabilities_`` to rounding; tied weights are ordered by (weight, child) here.
"""
import numpy as np

from . import _lib


def device_emst(X, device="cuda"):
    """clift_emst on ``device``: (a, b, w, info) as numpy arrays -- the n - 1 edges (a < b, w fp64) and the 4 info ints.  Raises CliftError
    when the tree is incomplete or a fault flag is set (non-finite input: flag 2)."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CliftError(f"DeviceHDBSCAN: clift_emst runs on a GPU device, got {dev}")
    x = torch.as_tensor(np.array(X, dtype=np.float32, order="C"), device=dev)          # (a copy: X may be read-only)
    n, d = x.shape
    if n < 2:
        raise ValueError(f"DeviceHDBSCAN: need at least 2 points (got {n})")
    with torch.cuda.device(dev):
        a = torch.empty((n - 1,), dtype=torch.int32, device=dev)
        b = torch.empty((n - 1,), dtype=torch.int32, device=dev)
        w = torch.empty((n - 1,), dtype=torch.float64, device=dev)
        info = torch.zeros((4,), dtype=torch.int32, device=dev)
        nbytes = max(int(_lib.load().clift_emst_work_bytes(n)), 8)
        work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        _lib.call("clift_emst", _lib.ptr(x), n, x.stride(0), d, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), _lib.ptr(info), _lib.ptr(work),
                  work.numel() * 8, _lib.stream())
        info = info.cpu().numpy()
    if info[2] != 0 or info[1] != 1:
        why = " (non-finite input)" if info[2] & 2 else ""
        raise _lib.CliftError(f"clift_emst: fault flags {int(info[2])}, {int(info[1])} components left after {int(info[0])} rounds{why}")
    return a.cpu().numpy().astype(np.int64), b.cpu().numpy().astype(np.int64), w.cpu().numpy(), info


def orient_edges(n, a, b):
    """(parent, child) of every edge of the spanning tree (a, b) rooted at point 0."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import breadth_first_order
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if a.shape != (n - 1,) or b.shape != (n - 1,) or (n > 1 and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n)):
        raise _lib.CliftError(f"DeviceHDBSCAN: the tree of {n} points needs {n - 1} edges between points 0 .. {n - 1}")
    g = csr_matrix((np.ones(2 * (n - 1)), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))
    order, pred = breadth_first_order(g, 0, directed=True, return_predecessors=True)
    down = pred[b] == a
    parent, child = np.where(down, a, b), np.where(down, b, a)
    if len(order) != n or not np.array_equal(pred[child], parent):
        raise _lib.CliftError("DeviceHDBSCAN: the edges do not form a spanning tree")
    return parent, child


def single_linkage(n, a, b, w):
    """The single-linkage tree of a spanning tree: (left, right, dist, size) of the n - 1 merges in weight order; merge i makes node n + i
    from ``left`` (the side of the edge's parent end) and ``right`` (its child end), nodes below n are points."""
    parent, child = orient_edges(n, a, b)
    w = np.asarray(w, dtype=np.float64)
    order = np.lexsort((child, w))
    cur, nxt = parent[order].tolist(), child[order].tolist()
    up = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    left, right = [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        x = cur[i]
        rx = x
        while up[rx] != rx:
            rx = up[rx]
        while up[x] != rx:
            up[x], x = rx, up[x]
        y = nxt[i]
        ry = y
        while up[ry] != ry:
            ry = up[ry]
        while up[y] != ry:
            up[y], y = ry, up[y]
        new = n + i
        left[i], right[i] = rx, ry
        up[rx] = up[ry] = new
        size[new] = size[rx] + size[ry]
    return np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64), w[order], np.asarray(size[n:], dtype=np.int64)


def _settle(jump):
    """Pointer jumping to the fixed point of ``jump`` (every chain ends in a node that maps to itself)."""
    while True:
        nxt = jump[jump]
        if np.array_equal(nxt, jump):
            return jump
        jump = nxt


def tree_labels(n, linkage, min_cluster_size, allow_single_cluster=True):
    """Condensed tree, stabilities, excess-of-mass selection (cluster_selection_epsilon = 0, no max_cluster_size), labels and probabilities of
    a single-linkage tree (``single_linkage``).  Returns (labels (n) int64 with -1 = noise, probabilities (n) fp64)."""
    mcs = int(min_cluster_size)
    L, R, dist, msize = linkage
    N, root, ids = 2 * n - 1, 2 * n - 2, np.arange(2 * n - 1)
    par = np.empty(N, dtype=np.int64)
    par[L] = par[R] = np.arange(n, N)
    par[root] = root
    sz = np.concatenate([np.ones(n, dtype=np.int64), msize])
    big = sz >= mcs
    big[root] = True
    with np.errstate(divide="ignore"):
        lam_node = np.concatenate([np.zeros(n), np.where(dist > 0.0, 1.0 / dist, np.inf)])       # lambda of the merge that made a node
    # depth of every node in the dendrogram (pointer doubling)
    anc, dep = par.copy(), (ids != root).astype(np.int64)
    while not np.all(anc == root):
        dep = dep + dep[anc]
        anc = anc[anc]
    # a point falls out of its cluster at the parent of its topmost small ancestor (itself included)
    small = ~big
    top = _settle(np.where(small & small[par], par, ids))[:n]
    fall = par[top]
    pt_lam, pt_dep = lam_node[fall], dep[fall]
    # clusters: the root, and both sides of every merge of two big nodes; numbered in breadth-first order of those merges
    is_split = np.zeros(N, dtype=bool)
    is_split[n:] = big[L] & big[R]
    head = _settle(np.where((ids == root) | is_split[par], ids, par))                            # top node of the cluster a big node is in
    splits = np.nonzero(is_split)[0]
    split_of = dict(zip(head[splits].tolist(), splits.tolist()))                                 # a cluster ends at its one split, if any
    rank, stack = {}, [split_of.get(root)]
    while stack:                                                                                 # preorder, left first: left-to-right at equal depth
        t = stack.pop()
        if t is None:
            continue
        rank[t] = len(rank)
        stack.append(split_of.get(int(R[t - n])))
        stack.append(split_of.get(int(L[t - n])))
    splits = np.asarray(sorted(rank, key=lambda t: (dep[t], rank[t])), dtype=np.int64)
    K = 1 + 2 * len(splits)
    label = np.zeros(N, dtype=np.int64)                                                          # cluster index of a head (root: 0)
    label[L[splits - n]] = 1 + 2 * np.arange(len(splits))
    label[R[splits - n]] = 2 + 2 * np.arange(len(splits))
    node_cluster = label[head]                                                                   # (meaningful on big nodes)
    cl_parent = np.zeros(K, dtype=np.int64)
    cl_parent[1:] = np.repeat(node_cluster[splits], 2)
    cl_birth = np.zeros(K)
    cl_birth[1:] = np.repeat(lam_node[splits], 2)
    cl_size = np.zeros(K, dtype=np.int64)
    cl_size[1::2], cl_size[2::2] = sz[L[splits - n]], sz[R[splits - n]]
    pt_cluster = node_cluster[fall]
    # stability: sum of (lambda - birth) * size over a cluster's rows, added down its spine as sklearn's row order adds them
    row_c = np.concatenate([pt_cluster, cl_parent[1:]])
    row_lam = np.concatenate([pt_lam, cl_birth[1:]])
    row_dep = np.concatenate([pt_dep, np.repeat(dep[splits], 2)])
    row_side = np.concatenate([np.zeros(n, dtype=np.int64), np.tile([0, 1], len(splits))])
    row_size = np.concatenate([np.ones(n, dtype=np.int64), cl_size[1:]])
    with np.errstate(invalid="ignore"):
        row_val = (row_lam - cl_birth[row_c]) * row_size
    o = np.lexsort((row_side, row_dep, row_c))
    stab = np.bincount(row_c[o], weights=row_val[o], minlength=K).tolist()
    deaths = np.zeros(K)
    np.maximum.at(deaths, row_c, row_lam)
    # excess of mass, children before parents
    kids = [[] for _ in range(K)]
    for c in range(1, K):
        kids[cl_parent[c]].append(c)
    keep = [False] * K
    for c in range(K - 1, -1 if allow_single_cluster else 0, -1):
        sub = float(np.sum([stab[k] for k in kids[c]]))
        if sub > stab[c]:
            stab[c] = sub
        else:
            keep[c] = True
    selected, covered, rep = [False] * K, [False] * K, [0] * K
    for c in range(K):
        above = covered[cl_parent[c]] if c else False
        selected[c] = keep[c] and not above
        covered[c] = above or keep[c]
        rep[c] = c if selected[c] else (rep[cl_parent[c]] if c else 0)
    chosen = [c for c in range(K) if selected[c]]
    number = np.full(K, -1, dtype=np.int64)
    number[chosen] = np.arange(len(chosen))
    pt_rep = np.asarray(rep, dtype=np.int64)[pt_cluster]
    labels = number[pt_rep]
    at_root = pt_rep == 0
    if selected[0]:                                               # the root alone: the points that stayed until its last row's lambda
        labels = np.where(at_root & (pt_lam < deaths[0]), -1, labels)
    else:
        labels = np.where(at_root, -1, labels)
    # membership strength: lambda at which the point left over the largest lambda of its cluster
    prob = np.zeros(n)
    m = labels >= 0
    top_lam = deaths[np.asarray(chosen, dtype=np.int64)[labels[m]]] if len(chosen) else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob[m] = np.where((top_lam == 0.0) | np.isinf(pt_lam[m]), 1.0, np.minimum(pt_lam[m], top_lam) / top_lam)
    return labels, prob


class DeviceHDBSCAN:
    """``sklearn.cluster.HDBSCAN(min_cluster_size, min_samples=1, allow_single_cluster)`` with the minimum spanning tree from ``clift_emst``
    and the tree pass of this module.  ``fit`` sets ``labels_`` (int64, -1 = noise), ``probabilities_`` (fp64), ``mst_`` (a, b, w) and
    ``n_rounds_`` (Boruvka rounds; None with ``mst_fn``).  X is taken as fp32 (the reference clusters fp32 features).  ``relabel(m)`` redoes
    only the tree pass for another ``min_cluster_size`` on the stored tree -- the tree does not depend on it, so a sweep costs one kernel run
    per point set.  ``mst_fn(X) -> (a, b, w)`` replaces the kernel (CPU tests of the host logic).  Only ``min_samples=1``, the reference's
    setting: with more, the mutual-reachability weights tie massively and the tree is not unique."""

    def __init__(self, min_cluster_size, min_samples=1, allow_single_cluster=True, device="cuda", mst_fn=None):
        if int(min_samples) != 1:
            raise ValueError(f"DeviceHDBSCAN supports min_samples=1 only (got {min_samples})")
        self.min_cluster_size = self._size(min_cluster_size)
        self.allow_single_cluster, self.device, self.mst_fn = bool(allow_single_cluster), device, mst_fn

    @staticmethod
    def _size(m):
        if int(m) != m or int(m) < 2:
            raise ValueError(f"min_cluster_size must be an integer >= 2 (got {m!r})")
        return int(m)

    def fit(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[0] < 2:
            raise ValueError(f"DeviceHDBSCAN.fit: need a (n >= 2, d) array (got shape {X.shape})")
        if self.mst_fn is not None:
            a, b, w = self.mst_fn(X)
            self.n_rounds_ = None
        else:
            a, b, w, info = device_emst(X, self.device)
            self.n_rounds_ = int(info[0])
        self.mst_ = (np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(w, dtype=np.float64))
        self._n = X.shape[0]
        self._linkage = single_linkage(self._n, *self.mst_)
        return self.relabel(self.min_cluster_size)

    def relabel(self, min_cluster_size):
        self.min_cluster_size = self._size(min_cluster_size)
        self.labels_, self.probabilities_ = tree_labels(self._n, self._linkage, self.min_cluster_size, self.allow_single_cluster)
        return self
