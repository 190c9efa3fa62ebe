"""Shared inputs of the linear-assignment tests (test_linear_assignment_host.py on the CPU, test_gpu_linear_assignment.py on the GPU):
the images of the fused loss, the matrices of the solver alone, the oracle's cost matrix restated so that a test can see it, and the margin
of an optimum.  Everything is generated from fixed seeds, in a fixed order; nothing here touches the GPU."""
import functools

import numpy as np
import scipy.optimize
import torch

MATCHING_SHAPES = [(6, 8, 64), (3, 2, 50), (25, 40, 300), (4, 4, 10), (64, 64, 1024), (65, 30, 257), (500, 30, 256)]      # (E, ids, n)


@functools.lru_cache(maxsize=None)
def matching_cases():
    """[(name, labels (n,) int64, scores (n, E) float32)]: 28 random images (four draws per shape, more ids than slots among them), one wide
    structured image, and two hand-built ones."""
    g = torch.Generator().manual_seed(0)
    out = []
    for E, ids, n in MATCHING_SHAPES:
        for k in range(4):
            y = torch.randint(1, ids + 1, (n,), generator=g)
            f = 3 * torch.randn(n, E, generator=g)
            out.append((f"E{E}_ids{ids}_n{n}_{k}", y, f))
    g = torch.Generator().manual_seed(3)
    E, ids, n = 500, 120, 1024
    y = torch.randint(1, ids + 1, (n,), generator=g)
    perm = torch.randperm(E, generator=g)
    f = torch.randn(n, E, generator=g)
    f[torch.arange(n), perm[y]] += 8
    out.append((f"structured_E{E}_ids{ids}_n{n}", y, f))
    g = torch.Generator().manual_seed(11)
    out.append(("one_id", torch.full((33,), 7, dtype=torch.int64), 3 * torch.randn(33, 5, generator=g)))
    # zero and negative ids are ids like any other; three ids, two slots: the largest id (5) stays unmatched
    out.append(("ids_0_5_-3_E2", torch.tensor([0, 5, -3] * 10, dtype=torch.int64), 3 * torch.randn(30, 2, generator=g)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def solver_cases():
    """[(name, kind, cost float32 (L, E))] with kind in "random" (unique optimum), "integer" (ties), "product" (long paths), "nan"."""
    rng = np.random.default_rng(7)
    out = []
    for L, E in [(1, 1), (1, 7), (5, 5), (25, 25), (30, 65), (64, 64), (100, 500), (256, 512), (512, 512)]:
        out.append((f"random_{L}x{E}", "random", rng.uniform(-1, 0, (L, E)).astype(np.float32)))
    for L, E in [(5, 5), (7, 20), (40, 64), (64, 65), (100, 500)]:
        out.append((f"integer_{L}x{E}", "integer", rng.integers(0, 4, (L, E)).astype(np.float32)))
    for L, E in [(40, 40), (60, 100)]:
        out.append((f"product_{L}x{E}", "product", np.outer(np.arange(1, L + 1), np.arange(1, E + 1)).astype(np.float32)))
    c = rng.uniform(-1, 0, (6, 6)).astype(np.float32)          # square: the NaN row (it counts as zeros) takes the column that is left, no tie
    c[2, :] = np.nan
    out.append(("nan_row_6x6", "nan", c))
    return tuple(out)


def oracle_cost(labels_gt, scores):
    """The cost matrix inside oracle.losses.virtual_labels_linear_assignment, by the same loop: (ids, cost float64 (L, E))."""
    ids = sorted(torch.unique(labels_gt).cpu().tolist())[:scores.shape[-1]]
    prob = torch.softmax(scores.detach(), dim=-1)
    cost = np.zeros([len(ids), prob.shape[-1]])
    for i, l in enumerate(ids):
        sel = labels_gt == l
        cost[i, :] = -(prob[sel, :].sum(dim=0) / (sel.sum() + 1e-4)).cpu().numpy()
    return ids, cost


def optimum(cost):
    """(col_of_row, value) of scipy's solution of np.nan_to_num(cost); the value summed in row order in float64."""
    c = np.nan_to_num(np.asarray(cost, dtype=np.float64))
    rows, cols = scipy.optimize.linear_sum_assignment(c)
    assert list(rows) == list(range(c.shape[0]))
    return cols, float(sum(c[r, cols[r]] for r in range(c.shape[0])))


def margin(cost):
    """Distance from the optimum to the best assignment that avoids one of its edges: forbid each matched edge in turn, re-solve, take the
    smallest increase.  Positive exactly when the optimum is unique."""
    c = np.nan_to_num(np.asarray(cost, dtype=np.float64))
    cols, best = optimum(c)
    big = 1e6 + 4.0 * float(np.abs(c).max()) * max(c.shape)
    m = np.inf
    for r in range(c.shape[0]):
        d = c.copy()
        d[r, cols[r]] = big
        rr, cc = scipy.optimize.linear_sum_assignment(d)
        m = min(m, float(d[rr, cc].sum()) - best)
    return m
