"""What the colour-layer tests share: the fp32 numpy restatement of clift_ray_layer_colour (np.float32 scalars, one operation
per statement, so that every statement rounds once like the kernel's separately rounded operations), the fp64 "column alone" reference,
the error check both test files use and made-up colours for the made-up marches of tests/layers_cases.py.  Test infrastructure only, not
a test module.

Definitions (include/clift.h states them; the kernel, this file and the tests use them as written):
  columns, skipped entries   those of clift_ray_layers (layers_cases._entries, layers_cases.column_of)
  coloured     list row j is coloured when row = rgb_row[j] (j itself when rgb_row is None) lies in [0, n_rgb); its colour is rgb[row, 0:3]
  colour       per ray and column, over the ray's list entries of that column in order: u = Tc * a; for a coloured entry R = R + (u * r),
               G = G + (u * g), B = B + (u * b); Tc = Tc * (1 - a); the row is [R, G, B, 1 - Tc]
  column alone the ordinary alpha composite of the ray with the alpha of every sample of another column set to 0, in fp64 on the fp32
               alphas and colours: A = 1 - prod (1 - a), RGB = sum over the coloured entries of a T c, T the product before the sample
"""
import numpy as np

from layers_cases import EPS, F32, _entries, column_of, made_up_layers


def _row_of(j, rgb_row, n_rgb):
    """The row of rgb that list row j reads, or -1: not coloured."""
    row = j if rgb_row is None else int(rgb_row[j])
    return row if 0 <= row < n_rgb else -1


def colour_restatement(alpha, ray_start, act_idx, slot, K, rgb, rgb_row):
    """The recurrence of clift_ray_layer_colour in fp32.  alpha (N, S) fp32, ray_start (N + 1), act_idx (M), slot (M) ints, rgb (n_rgb, >= 3)
    fp32 or None (n_rgb = 0), rgb_row (M) ints or None -> (N, K + 1, 4) fp32 rows [R, G, B, A]."""
    alpha = np.asarray(alpha, F32)
    rgb = np.zeros((0, 3), F32) if rgb is None else np.asarray(rgb, F32)
    N, S = alpha.shape
    M = 0 if act_idx is None else len(act_idx)
    out = np.zeros((N, K + 1, 4), F32)
    one = F32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(N):
            Tc = [one] * (K + 1)
            acc = [[F32(0)] * 3 for _ in range(K + 1)]
            for j, k in _entries(r, S, ray_start, act_idx, M):
                c = column_of(slot[j], K)
                a = alpha[r, k]
                u = F32(Tc[c] * a)
                row = _row_of(j, rgb_row, rgb.shape[0])
                if row >= 0:
                    for i in range(3):
                        uc = F32(u * rgb[row, i])
                        acc[c][i] = F32(acc[c][i] + uc)
                rest = F32(one - a)
                Tc[c] = F32(Tc[c] * rest)
            for c in range(K + 1):
                out[r, c] = (acc[c][0], acc[c][1], acc[c][2], F32(one - Tc[c]))
    return out


def colour_alone_reference(alpha, ray_start, act_idx, slot, K, rgb, rgb_row):
    """fp64: per (ray, column) the alpha composite of that column's entries with every other column's alpha set to 0; an entry without a
    colour attenuates and adds nothing.  -> (N, K + 1, 4) fp64 rows [R, G, B, A], and n_r (N,) = the entries of the ray."""
    alpha = np.asarray(alpha, np.float64)
    rgb = np.zeros((0, 3)) if rgb is None else np.asarray(rgb, np.float64)
    N, S = alpha.shape
    M = 0 if act_idx is None else len(act_idx)
    out = np.zeros((N, K + 1, 4))
    n_r = np.zeros(N, np.int64)
    for r in range(N):
        ent = list(_entries(r, S, ray_start, act_idx, M))
        n_r[r] = len(ent)
        cols = np.asarray([column_of(slot[j], K) for j, _ in ent], np.int64)
        for c in np.unique(cols):
            mine = [e for e, cc in zip(ent, cols) if cc == c]
            a = alpha[r, [k for _, k in mine]]
            T = np.concatenate([[1.0], np.cumprod(1.0 - a)[:-1]])
            col = np.zeros((len(mine), 3))
            for i, (j, _) in enumerate(mine):
                row = _row_of(j, rgb_row, rgb.shape[0])
                if row >= 0:
                    col[i] = rgb[row, :3]
            out[r, c, :3] = ((a * T)[:, None] * col).sum(0)
            out[r, c, 3] = 1.0 - np.prod(1.0 - a)
    return out, n_r


def check_colour(got, ref, n_r, what="", relative=True):
    """R, G, B of ``got`` (N, K + 1, 4) within (n_r + 3) 2^-23 of the fp64 reference ``ref`` -- relative to the reference (alphas of 0, 1
    or at least 1/16), or as an absolute error (``relative`` False: smaller alphas, as tests/test_layers_host.py treats Z's neighbour A).
    The bound is the one DESIGN.md 6i derives for Z: non-negative terms u_i c_i, u_i a product of at most i + 1 rounded factors, one more
    product, a running sum.  Prints the worst share of the bound, returns it."""
    got = np.asarray(got, F32).astype(np.float64)
    bound = ((n_r + 3) * EPS)[:, None, None]
    err = np.abs(got[..., :3] - ref[..., :3])
    scale = np.abs(ref[..., :3]) if relative else np.ones_like(err)
    worst = float((err / np.where(scale > 0, scale, 1.0) / bound).max()) if err.size else 0.0
    print(f"{what}: worst colour error {worst:.3f} of (n_r + 3) 2^-23 {'relative' if relative else 'absolute'}")
    assert (err <= bound * scale).all(), f"{what}: a colour outside (n_r + 3) 2^-23 {'relative' if relative else 'absolute'}"
    return worst


def made_up_colour_layers(N, S, K, seed, alpha_floor=0.02, stray=True):
    """``made_up_layers`` with colours: rgb (M, 3) fp32 uniform in [0, 1], one row per list row (what a NULL rgb_row reads), and an indirect
    arrangement of the same list -- rgb_perm (n_perm, 3) and rgb_row (M) int32, a random permutation into rgb_perm for most rows, with rows
    of -1 and of n_perm (both: not coloured) among them whenever the list has three rows or more."""
    m = made_up_layers(N, S, K, seed, alpha_floor=alpha_floor, stray=stray)
    rng = np.random.default_rng(seed + 77)
    M = m["act_idx"].size
    m["rgb"] = rng.uniform(0.0, 1.0, (M, 3)).astype(F32)
    n_perm = M + 2                                           # two rows of rgb_perm that no list row reads
    m["rgb_perm"] = rng.uniform(0.0, 1.0, (n_perm, 3)).astype(F32)
    row = rng.permutation(n_perm)[:M].astype(np.int32)
    if M >= 3:
        row[rng.choice(M, max(M // 5, 2), replace=False)] = -1
        row[rng.choice(M, max(M // 7, 1), replace=False)] = n_perm
        row[0] = -1
    m["rgb_row"] = row
    return m
