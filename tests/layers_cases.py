"""What the amodal-layer tests share: the fp32 numpy restatements of clift_sample_slots and clift_ray_layers (np.float32
scalars, one operation per statement, so that every statement rounds once like the kernels' separately rounded operations), the fp64
"object alone" reference, the fp64 sample distances and the case builders.  Test infrastructure only, not a test module.

Definitions (include/clift.h states them; the kernels, this file and the tests use them as written):
  slot        class = first maximum of the row's semantic output; (off, cnt) of that class cut to [0, K); mode 0: nearest centroid of the cut
              range with d = f - c, d2 = d2 + d * d, a strict < against a minimum that starts at +inf (no winner: -1); mode 1: lo + first
              maximum of the first min(hi - lo, E) features
  layers      per ray and column, over the ray's list entries of that column in order: zf = z of the first, u = Tc * a, Z = Z + (u * z),
              V = V + w, Tc = Tc * (1 - a); the row is [1 - Tc, V, Z, zf]
  object alone  the ordinary alpha composite of the ray with every sample of another column given alpha 0, in fp64 on the fp32 alphas and
              weights and the fp64 distances: A = 1 - prod (1 - a), V = sum w, Z = sum a T z with T the product before the sample
"""
import numpy as np

from surface_cases import made_up_march, sample_z, two_surface_ray  # noqa: F401  (the tests take them from here)

F32 = np.float32
EPS = 2.0 ** -23


# ----------------------------------------------------------------------------- slots
def first_max(v):
    """Index of the first maximum by the rule c* = 0; for c = 1 ..: if v[c] > v[c*] then c* = c (a NaN never compares greater)."""
    best = 0
    for c in range(1, len(v)):
        if v[c] > v[best]:
            best = c
    return best


def slots_restatement(sem, feat, add, cls_slots, cent, K, mode):
    """sem (n, C), feat (n, E), add (n, E) or None, cls_slots (C, 2) ints, cent (K, E) or None -> (n,) int32, every operation in fp32."""
    sem, feat = np.asarray(sem, F32), np.asarray(feat, F32)
    n, E = feat.shape
    out = np.full(n, -1, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        _slots_rows(out, sem, feat, add, cls_slots, cent, K, mode)
    return out


def _slots_rows(out, sem, feat, add, cls_slots, cent, K, mode):
    n, E = feat.shape
    for row in range(n):
        cls = first_max(sem[row])
        off, cnt = int(cls_slots[cls][0]), int(cls_slots[cls][1])
        lo, hi = max(off, 0), min(off + cnt, K)
        if cnt <= 0 or hi <= lo:
            continue
        f = feat[row]
        if add is not None:
            f = np.asarray([F32(feat[row, e]) + F32(add[row, e]) for e in range(E)], F32)
        if mode == 0:
            best, win = F32(np.inf), -1
            for c in range(lo, hi):
                d2 = F32(0)
                for e in range(E):
                    d = F32(f[e]) - F32(cent[c, e])
                    dd = F32(d * d)
                    d2 = F32(d2 + dd)
                if d2 < best:
                    best, win = d2, c
            out[row] = win
        else:
            out[row] = lo + first_max(f[:min(hi - lo, E)])


# ----------------------------------------------------------------------------- layers
def _entries(r, S, ray_start, act_idx, M):
    """(j, k) of the list entries of ray r that belong to it, in list order; ray_start clamped to [0, M]."""
    j0, j1 = min(max(int(ray_start[r]), 0), M), min(max(int(ray_start[r + 1]), 0), M)
    for j in range(j0, j1):
        k = int(act_idx[j]) - r * S
        if 0 <= k < S:
            yield j, k


def column_of(slot, K):
    return int(slot) if 0 <= int(slot) < K else K


def layers_restatement(alpha, w, z, ray_start, act_idx, slot, K):
    """The recurrence of clift_ray_layers in fp32.  alpha, w (N, S) fp32, z (N, >= S) fp32 (``sample_z``), ray_start (N + 1), act_idx (M),
    slot (M) ints -> (N, K + 1, 4) fp32."""
    alpha, w, z = np.asarray(alpha, F32), np.asarray(w, F32), np.asarray(z, F32)
    N, S = alpha.shape
    M = len(act_idx)
    out = np.zeros((N, K + 1, 4), F32)
    one = F32(1)
    for r in range(N):
        Tc = [one] * (K + 1)
        V, Z, zf = [F32(0)] * (K + 1), [F32(0)] * (K + 1), [F32(0)] * (K + 1)
        seen = [False] * (K + 1)
        for j, k in _entries(r, S, ray_start, act_idx, M):
            c = column_of(slot[j], K)
            a, zz = alpha[r, k], z[r, k]
            if not seen[c]:
                zf[c], seen[c] = zz, True
            u = F32(Tc[c] * a)
            uz = F32(u * zz)
            Z[c] = F32(Z[c] + uz)
            V[c] = F32(V[c] + w[r, k])
            rest = F32(one - a)
            Tc[c] = F32(Tc[c] * rest)
        for c in range(K + 1):
            out[r, c] = (F32(one - Tc[c]), V[c], Z[c], zf[c])
    return out


def object_alone_reference(alpha, w, z64, ray_start, act_idx, slot, K):
    """fp64: per (ray, column) the alpha composite of the ray with the alpha of every sample of another column set to 0.
    -> (N, K + 1, 4) fp64 rows [A, V, Z, zf], and n_r (N,) = the entries of the ray."""
    alpha, w = np.asarray(alpha, np.float64), np.asarray(w, np.float64)
    N, S = alpha.shape
    M = len(act_idx)
    out = np.zeros((N, K + 1, 4))
    n_r = np.zeros(N, np.int64)
    for r in range(N):
        ent = list(_entries(r, S, ray_start, act_idx, M))
        n_r[r] = len(ent)
        cols = np.asarray([column_of(slot[j], K) for j, _ in ent], np.int64)
        ks = np.asarray([k for _, k in ent], np.int64)
        for c in np.unique(cols):
            kc = ks[cols == c]
            a = alpha[r, kc]
            T = np.concatenate([[1.0], np.cumprod(1.0 - a)[:-1]])
            out[r, c] = (1.0 - np.prod(1.0 - a), w[r, kc].sum(), (a * T * z64[r, kc]).sum(), z64[r, kc[0]])
    return out, n_r


def sample_z64(rays, lo, hi, step, S, jitter=None):
    """(N, S) fp64: the expressions of ``sample_z`` evaluated in fp64 on the fp32 inputs (the step as the fp32 number the record holds)."""
    rays = np.asarray(rays, F32).astype(np.float64)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    vec = np.where(d == 0, np.float64(F32(1e-6)), d)
    ra = (np.asarray(hi, F32).astype(np.float64)[None] - o) / vec
    rb = (np.asarray(lo, F32).astype(np.float64)[None] - o) / vec
    tmin = np.minimum(np.maximum(np.minimum(ra, rb).max(1), near), far)
    k = np.arange(S, dtype=np.float64)[None].repeat(rays.shape[0], 0)
    if jitter is not None:
        k = k + np.asarray(jitter, F32).astype(np.float64).reshape(-1, 1)
    return tmin[:, None] + np.float64(F32(step)) * k


def check_layers(got, rest, ref, n_r, what="", bits=True):
    """``got`` (N, K + 1, 4) against the fp32 restatement ``rest`` and the fp64 reference ``ref``: A and V bit-equal to the restatement
    (``bits``), Z within (n_r + 3) 2^-23 relative of the reference, zf within 2^-22 relative of the fp64 z.  Prints the worst figures first."""
    got = np.asarray(got, F32)
    bound = ((n_r + 3) * EPS)[:, None]
    ez = np.abs(got[..., 2].astype(np.float64) - ref[..., 2])
    ef = np.abs(got[..., 3].astype(np.float64) - ref[..., 3])
    relz = (ez / np.where(ref[..., 2] != 0, np.abs(ref[..., 2]), 1.0) / bound).max() if got.size else 0.0
    relf = (ef / np.where(ref[..., 3] != 0, np.abs(ref[..., 3]), 1.0)).max() if got.size else 0.0
    print(f"{what}: worst Z error {relz:.3f} of its bound, worst zf error {relf / 2.0 ** -22:.3f} of 2^-22; "
          f"A and V equal to the restatement on {int((got[..., :2].view(np.uint32) == rest[..., :2].view(np.uint32)).sum())} of {got[..., :2].size}")
    if bits:
        assert np.array_equal(got[..., 0].view(np.uint32), rest[..., 0].view(np.uint32)), f"{what}: A differs from the fp32 restatement"
        assert np.array_equal(got[..., 1].view(np.uint32), rest[..., 1].view(np.uint32)), f"{what}: V differs from the fp32 restatement"
    assert (ez <= bound * np.abs(ref[..., 2])).all(), f"{what}: Z outside (n_r + 3) 2^-23 relative"
    assert (ef <= 2.0 ** -22 * np.abs(ref[..., 3])).all(), f"{what}: zf outside 2^-22 relative"


# ----------------------------------------------------------------------------- case builders
LENGTHS = (-1, 0, 1, 63, 64, 65)          # -1: all S samples; rays past these draw a random length


def made_up_layers(N, S, K, seed, alpha_floor=0.02, stray=True):
    """A made-up march with its alpha-list and slots.  Ray r lists LENGTHS[r] samples (clipped to S; a random subset in increasing order),
    later rays a random count.  alpha: uniform(``alpha_floor``, 0.6), every fifth exactly 0 and every seventh exactly 1; w: random fp32 (the
    kernel only sums it).  Slots: random in [-1, K + 7], the first three list rows -1, K and K + 7.  ``stray`` (N >= 3): an entry of
    another ray, one past N S and a negative one are put into ray 2's range -- every implementation has to skip them.
    -> dict(alpha, w (N, S) fp32, ray_start (N + 1) int32, act_idx (M) int32, slot (M) int32)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(alpha_floor, 0.6, (N, S)).astype(F32)
    flat = alpha.reshape(-1)
    flat[::5] = 0.0
    flat[3::7] = 1.0
    w = rng.uniform(0.0, 0.2, (N, S)).astype(F32)
    act, start = [], [0]
    for r in range(N):
        want = LENGTHS[r] if r < len(LENGTHS) else int(rng.integers(0, S + 1))
        n = S if want < 0 else min(want, S)
        ks = np.sort(rng.choice(S, n, replace=False))
        ids = list(r * S + ks)
        if stray and r == 2 and N >= 3:
            ids = ids[:len(ids) // 2] + [0 * S + min(3, S - 1), N * S + 3, -5] + ids[len(ids) // 2:]
        act += ids
        start.append(len(act))
    act_idx = np.asarray(act, np.int64).astype(np.int32)
    slot = rng.integers(-1, K + 8, act_idx.size).astype(np.int32)
    for i, v in enumerate((-1, K, K + 7)):
        if i < slot.size:
            slot[i] = v
    return dict(alpha=alpha, w=w, ray_start=np.asarray(start, np.int32), act_idx=act_idx, slot=slot)


def made_up_slot_rows(n, C, E, K, seed, mode):
    """Rows for clift_sample_slots: sem (n, C), feat (n, E), add (n, E), cls_slots (C, 2), cent (K, E).  Class 0 is a stuff class (count 0)
    when C > 1; the last class's range runs past K (clamped); row 1 has NaN features, row 2 an exact tie between two centroids (its feature is
    their midpoint in exactly representable numbers) resp. between two scores, row 3 a NaN in its semantic output."""
    rng = np.random.default_rng(seed)
    sem = rng.standard_normal((n, C)).astype(F32)
    feat = rng.standard_normal((n, E)).astype(F32)
    add = rng.standard_normal((n, E)).astype(F32)
    cent = rng.standard_normal((K, E)).astype(F32)
    cls_slots = np.zeros((C, 2), np.int32)
    things = list(range(1, C)) if C > 1 else [0]
    per = max(K // len(things), 1)
    for i, c in enumerate(things):
        cls_slots[c] = (i * per, per)
    cls_slots[things[-1], 1] += 9                            # runs past K: clamped
    if n > 1:
        feat[1] = np.nan
    if n > 2:
        c = things[0]
        sem[2] = -1.0
        sem[2, c] = 2.0
        lo = int(cls_slots[c, 0])
        if mode == 0 and K >= lo + 2:
            cent[lo], cent[lo + 1] = 0.5, -0.5                # the midpoint 0 is equally far from both, to the bit
            cent[lo + 2:lo + per] += 4.0
            feat[2], add[2] = 0.0, 0.0
        else:
            feat[2], add[2] = 1.25, 0.0                        # all scores equal: the first wins
    if n > 3:
        sem[3, 0] = np.nan
    return dict(sem=sem, feat=feat, add=add, cls_slots=cls_slots, cent=cent)
