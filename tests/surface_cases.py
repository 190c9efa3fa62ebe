"""What the surface-output tests share: the fp64 gradient reference, the literal numpy restatement of the median hit and the
normal sums, the fp32 sample distances of the march, and the made-up marches.  Test infrastructure only, not a test module.

Definitions (the kernels, this file and the tests use them as written):
  field gradient   autograd of ``oracle.field.density_raw(explicit=True)`` with respect to the normalised point: floor selects the cell, so on a
                   texel line the derivative is right-sided, and a tap outside the table is the value 0
  median hit       rem_k = T[k] - w[k] and thr = 1 - q, each ONE fp32 subtraction; k_med = min{k : rem_k <= thr}, else -1 (z_med = 0);
                   prev = rem_{k_med - 1} (1 for k_med = 0), den = prev - rem_k, f = den > 0 ? clamp((prev - thr) / den, 0, 1) : 0 and
                   z_med = z_k + f delta_k in fp64 on those fp32 values
  normal map       sum over the ray's segment of the active list of w_k n_k, n = -g / |g| where |g|^2 >= 1e-30 else 0, in fp64
"""
import numpy as np
import torch

from oracle import field as fld

F32 = np.float32


# ----------------------------------------------------------------------------- field gradient
def grad_reference(P, xn, shift):
    """fp64: (n, 3) d sigma_raw / d xn and (n,) sigma_raw at the points ``xn`` (any float array; taken to fp64 as they are)."""
    P64 = {k: v.double() for k, v in P.items() if k.startswith("density_")}
    x = torch.as_tensor(np.asarray(xn, dtype=np.float64)).clone().requires_grad_(True)
    raw = fld.density_raw(P64, x, float(shift), explicit=True)
    g, = torch.autograd.grad(raw.sum(), x)
    return g.numpy(), raw.detach().numpy()


def texel_coordinates(xn, res):
    """fp64 texel coordinate of every point on every axis: (x + 1) / 2 (R - 1)."""
    return (np.asarray(xn, np.float64) + 1.0) / 2.0 * (np.asarray(res, np.float64) - 1.0)


def near_texel_line(xn, res, eps=1e-4):
    """(n,) bool: the fp64 texel coordinate is within ``eps`` of an integer on some axis -- an fp32 and an fp64 floor may disagree there."""
    f = texel_coordinates(xn, res)
    return (np.abs(f - np.rint(f)) < eps).any(1)


# ----------------------------------------------------------------------------- the march's sample distances
def sample_z(rays, lo, hi, step, S, jitter=None):
    """(N, S + 1) fp32: z_k = tmin + step (k + jitter) for k = 0 .. S, every operation rounded to fp32 on its own like the device's
    ``load_ray`` / ``sample_z``.  Column S only serves delta_{S-1}, which the march sets to 0."""
    rays = np.asarray(rays, F32)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    vec = np.where(d == 0, F32(1e-6), d)
    with np.errstate(over="ignore", invalid="ignore"):
        ra = (np.asarray(hi, F32)[None] - o) / vec
        rb = (np.asarray(lo, F32)[None] - o) / vec
    tmin = np.minimum(np.maximum(np.minimum(ra, rb).max(1), near), far).astype(F32)
    k = np.arange(S + 1, dtype=F32)[None].repeat(rays.shape[0], 0)
    if jitter is not None:
        k = (k + np.asarray(jitter, F32).reshape(-1, 1)).astype(F32)
    return (tmin[:, None] + (F32(step) * k).astype(F32)).astype(F32)


def deltas(z):
    """z (N, S + 1) -> (z (N, S), delta (N, S)) with delta_{S-1} = 0, fp32."""
    d = (z[:, 1:] - z[:, :-1]).astype(F32)
    d[:, -1] = 0
    return z[:, :-1], d


# ----------------------------------------------------------------------------- median hit and normal map
def ray_surface_reference(T, w, z, delta, ray_start, act_idx, G, q):
    """The definitions, literally.  T, w, z, delta (N, S) fp32; ray_start (N + 1), act_idx (M) ints (sample id r S + k); G (M, >= 3) fp32.
    -> dict(k_med (N,) int64, z_med (N,) fp64, f, den, prev (N,) fp64 (0 where there is no hit), normal (N, 3) fp64)."""
    T, w = np.asarray(T, F32), np.asarray(w, F32)
    N, S = T.shape
    rem = (T - w).astype(F32)                               # one fp32 subtraction
    thr = F32(1.0) - F32(q)                                 # one fp32 subtraction
    k_med = np.full(N, -1, np.int64)
    z_med, fs, dens, prevs = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for r in range(N):
        below = np.nonzero(rem[r] <= thr)[0]
        if below.size == 0:
            continue
        k = int(below[0])
        prev = np.float64(rem[r, k - 1]) if k > 0 else 1.0
        den = prev - np.float64(rem[r, k])
        f = min(max((prev - np.float64(thr)) / den, 0.0), 1.0) if den > 0 else 0.0
        k_med[r], fs[r], dens[r], prevs[r] = k, f, den, prev
        z_med[r] = np.float64(z[r, k]) + f * np.float64(delta[r, k])
    normal = np.zeros((N, 3))
    if G is not None and len(act_idx):
        g = np.asarray(G, np.float64)[:, :3]
        len2 = (g * g).sum(1)
        ok = len2 >= 1e-30
        n = np.zeros_like(g)
        n[ok] = -g[ok] / np.sqrt(len2[ok])[:, None]
        wa = w.reshape(-1)[np.asarray(act_idx, np.int64)].astype(np.float64)
        for r in range(N):
            a, b = int(ray_start[r]), int(ray_start[r + 1])
            normal[r] = (wa[a:b, None] * n[a:b]).sum(0)
    return dict(k_med=k_med, z_med=z_med, f=fs, den=dens, prev=prevs, normal=normal)


def depth_bound(ref, z, delta):
    """Per hit ray: how far an fp32 evaluation of z_med may sit from the fp64 one -- two fp32 subtractions of numbers <= 1 (2^-24 each), one
    division and one multiply-add: delta_k (2^-21 / den + 2^-21) + 2^-21 |z|.  Rays without a hit get 0 (their z_med is exactly 0)."""
    k = np.maximum(ref["k_med"], 0)
    r = np.arange(k.shape[0])
    e = 2.0 ** -21
    den = np.where(ref["den"] > 0, ref["den"], 1.0)
    b = np.float64(delta[r, k]) * (e / den + e) + e * np.abs(ref["z_med"])
    return np.where(ref["k_med"] >= 0, b, 0.0)


def check_ray_surface(ref, z, delta, depth, k_med, what=""):
    """k_median equal as integers; depth_median inside ``depth_bound``; a ray with den < 2^-12 only inside its sample's interval."""
    assert np.array_equal(np.asarray(k_med, np.int64), ref["k_med"]), f"{what}: k_median differs"
    hit = ref["k_med"] >= 0
    depth = np.asarray(depth, np.float64)
    assert (depth[~hit] == 0).all(), f"{what}: a ray without a hit has a depth"
    k = np.maximum(ref["k_med"], 0)
    r = np.arange(k.shape[0])
    z0, z1 = np.float64(z[r, k]), np.float64(z[r, k]) + np.float64(delta[r, k])
    flat = hit & (ref["den"] < 2.0 ** -12)
    assert ((depth >= z0) & (depth <= z1 + 2.0 ** -21 * np.abs(z1)))[hit].all(), f"{what}: a depth outside its sample's interval"
    err, bound = np.abs(depth - ref["z_med"]), depth_bound(ref, z, delta)
    tight = hit & ~flat
    if tight.any():
        i = int(np.argmax(np.where(tight, err - bound, -np.inf)))
        print(f"{what}: worst depth error {err[tight].max():.3g}, at the ray nearest its bound {err[i]:.3g} of {bound[i]:.3g}; "
              f"{int(flat.sum())} rays with den < 2^-12")
    assert (err <= bound)[tight].all(), f"{what}: depth_median outside its bound"
    return int(flat.sum())


# ----------------------------------------------------------------------------- made-up marches
def two_surface_ray(S=64, shell=5, wall=40, alpha_shell=0.4):
    """One ray: a shell of alpha ``alpha_shell`` at sample ``shell``, an opaque wall at sample ``wall``; z_k = 1 + 0.05 k.
    -> T, w, z, delta (1, S) fp32."""
    alpha = np.zeros(S, F32)
    alpha[shell], alpha[wall] = alpha_shell, 1.0
    T = np.concatenate([[1.0], np.cumprod(1.0 - alpha.astype(np.float64))[:-1]]).astype(F32)
    w = (alpha * T).astype(F32)
    z = (1.0 + 0.05 * np.arange(S + 1)).astype(F32)[None]
    zk, d = deltas(z)
    return T[None], w[None], zk, d


def made_up_march(N, S, q, seed):
    """Random monotone marches with the edge cases forced on chosen rays (a case that S is too short for leaves its ray as drawn).
    -> dict(T, w (N, S) fp32, ray_start (N + 1) int32, act_idx (M) int32, G (M, 4) fp32, forced {name: ray}).
    ray 0: no hit (nearly transparent);  1: a hit at k = 0;  2: a hit at k = S - 1;  3: a hit at k = 64 (S > 64);  4: a hit at k = S - 2 >= 65;
    5: rem_k == thr exactly;  6: no hit with T == 1, w == 0 everywhere.  Active lists: ray 7 none, 8 one sample, 9 64, 10 65, 11 all S;
    the others a random subset.  G: random rows, every seventh exactly zero.
    Every hit has den >= 2^-12: the alphas are 0 or >= 0.02 and the ray crosses thr while T >= thr."""
    rng = np.random.default_rng(seed)
    thr = F32(1.0) - F32(q)
    alpha = np.where(rng.random((N, S)) < 0.5, 0.0, rng.uniform(0.02, 0.35, (N, S))).astype(F32)
    forced = {}

    def opaque_at(r, k, name):
        if 0 <= k < S:
            alpha[r] = 0
            alpha[r, :k] = F32(1e-4) * (rng.random(k) < 0.5)
            alpha[r, k] = 0.97
            forced[name] = r
    alpha[0] = F32(1e-4)
    forced["no hit"] = 0
    opaque_at(1, 0, "hit at 0")
    opaque_at(2, S - 1, "hit at S-1")
    if S > 64:
        opaque_at(3, 64, "hit at 64")
    if S - 2 >= 65:
        opaque_at(4, S - 2, "hit above 64")
    alpha[6] = 0
    forced["empty"] = 6
    T = np.ones((N, S), F32)
    for k in range(1, S):                                   # fp32 running product, like a march would store it
        T[:, k] = (T[:, k - 1] * (F32(1.0) - alpha[:, k - 1])).astype(F32)
    w = (alpha * T).astype(F32)
    if S >= 3:                                              # equality: w chosen so that T - w is thr to the bit (Sterbenz: T in [thr, 2 thr])
        k = min(2, S - 1)
        T[5], w[5] = 1.0, 0.0
        T[5, k] = F32(1.5) * thr if F32(1.5) * thr <= 1 else F32(1.0)
        w[5, k] = T[5, k] - thr
        T[5, k + 1:] = thr
        assert F32(T[5, k] - w[5, k]) == thr
        forced["equality"] = 5
    counts = rng.integers(0, S + 1, N)
    for r, c in ((7, 0), (8, 1), (9, 64), (10, 65), (11, S)):
        counts[r] = min(c, S)
    act, start = [], [0]
    for r in range(N):
        ks = np.sort(rng.choice(S, int(counts[r]), replace=False))
        act.append(r * S + ks)
        start.append(start[-1] + ks.size)
    act_idx = np.concatenate(act).astype(np.int32)
    G = rng.standard_normal((act_idx.size, 4)).astype(F32)
    G[::7, :3] = 0
    return dict(T=T, w=w, ray_start=np.asarray(start, np.int32), act_idx=act_idx, G=G, forced=forced)
