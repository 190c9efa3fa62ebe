"""Shared inputs of the ray-march tests (test_march_cases_host.py on the CPU, test_gpu_march.py on the GPU): seeded cases for every entry
point of csrc/march.hip, a reference of each operation, and the yardstick of a case.

How the reference is split.  The sampling geometry is discontinuous (in-box mask, floor) and clift_dev.h declares it bit-faithful fp32 with
every operation rounded separately, so ``geometry`` spells it in numpy float32, operation by operation as the header does: load_ray (1e-6
for a zero direction component, min / max, clamp to near / far), sample_z, sample_xn with its mask !(lo > p) && !(p > hi), and make_tap's
f = ((x + 1) / 2) * (size - 1) with its floor.  Everything downstream is fp64 from those fp32 values: tap weights (out-of-range taps weigh
zero), the three plane x line products summed over the channels, softplus with the shift, alpha, the exclusive cumprod T, w, the per-ray
sums, the distortion loss by its O(S^2) pairwise definition, n_active; dsigma and the table gradients by autograd on that graph.

The yardstick of a quantity is the same formulas in fp32 on the CPU -- the backward and the distortion loss in the kernels' own prefix /
suffix-sum form -- with every reduction (channel sum, cumprod, prefix and suffix sums, the per-texel scatter sum) in three orders, measured
against fp64.  A device result is held to ``loss_cases.bound(yardstick, scale)``; a case whose yardstick exceeds 1e-5 * scale is
ill-conditioned and has to be redrawn.  Nothing here touches the GPU."""
import functools

import numpy as np
import torch

from loss_cases import F32, F64, HALF_ULP, ILL_CONDITIONED, ORDERS, Case, _index, _S, bound, exceeds, f32r, max_error, scale_of  # noqa: F401

f32 = np.float32
AXES = ((0, 1, 2), (0, 2, 1), (1, 2, 0))          # (a, b, v) of plane / line pair i: the plane is [res[b]][res[a]][C], the line [res[v]][C]
DU_SEG, DENS_SEG, SWEEP = 32, 4, 64               # wave-walk chunk, group-walk segment, lanes of a march sweep
LDS_LIMIT = 160 * 1024 - 512
WAVE_REC_BYTES = 3 * DU_SEG * 64                  # the wave walk's records: 3 planes x 32 steps x 64 bytes per wave
FACE_ULPS = 16
BOX_LO, BOX_HI = (-0.9, -0.8, -0.7), (0.8, 0.9, 0.75)
MARCH_QUANTITIES = ("sigma", "alpha", "T", "w", "opacity", "depth", "Tlast", "Wsum", "WMsum", "dist", "dsigma", "gp0", "gp1", "gp2", "gl0", "gl1",
                    "gl2")


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


# ---------------------------------------------------------------------------------------------------------------- fp32 geometry
class Geometry:
    pass


def geometry(c):
    """The sampling geometry of a march case in numpy float32, every operation rounded on its own (clift_dev.h: load_ray, sample_z,
    sample_xn).  z has S + 1 columns (z_S feeds the last delta and nothing else)."""
    g = getattr(c, "_geometry", None)
    if g is not None:
        return g
    g = Geometry()
    rays, S = c.rays, c.S
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with np.errstate(all="ignore"):
        vec = np.where(d == 0, f32(1e-6), d)
        ra, rb = (c.hi[None] - o) / vec, (c.lo[None] - o) / vec
        t = np.max(np.minimum(ra, rb), axis=1)
    g.tmin = np.minimum(np.maximum(t, near), far).astype(f32)
    jit = np.zeros(c.N, f32) if c.jitter is None else c.jitter
    kf = np.arange(S + 1, dtype=f32)[None] + jit[:, None]
    g.z = g.tmin[:, None] + f32(c.step) * kf
    z = g.z[:, :S]
    g.p = o[:, None, :] + d[:, None, :] * z[:, :, None]
    g.mask = np.all(~(c.lo > g.p) & ~(g.p > c.hi), axis=2)
    g.xn = (g.p - c.lo) * c.inv2 - f32(1.0)
    g.delta_raw = g.z[:, 1:] - g.z[:, :S]
    g.delta = g.delta_raw.copy()
    g.delta[:, S - 1] = 0
    g.mid = ((g.z[:, 1:] + g.z[:, :S]) * f32(0.5)).astype(f32)
    g.mid[:, S - 1] = g.z[:, max(S - 2, 0)]
    for a in (g.z, g.p, g.xn, g.delta, g.mid):
        assert a.dtype == f32
    c._geometry = g
    return g


def face_margin_ulps(c):
    """Smallest distance of any sample point from any box face, in fp32 ulps of max(|lo|, |hi|) of that axis."""
    g = geometry(c)
    ulp = np.spacing(np.maximum(np.abs(c.lo), np.abs(c.hi)).astype(f32)).astype(np.float64)
    p = g.p.astype(np.float64)
    return float(np.min(np.minimum(np.abs(p - c.lo.astype(np.float64)), np.abs(p - c.hi.astype(np.float64))) / ulp))


class Tap:
    pass


# Not a mistake: the mode of the grid_sample cross-check, which forms the tap position in fp64 as grid_sample does (the reference proper
# rounds it to fp32 first, as make_tap does, and the two differ by that rounding).
INDEX_FP64 = "tap_position_in_fp64"


def _tap(x32, size, mistake):
    """make_tap: the position and its floor in fp32, the weights in fp64 from those; out-of-range taps clamped and weighted zero."""
    assert x32.dtype == f32
    fpos = ((x32 + f32(1.0)) / f32(2.0)) * f32(size - 1)
    if mistake == "align_corners_false":
        fpos = ((x32 + f32(1.0)) * f32(size) - f32(1.0)) / f32(2.0)
    if mistake == INDEX_FP64:
        fpos = ((x32.astype(np.float64) + 1.0) / 2.0) * (size - 1)
    fl = np.floor(fpos)
    t = Tap()
    i0 = fl.astype(np.int64)
    i1 = i0 + 1
    w1, w0 = fpos.astype(np.float64) - fl, (fl.astype(np.float64) + 1.0) - fpos
    if mistake == "tap_weights_swapped":
        w0, w1 = w1, w0
    if mistake != "clamped_tap_weighted":
        w0 = np.where((i0 < 0) | (i0 >= size), 0.0, w0)
        w1 = np.where((i1 < 0) | (i1 >= size), 0.0, w1)
    t.i0, t.i1 = torch.from_numpy(np.clip(i0, 0, size - 1)), torch.from_numpy(np.clip(i1, 0, size - 1))
    t.w0, t.w1 = w0, w1
    return t


def _tables(c, dt, grad):
    planes = [_t(c.plane[i], dt).requires_grad_(grad) for i in range(3)]
    lines = [_t(c.line[i], dt).requires_grad_(grad) for i in range(3)]
    return planes, lines


def _lookup(c, xn, planes, lines, dt, order, mistake):
    """sum_i sum_c plane_i(xn_a, xn_b)[c] * line_i(xn_v)[c] at the points xn (M, 3) fp32, channels-last tables.
    Returns (feature (M,), the plane values, the line values, the taps)."""
    C, res = c.comps, c.res
    Ps, Ls, taps, prods = [], [], [], []
    for i, (a, b, v) in enumerate(AXES):
        xa, xb, xv = a, b, v
        if mistake == "plane1_axes_swapped" and i == 1:
            xa, xb = xb, xa
        if mistake == "line_axes_0_2_exchanged" and i != 1:
            xv = 2 - xv
        tx, ty, tz = _tap(xn[:, xa], res[a], mistake), _tap(xn[:, xb], res[b], mistake), _tap(xn[:, xv], res[v], mistake)
        flat, W = planes[i].reshape(-1, C), res[a]
        P = 0
        for iy, wy in ((ty.i0, ty.w0), (ty.i1, ty.w1)):
            for ix, wx in ((tx.i0, tx.w0), (tx.i1, tx.w1)):
                P = P + (_t(wx, dt) * _t(wy, dt))[:, None] * flat[iy * W + ix]
        L = _t(tz.w0, dt)[:, None] * lines[i][tz.i0] + _t(tz.w1, dt)[:, None] * lines[i][tz.i1]
        Ps.append(P), Ls.append(L), taps.append((tx, ty, tz))
        pl = P * L
        prods.append(pl[:, :16] if mistake == "channels_ge16_dropped" else pl)
    return _S(torch.cat(prods, 1), 1, order), Ps, Ls, taps


def _softplus(x):
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


# ---------------------------------------------------------------------------------------------------------------- scans in three associations
def _scan(x, op, order, seg=None):
    """Inclusive scan along dim 1: "natural" = the running one, "reversed" = doubling steps (what a wave does), "permuted" = blocks of 7
    scanned on their own and joined through the scan of their totals.  ``seg``: restart every seg elements (a mistake)."""
    S = x.shape[1]
    if seg is not None:
        return torch.cat([_scan(x[:, s:s + seg], op, order) for s in range(0, S, seg)], 1)
    if order == "natural" or S == 1:
        return torch.cumprod(x, 1) if op == "prod" else torch.cumsum(x, 1)
    f = torch.mul if op == "prod" else torch.add
    if order == "reversed":
        d = 1
        while d < S:
            x = torch.cat([x[:, :d], f(x[:, d:], x[:, :-d])], 1)
            d *= 2
        return x
    B, ident = 7, (1.0 if op == "prod" else 0.0)
    nb = (S + B - 1) // B
    xp = torch.cat([x, torch.full((x.shape[0], nb * B - S), ident, dtype=x.dtype)], 1).reshape(x.shape[0], nb, B)
    inner = _scan(xp.reshape(-1, B), op, "reversed").reshape(x.shape[0], nb, B)
    tot = _scan(inner[:, :, -1], op, "reversed")
    carry = torch.cat([torch.full((x.shape[0], 1), ident, dtype=x.dtype), tot[:, :-1]], 1)
    return f(inner, carry[:, :, None]).reshape(x.shape[0], nb * B)[:, :S]


def _excl(incl, ident, seg=None):
    out = torch.cat([torch.full((incl.shape[0], 1), ident, dtype=incl.dtype), incl[:, :-1]], 1)
    if seg is not None:
        out = out.clone()
        out[:, seg::seg] = ident
    return out


def _suffix_excl(x, order, seg=None):
    """sum over the samples strictly after each one"""
    if seg is not None:
        return torch.cat([_suffix_excl(x[:, s:s + seg], order) for s in range(0, x.shape[1], seg)], 1)
    return _excl(_scan(x.flip(1), "sum", order), 0.0).flip(1)


def pairwise_dist(w, mid, delta):
    """The distortion loss of each ray by its definition: sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i (O(S^2), rays in blocks)."""
    out = []
    for r0 in range(0, w.shape[0], 32):
        ww, mm = w[r0:r0 + 32], mid[r0:r0 + 32]
        out.append(((ww[:, :, None] * ww[:, None, :]) * (mm[:, :, None] - mm[:, None, :]).abs()).sum((1, 2)))
    return torch.cat(out) + (w * w * delta).sum(1) / 3.0


def prefix_dist(w, mid, delta, order, seg=None):
    """The same loss as k_march_fwd forms it: sum_k (1/3) delta w^2 + 2 w (mid * Wpre - WMpre)."""
    wm = w * mid
    wpre, wmpre = _excl(_scan(w, "sum", order, seg), 0.0, seg), _excl(_scan(wm, "sum", order, seg), 0.0, seg)
    return _S((1.0 / 3.0) * delta * w * w + 2.0 * w * (mid * wpre - wmpre), 1, order)


# ---------------------------------------------------------------------------------------------------------------- the march evaluator
def _eval_march(c, dt, order, mistake, manual=None):
    """Every quantity of a march case.  ``manual`` (default: whenever dt is fp32 or a mistake is built in): distortion loss and dsigma in the
    kernels' prefix / suffix-sum form instead of the pairwise definition and autograd."""
    manual = (dt != F64 or mistake is not None) if manual is None else manual
    g, N, S, C = geometry(c), c.N, c.S, c.comps
    planes, lines = _tables(c, dt, True)
    sel = torch.from_numpy(g.mask.reshape(-1)).nonzero()[:, 0]
    if order != "natural" and sel.numel() > 1:                 # the order the samples reach their texels in (the scatter sums of autograd)
        sel = sel[_index(sel.numel(), order)]
    feat, Ps, Ls, taps = _lookup(c, g.xn.reshape(-1, 3)[sel.numpy()], planes, lines, dt, order, mistake)
    x = feat if mistake == "shift_dropped" else feat + torch.tensor(c.shift, dtype=dt)
    sig_in = _softplus(x)
    sigma_graph = torch.zeros(N * S, dtype=dt).index_add(0, sel, sig_in).reshape(N, S)
    out = {"sigma": sigma_graph.detach(), "x": x.detach()}
    # ---- transmittance
    sg = sigma_graph.detach().clone().requires_grad_(True)
    delta = _t(g.delta_raw if mistake == "delta_last_nonzero" else g.delta, dt)
    scale = torch.tensor(1.0 if mistake == "dist_scale_dropped" else c.dist_scale, dtype=dt)
    z0, mid = _t(g.z[:, :S], dt), _t(g.mid, dt)
    if mistake == "last_mid_z_last":
        mid = mid.clone()
        mid[:, -1] = z0[:, -1]
    alpha = 1.0 - torch.exp(-(sg * (delta * scale)))
    om = (1.0 - alpha) + torch.tensor(1e-10, dtype=dt)
    seg_T = SWEEP if mistake == "T_restart_64" else None
    incl = _scan(om, "prod", order, seg_T)
    T = incl if mistake == "T_inclusive" else _excl(incl, 1.0, seg_T)
    w = alpha * T
    wm = w * mid
    opacity = _S(w, 1, order)
    seg_d = SWEEP if mistake == "dist_prefix_restart_64" else None
    dist = prefix_dist(w, mid, delta, order, seg_d) if manual else pairwise_dist(w, mid, delta)
    thres = torch.tensor(c.thres, dtype=F32).to(dt)
    out.update(alpha=alpha.detach(), T=T.detach(), w=w.detach(), opacity=opacity.detach(), Wsum=opacity.detach(),
               depth=_S(w * (mid if mistake == "depth_from_mid" else z0), 1, order).detach(), Tlast=_scan(om, "prod", order)[:, -1].detach(),
               WMsum=_S(wm, 1, order).detach(), dist=dist.detach(), n_active=(w.detach() > thres).sum(1).to(torch.int32))
    # ---- march backward
    zero = torch.zeros((), dtype=dt)
    g_w = _t(c.g_w, dt) if "w" in c.cots else None
    g_op = _t(c.g_op, dt) if "op" in c.cots and mistake != "g_opacity_dropped" else None
    g_d = (torch.tensor(c.g_dist, dtype=dt) / (1.0 if mistake == "g_dist_not_over_N" else float(N))) if "dist" in c.cots else None
    if not manual:
        loss = zero + (0 if g_w is None else (g_w * w).sum()) + (0 if g_op is None else (g_op * opacity).sum()) + (0 if g_d is None else g_d * dist.sum())
        dsigma = torch.autograd.grad(loss, sg)[0] if loss.requires_grad else torch.zeros_like(sg)
    else:
        with torch.no_grad():
            seg_s = SWEEP if mistake == "suffix_restart_64" else None
            Wsuf, WMsuf = _suffix_excl(w, order, seg_s), _suffix_excl(wm, order, seg_s)
            Wpre, WMpre = _excl(_scan(w, "sum", order), 0.0), _excl(_scan(wm, "sum", order), 0.0)
            gk = torch.zeros_like(w) + (0 if g_w is None else g_w) + (0 if g_op is None else g_op[:, None])
            if g_d is not None:
                gk = gk + g_d * ((2.0 / 3.0) * delta * w + 2.0 * (mid * (Wpre - Wsuf) + (WMsuf - WMpre)))
            dalpha = gk * T - _suffix_excl(gk * w, order, seg_s) / om
            dsigma = dalpha * (1.0 if mistake == "one_minus_alpha_dropped" else (1.0 - alpha)) * (delta * scale)
    out["dsigma"] = dsigma.detach()
    # ---- density backward: the table gradients of sum(sigma * ds_in), on top of the pre-fill
    ds = _t(c.ds_in, dt).reshape(-1)[sel]
    tabs = planes + lines
    head = feat if mistake == "softplus_derivative_one" else sig_in
    grads = list(torch.autograd.grad((head * ds).sum(), tabs, retain_graph=True))
    k_of = sel % S
    if mistake == "chunk32_last_plane_lost":
        keep = ((k_of % DU_SEG != DU_SEG - 1) & (k_of != S - 1)).to(dt)
        grads[:3] = torch.autograd.grad((head * ds * keep).sum(), planes, retain_graph=True)
    if mistake == "line_grad_wrong_plane":
        up = torch.autograd.grad(head.sum(), feat, retain_graph=True)[0] * ds
        wrong = sum((up[:, None] * Ps[(i + 1) % 3].detach() * Ls[i]).sum() for i in range(3))
        grads[3:] = torch.autograd.grad(wrong, lines, retain_graph=True)
    if mistake == "texel_sum_not_restarted":                  # a texel the walk has left is written again into the one that takes its slot
        assert order == "natural"
        up = torch.autograd.grad(head.sum(), feat, retain_graph=True)[0] * ds
        tx, ty, _ = taps[0]
        key = ty.i0 * c.res[0] + tx.i0
        nxt = (sel[1:] == sel[:-1] + 1) & (sel[1:] // S == sel[:-1] // S) & (key[1:] != key[:-1])
        extra = ((_t(tx.w0, dt) * _t(ty.w0, dt) * up)[:, None] * Ls[0].detach())[:-1][nxt]
        grads[0] = grads[0] + torch.zeros_like(grads[0]).reshape(-1, C).index_add(0, key[1:][nxt], extra).reshape(grads[0].shape)
    for i in range(3):
        out[f"gp{i}"] = (_t(c.prefill_plane[i], dt) + grads[i]).detach()
        out[f"gl{i}"] = (_t(c.prefill_line[i], dt) + grads[3 + i]).detach()
        out[f"touched_p{i}"] = grads[i].detach() != 0
        out[f"touched_l{i}"] = grads[3 + i].detach() != 0
    return out


# ---------------------------------------------------------------------------------------------------------------- march cases
def _unit(v):
    return v / np.linalg.norm(v)


def _slab_entry(o, d, lo, hi):
    with np.errstate(all="ignore"):
        vec = np.where(d == 0, 1e-6, d)
        return float(np.max(np.minimum((hi - o) / vec, (lo - o) / vec)))


KINDS = ("through", "inside", "miss", "zero1", "zero2", "early", "through", "inside")


def _make_rays(rng, N, lo, hi, step, jitter, along):
    """(N, 8) rays [origin, direction, near, far]: through the box from outside, from inside it (tmin clamps to near), missing it, with one and
    with two direction components exactly 0, and clipping an edge (leaves the box early).  Without jitter a ray from outside gets
    near = slab entry + 0.37 step, so that no sample sits on the entry face."""
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    ext = hi - lo
    rays = np.zeros((N, 8))
    for r in range(N):
        kind = KINDS[r % len(KINDS)]
        if along is not None and kind in ("through", "zero1", "early"):
            kind = "along"
        target = lo + ext * rng.uniform(0.2, 0.8, 3)
        d = _unit(rng.standard_normal(3))
        near = 0.05
        if kind == "along":
            d = rng.uniform(-0.04, 0.04, 3)
            d[along] = (-1.0) ** r
            d = _unit(d)
        elif kind == "zero1":
            d[rng.integers(3)] = 0.0
            d = _unit(d)
        elif kind == "zero2":
            ax = int(rng.integers(3))
            d = np.zeros(3)
            d[ax] = (-1.0) ** r
        elif kind == "early":
            target = lo + ext * np.array([0.06, 0.08, 0.5])[rng.permutation(3)]
        if kind == "inside":
            o = lo + ext * rng.uniform(0.25, 0.75, 3)
        elif kind == "miss":
            o, d = hi + rng.uniform(0.3, 0.5, 3), _unit(rng.uniform(0.2, 1.0, 3))
        else:
            o = target - d * 2.5
        o, d = o.astype(f32).astype(np.float64), d.astype(f32).astype(np.float64)
        if not jitter and kind not in ("inside", "miss"):
            near = _slab_entry(o, d, lo, hi) + 0.37 * step
        rays[r] = [*o, *d, near, 10.0]
    return rays.astype(f32)


def _march_case(name, seed, N, S, comps, res, jitter=True, sd=2.5, shift=-1.0, along=None, tau=3.0, cots=("w", "op", "dist"), only=None,
                saturate=False):
    f = f32
    for attempt in range(50):
        rng = np.random.default_rng(seed + 7919 * attempt)
        lo, hi = np.array(BOX_LO, f), np.array(BOX_HI, f)
        step = f32r(min(1.9 / S, 0.25))
        c = Case("march", name, N=N, S=S, comps=comps, res=tuple(res), lo=lo, hi=hi, inv2=(f(2.0) / (hi - lo)).astype(f), step=step, shift=f32r(shift),
                 cots=tuple(cots), only=only, on_face=False, seed=seed + 7919 * attempt)
        c.rays = _make_rays(rng, N, lo, hi, step, jitter, along)
        c.jitter = rng.uniform(0.05, 0.95, N).astype(f) if jitter else None
        amp = (sd * sd / (0.9 * comps)) ** 0.25
        c.plane = [(rng.standard_normal((res[b], res[a], comps)) * amp).astype(f) for a, b, v in AXES]
        c.line = [(rng.standard_normal((res[v], comps)) * amp).astype(f) for a, b, v in AXES]
        g = geometry(c)
        if face_margin_ulps(c) <= FACE_ULPS or g.mask.mean() < 0.25:
            continue
        return _finish_march_case(c, rng, tau, saturate)
    raise AssertionError(f"no draw of {name} keeps its samples off the box faces")


def _finish_march_case(c, rng, tau, saturate):
    """dist_scale from the case's own optical depths (about ``tau`` per ray, sigma * delta * dist_scale <= 1.5 everywhere, so that
    1 - alpha stays above 0.2), weight_thres in the widest gap of the middle of the in-box weights, cotangents, dsigma fed to the density
    backward (zeros inside chunks and over whole chunks), gradient pre-fills."""
    f, N, S = f32, c.N, c.S
    g = geometry(c)
    c.dist_scale, c.thres = 1.0, 0.0
    c.g_w, c.g_op, c.g_dist = np.zeros((N, S), f), np.zeros(N, f), 0.0
    c.ds_in = np.zeros((N, S), f)
    c.prefill_plane, c.prefill_line = [np.zeros_like(p) for p in c.plane], [np.zeros_like(p) for p in c.line]
    sigma = _eval_march(c, F64, "natural", None)["sigma"].numpy()
    depth = (sigma * g.delta.astype(np.float64)).sum(1)
    lit = depth[depth > 0]
    c.dist_scale = f32r(min(tau / float(lit.mean()), 1.5 / (c.step * float(sigma.max()))) if lit.size else 1.0)
    if saturate:
        c.dist_scale = f32r(40.0 / (c.step * float(sigma.max())))
    w = _eval_march(c, F64, "natural", None)["w"].numpy()
    ws = np.sort(w[g.mask & (w > 0)])
    if ws.size >= 4:
        mid = ws[int(0.3 * ws.size):max(int(0.7 * ws.size), int(0.3 * ws.size) + 2)]
        j = int(np.argmax(np.diff(mid)))
        c.thres = f32r(0.5 * (mid[j] + mid[j + 1]))
    else:
        c.thres = f32r(1e-4)
    c.g_w = rng.standard_normal((N, S)).astype(f)
    c.g_op = rng.standard_normal(N).astype(f)
    c.g_dist = f32r(rng.uniform(0.5, 2.0) * N)
    ds = rng.standard_normal((N, S)) * (rng.uniform(0, 1, (N, S)) > 0.15)
    ds[1::2, DU_SEG:2 * DU_SEG] = 0.0                          # a whole 32-sample chunk of every other ray
    ds[2::3, :DENS_SEG] = 0.0
    ds[0, 0] = 1.25                                           # (S = 1: the one sample there is carries a gradient)
    c.ds_in = ds.astype(f)
    c.prefill_plane = [rng.uniform(-0.5, 0.5, p.shape).astype(f) for p in c.plane]
    c.prefill_line = [rng.uniform(-0.5, 0.5, p.shape).astype(f) for p in c.line]
    return c


def _on_face_case():
    """Two axis-aligned rays whose origin, step and box are powers of two: sample 12 of each lies exactly on a face (p == hi, p == lo); the mask
    is inclusive there, xn == +-1, and at +1 the far tap is out of range."""
    f = f32
    lo, hi = np.array((-1, -1, -1), f), np.array((1, 1, 1), f)
    c = Case("march", "on_face_N2_S16_C16", N=2, S=16, comps=16, res=(5, 7, 9), lo=lo, hi=hi, inv2=np.array((1, 1, 1), f), step=0.125, shift=f32r(-1.0),
             cots=("w", "op", "dist"), only=None, on_face=True, seed=4242)
    c.rays = np.array([[0.25, -0.5, -0.5, 0, 0, 1, 0, 10], [-0.25, 0.5, 0.5, 0, 0, -1, 0, 10]], f)
    c.jitter = None
    rng = np.random.default_rng(4242)
    amp = (2.5 * 2.5 / (0.9 * 16)) ** 0.25
    c.plane = [(rng.standard_normal((c.res[b], c.res[a], 16)) * amp).astype(f) for a, b, v in AXES]
    c.line = [(rng.standard_normal((c.res[v], 16)) * amp).astype(f) for a, b, v in AXES]
    return _finish_march_case(c, rng, 3.0, False)


@functools.lru_cache(maxsize=None)
def march_cases():
    small, mid = (5, 7, 9), (20, 28, 36)
    cot_sets = (("w", "op", "dist"), ("w",), ("op",), ("dist",), ("w", "op"), ("w", "dist"), ("op", "dist"))
    spec = [  # N, S, comps, res, jitter
        (1, 1, 16, small, True), (3, 2, 4, small, False), (4, 4, 8, small, True), (5, 5, 16, small, False), (5, 31, 16, mid, True),
        (4, 32, 8, mid, False), (257, 33, 16, small, True), (5, 63, 4, mid, True), (3, 64, 16, mid, False), (257, 65, 16, mid, True),
        (257, 129, 8, small, True), (257, 200, 16, mid, True), (5, 200, 4, small, False), (257, 64, 4, small, False),
        (5, 65, 32, small, True), (4, 33, 64, small, False), (3, 129, 32, mid, True), (5, 129, 64, small, True),
        (2100, 65, 16, mid, True)]      # (more chunks and segments than a persistent grid has waves and groups: the loops take a second trip)
    out = []
    for k, (N, S, C, res, jit) in enumerate(spec):
        out.append(_march_case(f"N{N}_S{S}_C{C}_{'x'.join(map(str, res))}{'' if jit else '_nojit'}", 3000 + k, N, S, C, res, jitter=jit,
                               cots=cot_sets[k % len(cot_sets)]))
    # elongated grids: one per LDS tier of either walk (density_bwd_branch), rays along the long axis
    for k, (N, S, res, along) in enumerate(((5, 129, (5, 6, 700), 2), (4, 65, (5, 6, 1010), 2), (5, 33, (6, 1400, 5), 1), (3, 200, (2600, 5, 6), 0))):
        out.append(_march_case(f"long_N{N}_S{S}_C16_{'x'.join(map(str, res))}", 3100 + k, N, S, 16, res, along=along, cots=cot_sets[k]))
    out.append(_march_case("long_N5_S64_C8_5x2100x6", 3110, 5, 64, 8, (5, 2100, 6), along=1))
    out.append(_march_case("long_N4_S40_C4_4200x5x6", 3111, 4, 40, 4, (4200, 5, 6), along=0))
    out.append(_march_case("softplus_span_N5_S64_C16", 3120, 5, 64, 16, small, sd=14.0, shift=2.0))
    out.append(_march_case("saturated_N3_S33_C16", 3130, 3, 33, 16, small, only=("alpha", "T", "w"), saturate=True))
    out.append(_on_face_case())
    return tuple(out)


def density_bwd_branch(c, walk_switch):
    """The launch path clift_density_bwd takes for a case: ("wave", lines in LDS?) or ("group", threads per block, 0 = no LDS slab), from
    the formulas of its dispatch and of scatter_geometry."""
    lds = sum(c.res) * c.comps * 4
    if c.comps <= 16 and not walk_switch:
        slab = (lds + 15) // 16 * 16
        return ("wave", slab + 16 * WAVE_REC_BYTES <= LDS_LIMIT)
    if lds <= 40 * 1024:
        return ("group", 256)
    if lds <= 80 * 1024:
        return ("group", 512)
    return ("group", 1024 if lds <= LDS_LIMIT else 0)


ALL_BRANCHES = frozenset([("wave", True), ("wave", False), ("group", 256), ("group", 512), ("group", 1024), ("group", 0)])


# ---------------------------------------------------------------------------------------------------------------- density at points
def _eval_points(c, dt, order, mistake):
    planes, lines = _tables(c, dt, False)
    feat = _lookup(c, c.xn, planes, lines, dt, order, mistake)[0]
    x = feat if mistake == "shift_dropped" else feat + torch.tensor(c.shift, dtype=dt)
    return {"raw": x, "sigma": _softplus(x)}


@functools.lru_cache(maxsize=None)
def points_cases():
    out = []
    for k, (n, comps, ldx) in enumerate(((1, 16, 3), (63, 8, 4), (65, 32, 3), (1000, 16, 4), (1000, 64, 3))):
        rng = np.random.default_rng(3200 + k)
        res, amp = (5, 7, 9), (2.5 * 2.5 / (0.9 * comps)) ** 0.25
        c = Case("points", f"n{n}_C{comps}_ldx{ldx}", n=n, comps=comps, res=res, ldx=ldx, shift=f32r(-1.0))
        c.xn = rng.uniform(-1.3, 1.3, (n, 3)).astype(f32)          # a third of the points has a coordinate outside [-1, 1]: zero padding
        c.plane = [(rng.standard_normal((res[b], res[a], comps)) * amp).astype(f32) for a, b, v in AXES]
        c.line = [(rng.standard_normal((res[v], comps)) * amp).astype(f32) for a, b, v in AXES]
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- alpha lattice and its box
def lattice_xn(c):
    """k_alpha_lattice's points in fp32: p = lo (1 - s) + hi s, xn = (p - lo) * inv2 - 1, voxel (i0, i1, i2) at (i0 g1 + i1) g2 + i2."""
    cols = []
    for a in range(3):
        s = c.ticks[a]
        p = c.lo[a] * (f32(1.0) - s) + c.hi[a] * s
        cols.append(((p - c.lo[a]) * c.inv2[a] - f32(1.0)).astype(f32))
    grid = np.meshgrid(*cols, indexing="ij")
    return np.stack([x.reshape(-1) for x in grid], 1).astype(f32)


def pool_box(alpha, dims, thr):
    """3^3 max-pool of clamp(alpha, 0, 1) (edges see fewer neighbours), and [min index per axis, max index per axis, count] of the voxels
    whose pooled value reaches thr -- 0x7fffffff / -1 / 0 where none does."""
    a = np.clip(np.asarray(alpha).reshape(dims), 0.0, 1.0)
    pad = np.pad(a, 1, constant_values=0.0)
    pooled = np.zeros_like(a)
    for d0 in range(3):
        for d1 in range(3):
            for d2 in range(3):
                pooled = np.maximum(pooled, pad[d0:d0 + dims[0], d1:d1 + dims[1], d2:d2 + dims[2]])
    idx = np.argwhere(pooled >= thr)
    if idx.shape[0] == 0:
        return pooled, [0x7fffffff] * 3 + [-1] * 3 + [0]
    return pooled, [int(v) for v in idx.min(0)] + [int(v) for v in idx.max(0)] + [int(idx.shape[0])]


def _eval_bbox(c, dt, order, mistake):
    planes, lines = _tables(c, dt, False)
    feat = _lookup(c, lattice_xn(c), planes, lines, dt, order, mistake)[0]
    x = feat if mistake == "shift_dropped" else feat + torch.tensor(c.shift, dtype=dt)
    return {"alpha": 1.0 - torch.exp(-_softplus(x) * torch.tensor(c.step, dtype=dt))}


@functools.lru_cache(maxsize=None)
def bbox_cases():
    out = []
    for k, (dims, comps, which) in enumerate((((6, 5, 7), 16, "middle"), ((1, 4, 9), 8, "middle"), ((2, 2, 3), 16, "middle"), ((7, 1, 2), 32, "middle"),
                                              ((6, 5, 7), 16, "none"), ((3, 4, 5), 4, "all"), ((17, 9, 5), 16, "middle"))):
        rng = np.random.default_rng(3300 + k)
        res, amp = (5, 7, 9), (2.5 * 2.5 / (0.9 * comps)) ** 0.25
        lo, hi = np.array(BOX_LO, f32), np.array(BOX_HI, f32)
        c = Case("bbox", f"{'x'.join(map(str, dims))}_C{comps}_{which}", dims=dims, comps=comps, res=res, lo=lo, hi=hi, inv2=(f32(2.0) / (hi - lo)).astype(f32),
                 shift=f32r(-1.0), step=f32r(0.31), which=which)
        c.ticks = [np.linspace(0.0, 1.0, n).astype(f32) for n in dims]
        c.plane = [(rng.standard_normal((res[b], res[a], comps)) * amp).astype(f32) for a, b, v in AXES]
        c.line = [(rng.standard_normal((res[v], comps)) * amp).astype(f32) for a, b, v in AXES]
        pooled = np.unique(pool_box(_eval_bbox(c, F64, "natural", None)["alpha"].numpy(), dims, 0.0)[0])
        if which == "middle" and pooled.size >= 2:
            mid = pooled[int(0.3 * pooled.size):max(int(0.7 * pooled.size), int(0.3 * pooled.size) + 2)]
            j = int(np.argmax(np.diff(mid)))
            c.thr = f32r(0.5 * (mid[j] + mid[j + 1]))
        else:
            c.thr = f32r({"none": 2.0, "all": -0.5}.get(which, 0.5 * float(pooled[0])))
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- scan, compaction, fold
def scan_reference(cnt, cap=None, overflow=0, mistake=None):
    """(ray_start (N + 1), limit, overflow): exclusive offsets and their total; capped: offsets and total clamped to cap, limit = min(total,
    cap), overflow raised to total by max when total > cap and left alone otherwise."""
    cs = np.cumsum(cnt.astype(np.int64))
    start = np.concatenate([[0], cs])
    if mistake == "ray_start_inclusive":
        start = np.concatenate([cs, cs[-1:] if cs.size else [0]])
    total = int(cs[-1]) if cs.size else 0
    if cap is None:
        return start.astype(np.int32), None, None
    return np.minimum(start, cap).astype(np.int32), min(total, cap), (max(overflow, total) if total > cap else overflow)


@functools.lru_cache(maxsize=None)
def scan_cases():
    out = []
    for k, N in enumerate((0, 1, 1023, 1024, 1025, 5000)):
        rng = np.random.default_rng(3400 + k)
        cnt = (rng.integers(0, 6, N) * (rng.uniform(0, 1, N) > 0.3)).astype(np.int32)
        if N == 1:
            cnt[:] = 3
        total = int(cnt.sum())
        caps = sorted({0, total, total + 7, max(total - 3, 0), total // 2})
        out.append(Case("scan", f"N{N}", N=N, cnt=cnt, total=total, caps=tuple(caps), overflows=(0, 5, total + 100)))
    return tuple(out)


def compact_reference(c, cap=None, mistake=None):
    """(n_active per ray, act_idx in ray-then-sample order cut at cap): sample r * S + k is active when w > thres."""
    on = (c.w >= f32(c.thres)) if mistake == "n_active_ge" else (c.w > f32(c.thres))
    ids = np.nonzero(on.reshape(-1))[0].astype(np.int32)
    return on.sum(1).astype(np.int32), (ids if cap is None else ids[:cap])


@functools.lru_cache(maxsize=None)
def compact_cases():
    out = []
    for k, (N, S) in enumerate((N, S) for S in (1, 63, 64, 65, 129) for N in (1, 5)):
        rng = np.random.default_rng(3500 + k)
        w = rng.uniform(0, 1, (N, S)).astype(f32)
        thres = f32r(0.45)
        w[rng.uniform(0, 1, (N, S)) < 0.15] = f32(thres)           # equal to the threshold: not active
        w[0, 0] = f32(thres) if k % 2 else f32(0.9)
        c = Case("compact", f"N{N}_S{S}", N=N, S=S, w=w, thres=thres)
        c.total = int(compact_reference(c)[1].size)
        c.caps = tuple(sorted({0, c.total, c.total + 10, max(c.total - 5, 0), c.total // 2}))
        out.append(c)
    return tuple(out)


def _eval_fold(c, dt, order, mistake):
    work = _t(c.work, dt).reshape(8, c.stride)[:, :c.n]
    if mistake == "fold_seven_copies":
        work = work[:7]
    terms = torch.cat([work, _t(c.dst, dt)[None]], 0)
    if mistake == "fold_overwrites_dst":
        terms = work
    return {"dst": _S(terms, 0, order)}


@functools.lru_cache(maxsize=None)
def fold_cases():
    out = []
    for k, (n, stride) in enumerate(((4, 4), (1020, 1020), (1024, 1024), (1028, 1028), (1024, 1100), (2048 * 256 * 4 + 4, 2048 * 256 * 4 + 4))):
        rng = np.random.default_rng(3600 + k)
        c = Case("fold", f"n{n}_stride{stride}", n=n, stride=stride)
        c.work = rng.standard_normal(8 * stride).astype(f32)
        c.dst = rng.standard_normal(n).astype(f32)
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- references, yardsticks, bounds
_EVAL = {"march": _eval_march, "points": _eval_points, "bbox": _eval_bbox, "fold": _eval_fold}
CASES = {"march": march_cases, "points": points_cases, "bbox": bbox_cases, "fold": fold_cases, "scan": scan_cases, "compact": compact_cases}
LOOKUP_MISTAKES = ("tap_weights_swapped", "align_corners_false", "clamped_tap_weighted", "plane1_axes_swapped", "line_axes_0_2_exchanged",
                   "shift_dropped", "channels_ge16_dropped")
# mistakes a kernel could plausibly make (each one is a real way for this code to go wrong), by the evaluator that can build them in
_IN_BOX_LOOKUP = tuple(m for m in LOOKUP_MISTAKES if m != "clamped_tap_weighted")       # (in the box an out-of-range tap has weight 0 anyway)
MISTAKES = {"march": _IN_BOX_LOOKUP + ("T_inclusive", "T_restart_64", "delta_last_nonzero", "dist_scale_dropped", "dist_prefix_restart_64",
                                        "depth_from_mid", "suffix_restart_64", "g_dist_not_over_N", "g_opacity_dropped", "one_minus_alpha_dropped",
                                        "softplus_derivative_one", "chunk32_last_plane_lost", "texel_sum_not_restarted", "line_grad_wrong_plane"),
            "points": LOOKUP_MISTAKES, "bbox": _IN_BOX_LOOKUP,
            "scan": ("ray_start_inclusive",), "compact": ("n_active_ge",),
            "fold": ("fold_overwrites_dst", "fold_seven_copies")}
# Built in, and provably without effect on any output: the last sample has delta = 0, so alpha = w = 0 there exactly, its midpoint is
# multiplied by zero in every sum, and dsigma of it carries the factor delta.  test_march_cases_host asserts exactly that.
INVISIBLE_MISTAKES = {"march": ("last_mid_z_last",)}
UNBOUNDED = ("x", "n_active")            # carried along by the march evaluator, not held to the bound


def _quantities(case, d):
    return {q: v for q, v in d.items() if not q.startswith("touched_") and q not in UNBOUNDED}


def _full(case):
    ref = getattr(case, "_reference", None)
    if ref is None:
        ref = case._reference = {q: v.detach() for q, v in _EVAL[case.kernel](case, F64, "natural", None).items()}
    return ref


def reference(case):
    """{quantity: fp64 tensor} of a march / points / bbox / fold case (cached on the case)."""
    return _quantities(case, _full(case))


def extras(case):
    """What the march reference carries beside the bounded quantities: softplus argument x, n_active, touched_* masks of the table gradients."""
    return {q: v for q, v in _full(case).items() if q.startswith("touched_") or q in UNBOUNDED}


def restate(case, order="natural", mistake=None):
    return {q: v.detach() for q, v in _EVAL[case.kernel](case, F32, order, mistake).items()}


def checked(case):
    """The quantities of a case that are compared (the saturated ray: alpha, T, w only)."""
    only = getattr(case, "only", None)
    return tuple(q for q in reference(case) if only is None or q in only)


def yardsticks(case):
    """{quantity: max over the three orders of max|fp32 - fp64|}."""
    y = getattr(case, "_yardsticks", None)
    if y is None:
        ref = reference(case)
        y = {q: 0.0 for q in ref}
        for order in ORDERS:
            r = restate(case, order)
            for q in ref:
                y[q] = max(y[q], max_error(r[q], ref[q]))
        case._yardsticks = y
    return y


def yardstick(case, quantity):
    return yardsticks(case)[quantity]


# Bounds that had to be widened (none so far).  An entry would be (kernel, case, quantity): (largest |device - fp64| measured on MI355X, the
# plain bound it missed, cause); bound_for then allows twice the measured error, never more than ILL_CONDITIONED * scale.
WIDENED = {}


def bound_for(case, quantity):
    ref = reference(case)[quantity]
    b = bound(yardstick(case, quantity), scale_of(ref))
    entry = WIDENED.get((case.kernel, case.name, quantity))
    return b if entry is None else max(b, min(2.0 * entry[0], ILL_CONDITIONED * scale_of(ref)))


def thres_margin(case):
    """min over the samples of |w - weight_thres| - bound(w): positive when n_active, ray_start and act_idx are exact integers."""
    w = reference(case)["w"]
    return float((w - float(f32(case.thres))).abs().min()) - bound_for(case, "w")
