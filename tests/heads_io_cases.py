"""Shared inputs of the appearance-gather / input-assembly / compositing tests (test_heads_io_cases_host.py on the CPU, test_gpu_heads_io.py on
the GPU): seeded cases for every entry point of csrc/heads_io.hip, a reference of each operation, and the yardstick of a case.

How the reference is split (as in march_cases).  The sampling geometry -- ray slab, sample_z, sample_xn, make_tap's position and floor -- is
bit-faithful numpy float32 (``march_cases.geometry`` and ``_tap``).  Everything downstream of those fp32 values is fp64: the bilinear plane x
linear line products (align_corners=True, zero padding, channels-last tables), the six table gradients by autograd over that lookup with
cotangent dF; the MLP input row [feat | dir | sin(feat 2^p), f-major | cos | sin(dir 2^p) | cos | zero pad] with sin / cos of the product
v 2^p, which is exact in fp32, and its backward by autograd; feat = F Wb^T of the front end; the per-ray compositing sums, the clamp, the white
background, the log-normalised semantics and the compositing backward by autograd, the clamp mask taken from the GIVEN rgb_raw and the
log-normalisation's Jacobian at the GIVEN sem_raw, as the kernels take them.

The yardstick of a quantity is the same formulas in fp32 on the CPU -- the backward passes in the kernels' own explicit form -- with every sum
(the texel scatter, the sum over the PE frequencies, the basis contraction, the per-ray and per-row sums) in three orders, measured against
fp64.  A device result is held to ``loss_cases.bound(yardstick, scale)``; a case whose yardstick exceeds 1e-5 * scale is ill-conditioned and
has to be redrawn.  Nothing here touches the GPU."""
import functools

import numpy as np
import torch

import march_cases as mc
from loss_cases import F32, F64, ILL_CONDITIONED, ORDERS, Case, _index, _S, bound, exceeds, f32r, max_error, scale_of  # noqa: F401
from march_cases import AXES, _lookup, _make_rays, _t, _tables, _tap, geometry  # noqa: F401

f32 = np.float32
AU_SEG, AU_U, APP_SEG = 32, 4, 16                 # wave-walk segment, steps whose loads are issued together, lane-walk segment
REC_BYTES = AU_SEG * 64                           # one wave's records
LDS = 160 * 1024
AF_NF, AF_TS = 28, 64                             # feature columns of the front end in memory, samples of one of its tiles
GRADS = ("gp0", "gp1", "gp2", "gl0", "gl1", "gl2")
LOOKUP_MISTAKES = ("tap_weights_swapped", "align_corners_false", "clamped_tap_weighted", "plane1_axes_swapped", "line_axes_0_2_exchanged")


# ---------------------------------------------------------------------------------------------------------------- the dispatcher's formulas
def gather_bwd_branch(comps, res, with_xa):
    """The launch path clift_app_gather_bwd takes: ("wave", blocks per CU; 0 = no LDS line slab) or ("lane", threads per block; 0 = no LDS
    slab), from the formulas of its dispatch and of scatter_geometry."""
    if with_xa and comps <= 64:
        slab = (max(res) * comps * 4 + 15) // 16 * 16
        wpb, bpc, lds = 8, 3, True
        if 3 * (slab + 8 * REC_BYTES) > LDS - 1536:
            wpb, bpc = 12, 2
        if bpc == 2 and 2 * (slab + 12 * REC_BYTES) > LDS - 1024:
            wpb, bpc = 16, 1
        if bpc == 1 and slab + 16 * REC_BYTES > LDS - 512:
            lds, wpb, bpc = False, 8, 3
        return ("wave", bpc if lds else 0)
    lds = sum(res) * comps * 4
    if lds <= 40 * 1024:
        return ("lane", 256)
    if lds <= 80 * 1024:
        return ("lane", 512)
    return ("lane", 1024 if lds <= LDS - 512 else 0)


def gather_bwd_rows_per_trip(comps, res, with_xa, cus):
    """Rows one trip of the persistent grid covers with ``cus`` CUs: more rows than this and the grid-stride loop takes a second trip."""
    kind, shape = gather_bwd_branch(comps, res, with_xa)
    if kind == "wave":
        wpb, bpc = {3: (8, 3), 2: (12, 2), 1: (16, 1), 0: (8, 3)}[shape]
        return (cus * bpc) // 3 * wpb * AU_SEG
    threads, per_cu = {256: (256, 4), 512: (512, 2), 1024: (1024, 1), 0: (256, 4)}[shape]
    return (cus * per_cu * threads) // (3 * comps) * APP_SEG


ALL_BRANCHES = frozenset([("wave", 3), ("wave", 2), ("wave", 1), ("wave", 0), ("lane", 256), ("lane", 512), ("lane", 1024), ("lane", 0)])
RESERVE = 128                                     # clift_set_cu_reserve of the second-trip cases: 256 - 128 CUs


def composite_form(C, D, ld_sem):
    """Which sample kernel clift_composite_bwd_act launches."""
    return "lanes16" if C <= 48 and D <= 8 and ld_sem <= 48 else "scalar"


# ---------------------------------------------------------------------------------------------------------------- products and their scatter
def _products(c, xn, dt, mistake, grad=False):
    planes, lines = _tables(c, dt, grad)
    lm = mistake if mistake in LOOKUP_MISTAKES else None
    _, Ps, Ls, taps = _lookup(c, xn, planes, lines, dt, "natural", lm)
    return planes, lines, Ps, Ls, taps


def _eval_scatter(c, dt, order, mistake, manual=None):
    """F (M, 3 comps) and the six table gradients of sum(F * dF) on top of the pre-fill.  ``manual`` (default: whenever dt is fp32 or a
    mistake is built in): the gradients in the kernels' explicit form (gP = dF L, gL = dF P, weighted into the taps) instead of autograd.
    order: the order the samples reach their texels in."""
    manual = (dt != F64 or mistake is not None) if manual is None else manual
    xn, M, C = c.xn, c.M, c.comps
    perm = _index(M, order).numpy() if (order != "natural" and M > 1) else np.arange(M)
    planes, lines, Ps, Ls, taps = _products(c, xn[perm], dt, mistake, grad=not manual)
    Fp = torch.cat([Ps[i] * Ls[i] for i in range(3)], 1)
    dF = _t(c.dF[:M][perm], dt)
    out = {"F": torch.zeros_like(Fp.detach()).index_copy(0, torch.from_numpy(perm), Fp.detach())}
    if not manual:
        grads = list(torch.autograd.grad((Fp * dF).sum(), planes + lines))
    else:
        s = torch.from_numpy(perm)                               # position of each row in the compacted list
        last = (s % AU_SEG == AU_SEG - 1) | (s == M - 1)
        keep_all = torch.ones(M, dtype=dt)
        if mistake == "last_n_mod_4_dropped":
            n_last = M % AU_SEG
            keep_all = (s < M - (n_last % AU_U)).to(dt)
        gps, gls = [], []
        for i, (a, b, v) in enumerate(AXES):
            tx, ty, tz = taps[i]
            d = dF[:, i * C:(i + 1) * C] * keep_all[:, None]
            P, L = Ps[i].detach(), Ls[i].detach()
            gP = d * (P if mistake == "product_grad_P_for_gP" else L)
            gL = d * (Ps[(i + 1) % 3].detach() if mistake == "line_from_wrong_plane" else P)
            if mistake == "channels_ge64_dropped":
                gP, gL = gP.clone(), gL.clone()
                gP[:, 64:], gL[:, 64:] = 0, 0
            W = c.res[a]
            gp = torch.zeros((c.res[b] * W, C), dtype=dt)
            keep_p = (~last).to(dt) if mistake == "segment_open_texel_lost" else keep_all
            for iy, wy in ((ty.i0, ty.w0), (ty.i1, ty.w1)):
                for ix, wx in ((tx.i0, tx.w0), (tx.i1, tx.w1)):
                    gp.index_add_(0, iy * W + ix, (_t(wx, dt) * _t(wy, dt) * keep_p)[:, None] * gP)
            if mistake == "texel_sum_not_restarted":             # a texel the walk has left is written again into the one that takes its slot
                assert order == "natural"
                key = ty.i0 * W + tx.i0
                nxt = (key[1:] != key[:-1]) & ~last[:-1]
                extra = ((_t(tx.w0, dt) * _t(ty.w0, dt))[:, None] * gP)[:-1][nxt]
                gp.index_add_(0, key[1:][nxt], extra)
            gl = torch.zeros((c.res[v], C), dtype=dt)
            for iz, wz in ((tz.i0, tz.w0), (tz.i1, tz.w1)):
                keep_l = keep_all
                if mistake == "line_sum_restarted_every_step":   # only the last step of a run on one line entry reaches memory
                    assert order == "natural"
                    ends = torch.cat([iz[1:] != iz[:-1], torch.ones(1, dtype=torch.bool)]) | last
                    keep_l = ends.to(dt)
                gl.index_add_(0, iz, (_t(wz, dt) * keep_l)[:, None] * gL)
            gps.append(gp.reshape(c.res[b], W, C)), gls.append(gl)
        grads = gps + gls
    pre = list(c.prefill_plane) + list(c.prefill_line)
    for j, q in enumerate(GRADS):
        out[q] = (_t(pre[j], dt) + grads[j]).detach()
        out["touched_" + q] = grads[j].detach() != 0
    return out


def _eval_points(c, dt, order, mistake):
    _, _, Ps, Ls, _ = _products(c, c.xn, dt, mistake)
    return {"F": torch.cat([Ps[i] * Ls[i] for i in range(3)], 1)}


def _tables_of(rng, res, comps):
    amp = (2.5 * 2.5 / (0.9 * comps)) ** 0.25
    return ([(rng.standard_normal((res[b], res[a], comps)) * amp).astype(f32) for a, b, v in AXES],
            [(rng.standard_normal((res[v], comps)) * amp).astype(f32) for a, b, v in AXES])


def _ray_case(kernel, name, seed, N, S, comps, res, jitter=True, along=None, distinct=None):
    """Rays, box and tables as the march cases draw them, redrawn until every sample keeps FACE_ULPS off the box faces.  ``distinct``: that
    many different rays, repeated up to N (the large cases: many samples, few texels touched)."""
    for attempt in range(50):
        rng = np.random.default_rng(seed + 7919 * attempt)
        lo, hi = np.array(mc.BOX_LO, f32), np.array(mc.BOX_HI, f32)
        step = f32r(min(1.9 / S, 0.25))
        c = Case(kernel, name, N=N, S=S, comps=comps, res=tuple(res), lo=lo, hi=hi, inv2=(f32(2.0) / (hi - lo)).astype(f32), step=step, shift=0.0,
                 ray_derived=True, seed=seed + 7919 * attempt)
        n0 = N if distinct is None else min(distinct, N)
        rays = _make_rays(rng, n0, lo, hi, step, jitter, along)
        jit = rng.uniform(0.05, 0.95, n0).astype(f32) if jitter else None
        rep = -(-N // n0)
        c.rays = np.tile(rays, (rep, 1))[:N].copy()
        c.jitter = None if jit is None else np.tile(jit, rep)[:N].copy()
        c.plane, c.line = _tables_of(rng, res, comps)
        g = geometry(c)
        if mc.face_margin_ulps(c) <= mc.FACE_ULPS or g.mask.mean() < 0.2:
            continue
        c.rng = rng
        return c
    raise AssertionError(f"no draw of {name} keeps its samples off the box faces")


def _pick_active(c, M):
    """M in-box samples in ray-then-sample order: runs of consecutive samples of a ray (three quarters of the in-box samples, dropped in
    short runs so that footprints overlap inside a run and jump between runs and between rays)."""
    g = geometry(c)
    ids = np.nonzero(g.mask.reshape(-1))[0]
    drop = (c.rng.uniform(0, 1, ids.size // 4 + 1) < 0.25).repeat(4)[:ids.size]
    ray = ids // c.S
    rank = np.arange(ids.size) - np.searchsorted(ray, ray, side="left")      # position among the in-box samples of its ray
    drop |= (rank == 2) | (rank == 3)                          # (a gap inside every ray that is long enough)
    if M < 200:
        drop |= rank >= max(7, -(-M // 3) + 2)                 # (a short list still spans several rays)
    ids = ids[~drop]
    assert ids.size >= M, (c, ids.size, M)
    c.act = ids[:M].astype(np.int32)
    c.M = M
    c.xn = g.xn.reshape(-1, 3)[c.act]
    return c


def _finish_scatter(c, rng, cap=None):
    M, C = c.M, c.comps
    cap = M if cap is None else cap
    c.cap = cap
    dF = rng.standard_normal((cap, 3 * C)).astype(f32)
    dF[rng.uniform(0, 1, dF.shape) < 0.1] = 0.0
    dF[M:] = np.nan                                             # rows past the true count: never read under the row limit
    c.dF = dF
    c.prefill_plane = [rng.uniform(-0.5, 0.5, p.shape).astype(f32) for p in c.plane]
    c.prefill_line = [rng.uniform(-0.5, 0.5, p.shape).astype(f32) for p in c.line]
    return c


def _scatter_case(name, seed, M, comps, res, jitter=True, along=None, big=False, cap=None):
    S = 129 if big else (33 if M <= 40 else 65)
    if along is not None:
        S = 200
    per_ray = max(int(0.2 * S), 1)
    N = max(-(-M // per_ray) * 2, 3)
    c = _ray_case("scatter", name, seed, N, S, comps, res, jitter=jitter, along=along, distinct=8 if big else None)
    _pick_active(c, M)
    return _finish_scatter(c, c.rng, cap)


def _node_path(res):
    """Texel-space positions (fx, fy, fz) whose taps are exact in fp32 (every res - 1 is a power of two): footprints that step by one texel
    in the first axis only, the second only, both, and back again; samples exactly on texel nodes (one weight exactly 0); samples exactly on
    the faces -1 and +1."""
    top = [r - 1 for r in res]
    pts = [(1.5, 1.5, 1.5), (2.5, 1.5, 1.5), (2.5, 2.5, 1.5), (2.5, 2.5, 2.5), (3.5, 3.5, 3.5), (2.5, 2.5, 2.5), (1.5, 2.5, 1.5), (1.5, 1.5, 2.5),
           (2.0, 2.0, 2.0), (2.0, 2.5, 3.0), (3.0, 2.0, 2.5), (2.25, 3.0, 2.0), (3.0, 3.0, 3.0), (3.0, 3.0, 3.0),
           (0.0, 0.0, 0.0), (0.0, 1.5, 2.5), (1.5, 0.0, 0.0), (0.5, 0.5, 0.0),
           (top[0], top[1], top[2]), (top[0], 1.5, 2.5), (top[0] - 0.5, top[1], top[2] - 0.5), (2.5, top[1] - 0.5, top[2]), (top[0], top[1] - 1, 0.0)]
    return np.array(pts, np.float64)


def _explicit_scatter_case(name, seed, comps, M=41):
    """Positions given as xa, not derived from rays: the texel-exact path above, then uniform points, 41 rows (a second segment of 9)."""
    rng = np.random.default_rng(seed)
    res = (17, 9, 33)
    c = Case("scatter", name, comps=comps, res=res, ray_derived=False, seed=seed, N=0, S=1)
    c.plane, c.line = _tables_of(rng, res, comps)
    path = _node_path(res)
    fill = rng.uniform(0.0, 1.0, (M - path.shape[0], 3)) * (np.array(res) - 1)
    ft = np.concatenate([path, fill])[:M]
    c.xn = (2.0 * ft / (np.array(res, np.float64) - 1.0) - 1.0).astype(f32)
    c.texel_pos, c.n_exact = ft, path.shape[0]
    c.act, c.M, c.rays, c.jitter = None, M, None, None
    return _finish_scatter(c, rng)


@functools.lru_cache(maxsize=None)
def scatter_cases():
    mid, small = (20, 28, 36), (5, 7, 9)
    out = []
    # M: 1, 3, 31, 32, 33 and last segments of 1, 2, 3, 5 steps of either walk (32-long and 16-long segments)
    spec = [(1, 16, small), (3, 4, small), (31, 16, mid), (32, 48, mid), (33, 16, mid), (65, 64, mid), (66, 16, mid), (67, 4, mid), (69, 48, mid),
            (49, 16, mid), (50, 64, mid), (51, 16, mid), (53, 72, mid), (257, 72, mid), (300, 48, (40, 44, 48)), (200, 64, (60, 52, 44))]
    for k, (M, comps, res) in enumerate(spec):
        out.append(_scatter_case(f"M{M}_C{comps}_{'x'.join(map(str, res))}", 5000 + k, M, comps, res, jitter=k % 3 != 1))
    # elongated grids, comps = 16: one per LDS tier of the wave walk (longest axis) and, without xa, of the lane walk (sum of the axes)
    for k, (M, res, along) in enumerate(((130, (580, 5, 6), 0), (131, (5, 6, 880), 2), (133, (6, 2000, 5), 1), (200, (2600, 5, 6), 0))):
        out.append(_scatter_case(f"long_M{M}_C16_{'x'.join(map(str, res))}", 5100 + k, M, 16, res, along=along))
    out.append(_explicit_scatter_case("nodes_faces_steps_C16", 5200, 16))
    out.append(_explicit_scatter_case("nodes_faces_steps_C72", 5201, 72))
    # rows past the true count poisoned, under the device row limit
    out.append(_scatter_case("limit_M70_cap133_C16", 5210, 70, 16, mid, cap=133))
    out.append(_scatter_case("limit_M70_cap133_C72", 5211, 70, 72, mid, cap=133))
    # a second trip of the grid-stride loop with RESERVE CUs held back: the thresholds come from the dispatcher's own formulas
    big = (48, 56, 64)
    for k, (comps, res, along) in enumerate(((16, big, None), (16, (2000, 5, 6), 0), (72, big, None))):
        rows = gather_bwd_rows_per_trip(comps, res, True, 256 - RESERVE)
        M = rows + 3 * AU_SEG + 5
        c = _scatter_case(f"trip2_M{M}_C{comps}_{'x'.join(map(str, res))}", 5300 + k, M, comps, res, along=along, big=True)
        c.second_trip = True
        out.append(c)
    for c in out:
        c.second_trip = getattr(c, "second_trip", False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def points_cases():
    """clift_vm_products_points: points outside [-1, 1] (clamped taps contribute exactly 0), ldx > 3 with a poisoned pad, n = 1."""
    out = []
    for k, (n, comps, ldx) in enumerate(((1, 16, 3), (63, 4, 4), (65, 48, 5), (1000, 16, 7))):
        rng = np.random.default_rng(5400 + k)
        res = (5, 7, 9)
        c = Case("points", f"n{n}_C{comps}_ldx{ldx}", n=n, comps=comps, res=res, ldx=ldx)
        c.xn = rng.uniform(-1.3, 1.3, (n, 3)).astype(f32)
        c.plane, c.line = _tables_of(rng, res, comps)
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- forward gather (rays)
@functools.lru_cache(maxsize=None)
def gather_cases():
    """clift_app_gather_fwd / clift_active_xyz: comps 4, 16, 48, with and without jitter, a capacity above M for the row limit."""
    out = []
    for k, (M, comps, jit) in enumerate(((1, 4, True), (33, 16, False), (257, 48, True), (300, 16, True), (129, 4, False))):
        c = _ray_case("gather", f"M{M}_C{comps}{'' if jit else '_nojit'}", 5500 + k, max(M // 4, 8), 65, comps, (20, 28, 36), jitter=jit)
        _pick_active(c, M)
        c.cap = M + 37
        out.append(c)
    return tuple(out)


def _eval_gather(c, dt, order, mistake):
    _, _, Ps, Ls, _ = _products(c, c.xn, dt, mistake)
    return {"F": torch.cat([Ps[i] * Ls[i] for i in range(3)], 1)}


# ---------------------------------------------------------------------------------------------------------------- MLP input assembly
def encode_width(nf, pef, pev):
    return nf + 3 + 2 * nf * pef + 2 * 3 * pev


def _pe(v, P, dt, mistake):
    fr = torch.tensor([float(2 * p if mistake == "frequency_2p" else 2 ** p) for p in range(P)], dtype=dt)
    arg = v[:, :, None] * fr                                   # (M, n, P): v 2^p is exact in fp32
    if mistake == "pe_p_major":
        arg = arg.transpose(1, 2)
    arg = arg.reshape(v.shape[0], -1)
    s, co = torch.sin(arg), torch.cos(arg)
    return (co, s) if mistake == "sin_cos_exchanged" else (s, co)


def encode_row(feat, dirs, pef, pev, dt, mistake=None):
    """[feat | dir | sin(feat 2^p) f-major | cos | sin(dir 2^p) | cos]"""
    sf, cf = _pe(feat, pef, dt, mistake)
    sd, cd = _pe(dirs, pev, dt, mistake)
    return torch.cat([feat, dirs, sf, cf, sd, cd], 1)


def _dirs_of(c, dt, mistake):
    if c.dirs is not None:
        return _t(c.dirs[:, :3], dt)
    ray = (c.act.astype(np.int64) % c.N) if mistake == "dir_from_sample_index" else (c.act.astype(np.int64) // c.S)
    return _t(c.rays[ray, 3:6], dt)


def _eval_encode(c, dt, order, mistake, manual=None):
    manual = (dt != F64 or mistake is not None) if manual is None else manual
    nf, pef = c.nf, c.pef
    feat = _t(c.feat[:c.M, :nf], dt).requires_grad_(not manual)
    X = encode_row(feat, _dirs_of(c, dt, mistake), pef, c.pev, dt, mistake)
    out = {"X": X.detach()}
    g = _t(c.dX[:c.M, :X.shape[1]], dt)
    if not manual:
        out["dfeat"] = torch.autograd.grad((X * g).sum(), feat)[0]
        return out
    bs, bc = nf + 3, nf + 3 + nf * pef
    terms = [g[:, :nf]]
    for p in range(pef):
        fr = float(2 ** p)
        sn, cs = torch.sin(feat * fr), torch.cos(feat * fr)
        gs, gc = g[:, bs + p:bs + nf * pef:pef], g[:, bc + p:bc + nf * pef:pef]
        t = cs * gs + sn * gc if mistake == "encode_bwd_cos_sign" else cs * gs - sn * gc
        terms.append(t if mistake == "encode_bwd_no_frequency" else fr * t)
    out["dfeat"] = _S(torch.stack(terms, 0), 0, order)
    return out


@functools.lru_cache(maxsize=None)
def encode_cases():
    """(nf, pe_feat, pe_view) x M in {1, 255, 257}, ldx minimal and padded, ldf > nf, lddf > nf; with ``dirs`` (M, ldd > 3) the points API."""
    out, k = [], 0
    for nf, pef, pev in ((1, 1, 1), (27, 2, 2), (28, 2, 2), (5, 4, 3)):
        for M in (1, 255, 257):
            rng = np.random.default_rng(5600 + k)
            wid = encode_width(nf, pef, pev)
            N, S = 9, 40
            c = Case("encode", f"nf{nf}_pe{pef}_{pev}_M{M}", nf=nf, pef=pef, pev=pev, M=M, N=N, S=S, width=wid, cap=M + 9,
                     ldx=wid if k % 2 == 0 else (wid + 3) // 4 * 4 + 4, ldf=nf + (0 if k % 3 == 0 else 3), lddf=nf + (0 if k % 3 == 1 else 5), dirs=None)
            c.act = np.sort(rng.choice(N * S, M, replace=False)).astype(np.int32)
            d = rng.standard_normal((N, 3))
            c.rays = np.concatenate([rng.uniform(-1, 1, (N, 3)), d / np.linalg.norm(d, axis=1, keepdims=True), np.zeros((N, 2))], 1).astype(f32)
            c.feat = np.full((c.cap, c.ldf), np.nan, f32)
            c.feat[:, :nf] = rng.standard_normal((c.cap, nf)).astype(f32)
            c.dX = rng.standard_normal((c.cap, c.ldx)).astype(f32)
            out.append(c)
            k += 1
    for nf, pef, pev, M, ldd in ((5, 4, 3, 257, 5), (27, 2, 2, 1, 4), (1, 1, 1, 63, 7)):
        rng = np.random.default_rng(5600 + k)
        wid = encode_width(nf, pef, pev)
        c = Case("encode", f"points_nf{nf}_pe{pef}_{pev}_n{M}_ldd{ldd}", nf=nf, pef=pef, pev=pev, M=M, N=0, S=1, width=wid, cap=M, ldx=wid + 2, ldf=nf + 2,
                 lddf=nf, act=None, rays=None)
        d = rng.standard_normal((M, 3))
        c.dirs = np.full((M, ldd), np.nan, f32)
        c.dirs[:, :3] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
        c.feat = np.full((M, c.ldf), np.nan, f32)
        c.feat[:, :nf] = rng.standard_normal((M, nf)).astype(f32)
        c.dX = rng.standard_normal((M, c.ldx)).astype(f32)
        out.append(c)
        k += 1
    return tuple(out)


def literal_encode(feat, dirs, pef, pev):
    """The reference implementation's own lines, restated: indata = [features, viewdirs], then positional_encoding of each appended, where
    positional_encoding(x, freqs) = cat([sin(pts), cos(pts)]) of pts = (x[..., None] * 2^arange(freqs)).reshape(x.shape[:-1] + (freqs * C,))."""
    def positional_encoding(positions, freqs):
        freq_bands = 2 ** torch.arange(freqs, dtype=positions.dtype)
        pts = (positions[..., None] * freq_bands).reshape(positions.shape[:-1] + (freqs * positions.shape[-1],))
        return torch.cat([torch.sin(pts), torch.cos(pts)], dim=-1)
    indata = [feat, dirs]
    indata += [positional_encoding(feat, pef)]
    indata += [positional_encoding(dirs, pev)]
    return torch.cat(indata, dim=-1)


# ---------------------------------------------------------------------------------------------------------------- the fused front end
def _eval_front(c, dt, order, mistake):
    _, _, Ps, Ls, _ = _products(c, c.xn, dt, mistake)
    Fp = torch.cat([Ps[i] * Ls[i] for i in range(3)], 1)
    nc = 3 * c.comps
    k = nc // 2 if mistake == "basis_half_k" else nc
    Wb = _t(c.Wb[:c.nf, :nc], dt)
    feat = _S(Fp[:, None, :k] * Wb[None, :, :k], 2, order)
    X = encode_row(feat, _dirs_of(c, dt, mistake), c.pef, c.pev, dt, mistake)
    return {"F": Fp, "feat": feat, "X": X}


@functools.lru_cache(maxsize=None)
def front_cases():
    """comps 16 / 32 / 48 x M in {1, 63, 64, 65, 128, 64 k + 3} x nf in {1, 27, 28}; ldb > 3 comps with NaN in the pad columns and in the rows
    >= nf of Wb; which of F / xa the caller asks for."""
    out = []
    spec = [(1, 16, 1, 1, 1), (63, 32, 27, 2, 2), (64, 48, 28, 2, 2), (65, 16, 28, 2, 2), (128, 32, 1, 1, 1), (128, 48, 27, 2, 2), (65, 48, 5, 4, 3),
            (64, 16, 27, 2, 2), (64 * 1024 + 3, 16, 1, 1, 1)]
    for k, (M, comps, nf, pef, pev) in enumerate(spec):
        big = M > 1000
        S = 129 if big else 65
        N = max(-(-M // max(int(0.2 * S), 1)) * 2, 3)
        c = _ray_case("front", f"M{M}_C{comps}_nf{nf}_pe{pef}_{pev}", 5700 + k, N, S, comps, (20, 28, 36), jitter=k % 2 == 0, distinct=8 if big else None)
        _pick_active(c, M)
        rng = c.rng
        wid = encode_width(nf, pef, pev)
        c.nf, c.pef, c.pev, c.width, c.dirs = nf, pef, pev, wid, None
        c.ldx = (wid + 3) // 4 * 4 + (4 if k % 2 else 0)
        c.ldb = 3 * comps + 4 * (1 + k % 2)
        c.Wb = np.full((AF_NF, c.ldb), np.nan, f32)
        c.Wb[:nf, :3 * comps] = (rng.standard_normal((nf, 3 * comps)) / np.sqrt(3 * comps)).astype(f32)
        c.cap = M + 70
        c.want_F, c.want_xa = (k % 4 < 2) and not big, k % 2 == 0
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- compositing
COUNTS = (17, 0, 1, 7, 8, 9, 3, 12, 0, 16, 2)
DPRE = ("dpre_rgb", "dpre_sem", "dpre_i0", "dpre_i1")


def _ray_sum(c, vals, order, mistake):
    """(N, ch): the sum of vals (M, ch) over each ray's slice [start, end) of the compacted list."""
    N, M = c.N, c.M
    if M == 0:
        return torch.zeros((N, vals.shape[1]), dtype=vals.dtype)
    start, end = torch.from_numpy(c.start[:-1].astype(np.int64)), torch.from_numpy(c.start[1:].astype(np.int64))
    if mistake == "slice_inclusive_end":
        end = torch.clamp(end + 1, max=M)
    K = int((end - start).max())
    idx = start[:, None] + torch.arange(max(K, 1))[None]
    valid = idx < end[:, None]
    terms = vals[idx.clamp(max=M - 1)] * valid[:, :, None].to(vals.dtype)
    return _S(terms, 1, order)


def _log_norm(s, order, mistake):
    t = _S(s, 1, order)[:, None] + 1e-8
    return torch.log(s / t) if mistake == "eps_dropped_in_log" else torch.log(s / t + 1e-8)


def _pad_cols(x, n):
    return x if x.shape[1] >= n else torch.cat([x, torch.zeros((x.shape[0], n - x.shape[1]), dtype=x.dtype)], 1)


def _eval_composite(c, dt, order, mistake, manual=None):
    """Forward (rgb_raw pre-clamp, rgb_map, sem_raw, sem_map, inst_map) and backward (d_rgb, d_sem, d_inst, g_w at the active samples,
    g_opacity; the dpre_* of the form with the output activations folded in) of a compositing case.  ``manual``: the backward in the
    kernels' explicit form (per-ray effective gradients, then per-sample products) instead of autograd."""
    manual = (dt != F64 or mistake is not None) if manual is None else manual
    N, S, C, D, E, M = c.N, c.S, c.C, c.D, c.E, c.M
    ray = torch.from_numpy((c.act.astype(np.int64) // S))
    req = not manual
    w = _t(c.w.reshape(-1)[c.act], dt).requires_grad_(req)
    op = _t(c.ray_out[:, 0], dt).requires_grad_(req)
    rgb, sem, inst = (_t(x, dt).requires_grad_(req) for x in (c.rgb_s, c.sem_s, c.inst_s))
    zero3, zeroC, zeroD = (torch.zeros((N, n), dtype=dt) for n in (3, C, D))
    add = (1.0 - op)[:, None] if c.white_bg else 0.0
    rgb_sum = _ray_sum(c, w[:, None] * rgb, order, mistake)
    rgb_raw = rgb_sum + add
    rgb_map = (rgb_sum.clamp(0.0, 1.0) + add) if mistake == "white_bg_after_clamp" else rgb_raw.clamp(0.0, 1.0)
    w_s = w.detach() if c.stop_grad else w
    sem_raw = _ray_sum(c, w_s[:, None] * sem, order, mistake)
    inst_map = _ray_sum(c, w_s[:, None] * inst, order, mistake)
    sem_map = _log_norm(sem_raw, order, mistake) if (c.softmax_mode and C > 0) else sem_raw
    out = {"rgb_raw": rgb_raw.detach(), "rgb_map": rgb_map.detach(), "sem_raw": sem_raw.detach(), "sem_map": sem_map.detach(), "inst_map": inst_map.detach()}
    # ---- backward, from the GIVEN rgb_raw (clamp mask) and sem_raw (log-normalisation's Jacobian)
    raw_in, s_in = _t(c.rgb_raw_in, dt), _t(c.sem_raw_in, dt)
    g_rgb = zero3 if c.g_rgb is None else _t(c.g_rgb, dt)
    g_sem = zeroC if c.g_sem is None else _t(c.g_sem, dt)
    g_inst = zeroD if c.g_inst is None else _t(c.g_inst, dt)
    mask = ((raw_in > 0) & (raw_in < 1)) if mistake == "clamp_mask_exclusive" else ((raw_in >= 0) & (raw_in <= 1))
    e_rgb = g_rgb * mask.to(dt)
    if not manual:
        if c.softmax_mode and C > 0:
            sl = s_in.clone().requires_grad_(True)
            e_sem = torch.autograd.grad((_log_norm(sl, "natural", None) * g_sem).sum(), sl)[0]
        else:
            e_sem = g_sem
        loss = (e_rgb * rgb_raw).sum() + (e_sem * sem_raw).sum() + (g_inst * inst_map).sum()
        gr = torch.autograd.grad(loss, [rgb, sem, inst, w, op], allow_unused=True) if loss.requires_grad else [None] * 5
        d_rgb, d_sem, d_inst, g_w, g_op = [torch.zeros_like(x) if g is None else g for g, x in zip(gr, (rgb, sem, inst, w, op))]
    else:
        g_op = -_S(e_rgb, 1, order) if c.white_bg else torch.zeros(N, dtype=dt)
        if c.softmax_mode and C > 0:
            t = _S(s_in, 1, order)[:, None] + 1e-8
            q = g_sem / (s_in / t + 1e-8)
            dot = _S(q * s_in, 1, order)[:, None]
            e_sem = q / t if mistake == "softmax_jacobian_without_dot" else q / t - dot / (t * t)
        else:
            e_sem = g_sem
        wv = w[:, None]
        d_rgb, d_sem, d_inst = wv * e_rgb[ray], wv * e_sem[ray], wv * g_inst[ray]
        colour = rgb * e_rgb[ray]
        rest = torch.cat([sem * e_sem[ray], inst * g_inst[ray]], 1)
        if c.stop_grad:
            rest = torch.zeros_like(rest)
            if mistake == "stop_grad_drops_colour":
                colour = torch.zeros_like(colour)
        g_w = _S(torch.cat([colour, rest], 1), 1, order)
    out.update(d_rgb=d_rgb.detach(), d_sem=d_sem.detach(), d_inst=d_inst.detach(), g_w=g_w.detach(), g_opacity=g_op.detach())
    # ---- the output activations folded in, written in the head outputs o
    d_rgb, d_sem, d_inst, o, so = d_rgb.detach(), d_sem.detach(), d_inst.detach(), rgb.detach(), sem.detach()
    out["dpre_rgb"] = d_rgb * o * (1.0 - o)
    if c.sem_kind == 2 and C > 0:
        k = C - 1 if mistake == "softmax_dot_C_minus_1" else C
        dot = _S((d_sem * so)[:, :k], 1, order)[:, None]
        out["dpre_sem"] = so * (d_sem - dot)
    else:
        out["dpre_sem"] = d_sem * so * (1.0 - so) if mistake == "sigmoid_on_identity_heads" else d_sem
    i0, i1 = _pad_cols(d_inst[:, :E], E), _pad_cols(d_inst[:, E:2 * E], E)
    out["dpre_i0"], out["dpre_i1"] = (i1, i0) if mistake == "slow_half_to_dpre_i0" else (i0, i1)
    return out


def _composite_case(k, N, C, D, E, ld_sem=None, empty=False, g_null=()):
    rng = np.random.default_rng(5800 + k)
    S = 20
    cnt = np.array([COUNTS[(r + k) % len(COUNTS)] for r in range(N)])
    if empty:
        cnt[:] = 0
    softmax_mode, white_bg, stop_grad = k & 1, (k >> 1) & 1, (k >> 2) & 1
    sem_kind = 2 if (k % 3 != 0 and C > 0) else 0
    c = Case("composite", f"N{N}_C{C}_D{D}_E{E}{'_empty' if empty else ''}_sm{softmax_mode}_wb{white_bg}_sg{stop_grad}_k{sem_kind}" + (f"_lds{ld_sem}" if ld_sem else ""),
             N=N, S=S, C=C, D=D, E=E, softmax_mode=softmax_mode, white_bg=white_bg, stop_grad=stop_grad, sem_kind=sem_kind, empty=empty)
    act = np.concatenate([r * S + np.sort(rng.choice(S, n, replace=False)) for r, n in enumerate(cnt)] + [np.zeros(0, np.int64)]).astype(np.int32)
    c.act, c.M, c.start = act, int(act.size), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    M = c.M
    c.cap = M + 11
    c.w = rng.uniform(0.05, 0.6, (N, S)).astype(f32)
    c.ray_out = rng.uniform(0.0, 1.0, (N, 8)).astype(f32)
    c.ray_out[:, 0] = rng.uniform(0.2, 1.0, N).astype(f32)
    c.rgb_s = (1.0 / (1.0 + np.exp(-rng.standard_normal((M, 3)) * 1.5))).astype(f32)
    z = rng.standard_normal((M, C)) * 1.5
    soft = np.exp(z - (z.max(1, keepdims=True) if C else 0.0))
    c.sem_s = (soft / soft.sum(1, keepdims=True) if sem_kind == 2 else rng.uniform(0.1, 1.0, (M, C))).astype(f32)
    c.inst_s = rng.standard_normal((M, D)).astype(f32)
    c.g_rgb = None if "g_rgb" in g_null else rng.standard_normal((N, 3)).astype(f32)
    c.g_sem = None if "g_sem" in g_null else rng.standard_normal((N, C)).astype(f32)
    c.g_inst = None if "g_inst" in g_null else rng.standard_normal((N, D)).astype(f32)
    c.ld_rgb = 4 + 4 * (k % 2)
    c.ld_sem = ld_sem if ld_sem else min((C + 3) // 4 * 4 + 4 * (k % 2), 48 if C <= 48 else 1 << 20)
    c.ld_sem = max(c.ld_sem, 4)
    c.ld_inst = (E + 3) // 4 * 4 + 4 * ((k + 1) % 2)
    raw = rng.normal(0.5, 0.6, (N, 3))
    edge = np.array([0.0, 1.0, 1.5, -0.25, 1.0, 0.0])
    raw.reshape(-1)[:min(edge.size, raw.size)] = edge[:raw.size]
    c.rgb_raw_in = raw.astype(f32)
    c.sem_raw_in = np.zeros((N, C), f32)
    c.sem_raw_in = _eval_composite(c, F64, "natural", None, manual=True)["sem_raw"].numpy().astype(f32)
    return c


@functools.lru_cache(maxsize=None)
def composite_cases():
    # (C = 1 sits at an even index: with one class the log-normalised map is constant, its gradient an exact 0 reached through a
    # cancellation, and no draw of that is well-conditioned; it runs with softmax_mode = 0)
    spec = [  # N, C, D, E -- the 16-lane form
        (1, 0, 0, 1, {}), (257, 5, 6, 3, {}), (255, 1, 3, 3, {}), (255, 22, 6, 6, {}), (257, 48, 8, 4, {}), (1, 5, 6, 3, {}), (257, 22, 6, 3, {}), (255, 5, 6, 3, {}),
        # the scalar form: C > 48, D > 8, ld_sem > 48
        (257, 49, 6, 3, {}), (255, 22, 10, 5, {}), (257, 22, 6, 3, dict(ld_sem=52)), (1, 49, 6, 3, {}), (255, 49, 10, 5, {}),
        # E < D < 2 E and D < E, both forms; E > 8 in the 16-lane form
        (257, 5, 5, 3, {}), (255, 5, 2, 3, {}), (257, 49, 5, 3, {}), (255, 49, 2, 3, {}), (257, 5, 6, 12, {}), (255, 22, 7, 4, dict(ld_sem=52)),
        # a chunk without a single active sample; gradients that are not given
        (255, 5, 6, 3, dict(empty=True)), (257, 5, 6, 3, dict(g_null=("g_rgb",))), (255, 22, 6, 3, dict(g_null=("g_sem", "g_inst"))),
        (257, 49, 6, 3, dict(g_null=("g_sem",))), (257, 5, 6, 3, {})]
    return tuple(_composite_case(k, N, C, D, E, **kw) for k, (N, C, D, E, kw) in enumerate(spec))


def activation_check(c):
    """dpre_rgb and dpre_sem of a case by autograd through sigmoid / softmax from pre-activations (logit(o), log(o)), in fp64."""
    ref = reference(c)
    o = _t(c.rgb_s, F64)
    pre = torch.log(o / (1.0 - o)).requires_grad_(True)
    out = {"dpre_rgb": torch.autograd.grad((torch.sigmoid(pre) * ref["d_rgb"]).sum(), pre)[0], "o_rgb": torch.sigmoid(pre).detach()}
    if c.sem_kind == 2:
        so = _t(c.sem_s, F64)
        so = so / so.sum(1, keepdim=True)                        # (the fp32 rows sum to 1 within an ulp; the formula is exact for rows that do)
        ps = torch.log(so).requires_grad_(True)
        out["dpre_sem"] = torch.autograd.grad((torch.softmax(ps, 1) * ref["d_sem"]).sum(), ps)[0]
        out["dpre_sem_formula"] = so * (ref["d_sem"] - (ref["d_sem"] * so).sum(1, keepdim=True))
    return out


# ---------------------------------------------------------------------------------------------------------------- references, yardsticks, bounds
_EVAL = {"scatter": _eval_scatter, "points": _eval_points, "gather": _eval_gather, "encode": _eval_encode, "front": _eval_front,
         "composite": _eval_composite}
CASES = {"scatter": scatter_cases, "points": points_cases, "gather": gather_cases, "encode": encode_cases, "front": front_cases,
         "composite": composite_cases}
_IN_RANGE_LOOKUP = tuple(m for m in LOOKUP_MISTAKES if m != "clamped_tap_weighted")      # (inside [-1, 1] an out-of-range tap has weight 0 anyway)
_ENCODE_FWD = ("sin_cos_exchanged", "pe_p_major", "frequency_2p", "dir_from_sample_index")
# mistakes a kernel could plausibly make, by the evaluator that can build them in
MISTAKES = {"scatter": _IN_RANGE_LOOKUP + ("product_grad_P_for_gP", "line_from_wrong_plane", "segment_open_texel_lost", "texel_sum_not_restarted",
                                           "line_sum_restarted_every_step", "last_n_mod_4_dropped", "channels_ge64_dropped"),
            "points": LOOKUP_MISTAKES,
            "encode": _ENCODE_FWD + ("encode_bwd_no_frequency", "encode_bwd_cos_sign"),
            "front": ("basis_half_k", "dir_from_sample_index", "pe_p_major", "plane1_axes_swapped"),
            "composite": ("white_bg_after_clamp", "clamp_mask_exclusive", "softmax_jacobian_without_dot", "eps_dropped_in_log", "stop_grad_drops_colour",
                          "sigmoid_on_identity_heads", "softmax_dot_C_minus_1", "slow_half_to_dpre_i0", "slice_inclusive_end")}
# Built in nowhere, because it provably changes no bit: with pe = 1 the f-major and the p-major order of the PE columns are the same
# permutation (test_heads_io_cases_host asserts that on the pe = 1 cases).
INVISIBLE_MISTAKES = {"encode": ("pe_p_major at pe_feat = pe_view = 1",)}


def _quantities(d):
    return {q: v for q, v in d.items() if not q.startswith("touched_")}


def _full(case):
    ref = getattr(case, "_reference", None)
    if ref is None:
        ref = case._reference = {q: v.detach() for q, v in _EVAL[case.kernel](case, F64, "natural", None).items()}
    return ref


def reference(case):
    """{quantity: fp64 tensor} of a case (cached on the case)."""
    return _quantities(_full(case))


def touched(case):
    """{gradient: mask of the texels that receive a contribution} of a scatter case."""
    return {q[len("touched_"):]: v for q, v in _full(case).items() if q.startswith("touched_")}


def restate(case, order="natural", mistake=None):
    return {q: v.detach() for q, v in _EVAL[case.kernel](case, F32, order, mistake).items()}


def checked(case):
    return tuple(reference(case))


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


# Bounds that had to be widened (none).  An entry would be (kernel, case, quantity): (largest |device - fp64| measured on MI355X, the plain
# bound it missed, cause) -- for order-dependent atomic sums only; bound_for then allows twice the measured error, never more than
# ILL_CONDITIONED * scale.
WIDENED = {}


def bound_for(case, quantity):
    ref = reference(case)[quantity]
    b = bound(yardstick(case, quantity), scale_of(ref))
    entry = WIDENED.get((case.kernel, case.name, quantity))
    return b if entry is None else max(b, min(2.0 * entry[0], ILL_CONDITIONED * scale_of(ref)))
