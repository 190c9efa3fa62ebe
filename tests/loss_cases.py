"""Shared inputs of the loss and optimiser tests (test_loss_cases_host.py on the CPU, test_gpu_losses.py on the GPU): seeded cases for every
entry point of csrc/losses.hip, an fp64 reference of each operation written out with explicit differences and sums (gradients by autograd
on it), and the yardstick of a case: the same formulas in fp32 on the CPU with every reduction in three orders, measured against fp64.

A device result is held to ``bound(yardstick, scale) = 8 * yardstick + 4 * 2^-24 * scale`` -- scale = |loss| of a scalar, max|.| of a
gradient or a moment.  The 8 covers what legitimately differs on the device (expf / logf / division a few ulp from libm's, other FMA
contraction, atomically ordered block sums).  A case whose yardstick exceeds 1e-5 * scale is ill-conditioned and has to be redrawn.

Every scalar argument is rounded to fp32 first (``f32r``): the kernels receive floats, and 1 - 0.999f is not 1 - 0.999.
Nothing here touches the GPU."""
import functools
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
ORDERS = ("natural", "reversed", "permuted")
HALF_ULP = 2.0 ** -24          # half an fp32 ulp at 1
ILL_CONDITIONED = 1e-5
CL_MAXE = 32
TV_MAX = 8                     # CLIFT_TV_MAX of include/clift.h


def f32r(x):
    return float(np.float32(x))


class Case:
    def __init__(self, kernel, name, **fields):
        self.kernel, self.name = kernel, name
        self.__dict__.update(fields)

    def __repr__(self):
        return f"{self.kernel}:{self.name}"


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- ordered reductions
@functools.lru_cache(maxsize=None)
def _index(n, order):
    if order == "reversed":
        return torch.arange(n - 1, -1, -1)
    return torch.randperm(n, generator=torch.Generator().manual_seed(20240 + n))


def _S(x, dim, order):
    """Sum over ``dim`` with the terms taken in the given order, as a fixed tree of elementwise additions (first half plus second half, an
    odd term carried): torch.sum splits its work by thread count and vector width, and its fp32 result moves from one CPU to the next."""
    if order != "natural" and x.shape[dim] > 1:
        x = x.index_select(dim, _index(x.shape[dim], order))
    x = x.movedim(dim, 0)
    if x.shape[0] == 0:
        return x.sum(0)
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        y = x[:h] + x[h:2 * h]
        x = y if x.shape[0] == 2 * h else torch.cat([y, x[2 * h:]])
    return x[0]


def _grad(y, x):
    if not y.requires_grad:
        return torch.zeros_like(x)
    g = torch.autograd.grad(y, x, allow_unused=True)[0]
    return torch.zeros_like(x) if g is None else g


def _c(v, dt):
    return torch.tensor(v, dtype=dt)


# ---------------------------------------------------------------------------------------------------------------- contrastive
def _eval_contrastive(c, dt, order, mistake):
    """l_ij = exp(exp(-d2_ij / tau_ij)), tau = temperature for positive pairs (same label, i != j) and 1 otherwise; p_i over the positives,
    Z_i over all j (diagonal included); loss = -sum_{p_i != 0} log(p_i / Z_i) / B."""
    f = c.f.to(dt).requires_grad_(True)
    B = f.shape[0]
    same = c.y[:, None] == c.y[None, :]
    pos = same if mistake == "diagonal_positive" else same & ~torch.eye(B, dtype=torch.bool)
    other = f.detach() if mistake == "row_j_term_dropped" else f
    diff = f[:, None, :] - other[None, :, :]
    d2 = _S(diff * diff, 2, order)
    t, one = _c(c.temperature, dt), _c(1.0, dt)
    tau = torch.where(pos, one, t) if mistake == "temperature_on_negatives" else torch.where(pos, t, one)
    l = torch.exp(torch.exp(-d2 / tau))
    p, Z = _S(l * pos.to(dt), 1, order), _S(l, 1, order)
    keep = torch.ones(B, dtype=torch.bool) if mistake == "p0_rows_kept" else p != 0
    loss = -_S(torch.log(p[keep] / Z[keep]), 0, order) / B
    return {"loss": loss.detach(), "grad": _grad(loss, f)}


def _zipf_labels(rng, B):
    """Zipf labels: a few large classes and, from B = 3 on, at least one singleton (a row with p == 0)."""
    y = rng.zipf(1.6, size=B).clip(max=25).astype(np.int64)
    if B >= 3:
        y[B // 2] = 1001
        y[0] = y[1] = 1
    return torch.from_numpy(y)


@functools.lru_cache(maxsize=None)
def contrastive_cases():
    out, k = [], 0
    for B in (1, 2, 255, 256, 257, 513):
        for E in (1, 3, 16, 32):
            rng = np.random.default_rng(1000 + k)
            temp = (100.0, 0.5)[(k + k // 4) % 2]
            out.append(Case("contrastive", f"zipf_B{B}_E{E}_t{temp:g}", f=_t(rng.standard_normal((B, E)) / math.sqrt(E)), y=_zipf_labels(rng, B),
                            temperature=temp, labels="zipf"))
            k += 1
    # (all labels equal: p = Z - e in every row, the gradient is a difference of 1 / p and 1 / Z of size e / B^2, and the fp32 round-off of the
    # two sums is 1e-7 * B / e of it -- 1e-5 at B = 257, ill-conditioned.  The all-equal sets stay small.)
    for B, temp in ((2, 100.0), (2, 0.5), (16, 100.0), (33, 0.5)):
        rng = np.random.default_rng(1100 + k)
        f = _t(rng.standard_normal((B, 3)) / math.sqrt(3))
        out.append(Case("contrastive", f"equal_B{B}_t{temp:g}", f=f, y=torch.full((B,), 4, dtype=torch.int64), temperature=temp, labels="equal"))
        k += 1
    for B, temp in ((2, 100.0), (2, 0.5), (257, 100.0), (257, 0.5)):
        rng = np.random.default_rng(1100 + k)
        f = _t(rng.standard_normal((B, 3)) / math.sqrt(3))
        out.append(Case("contrastive", f"distinct_B{B}_t{temp:g}", f=f, y=torch.arange(B, dtype=torch.int64) * 3 - 5, temperature=temp,
                        labels="distinct"))
        k += 1
    for temp in (100.0, 0.5):
        rng = np.random.default_rng(1200 + k)
        B, E = 64, 3
        f = _t(rng.standard_normal((B, E)) / math.sqrt(E))
        y = _zipf_labels(rng, B)
        f[1] = f[0]                      # identical rows, equal labels (y[0] == y[1] == 1)
        f[3] = f[2]
        y[2], y[3] = 2, 3                # identical rows, different labels
        out.append(Case("contrastive", f"identical_rows_t{temp:g}", f=f.clone(), y=y.clone(), temperature=temp, labels="zipf"))
        g = f.clone()
        g[5] = 1000.0                    # exp(-d2 / tau) underflows to 0 for every pair of this row, at either temperature
        y[5] = 1
        out.append(Case("contrastive", f"outlier_t{temp:g}", f=g, y=y.clone(), temperature=temp, labels="zipf"))
        k += 1
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- slow-fast
def _eval_slow_fast(c, dt, order, mistake):
    """Fast set = rays [0, B/2) with the fast features x[:, :E]; slow set = rays [B/2, B) with the detached slow features x[:, E:] (an odd
    ray belongs to the slow set).  Concentration: per intersecting label the mean over its fast rays of -exp(-|f_i - c_l|^2) conf_i, c_l the
    slow centroid, averaged over the intersecting labels.  Contrast: l_ij = exp(exp(-|f_i - s_j|)) with the plain distance, mean over the
    rows with a positive of -log(num_i / Z_i).  A pair at zero distance has zero gradient."""
    x = c.inst.to(dt).requires_grad_(True)
    y, conf = c.y, c.conf.to(dt)
    B, E = x.shape[0], x.shape[1] // 2
    H = (B + 1) // 2 if mistake == "odd_ray_fast" else B // 2
    if H == 0 or H == B:
        return {"loss": torch.zeros((), dtype=dt), "grad": torch.zeros_like(x).detach()}
    fast, slow = x[:H, :E], x[H:, E:].detach()
    slow_c = x[H:, E:] if mistake == "centroid_not_detached" else slow
    yf, ys = y[:H], y[H:]
    labf = (yf[:, None] == ys[None, :]).to(dt)
    ns = labf.sum(1)
    nf = (yf[:, None] == (y if mistake == "nf_over_all_rays" else yf)[None, :]).to(dt).sum(1)
    has = ns > 0
    nl = int(torch.unique(yf[has]).numel())
    loss = torch.zeros((), dtype=dt)
    if nl > 0:
        cent = _S(labf[:, :, None] * slow_c[None, :, :], 1, order) / ns.clamp(min=1)[:, None]
        dc = fast - cent
        conc = -torch.exp(-_S(dc * dc, 1, order)) * conf[:H] / nf
        loss = _S(conc[has], 0, order) / nl
    diff = fast[:, None, :] - slow[None, :, :]
    d2 = _S(diff * diff, 2, order)
    if mistake == "squared_distance":
        dist = d2
    else:
        zero = d2 == 0
        dist = torch.where(zero, torch.zeros_like(d2), torch.sqrt(torch.where(zero, torch.ones_like(d2), d2)))
    l = torch.exp(torch.exp(-dist))
    num, Z = _S(l * labf, 1, order), _S(l, 1, order)
    valid = num != 0
    loss = loss + -_S(torch.log(num[valid] / Z[valid]), 0, order) / int(valid.sum())      # 0 / 0 = NaN, like the mean of an empty tensor
    return {"loss": loss.detach(), "grad": _grad(loss, x).detach()}


@functools.lru_cache(maxsize=None)
def slow_fast_cases():
    out, k = [], 0
    for B in (1, 2, 3, 256, 511, 513, 1026):
        for E in (1, 3, 16, 32):
            rng = np.random.default_rng(2000 + k)
            H = B // 2
            x = _t(rng.standard_normal((B, 2 * E)) / math.sqrt(E))
            conf = rng.uniform(0.1, 1, B)
            if B <= 3:
                y = torch.tensor([1, 1, 2][:B], dtype=torch.int64)
            else:
                y = torch.from_numpy(rng.zipf(1.6, size=B).clip(max=25).astype(np.int64))
                y[:H][y[:H] == 7] = 26
                y[1] = 26                # a label only in the fast half
                y[B - 2] = 27            # and one only in the slow half
                y[0] = y[H] = 1
                x[0, :E] = x[H, E:]      # a coincident fast / slow pair
                conf[::5] = 0.0
            out.append(Case("slow_fast", f"B{B}_E{E}", inst=x, y=y, conf=_t(conf), kind="zipf"))
            k += 1
    # 210 intersecting labels with n_f cycling through 1, 3, 7: the kernel recovers the count as rint(sum 1 / n_f)
    rng = np.random.default_rng(2100)
    nfs = [(1, 3, 7)[i % 3] for i in range(210)]
    yf = np.repeat(np.arange(210), nfs)
    ys = np.concatenate([np.arange(210), rng.integers(0, 210, yf.size - 210)])
    rng.shuffle(yf)
    rng.shuffle(ys)
    y = torch.from_numpy(np.concatenate([yf, ys]).astype(np.int64))
    B = y.numel()
    out.append(Case("slow_fast", "labels210_nf137", inst=_t(rng.standard_normal((B, 6)) / math.sqrt(3)), y=y, conf=_t(rng.uniform(0.1, 1, B)),
                    kind="many_labels"))
    rng = np.random.default_rng(2101)
    B = 64
    y = torch.from_numpy(np.concatenate([rng.integers(1, 6, 32), rng.integers(6, 11, 32)]).astype(np.int64))
    out.append(Case("slow_fast", "no_common_label", inst=_t(rng.standard_normal((B, 6)) / math.sqrt(3)), y=y, conf=_t(rng.uniform(0.1, 1, B)),
                    kind="no_common"))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- pixel losses
def _sem_rows(x, p, w, sce, alpha, beta, order, mistake):
    """sce == 0: -sum_c w_c p_c log_softmax(x)_c.  sce != 0: alpha * that + beta * RCE, RCE = -sum_c clamp(softmax(w . x), 1e-8, 1)_c
    log(clamp(p_c, 1e-8, 1)) w_c; the clamp passes no gradient where it is active."""
    mx = x.max(1, keepdim=True).values.detach()
    lse = mx[:, 0] + torch.log(_S(torch.exp(x - mx), 1, order))
    ce = -_S(w * p * (x - lse[:, None]), 1, order)
    if not sce:
        return ce
    z = w * x
    ez = torch.exp(z - z.max(1, keepdim=True).values.detach())
    q = ez / _S(ez, 1, order)[:, None]
    qc = q.clamp(1e-8, 1.0)
    if mistake == "clamp_passes_gradient":
        qc = q + (qc - q).detach()
    L = torch.log(p.clamp(1e-8, 1.0))
    rce = -_S(qc * L * (1.0 if mistake == "reverse_term_unweighted" else w), 1, order)
    return alpha * ce + beta * rce


def _opt(t, dt, n):
    return torch.ones(n, dtype=dt) if t is None else t.to(dt)


def _eval_pixel(c, dt, order, mistake):
    """out2[0] += mean((mask (rgb - gt))^2); out2[1] += mean_i(mask_i conf_i row_loss_i); g_rgb = w_rgb d out2[0] / d rgb, g_sem likewise."""
    N, C = c.N, c.C
    mk = _opt(c.maskf, dt, N)
    out = {"out0": c.prefill[0].to(dt), "out1": c.prefill[1].to(dt)}
    if c.rgb is not None:
        rgb = c.rgb.to(dt).requires_grad_(True)
        d = mk[:, None] * (rgb - c.gt.to(dt))
        l0 = _S((d * d).reshape(-1), 0, order) / (3 * N)
        out["out0"] = (out["out0"] + l0).detach()
        if c.want_g_rgb:
            out["g_rgb"] = c.w_rgb * _grad(l0, rgb)
    if c.sem is not None:
        sem = c.sem.to(dt).requires_grad_(True)
        rows = _sem_rows(sem, c.probs.to(dt), _opt(c.class_w, dt, C), c.sce, c.alpha, c.beta, order, mistake)
        l1 = _S(_opt(c.conf, dt, N) * mk * rows, 0, order) / N
        out["out1"] = (out["out1"] + l1).detach()
        if c.want_g_sem:
            out["g_sem"] = c.w_sem * _grad(l1, sem)
    return out


def _eval_rows(c, dt, order, mistake):
    x = c.pred.to(dt).requires_grad_(True)
    rows = _sem_rows(x, c.probs.to(dt), _opt(c.class_w, dt, c.C), c.sce, c.alpha, c.beta, order, mistake)
    out = {"rows": rows.detach()}
    if c.want_grad:
        out["grad"] = _grad(rows.sum(), x)
    return out


PIXEL_NULLS = (None, "conf", "class_w", "maskf", "rgb", "sem", "g_rgb", "g_sem")
SEM_MODES = ((0, 1.0, 0.0), (1, 1.0, 1.0), (1, 0.5, 2.0))            # (sce, alpha, beta)
PIXEL_SHAPES = tuple((N, C) for N in (1, 255, 256, 257, 777) for C in (1, 2, 22))


def _semantic_inputs(rng, N, C, onehot):
    """Logits, targets and class weights: class_w[0] = 0 (C > 1).  With more than one row, row 0 has a logit gap of 30 on class 1, so that
    every other q of that row is far below 1e-8 and the clamp of the reverse term is active (alone, such a row has a loss of 1e-13 that fp32
    cannot hold).  The lone row of N = 1, C = 22 has nineteen classes just below the clamp instead (class_w . x = -17.5, q = 8.4e-9 each; classes
    0, 1 and 4 share the rest at class_w . x = 0) under zero targets: a clamp that passed its gradient would move the gradients of classes 1
    and 4 by 2e-6 and more of their size there, where a single clamped class moves them by 1e-7 at the most.  The logits stay at or below 0:
    x - logsumexp(x) carries an absolute error of ulp(logsumexp), which one row alone does not average out.
    One-hot targets put exact 0 and 1 inside log(clamp(p))."""
    sem = rng.standard_normal((N, C)) * 2.0
    if onehot:
        probs = np.zeros((N, C))
        probs[np.arange(N), rng.integers(0, C, N)] = 1.0
    else:
        e = np.exp(rng.standard_normal((N, C)))
        probs = e / e.sum(1, keepdims=True)
    cw = np.ones(C)
    if C > 1:
        cw[0] = 0.0
        cw[1::3] = 2.0
        if N > 1:
            sem[0] = 0.0
            sem[0, 1] = 30.0
        elif C == 22:
            sem[0] = np.where(cw == 2.0, -8.75, -17.5)
            sem[0, 0], sem[0, 1], sem[0, 4] = -30.0, 0.0, 0.0
            probs[0] = 0.0
            probs[0, 1], probs[0, 4] = 0.7, 0.3
    else:
        cw[0] = 2.0
    return _t(sem), _t(probs), _t(cw)


def _pixel_case(name, seed, N, C, mode, null, onehot):
    rng = np.random.default_rng(seed)
    sem, probs, cw = _semantic_inputs(rng, N, C, onehot)
    conf = rng.uniform(0.05, 1, N)
    conf[3::7] = 0.0
    f = dict(N=N, C=C, rgb=_t(rng.uniform(0, 1, (N, 3))), gt=_t(rng.uniform(0, 1, (N, 3))), sem=sem, probs=probs, conf=_t(conf), class_w=cw,
             maskf=_t((rng.uniform(0, 1, N) > 0.2).astype(np.float64)), want_g_rgb=True, want_g_sem=True,
             prefill=torch.tensor([0.25, -1.5]), w_rgb=f32r(0.7), w_sem=f32r(0.1), sce=mode[0], alpha=mode[1], beta=mode[2], null=null,
             onehot=onehot)
    if null in ("conf", "class_w", "maskf"):
        f[null] = None
    elif null == "rgb":
        f["rgb"] = f["gt"] = None
    elif null == "sem":
        f["sem"] = f["probs"] = None
    elif null == "g_rgb":
        f["want_g_rgb"] = False
    elif null == "g_sem":
        f["want_g_sem"] = False
    return Case("pixel", name, **f)


@functools.lru_cache(maxsize=None)
def pixel_cases():
    out, k = [], 0
    for N, C in PIXEL_SHAPES:
        for mi, mode in enumerate(SEM_MODES):
            null = PIXEL_NULLS[k % 8]
            out.append(_pixel_case(f"N{N}_C{C}_m{mi}_null-{null}", 3000 + k, N, C, mode, null, onehot=k % 2 == 1))
            k += 1
    for mi, mode in enumerate(SEM_MODES):
        for null in PIXEL_NULLS:
            out.append(_pixel_case(f"N257_C22_m{mi}_null-{null}_all", 3000 + k, 257, 22, mode, null, onehot=k % 2 == 0))
            k += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rows_cases():
    out, k = [], 0
    for N, C in PIXEL_SHAPES:
        for mi, mode in enumerate(SEM_MODES):
            rng = np.random.default_rng(3500 + k)
            sem, probs, cw = _semantic_inputs(rng, N, C, onehot=k % 2 == 0)
            out.append(Case("rows", f"N{N}_C{C}_m{mi}", N=N, C=C, pred=sem, probs=probs, class_w=None if k % 4 == 1 else cw, sce=mode[0],
                            alpha=mode[1], beta=mode[2], want_grad=k % 5 != 4))
            k += 1
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- segment consistency
def _first_max(m):
    ar = torch.arange(m.shape[1])
    return torch.where(m == m.max(1, keepdim=True).values, ar, m.shape[1]).min(1).values


def _last_max(m):
    ar = torch.arange(m.shape[1])
    return torch.where(m == m.max(1, keepdim=True).values, ar, -1).max(1).values


def segment_sums(c, dt=F64, order="natural"):
    idx = torch.arange(c.B) if order == "natural" else _index(c.B, order)
    return torch.zeros(c.G, c.C, dtype=dt).index_add_(0, c.group[idx], c.feats.to(dt)[idx])


def _eval_segment(c, dt, order, mistake):
    """Target class of a segment = first maximum of its feature sums; loss += mean_i(class_w[t_i] conf_i CE(feats_i, t_i)); grad = scale *
    d loss / d feats."""
    f = c.feats.to(dt).requires_grad_(True)
    sums = segment_sums(c, dt, order)
    tg = (_last_max if mistake == "last_maximum" else _first_max)(sums)
    t = tg[c.group]
    mx = f.max(1, keepdim=True).values.detach()
    lse = mx[:, 0] + torch.log(_S(torch.exp(f - mx), 1, order))
    li = c.class_w.to(dt)[t] * c.conf.to(dt) * (lse - f[torch.arange(c.B), t])
    l = _S(li, 0, order) / c.B
    out = {"loss": (c.prefill.to(dt) + l).detach()}
    if c.want_grad:
        out["grad"] = c.scale * _grad(l, f)
    return out


def segment_gaps(c):
    """Per occupied segment: (top - second) / max|mean| of its fp64 mean feature row (inf for C == 1)."""
    sums = segment_sums(c)
    cnt = torch.bincount(c.group, minlength=c.G)
    mean = sums[cnt > 0] / cnt[cnt > 0, None]
    if c.C == 1:
        return torch.full((mean.shape[0],), float("inf"), dtype=F64)
    top = mean.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) / mean.abs().max(1).values


@functools.lru_cache(maxsize=None)
def segment_cases():
    out, k = [], 0
    for B in (1, 255, 257, 600):
        for C in (1, 3, 22):
            rng = np.random.default_rng(4000 + k)
            if k % 3 == 0:
                G, group = 1, np.zeros(B, dtype=np.int64)
            else:
                G, group = 7, rng.choice([0, 2, 3, 6], B)             # segments 1, 4 and 5 stay empty
            bias = rng.integers(0, C, G)
            feats = rng.standard_normal((B, C))
            feats[np.arange(B), bias[group]] += 2.0
            cw = np.ones(C)
            cw[0] = 0.5
            out.append(Case("segment", f"B{B}_C{C}_G{G}", B=B, C=C, G=G, feats=_t(feats), group=torch.from_numpy(group),
                            conf=_t(rng.uniform(0.05, 1, B)), class_w=_t(cw), ld=C + (0, 3)[k % 2], ldg=C + (5, 0)[k % 2],
                            want_grad=k % 5 != 4, scale=(1.0, 0.25)[k % 2], prefill=torch.tensor((0.0, 1.5)[(k // 2) % 2]), exact=False))
            k += 1
    # integer features: the sums are exact in any order, and segment 0 has its maximum twice (classes 1 and 3)
    feats = torch.tensor([[0, 2, 1, 2], [1, 3, 0, 3], [2, 0, 1, 0], [0, 1, 2, 1], [3, 1, 4, 0], [0, 0, 1, 2]], dtype=torch.float32)
    group = torch.tensor([0, 0, 0, 0, 1, 1])
    out.append(Case("segment", "integer_tie", B=6, C=4, G=2, feats=feats, group=group, conf=torch.tensor([1.0, 0.5, 0.25, 1.0, 0.75, 1.0]),
                    class_w=torch.tensor([0.5, 1.0, 2.0, 1.5]), ld=4, ldg=4, want_grad=True, scale=1.0, prefill=torch.tensor(0.0), exact=True))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- total variation
def _tv(x, dt, order, mistake):
    H, W, C = x.shape
    cnt_h = _c(float(C * (H - 1) * W), dt) + _c(1e-4, dt)
    cnt_w = _c(float(C * H * (W - 1)), dt) + _c(1e-4, dt)
    if mistake == "counts_swapped":
        cnt_h, cnt_w = cnt_w, cnt_h
    dh, dw = x[1:] - x[:-1], x[:, 1:] - x[:, :-1]
    return 2 * (_S((dh * dh).reshape(-1), 0, order) / cnt_h + _S((dw * dw).reshape(-1), 0, order) / cnt_w)


def _eval_tv(c, dt, order, mistake):
    """loss += weight * TV(x), grad += weight * dTV/dx for every plane of the case (a single-plane case has one)."""
    loss = c.loss_prefill.to(dt)
    out = {}
    for i, x in enumerate(c.planes):
        x = x.to(dt).requires_grad_(True)
        tv = _tv(x, dt, order, mistake)
        w = _c(c.weights[i], dt)
        loss = loss + w * tv.detach()
        if c.grad_prefill[i] is not None:
            out[f"grad{i}"] = c.grad_prefill[i].to(dt) + w * _grad(tv, x)
    out["loss"] = loss
    return out


TV_SHAPES = ((1, 1, 1), (1, 7, 3), (7, 1, 3), (2, 2, 1), (33, 29, 5), (128, 96, 48))


def _tv_case(kernel, name, seed, shapes, weights, null_grads=(), loss_prefill=0.5):
    rng = np.random.default_rng(seed)
    planes = [_t(rng.standard_normal(s)) for s in shapes]
    pre = [None if i in null_grads else _t(rng.standard_normal(s) * 0.1) for i, s in enumerate(shapes)]
    return Case(kernel, name, planes=planes, weights=[f32r(w) for w in weights], grad_prefill=pre, loss_prefill=torch.tensor(loss_prefill))


@functools.lru_cache(maxsize=None)
def tv_cases():
    out = []
    for k, s in enumerate(TV_SHAPES):
        tag = "x".join(str(v) for v in s)
        out.append(_tv_case("tv", f"{tag}_w0.37_accumulate", 5000 + k, [s], [0.37]))
        out.append(_tv_case("tv", f"{tag}_w1_nograd", 5100 + k, [s], [1.0], null_grads=(0,), loss_prefill=0.0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tv_multi_cases():
    six = [(33, 29, 5), (2, 2, 4), (64, 64, 48), (7, 1, 3), (8, 8, 12), (1, 7, 8)]
    eight = [(5, 6, 4), (1, 1, 1), (9, 3, 7), (16, 16, 8), (2, 2, 1), (3, 40, 4), (7, 1, 3), (12, 11, 16)]
    assert len(eight) == TV_MAX
    return (_tv_case("tv_multi", "one_plane", 5200, [(16, 16, 8)], [0.37]),
            _tv_case("tv_multi", "six_mixed", 5201, six, [0.37, 1.0, 0.01, 2.0, 0.5, 0.001], null_grads=(4,)),
            _tv_case("tv_multi", "max_planes", 5202, eight, [0.1 * (i + 1) for i in range(8)], null_grads=(1,)),
            _tv_case("tv_multi", "lone_1x1x3", 5203, [(1, 1, 3)], [0.37]),
            _tv_case("tv_multi", "lone_1x3x1", 5204, [(1, 3, 1)], [0.37]))


# ---------------------------------------------------------------------------------------------------------------- Adam / EMA
ADAM_STEPS = (1, 2, 3, 4, 5, 1000)
ADAM_EPS = f32r(1e-8)
# The trainer's two learning rates.  1 - beta2^step loses up to 3e-5 of its value in fp32 at steps 2..5 (beta2 = 0.999), which moves p by that
# fraction of the step; with weight decay 1e-3 that error returns through wd * p into elements whose gradient is no larger, and at lr = 1e-2
# the fp32 restatement is then up to 3.6e-5 of the step's scale away from fp64: ill-conditioned.  The decay 1e-3 runs at the smaller rate.
ADAM_LR = {0.0: f32r(1e-2), 1e-8: f32r(1e-2), 1e-3: f32r(5e-4)}


def _eval_adam(c, dt, order, mistake):
    """torch.optim.Adam's formulas (weight decay folded into the gradient before the moments), one dict entry per step: the moments m<k>,
    v<k>, the parameters p<k> and the step d<k> = p<k> - p<k-1> taken from the stored values."""
    b1, b2, lr, eps, wd = (_c(v, dt) for v in (c.beta1, c.beta2, c.lr, ADAM_EPS, c.wd))
    p, m, v = c.p0.to(dt), torch.zeros(c.n, dtype=dt), torch.zeros(c.n, dtype=dt)
    out = {}
    for k, (step, g) in enumerate(zip(ADAM_STEPS, c.grads)):
        g = g.to(dt)
        if mistake != "decay_after_moments":
            g = g + wd * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        t = step - 1 if mistake == "bias_step_minus_one" else step
        bc1, bc2s = 1 - b1 ** t, torch.sqrt(1 - b2 ** t)
        new = p - (lr / bc1) * m / (torch.sqrt(v) / bc2s + eps)
        if mistake == "decay_after_moments":
            new = new - lr * wd * p
        out[f"m{k}"], out[f"v{k}"], out[f"p{k}"], out[f"d{k}"] = m, v, new, new.to(F64) - p.to(F64)
        p = new
    return out


def adam_torch(c):
    """The same quantities from torch.optim.Adam in fp64 (the step counter set before every call)."""
    p = c.p0.to(F64).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=c.lr, betas=(c.beta1, c.beta2), eps=ADAM_EPS, weight_decay=c.wd)
    out = {}
    for k, (step, g) in enumerate(zip(ADAM_STEPS, c.grads)):
        before = p.detach().clone()
        p.grad = g.to(F64).clone()
        if k > 0:
            st = opt.state[p]
            if torch.is_tensor(st["step"]):
                st["step"].fill_(step - 1)
            else:
                st["step"] = step - 1
        opt.step()
        st = opt.state[p]
        out[f"m{k}"], out[f"v{k}"], out[f"p{k}"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone(), p.detach().clone()
        out[f"d{k}"] = p.detach() - before
    return out


ADAM_N = (1, 255, 257, 10007, 4096 * 256 + 3)
EMA_N = ADAM_N + (2048 * 256 + 3,)
ADAM_BETAS = ((0.9, 0.99), (0.9, 0.999))
ADAM_WD = (0.0, 1e-8, 1e-3)


def _adam_case(name, seed, n, betas, wd, lo=-8.0, hi=0.0):
    """Parameters at magnitude 1e-4 (the step, not the rounding of p, dominates); gradient magnitudes 10^lo .. 10^hi, log-uniform, random
    signs, every seventh element (from the fourth on) an exact zero."""
    rng = np.random.default_rng(seed)
    grads = []
    for _ in ADAM_STEPS:
        g = 10.0 ** rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)
        g[3::7] = 0.0
        grads.append(_t(g))
    return Case("adam", name, n=n, p0=_t(rng.standard_normal(n) * 1e-4), grads=grads, beta1=f32r(betas[0]), beta2=f32r(betas[1]), wd=f32r(wd),
                lr=ADAM_LR[wd])


@functools.lru_cache(maxsize=None)
def adam_cases():
    out, k = [], 0
    for n in ADAM_N:
        big = n > 100000
        for bi, betas in enumerate(ADAM_BETAS):
            for wi, wd in enumerate(ADAM_WD):
                # the long arrays: one run per beta pair.  (Not with decay 1e-3: an element with a zero gradient is driven by wd * p alone, p
                # feeds itself, and among 150 000 such elements the worst is 1.1e-5 of the step's scale off in fp32 -- ill-conditioned.)
                if big and (bi != wi):
                    continue
                out.append(_adam_case(f"n{n}_b{betas[1]}_wd{wd:g}", 6000 + k, n, betas, wd))
                k += 1
    # gradients no larger than the decay term wd * p, so that where the decay enters is visible in the moments
    out.append(_adam_case("n257_small_gradients_wd0.001", 6100, 257, ADAM_BETAS[0], 1e-3, lo=-8.0, hi=-7.0))
    return tuple(out)


def _eval_ema(c, dt, order, mistake):
    mom = _c(c.momentum, dt)
    s, f = c.slow.to(dt), c.fast.to(dt)
    return {"slow": s * (1 - mom) + mom * f if mistake == "momentum_on_fast" else s * mom + (1 - mom) * f}


@functools.lru_cache(maxsize=None)
def ema_cases():
    out, k = [], 0
    for n in EMA_N:
        for mom in (0.0, 0.9, 1.0):
            rng = np.random.default_rng(6500 + k)
            out.append(Case("ema", f"n{n}_mom{mom:g}", n=n, slow=_t(rng.standard_normal(n)), fast=_t(rng.standard_normal(n)), momentum=f32r(mom)))
            k += 1
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- nearest centroid
CENTROID_GAP = 1e-4
CENTROID_LEFT_OUT = 0.01


def centroid_reference(c):
    """(labels int64 (n,), sure bool (n,)): first minimum of the fp64 squared distances, -1 for an invalid row and for a row whose distances
    are all NaN; sure = the top-two gap is at least CENTROID_GAP relative (every row of an exact case, and of K == 1)."""
    f, cent = c.feat[:, :c.E].to(F64), c.cent.to(F64)
    d2 = ((f[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
    nan = torch.isnan(d2).all(1)
    d = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
    lab = torch.where(d == d.min(1, keepdim=True).values, torch.arange(c.K), c.K).min(1).values
    lab[nan] = -1
    if c.valid is not None:
        lab[c.valid == 0] = -1
    if c.exact or c.K == 1:
        sure = torch.ones(c.n, dtype=torch.bool)
    else:
        two = d.topk(2, dim=1, largest=False).values
        sure = (two[:, 1] - two[:, 0]) >= CENTROID_GAP * two[:, 1]
        sure |= lab < 0
    return lab, sure


@functools.lru_cache(maxsize=None)
def centroid_cases():
    out, k = [], 0
    for n in (1, 257):
        for K in (1, 2, 37):
            for E in (1, 3, 8):
                rng = np.random.default_rng(7000 + k)
                ldf = E + (0, 3)[k % 2]
                feat = rng.standard_normal((n, ldf))
                valid = None if k % 3 == 0 else torch.from_numpy((rng.uniform(0, 1, n) > 0.3).astype(np.uint8))
                out.append(Case("centroid", f"n{n}_K{K}_E{E}_ldf{ldf}", n=n, K=K, E=E, ldf=ldf, feat=_t(feat), cent=_t(rng.standard_normal((K, E))),
                                valid=valid, exact=False))
                k += 1
    # integer coordinates: exact distances in fp32, ties between two and between four centroids, a repeated centroid
    cent = torch.tensor([[0, 0], [2, 0], [0, 2], [2, 2], [2, 0]], dtype=torch.float32)
    feat = torch.tensor([[1, 0, 9], [1, 1, 9], [2, 1, 9], [0, 1, 9], [2, 0, 9], [1, 2, 9], [5, 5, 9]], dtype=torch.float32)
    out.append(Case("centroid", "integer_ties", n=7, K=5, E=2, ldf=3, feat=feat, cent=cent, valid=None, exact=True))
    rng = np.random.default_rng(7100)
    feat = _t(rng.integers(-3, 4, (257, 3)).astype(np.float64))
    feat[3, 1] = float("nan")
    feat[200, :] = float("nan")
    out.append(Case("centroid", "nan_rows", n=257, K=4, E=3, ldf=3, feat=feat, cent=_t(rng.integers(-3, 4, (4, 3)).astype(np.float64)),
                    valid=None, exact=True))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- reference, yardstick, bound
_EVAL = {"contrastive": _eval_contrastive, "slow_fast": _eval_slow_fast, "pixel": _eval_pixel, "rows": _eval_rows, "segment": _eval_segment,
         "tv": _eval_tv, "tv_multi": _eval_tv, "adam": _eval_adam, "ema": _eval_ema}
CASES = {"contrastive": contrastive_cases, "slow_fast": slow_fast_cases, "pixel": pixel_cases, "rows": rows_cases, "segment": segment_cases,
         "tv": tv_cases, "tv_multi": tv_multi_cases, "adam": adam_cases, "ema": ema_cases}

# mistakes a kernel could plausibly make; test_bounds_catch_known_mistakes applies each to the fp32 restatement
MISTAKES = {"contrastive": ("diagonal_positive", "temperature_on_negatives", "row_j_term_dropped", "p0_rows_kept"),
            "slow_fast": ("squared_distance", "nf_over_all_rays", "odd_ray_fast", "centroid_not_detached"),
            "pixel": ("reverse_term_unweighted", "clamp_passes_gradient"),
            "segment": ("last_maximum",),
            "tv": ("counts_swapped",),
            "adam": ("bias_step_minus_one", "decay_after_moments"),
            "ema": ("momentum_on_fast",)}


@functools.lru_cache(maxsize=4)
def reference(case):
    """{quantity: fp64 tensor}.  Adam's comes from torch.optim.Adam itself."""
    if case.kernel == "adam":
        return adam_torch(case)
    return {q: v.detach() for q, v in _EVAL[case.kernel](case, F64, "natural", None).items()}


def restate(case, order="natural", mistake=None):
    """{quantity: tensor}: the same formulas in fp32, reductions in ``order``, optionally with one of MISTAKES built in."""
    return {q: v.detach() for q, v in _EVAL[case.kernel](case, F32, order, mistake).items()}


def max_error(a, ref):
    """max |a - ref| in fp64; entries where both are NaN agree; inf where only one is NaN or the shapes differ."""
    a, ref = torch.as_tensor(a).detach().cpu().to(F64), torch.as_tensor(ref).detach().cpu().to(F64)
    if a.shape != ref.shape:
        return float("inf")
    if a.numel() == 0:
        return 0.0
    d = (a - ref).abs()
    d = torch.where(torch.isnan(a) & torch.isnan(ref), torch.zeros_like(d), d)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float(d.max())


def scale_of(ref):
    r = torch.as_tensor(ref).detach().to(F64).abs().reshape(-1)
    r = r[torch.isfinite(r)]
    return float(r.max()) if r.numel() else 0.0


@functools.lru_cache(maxsize=None)
def yardsticks(case):
    """{quantity: max over the three orders of max|fp32 - fp64|}."""
    ref = reference(case)
    out = {q: 0.0 for q in ref}
    for order in ORDERS:
        r = restate(case, order)
        for q in ref:
            out[q] = max(out[q], max_error(r[q], ref[q]))
        if case.kernel in ("adam", "ema"):          # no reduction in these: the three orders are one
            break
    return out


def yardstick(case, quantity):
    return yardsticks(case)[quantity]


def bound(yard, scale):
    return 8.0 * yard + 4.0 * HALF_ULP * scale


# Bounds that had to be widened, each for one named instruction sequence and to twice the largest error measured over 900 launches (never
# beyond the 1e-4 relative that tests/test_gpu_parity.py holds a loss to).  All three are the same sequence: every block of k_tv ends in one
# unsafeAtomicAdd of its partial sum on the loss word, so the value goes through a chain of n roundings of the running total T, n = 2048
# blocks for the (128, 96, 48) plane and 768 for the (64, 64, 48) plane run on its own: a random walk of about sqrt(n) * ulp(T) / sqrt(12),
# where the fp32 restatement's pairwise sum (the yardstick) stays within an ulp.  The order of the atomics is nearly the same from launch
# to launch, so the error is too.  k_tv_multi caps a plane at 128 blocks and stays inside the plain bound.  A sum in a fixed order needs a
# workspace argument, which clift_tv_fwd_bwd does not have.
# The widening belongs to clift_tv_fwd_bwd alone: an entry names the calls it covers ("raw" and the TVLoss "wrapper" of a tv case, "single"
# = the planes of a tv_multi case one by one through clift_tv_fwd_bwd), and the "multi" launch of the same planes keeps the plain bound.
#   (kernel, case, quantity): (largest |device - fp64| measured, plain bound it missed, calls)
WIDENED = {("tv", "128x96x48_w0.37_accumulate", "loss"): (3.411e-06, 1.407e-06, ("raw",)),
           ("tv", "128x96x48_w1_nograd", "loss"): (1.265e-05, 3.887e-06, ("raw", "wrapper")),
           ("tv_multi", "six_mixed", "loss"): (3.968e-05, 2.749e-05, ("single",))}


def bound_for(case, quantity, call="raw"):
    """The bound of a quantity of a case as reached through ``call``: ``bound`` of its yardstick and scale, or twice the measured error
    where WIDENED lists that call."""
    b = bound(yardstick(case, quantity), scale_of(reference(case)[quantity]))
    entry = WIDENED.get((case.kernel, case.name, quantity))
    return max(b, 2.0 * entry[0]) if entry is not None and call in entry[2] else b


def adam_step_bound(case, k):
    """Per-element bound on Adam's step d<k> = p<k> - p<k-1> taken from stored fp32 parameters: half an fp32 ulp at |p<k>| for the rounding
    of the stored result, plus the bound of the step itself."""
    ref = reference(case)
    return HALF_ULP * ref[f"p{k}"].abs() + bound(yardstick(case, f"d{k}"), scale_of(ref[f"d{k}"]))


def exceeds(err, bnd):
    """True where an error breaks a bound (a NaN error breaks it)."""
    return not err <= bnd
