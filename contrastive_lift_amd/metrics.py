"""Panoptic quality -- restatement of reference util/panoptic_quality.py:205-247 (a torchmetrics-derived PQ with the
reference's "non-robust class" filtering), vectorised over packed (category, instance) ids instead of Python dicts of
colour tuples.  Host-side evaluation code (not on the per-ray path); pinned by tests/golden/g11_metrics.npz.

Semantics kept: classes absent from both maps and classes covering < ``robust`` of either map are dropped from
things/stuff; stuff instance ids are zeroed; unknown categories become void = (1 + max id, 0); a (pred, target) segment
pair of equal category matches when IoU > 0.5 with the void overlaps removed from the union; unmatched segments that
are more than half void on the other side are ignored; PQ/SQ/RQ are averaged over the remaining categories.

Backends.  ``panoptic_quality_match`` is two halves: the first produces the sorted segment keys of each side, their areas and the
intersection table; the second (``_match_segments``) is the matching loop, ONE function for every backend, so the fp64 IoU sums are formed by
the same operations in the same order.  ``backend="host"`` (the default) is the first half as it always was: ``np.unique`` and ``np.add.at``
on the host.  ``backend="device"`` and ``backend="counts"`` take the first half from two label-overlap counts (overlap.py: the kernel
``clift_label_overlap`` resp. its numpy restatement) per CALL, however many frames the call scores:

1. classes against classes (no instances; the target's dropped classes have base -1, its merged classes the base of their new class): the
   per-frame confusion matrix, whose marginals give the classes present, the classes under the ``robust`` share and the unknown predicted
   categories;
2. segments against segments: per frame and side, the surviving categories in ascending order own the slots -- a stuff class one slot
   (stride 0), a thing class a run of I slots (stride 1, I = the side's largest instance id + 1), every other class the void slot behind
   them -- so slots ascend with ``category * base + instance`` like the keys ``np.unique`` sorts; only the non-zero (frame, slot, slot, n)
   entries come to the host.

Counting is integer work, so the three backends return identical bits.  The count backends need non-negative class and instance ids that fit
int32 and tables of at most 1 GiB (``CliftError`` otherwise: use "host").
"""
import numpy as np
import torch

from . import overlap

ROBUST = 0.005          # the reference's share under which a class is left out of things / stuff (every default below)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _non_robust(sem_pred, sem_tgt, thr):
    out = set()
    for s in (sem_pred, sem_tgt):
        u, c = np.unique(s, return_counts=True)
        out |= set(u[(c / c.sum()) < thr].tolist())
    return out


def panoptic_quality(preds, target, things, stuff, allow_unknown_preds_category=False, robust=ROBUST, backend="host"):
    """preds, target: (..., 2) integer [category, instance].  Returns (pq, sq, rq) as 0-dim float64 tensors.  ``backend``: see the module
    docstring ("device" takes CUDA tensors as they are)."""
    return panoptic_quality_compute(*panoptic_quality_match(preds, target, things, stuff, allow_unknown_preds_category, robust, backend))


def panoptic_quality_match(preds, target, things, stuff, allow_unknown_preds_category=False, robust=ROBUST, backend="host"):
    """The matching half of ``panoptic_quality`` (util/panoptic_quality.py:250-268): returns (things, stuff, iou_sum, tp, fp, fn) -- the
    categories kept after the robust-class filter and the per-category vectors (things first), float64 numpy arrays."""
    if overlap.check_backend(backend) != "host":
        counter = overlap.Counter(backend, preds.device if torch.is_tensor(preds) and preds.is_cuda else None)
        p, t = counter.labels(preds).reshape(-1, 2), counter.labels(target).reshape(-1, 2)          # (anything np.asarray takes, like the host path)
        if p.shape != t.shape:
            raise ValueError("Expected argument `preds` and `target` to have the same shape")
        return _count_frames(counter, p[:, 0], p[:, 1], t[:, 0], t[:, 1], [0, int(p.shape[0])], things, stuff, allow_unknown_preds_category, robust)[0]
    p = _np(preds).reshape(-1, 2).astype(np.int64).copy()
    t = _np(target).reshape(-1, 2).astype(np.int64).copy()
    if p.shape != t.shape:
        raise ValueError("Expected argument `preds` and `target` to have the same shape")
    things, stuff = set(int(x) for x in things), set(int(x) for x in stuff)
    present = set(np.unique(p[:, 0]).tolist()) | set(np.unique(t[:, 0]).tolist())
    drop = ((things | stuff) - present) | _non_robust(p[:, 0], t[:, 0], robust)
    things, stuff = things - drop, stuff - drop
    if things & stuff:
        raise ValueError("Expected arguments `things` and `stuffs` to have distinct keys.")
    void_cat = 1 + max([0] + list(things) + list(stuff))
    cats = list(things) + list(stuff)                      # things first, like the reference's continuous ids

    def prep(img, allow_unknown):
        is_stuff = np.isin(img[:, 0], list(stuff))
        is_thing = np.isin(img[:, 0], list(things))
        img[is_stuff, 1] = 0
        if not allow_unknown and not np.all(is_stuff | is_thing):
            raise ValueError("Unknown categories found in preds")
        unk = ~(is_stuff | is_thing)
        img[unk, 0], img[unk, 1] = void_cat, 0
        return img
    p, t = prep(p, allow_unknown_preds_category), prep(t, True)
    base = int(max(p[:, 1].max(initial=0), t[:, 1].max(initial=0))) + 1
    kp, kt = p[:, 0] * base + p[:, 1], t[:, 0] * base + t[:, 1]
    void_key = void_cat * base
    up, ip, ap = np.unique(kp, return_inverse=True, return_counts=True)
    ut, it, at = np.unique(kt, return_inverse=True, return_counts=True)
    inter = np.zeros((len(up), len(ut)), np.int64)
    np.add.at(inter, (ip, it), 1)
    return (things, stuff) + _match_segments(cats, base, void_key, up, ut, ap, at, inter)


def _match_segments(cats, base, void_key, up, ut, ap, at, inter):
    """The second half of the match, shared by every backend: ``up`` / ``ut`` the sorted segment keys (category * base + instance) of the
    predicted / target map, ``ap`` / ``at`` their areas, ``inter`` (len(up), len(ut)) int64 their intersections, ``cats`` the kept categories
    (things first).  Returns (iou_sum, tp, fp, fn) over ``cats``."""
    vp = int(np.searchsorted(up, void_key)) if void_key in up else -1          # void row / column, if present
    vt = int(np.searchsorted(ut, void_key)) if void_key in ut else -1
    p_void_t = inter[:, vt] if vt >= 0 else np.zeros(len(up), np.int64)         # pred segment ∩ void target
    void_p_t = inter[vp, :] if vp >= 0 else np.zeros(len(ut), np.int64)         # void pred ∩ target segment
    n = len(cats)
    cid = {c: i for i, c in enumerate(cats)}
    iou_sum, tp, fp, fn = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    matched_p, matched_t = np.zeros(len(up), bool), np.zeros(len(ut), bool)
    pi, ti = np.nonzero(inter)
    for a, b in zip(pi.tolist(), ti.tolist()):
        if ut[b] == void_key or up[a] // base != ut[b] // base:
            continue
        cat = int(up[a] // base)
        if cat not in cid:
            continue
        i_ab = inter[a, b]
        union = ap[a] - p_void_t[a] + at[b] - void_p_t[b] - i_ab
        iou = i_ab / union
        if iou > 0.5:
            matched_p[a] = matched_t[b] = True
            iou_sum[cid[cat]] += iou
            tp[cid[cat]] += 1
    for b in np.nonzero(~matched_t)[0].tolist():
        if ut[b] == void_key or void_p_t[b] / at[b] > 0.5:
            continue
        fn[cid[int(ut[b] // base)]] += 1
    for a in np.nonzero(~matched_p)[0].tolist():
        if up[a] == void_key or p_void_t[a] / ap[a] > 0.5:
            continue
        fp[cid[int(up[a] // base)]] += 1
    return iou_sum, tp, fp, fn


def panoptic_quality_compute(things, stuff, iou_sum, tp, fp, fn):
    """The scoring half (util/panoptic_quality.py:177-222, "all"): per-category PQ / SQ / RQ averaged over every entry of the vectors.
    Returns (pq, sq, rq) as 0-dim float64 tensors (NaN for empty vectors)."""
    iou_sum, tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (iou_sum, tp, fp, fn))
    den = tp + 0.5 * fp + 0.5 * fn
    with np.errstate(divide="ignore", invalid="ignore"):
        pq = np.where(den > 0, iou_sum / den, 0.0)
        sq = np.where(tp > 0, iou_sum / tp, 0.0)
        rq = np.where(den > 0, tp / den, 0.0)
    f = lambda v: torch.tensor(float(np.mean(v)) if len(v) else float("nan"), dtype=torch.float64)
    return f(pq), f(sq), f(rq)


def _count_frames(counter, p_cls, p_inst, t_cls, t_inst, frame_off, things, stuff, allow_unknown, robust, t_drop=(), t_merge=None):
    """The first half of the match from label-overlap counts, for all frames of ``frame_off`` in two counts, then the shared second half per
    frame.  p_cls .. t_inst: flat label arrays where ``counter`` counts.  ``t_drop``: target classes whose rows are left out of the frame
    (both maps); ``t_merge``: {target class: the class it becomes}.  Returns one (things, stuff, iou_sum, tp, fp, fn) per frame."""
    off = overlap.check_frame_off(frame_off)
    F = off.size - 1
    things0, stuff0 = set(int(x) for x in things), set(int(x) for x in stuff)
    t_drop, t_merge = set(int(x) for x in t_drop), dict(t_merge or {})
    if not (p_cls.shape[0] == p_inst.shape[0] == t_cls.shape[0] == t_inst.shape[0] == int(off[-1])):
        raise ValueError("label arrays and frame_off disagree about the number of rows")
    t_class = lambda c: t_merge.get(c, c)
    # instance ids count for thing classes only (the host half zeroes the others): what the kernel reads and what sizes the slot runs
    p_inst = counter.where_class_in(p_cls, things0, p_inst)
    t_inst = counter.where_class_in(t_cls, {c for c in things0 | set(t_merge) if t_class(c) in things0}, t_inst)
    ext = counter.extremes([p_cls, p_inst, t_cls, t_inst])                     # the one reduction: class and instance bounds of both sides
    p_cls, p_inst, t_cls, t_inst = (counter.int32(x, lo, hi) for x, (lo, hi) in zip((p_cls, p_inst, t_cls, t_inst), ext))
    Ca, Cb = max(ext[0][1] + 1, 1), max(ext[2][1] + 1, 1)
    Ia, Ib = max(ext[1][1] + 1, 1), max(ext[3][1] + 1, 1)
    base = max(Ia, Ib)

    # 1. classes against classes
    NB1 = max([Cb] + [t_class(c) + 1 for c in range(Cb)])
    b_base = np.array([-1 if c in t_drop else t_class(c) for c in range(Cb)], np.int32)
    ident = lambda v: np.tile(v[None], (F, 1))
    cm = counter.host(counter.count(p_cls, None, t_cls, None, off, ident(np.arange(Ca, dtype=np.int32)), np.zeros((F, Ca), np.int32),
                                    ident(b_base), np.zeros((F, Cb), np.int32), Ca, NB1))
    p_share, t_share = cm.sum(2), cm.sum(1)                                    # (F, Ca), (F, NB1): pixels per class of the frame

    # per frame: the surviving categories (as the host half finds them) and the slot tables
    frames = []
    a_base, a_stride = np.zeros((F, Ca), np.int32), np.zeros((F, Ca), np.int32)
    b_base, b_stride = np.zeros((F, Cb), np.int32), np.zeros((F, Cb), np.int32)
    NA = NB = 1
    t_can = {t_class(c) for c in range(Cb) if c not in t_drop}                 # the classes a target row can have after the merge
    for f in range(F):
        present, weak = set(), set()
        for c in (p_share[f], t_share[f]):
            u = np.nonzero(c)[0]
            c = c[u]
            present |= set(u.tolist())
            weak |= set(u[(c / c.sum()) < robust].tolist())
        drop = ((things0 | stuff0) - present) | weak
        th, st = things0 - drop, stuff0 - drop
        if th & st:
            raise ValueError("Expected arguments `things` and `stuffs` to have distinct keys.")
        if not allow_unknown and any(c not in th and c not in st for c in np.nonzero(p_share[f])[0].tolist()):
            raise ValueError("Unknown categories found in preds")
        void_cat = 1 + max([0] + list(th) + list(st))
        keys = []
        for side, I, C_, tab_b, tab_s, cls_of, dropped in ((0, Ia, Ca, a_base, a_stride, lambda c: c, set()), (1, Ib, Cb, b_base, b_stride, t_class, t_drop)):
            can = t_can if side else None
            start, key, pos = {}, [], 0
            for c in sorted(th | st):                                          # ascending category: slots ascend with category * base + instance
                start[c] = pos
                n = 1 if c not in th else (I if can is None or c in can else 0)     # a thing class no target row can have owns no slots
                key.append(c * base + np.arange(n, dtype=np.int64))
                pos += n
            key.append(np.array([void_cat * base], np.int64))                  # the void slot, behind every kept category
            for c in range(C_):
                k = cls_of(c)
                tab_b[f, c] = -1 if c in dropped else start.get(k, pos)
                tab_s[f, c] = 1 if (c not in dropped and k in th) else 0
            keys.append(np.concatenate(key))
        NA, NB = max(NA, keys[0].size), max(NB, keys[1].size)
        frames.append((th, st, list(th) + list(st), void_cat * base, keys[0], keys[1]))

    # 2. segments against segments; only the non-zero entries come to the host
    overlap.check_table(F, NA, NB)
    ff, sa, sb, n = counter.nonzero(counter.count(p_cls, p_inst, t_cls, t_inst, off, a_base, a_stride, b_base, b_stride, NA, NB))
    cut = np.searchsorted(ff, np.arange(F + 1))
    out = []
    for f, (th, st, cats, void_key, key_a, key_b) in enumerate(frames):
        lo, hi = cut[f], cut[f + 1]
        up, ip = np.unique(key_a[sa[lo:hi]], return_inverse=True)
        ut, it = np.unique(key_b[sb[lo:hi]], return_inverse=True)
        inter = np.zeros((len(up), len(ut)), np.int64)
        inter[ip.reshape(-1), it.reshape(-1)] = n[lo:hi]
        out.append((th, st) + _match_segments(cats, base, void_key, up, ut, inter.sum(1), inter.sum(0), inter))
    return out


def panoptic_quality_per_frame(sem_pred, inst_pred, sem_target, inst_target, is_thing, faulty_gt=(), backend="host", frame_off=None):
    """PQ of a set of frames scored frame by frame, as the reference's bandwidth search does it (inference/find_bandwidth.py:314-376,
    MY_calculate_panoptic_quality_per_frame_folders[_MOS]): per frame, target pixels whose class is in ``faulty_gt`` are dropped, every
    thing class of the target becomes the first thing class, and the frame is matched on its own (``panoptic_quality_match`` with unknown
    predicted categories allowed); the per-category vectors of all frames are concatenated and averaged (not a scene aggregate).
    Arguments are dicts {frame name: (H, W) integer image} keyed alike (names are numeric stems, taken in numeric order).
    With ``backend="device"`` / ``"counts"`` all frames are scored in two label-overlap counts (module docstring), and the four label
    arguments may also be stacked arrays / CUDA tensors: (F, ...) with equal frames, or flat with ``frame_off`` (F + 1 row offsets, a host
    sequence), the frames in their order.
    Returns (pq, sq, rq) floats."""
    things = set(i for i, t in enumerate(is_thing) if t)
    stuff = set(i for i, t in enumerate(is_thing) if not t)
    first_thing = list(things)[0]
    if overlap.check_backend(backend) != "host":
        stacked = not isinstance(sem_pred, dict)
        ref = sem_pred if stacked else next(iter(sem_pred.values()), None)
        counter = overlap.Counter(backend, ref.device if torch.is_tensor(ref) and ref.is_cuda else None)
        if stacked:
            if frame_off is None:
                F = int(sem_pred.shape[0])
                per = int(np.prod(tuple(sem_pred.shape)[1:], dtype=np.int64))
                frame_off = [per * f for f in range(F + 1)]
            flat = [counter.labels(x) for x in (sem_pred, inst_pred, sem_target, inst_target)]
        else:
            names = sorted(sem_pred, key=lambda x: int(str(x).split(".")[0]))
            maps = [[counter.labels(d[nm]) for nm in names] for d in (sem_pred, inst_pred, sem_target, inst_target)]
            frame_off = np.concatenate([[0], np.cumsum([int(x.shape[0]) for x in maps[0]])]).astype(np.int64)
            flat = [counter.cat(m) if m else counter.labels(np.zeros(0, np.int64)) for m in maps]
        per_frame = _count_frames(counter, *flat, frame_off, things, stuff, True, ROBUST, t_drop=faulty_gt,
                                  t_merge={c: first_thing for c in things})
        parts = [[m[2 + j] for m in per_frame] for j in range(4)]
        pq, sq, rq = panoptic_quality_compute(things, stuff, *(np.concatenate(p_) for p_ in parts))
        return float(pq), float(sq), float(rq)
    if frame_off is not None or not isinstance(sem_pred, dict):
        raise ValueError('backend="host" scores dicts of frames; stacked label arrays go with backend="device" or "counts"')
    parts = [[], [], [], []]
    for name in sorted(sem_pred, key=lambda x: int(str(x).split(".")[0])):
        ts = np.asarray(sem_target[name])
        valid = ~np.isin(ts, list(faulty_gt))
        ts = ts[valid].astype(np.int64)
        ts = np.where(np.isin(ts, list(things)), first_thing, ts)
        pred = np.stack([np.asarray(sem_pred[name])[valid], np.asarray(inst_pred[name])[valid]], -1).astype(np.int64)
        tgt = np.stack([ts, np.asarray(inst_target[name])[valid]], -1).astype(np.int64)
        m = panoptic_quality_match(pred, tgt, things, stuff, True)
        for j in range(4):
            parts[j].append(m[2 + j])
    pq, sq, rq = panoptic_quality_compute(things, stuff, *(np.concatenate(p_) for p_ in parts))
    return float(pq), float(sq), float(rq)
