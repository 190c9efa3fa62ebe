"""Every entry point of csrc/heads_io.hip against the references of tests/heads_io_cases.py, called through _lib.call with raw pointers and
the ctypes March / VM / VMGrad structs.

A device result is held to |device - fp64| <= 8 * yardstick + 4 * 2^-24 * scale (loss_cases.bound; heads_io_cases.WIDENED would list what
needs more).  xa, zero pads, rows past the device-side row limit, bf16 roundings, products of clamped taps and gradient texels without a
contribution are compared exactly.  Output buffers start as NaN: a column that is not written shows.  Each test prints the worst
``yardstick | device error | bound`` row per quantity."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import heads_io_cases as hc
from test_gpu_march import DEV, SENTINEL, Table, _L, _d, _march_struct, _stop_after_a_device_error, _vm  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF16_NAN = 0x7FC0


@contextlib.contextmanager
def _rows(M):
    """The device-side row limit set to M around a launch sized by a capacity."""
    from contrastive_lift_amd import engine
    lim = engine.rows_limit(torch.device(DEV))
    lim[0:1].fill_(M)
    try:
        yield
    finally:
        engine.reset_rows_limit()


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _act(c, rows):
    """act_idx padded to ``rows`` entries (a valid sample id: what lies past the row limit is never used, and never out of range either)."""
    a = np.zeros(max(rows, 1), np.int32)
    if c.act is not None:
        a[:c.M] = c.act
    return _d(a, torch.int32)


def _untouched(t, buf, rows, what, case):
    if rows < buf.shape[0] and not bool(torch.isnan(buf[rows:].float()).all()):
        t.fail(case, f"{what}: rows past the row limit were written")


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- forward gather
def _gather_fwd(L, c, with_xa):
    m, (v, tabs) = _march_struct(L, c), _vm(L, c)
    rays, jit, act = _d(c.rays), _d(c.jitter), _act(c, c.cap)
    F, xa = _nan(c.cap, 3 * c.comps), (_nan(c.cap, 4) if with_xa else None)
    with _rows(c.M):
        L.call("clift_app_gather_fwd", C.byref(m), C.byref(v), L.ptr(rays), L.ptr(jit), L.ptr(act), c.cap, L.ptr(F), L.ptr(xa), L.stream())
        torch.cuda.synchronize()
    return F, xa


def _check_xa(t, c, xa, what):
    got = xa[:c.M].cpu().numpy()
    if not (np.array_equal(got[:, :3].view(np.int32), c.xn.view(np.int32)) and (got[:, 3] == 0).all()):
        t.fail(c, f"{what}: xa is not the fp32 sample position, or its pad not 0")
    _untouched(t, xa, c.M, what + " xa", c)


def test_gather_fwd_and_active_xyz(capsys):
    L, t = _L(), Table(hc)
    for c in hc.gather_cases():
        F0, _ = _gather_fwd(L, c, False)
        F1, xa = _gather_fwd(L, c, True)
        t.hold(c, "F", F0[:c.M].cpu(), "no_xa")
        t.hold(c, "F", F1[:c.M].cpu(), "xa")
        if not torch.equal(_bits(F0[:c.M]), _bits(F1[:c.M])):
            t.fail(c, "F differs in some bit with and without xa")
        _untouched(t, F0, c.M, "F", c), _untouched(t, F1, c.M, "F", c)
        _check_xa(t, c, xa, "gather_fwd")
        m, rays, jit, act = _march_struct(L, c), _d(c.rays), _d(c.jitter), _act(c, c.cap)
        xb = _nan(c.cap, 4)
        with _rows(c.M):
            L.call("clift_active_xyz", C.byref(m), L.ptr(rays), L.ptr(jit), L.ptr(act), c.cap, L.ptr(xb), L.stream())
            torch.cuda.synchronize()
        _check_xa(t, c, xb, "active_xyz")
        if not torch.equal(_bits(xa[:c.M]), _bits(xb[:c.M])):
            t.fail(c, "xa of clift_app_gather_fwd and of clift_active_xyz differ")
    t.close(capsys)


def test_vm_products_points(capsys):
    L, t = _L(), Table(hc)
    explicit = [c for c in hc.scatter_cases() if not c.ray_derived]
    for c in list(hc.points_cases()) + explicit:
        n, ldx = c.xn.shape[0], getattr(c, "ldx", 4)
        v, tabs = _vm(L, c)
        x = _nan(n, ldx)                                           # (the pad columns of a point row are poisoned)
        x[:, :3] = _d(c.xn)
        F = torch.full((n + 8, 3 * c.comps), float(SENTINEL), device=DEV)
        L.call("clift_vm_products_points", C.byref(v), L.ptr(x), ldx, n, L.ptr(F), L.stream())
        got = F[:n].cpu()
        t.hold(c, "F", got, "points")
        zero = hc.reference(c)["F"] == 0                             # a product with a clamped tap on every side: exactly 0
        if c.kernel == "points" and n >= 1000 and not bool(zero.any()):
            t.fail(c, "no product is exactly 0 in the reference")
        if not bool((got[zero] == 0).all()):
            t.fail(c, "a clamped tap contributes")
        if not bool((F[n:] == SENTINEL).all()):
            t.fail(c, "wrote past n")
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- backward gather
def _gather_bwd(L, c, with_xa, xcd):
    """The six gradient tensors after clift_app_gather_bwd on top of the pre-fill: straight into them (xcd_stride = 0), or into eight zeroed
    accumulation copies that clift_xcd_reduce folds onto the pre-fill.  A case with a capacity runs under the device row limit, the rows
    past M of dF and xa being NaN."""
    (v, tabs) = _vm(L, c)
    if c.ray_derived:
        m, rays, jit, act = _march_struct(L, c), _d(c.rays), _d(c.jitter), _act(c, c.cap)
    else:
        m, rays, jit, act = L.March(), None, None, None
    dF = _d(c.dF)
    xa = None
    if with_xa:
        xa = _nan(c.cap, 4)
        xa[:c.M, :3] = _d(c.xn)
        xa[:c.M, 3] = 0.0
    pre = list(c.prefill_plane) + list(c.prefill_line)
    offs = np.concatenate([[0], np.cumsum([p.size for p in pre])])
    n = int(offs[-1])
    dst = _d(np.concatenate([p.reshape(-1) for p in pre]))
    work = torch.zeros((8 * n,), device=DEV) if xcd else None
    g = L.VMGrad()
    base = (work if xcd else dst).data_ptr()
    for i in range(3):
        g.plane[i], g.line[i] = base + 4 * int(offs[i]), base + 4 * int(offs[3 + i])
    g.xcd_stride = n if xcd else 0
    if c.second_trip:
        L.call("clift_set_cu_reserve", hc.RESERVE)
    try:
        with (_rows(c.M) if c.cap > c.M else contextlib.nullcontext()):
            L.call("clift_app_gather_bwd", C.byref(m), C.byref(v), C.byref(g), L.ptr(rays), L.ptr(jit), L.ptr(act), c.cap, L.ptr(dF), L.ptr(xa), L.stream())
            torch.cuda.synchronize()
    finally:
        if c.second_trip:
            L.call("clift_set_cu_reserve", 0)
    if xcd:
        L.call("clift_xcd_reduce", L.ptr(work), n, n, L.ptr(dst), L.stream())
        assert float(work.abs().max()) == 0.0, (c, "the accumulation copies are not left zero")
    out = dst.cpu()
    return {q: out[int(offs[j]):int(offs[j + 1])].reshape(pre[j].shape) for j, q in enumerate(hc.GRADS)}


def test_gather_bwd_every_path(capsys):
    L, t = _L(), Table(hc)
    reached, trips = set(), set()
    for c in hc.scatter_cases():
        pre = dict(zip(hc.GRADS, list(c.prefill_plane) + list(c.prefill_line)))
        tch = hc.touched(c)
        for with_xa in ((True, False) if (c.ray_derived and not c.second_trip) else (True,)):
            branch = hc.gather_bwd_branch(c.comps, c.res, with_xa)
            if c.second_trip:
                assert c.M > hc.gather_bwd_rows_per_trip(c.comps, c.res, with_xa, 256 - hc.RESERVE)
                trips.add(branch)
            for xcd in (False, True):
                reached.add(branch + (xcd, with_xa))
                how = f"{branch[0]}{branch[1]}" + ("_xcd" if xcd else "") + ("" if with_xa else "_noxa")
                got = _gather_bwd(L, c, with_xa, xcd)
                for q in hc.GRADS:
                    t.hold(c, q, got[q], branch[0] + ("_xcd" if xcd else ""))       # (one printed row per walk, not per launch shape)
                    same = _bits(got[q]) == torch.from_numpy(pre[q]).view(torch.int32)
                    if not bool(same[~tch[q]].all()):
                        t.fail(c, f"{how} {q}: a texel without a contribution lost its pre-fill")
    want = {("wave", b, x, True) for b in (3, 2, 1, 0) for x in (False, True)} | {("lane", b, x, False) for b in (256, 512, 1024, 0) for x in (False, True)}
    assert want <= reached, want - reached
    assert {r for r in reached if r[0] == "lane" and r[3]} >= {("lane", 256, False, True), ("lane", 256, True, True)}, "the lane walk with xa (comps > 64)"
    assert trips == {("wave", 3), ("wave", 1), ("lane", 512)}, trips
    t.close(capsys)


def test_gather_bwd_refuses_other_widths():
    L = _L()
    c = hc.scatter_cases()[0]
    (v, tabs), g = _vm(L, c), L.VMGrad()
    for comps in (2, 18):
        v.comps = comps
        with pytest.raises(L.CliftError):
            L.call("clift_app_gather_bwd", C.byref(L.March()), C.byref(v), C.byref(g), None, None, None, 1, None, None, L.stream())


# ---------------------------------------------------------------------------------------------------------------- MLP input assembly
def _rne_bf16(x32):
    return x32.to(torch.bfloat16).view(torch.int16)


def _check_X(t, c, X32, Xh, rows, what):
    """The fp32 rows against the reference, pads exactly 0, rows past the limit untouched; the bf16 rows bit-equal to round-to-nearest-even of
    the fp32 rows of the same inputs."""
    M = c.M
    t.hold(c, "X", X32[:M, :c.width].cpu(), what)
    if not bool((X32[:M, c.width:] == 0).all()):
        t.fail(c, f"{what}: a pad column of X is not exactly 0")
    _untouched(t, X32, rows, what + " X", c)
    if Xh is not None:
        if not torch.equal(Xh[:M], _rne_bf16(X32[:M])):
            t.fail(c, f"{what}: the bf16 X is not the round-to-nearest-even of the fp32 X")
        if rows < Xh.shape[0] and not bool((Xh[rows:] == BF16_NAN).all()):
            t.fail(c, f"{what}: bf16 rows past the row limit were written")


def test_encode_fwd_bwd_and_points(capsys):
    L, t = _L(), Table(hc)
    for c in hc.encode_cases():
        feat, dX, M = _d(c.feat), _d(c.dX), c.M
        if c.dirs is not None:                                     # the points API: explicit view directions, ldd > 3
            dirs, X = _d(c.dirs), _nan(M + 8, c.ldx)
            L.call("clift_app_encode_points", L.ptr(feat), c.ldf, c.nf, c.pef, c.pev, L.ptr(dirs), c.dirs.shape[1], M, L.ptr(X), c.ldx, L.stream())
            _check_X(t, c, X, None, M, "points")
            continue
        rays, act = _d(c.rays), _act(c, c.cap)
        X, Xh = _nan(c.cap, c.ldx), torch.full((c.cap, c.ldx), BF16_NAN, dtype=torch.int16, device=DEV)
        with _rows(M):
            L.call("clift_app_encode_fwd", L.ptr(feat), c.ldf, c.nf, c.pef, c.pev, L.ptr(rays), L.ptr(act), c.S, c.cap, L.ptr(X), c.ldx, 0, L.stream())
            L.call("clift_app_encode_fwd", L.ptr(feat), c.ldf, c.nf, c.pef, c.pev, L.ptr(rays), L.ptr(act), c.S, c.cap, L.ptr(Xh), c.ldx, 1, L.stream())
            torch.cuda.synchronize()
        _check_X(t, c, X, Xh, M, "fwd")
        dfeat = _nan(c.cap, c.lddf)
        with _rows(M):
            L.call("clift_app_encode_bwd", L.ptr(feat), c.ldf, c.nf, c.pef, L.ptr(dX), c.ldx, c.cap, L.ptr(dfeat), c.lddf, L.stream())
            torch.cuda.synchronize()
        t.hold(c, "dfeat", dfeat[:M, :c.nf].cpu(), "bwd")
        if not bool((dfeat[:M, c.nf:] == 0).all()):
            t.fail(c, "a pad column of dfeat is not exactly 0")
        _untouched(t, dfeat, M, "dfeat", c)
    with pytest.raises(L.CliftError):
        L.call("clift_app_encode_fwd", None, 4, 4, 2, 2, None, None, 1, 1, None, 4 + 3 + 16 + 12 - 1, 0, L.stream())
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- the fused front end
def test_front_fwd(capsys):
    L, t = _L(), Table(hc)
    for c in hc.front_cases():
        M, cap, nc = c.M, c.cap, 3 * c.comps
        m, (v, tabs) = _march_struct(L, c), _vm(L, c)
        rays, jit, act, Wb = _d(c.rays), _d(c.jitter), _act(c, cap), _d(c.Wb)
        small = M <= 1000
        Fg = xg = None
        if small:                                                  # the unfused gather of the same samples: F and xa bit for bit
            Fg, xg = _nan(M, nc), _nan(M, 4)
            L.call("clift_app_gather_fwd", C.byref(m), C.byref(v), L.ptr(rays), L.ptr(jit), L.ptr(act), M, L.ptr(Fg), L.ptr(xg), L.stream())
        outs = {}
        for bf in (0, 1):
            xa = _nan(cap, 4) if c.want_xa else None
            F = _nan(cap, nc) if c.want_F else None
            feat = _nan(cap, hc.AF_NF)
            X = torch.full((cap, c.ldx), BF16_NAN, dtype=torch.int16, device=DEV) if bf else _nan(cap, c.ldx)
            args = (C.byref(m), C.byref(v), L.ptr(rays), L.ptr(jit), L.ptr(act), cap, L.ptr(Wb), c.ldb, c.nf, c.pef, c.pev, L.ptr(xa), L.ptr(feat), hc.AF_NF,
                    L.ptr(X), c.ldx, L.ptr(F))
            with _rows(M):
                if bf:
                    L.call("clift_app_front_fwd_x", *args, 1, L.stream())
                else:
                    L.call("clift_app_front_fwd", *args, L.stream())
                torch.cuda.synchronize()
            outs[bf] = (xa, F, feat, X)
            how = "bf16" if bf else "fp32"
            t.hold(c, "feat", feat[:M, :c.nf].cpu(), how)
            if not bool((feat[:M, c.nf:] == 0).all()):
                t.fail(c, f"{how}: feat columns [nf, 28) are not exactly 0")
            _untouched(t, feat, M, how + " feat", c)
            if xa is not None:
                _check_xa(t, c, xa, how)
                if small and not torch.equal(_bits(xa[:M]), _bits(xg)):
                    t.fail(c, f"{how}: xa differs from clift_app_gather_fwd's")
            if F is not None:
                t.hold(c, "F", F[:M].cpu(), how)
                _untouched(t, F, M, how + " F", c)
                if small and not torch.equal(_bits(F[:M]), _bits(Fg)):
                    t.fail(c, f"{how}: F differs from clift_app_gather_fwd's")
        if not torch.equal(_bits(outs[0][2][:M]), _bits(outs[1][2][:M])):
            t.fail(c, "feat differs between the fp32 and the bf16 store of X")
        _check_X(t, c, outs[0][3], outs[1][3], M, "front")
        if not bool(torch.isnan(Wb[c.nf:]).all() and torch.isnan(Wb[:, nc:]).all()):
            t.fail(c, "the poisoned part of Wb changed")
    c = hc.front_cases()[0]
    m, (v, tabs) = _march_struct(L, c), _vm(L, c)
    v.comps = 64
    with pytest.raises(L.CliftError):
        L.call("clift_app_front_fwd", C.byref(m), C.byref(v), None, None, None, 1, None, 196, 1, 1, 1, None, None, hc.AF_NF, None, 12, None, L.stream())
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- compositing
def _heads(c):
    """(rgb_s, sem_s, inst_s) on the device; NULL for a head without channels, and for every head of a chunk without an active sample."""
    if c.M == 0:
        return None, None, None
    return _d(c.rgb_s), (_d(c.sem_s) if c.C else None), (_d(c.inst_s) if c.D else None)


FWD_OUT = ("rgb_raw", "rgb_map", "sem_raw", "sem_map", "inst_map")
FWD_NULLS = ((), ("rgb_raw", "rgb_map"), ("sem_map",), ("inst_map",), ("sem_raw", "sem_map"), ("rgb_map",))


def test_composite_fwd(capsys):
    L, t = _L(), Table(hc)
    nulled = set()
    for k, c in enumerate(hc.composite_cases()):
        w, start, act, ray_out = _d(c.w), _d(c.start, torch.int32), _act(c, c.M), _d(c.ray_out)
        rgb_s, sem_s, inst_s = _heads(c)
        for nulls in ((), FWD_NULLS[k % len(FWD_NULLS)]):
            nulled |= set(nulls)
            width = dict(rgb_raw=3, rgb_map=3, sem_raw=c.C, sem_map=c.C, inst_map=c.D)
            head = dict(rgb_raw=rgb_s, rgb_map=rgb_s, sem_raw=sem_s, sem_map=sem_s, inst_map=inst_s)
            # (a sum whose head is NULL is not written: it is the caller's zeros, finished all the same)
            out = {q: None if q in nulls else (_nan(c.N, width[q]) if head[q] is not None else torch.zeros((c.N, width[q]), device=DEV)) for q in FWD_OUT}
            L.call("clift_composite_fwd", L.ptr(w), L.ptr(start), L.ptr(act), c.N, c.C, c.D, L.ptr(rgb_s), L.ptr(sem_s), L.ptr(inst_s), L.ptr(ray_out),
                   c.softmax_mode, c.white_bg, *[L.ptr(out[q]) for q in FWD_OUT], L.stream())
            finished = {"rgb_raw": "rgb_map" not in nulls, "rgb_map": "rgb_raw" not in nulls, "sem_map": "sem_raw" not in nulls}
            for q in FWD_OUT:
                if out[q] is None or not finished.get(q, True):
                    continue
                t.hold(c, q, out[q].cpu(), "all" if not nulls else "some_null")
            if not nulls:
                none = torch.from_numpy(np.diff(c.start) == 0)
                want = (1.0 - ray_out[:, 0].cpu()) if c.white_bg else torch.zeros(c.N)
                if not torch.equal(out["rgb_raw"].cpu()[none], want[none][:, None].expand(-1, 3)):
                    t.fail(c, "rgb_raw of a ray without samples is not exactly the background")
    assert nulled == set(FWD_OUT)
    t.close(capsys)


BWD_OUT = ("d_rgb", "d_sem", "d_inst", "g_w", "g_opacity")


def _bwd_common(c, limited):
    rows = c.cap if limited else c.M
    w, act = _d(c.w), _act(c, rows)
    rgb_s, sem_s, inst_s = _heads(c)
    pad = (lambda x: None if x is None else torch.cat([x, _nan(rows - c.M, x.shape[1])])) if limited else (lambda x: x)
    g = [None if x is None else _d(x) for x in (c.g_rgb, c.g_sem if c.C else None, c.g_inst if c.D else None)]
    ge = _nan(c.N * (3 + c.C + c.D) + 1)
    return rows, w, act, pad(rgb_s), pad(sem_s), pad(inst_s), _d(c.rgb_raw_in), (_d(c.sem_raw_in) if c.C else None), g, ge


def _check_g_w(t, c, g_w, how):
    got = g_w.cpu().reshape(-1)
    t.hold(c, "g_w", got[torch.from_numpy(c.act.astype(np.int64))], how)
    rest = torch.ones(got.numel(), dtype=torch.bool)
    rest[torch.from_numpy(c.act.astype(np.int64))] = False
    if not bool((got[rest] == 0).all()):
        t.fail(c, f"{how}: g_w written off the active samples")


def test_composite_bwd(capsys):
    L, t = _L(), Table(hc)
    nulled = set()
    for k, c in enumerate(hc.composite_cases()):
        limited = k % 2 == 1 and c.M > 0
        rows, w, act, rgb_s, sem_s, inst_s, raw, sraw, g, ge = _bwd_common(c, limited)
        null = (None,) + BWD_OUT
        null = null[k % len(null)]
        nulled.add(null)
        out = dict(d_rgb=_nan(rows, 3), d_sem=_nan(rows, c.C), d_inst=_nan(rows, c.D), g_w=torch.zeros((c.N, c.S), device=DEV), g_opacity=_nan(c.N))
        if null:
            out[null] = None
        with (_rows(c.M) if limited else contextlib.nullcontext()):
            L.call("clift_composite_bwd", L.ptr(w), None, L.ptr(act), c.N, c.S, rows if c.M else 0, c.C, c.D, L.ptr(rgb_s), L.ptr(sem_s), L.ptr(inst_s), L.ptr(raw),
                   L.ptr(sraw), c.softmax_mode, c.white_bg, c.stop_grad, L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(ge), L.ptr(out["d_rgb"]),
                   L.ptr(out["d_sem"]), L.ptr(out["d_inst"]), L.ptr(out["g_w"]), L.ptr(out["g_opacity"]), L.stream())
            torch.cuda.synchronize()
        how = "limit" if limited else "plain"
        if out["g_opacity"] is not None:
            t.hold(c, "g_opacity", out["g_opacity"].cpu(), how)
        if c.M == 0:
            continue
        for q, head in (("d_rgb", rgb_s), ("d_sem", sem_s), ("d_inst", inst_s)):
            if out[q] is not None and head is not None:
                t.hold(c, q, out[q][:c.M].cpu(), how)
                _untouched(t, out[q], c.M, q, c)
        if out["g_w"] is not None:
            _check_g_w(t, c, out["g_w"], how)
    assert nulled == set((None,) + BWD_OUT)
    t.close(capsys)


def test_composite_bwd_act_both_forms(capsys):
    """The form with the heads' output activations folded in: every column of [0, ld) of a row below M comes back written, the pads and the
    columns of an instance half that D does not fill (D < E, E < D < 2 E) exactly 0, rows past the row limit untouched."""
    L, t = _L(), Table(hc)
    forms, nulled = set(), set()
    for k, c in enumerate(hc.composite_cases()):
        limited = k % 2 == 0 and c.M > 0
        rows, w, act, rgb_s, sem_s, inst_s, raw, sraw, g, ge = _bwd_common(c, limited)
        null = (None, None) + hc.DPRE + ("g_w", "g_opacity")
        null = null[(k + 3) % len(null)]                          # (the cases with E < D < 2 E and D < E keep both instance buffers)
        nulled.add(null)
        ld = dict(dpre_rgb=c.ld_rgb, dpre_sem=c.ld_sem, dpre_i0=c.ld_inst, dpre_i1=c.ld_inst)
        width = dict(dpre_rgb=3, dpre_sem=c.C, dpre_i0=c.E, dpre_i1=c.E)
        out = {q: _nan(rows, ld[q]) for q in hc.DPRE}
        out.update(g_w=torch.zeros((c.N, c.S), device=DEV), g_opacity=_nan(c.N))
        if null:
            out[null] = None
        form = hc.composite_form(c.C, c.D, c.ld_sem)
        with (_rows(c.M) if limited else contextlib.nullcontext()):
            L.call("clift_composite_bwd_act", L.ptr(w), L.ptr(act), c.N, c.S, rows if c.M else 0, c.C, c.D, L.ptr(rgb_s), L.ptr(sem_s), L.ptr(inst_s), L.ptr(raw),
                   L.ptr(sraw), c.softmax_mode, c.white_bg, c.stop_grad, L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(ge), c.sem_kind, L.ptr(out["dpre_rgb"]),
                   c.ld_rgb, L.ptr(out["dpre_sem"]), c.ld_sem, L.ptr(out["dpre_i0"]), L.ptr(out["dpre_i1"]), c.ld_inst, c.E, L.ptr(out["g_w"]),
                   L.ptr(out["g_opacity"]), L.stream())
            torch.cuda.synchronize()
        how = form + ("_limit" if limited else "")
        if out["g_opacity"] is not None:
            t.hold(c, "g_opacity", out["g_opacity"].cpu(), how)
        if c.M == 0:
            continue
        forms.add((form, "E<D<2E" if c.E < c.D < 2 * c.E else "D<E" if c.D < c.E else "D=E" if c.D == c.E else "D=2E"))
        head = dict(dpre_rgb=rgb_s, dpre_sem=sem_s, dpre_i0=inst_s, dpre_i1=inst_s)
        for q in hc.DPRE:
            if out[q] is None or head[q] is None:
                continue
            got = out[q][:c.M].cpu()
            t.hold(c, q, got[:, :width[q]], how)
            if bool(torch.isnan(got).any()):
                t.fail(c, f"{how} {q}: a column of [0, ld) was not written")
            if not bool((got[:, width[q]:] == 0).all()):
                t.fail(c, f"{how} {q}: a pad column is not exactly 0")
            dead = hc.reference(c)[q] == 0                        # (the columns of a half that D does not fill: exactly 0 on the device too)
            if q in ("dpre_i0", "dpre_i1") and not bool((got[:, :width[q]][:, dead.all(0)] == 0).all()):
                t.fail(c, f"{how} {q}: an instance column that D does not reach is not exactly 0")
            _untouched(t, out[q], c.M, q, c)
        if out["g_w"] is not None:
            _check_g_w(t, c, out["g_w"], how)
    assert forms >= {(f, d) for f in ("lanes16", "scalar") for d in ("E<D<2E", "D<E", "D=2E")} | {("lanes16", "D=E")}, forms
    assert nulled == set((None,) + hc.DPRE + ("g_w", "g_opacity"))
    with pytest.raises(L.CliftError):                                # D > 2 E has no place to go
        L.call("clift_composite_bwd_act", None, None, 1, 1, 1, 0, 7, None, None, None, None, None, 0, 0, 0, None, None, None, None, 0, None, 4, None, 4,
               L.ptr(_nan(1, 4)), None, 4, 3, None, None, L.stream())
    t.close(capsys)
