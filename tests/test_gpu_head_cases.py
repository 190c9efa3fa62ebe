"""The MLP-head entry points that do not go through clift_gemm against the fp64 references of tests/head_cases.py, launched through _lib.call
with raw pointers.  Per case: the result is held element by element to head_cases.check; whatever the entry point must not write -- output
pad columns, the two rows past the output -- keeps the bits of its pre-fill; a second launch gives the same bits wherever the entry point does
not end in atomics.  Operand rows past the row count and operand pad columns are NaN, so a kernel that reads what it should not returns a NaN.
Each test prints ``yardstick | device error / S | bound factor | worst error / bound`` per case."""
import contextlib

import numpy as np
import pytest
import torch

import head_cases as hc
from test_gpu_gemm_cases import _limit
from test_gpu_march import DEV, _L, _stop_after_a_device_error  # noqa: F401

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
CALLED = set()


@contextlib.contextmanager
def _reserve(L, c):
    if c.reserve:
        L.call("clift_set_cu_reserve", c.reserve)
    try:
        yield
    finally:
        if c.reserve:
            L.call("clift_set_cu_reserve", 0)


class Launch:
    """The device buffers of a case (inputs once, outputs fresh from their pre-fill per run) and its launches."""

    def __init__(self, L, c, d=None):
        self.L, self.c, self.d = L, c, (hc.inputs(c) if d is None else d)
        self.outs = tuple(hc.reference(c))
        self.dev = {k: self._up(k, v) for k, v in self.d.items() if not k.startswith("_") and v is not None and k not in self.outs}

    def _up(self, name, a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return (t.to(BF16) if hc.stored_bf16(self.c, name) else t).to(DEV).contiguous()

    def run(self, M=None, row0=0, outs=None, extra=None):
        """One launch; returns {output buffer: image as float64}.  ``M`` / ``row0``: a launch of M rows of its own from sample row row0 (forwards);
        ``outs``: device tensors to write into instead of fresh copies of the pre-fill."""
        c, L = self.c, self.L
        o = {k: (outs[k] if outs and k in outs else self._up(k, self.d[k])) for k in self.outs}
        a = dict(self.dev, **o)
        if extra:
            a.update(extra)

        def p(name, row=0, ld=0):
            t = a.get(name)
            return None if t is None else t.data_ptr() + t.element_size() * row * ld

        M = c.M if M is None else M
        s = L.stream()
        e = c.entry
        if e == "clift_linear_k3_fwd":
            L.call(e, p("x4", row0, 4), p("W"), 4, p("b"), M, c.Nout, c.relu, p("out", row0, c.ldo), c.ldo, c.out_bf16, s)
        elif e == "clift_linear_k3_bwd":
            L.call(e, p("x4"), p("dH"), c.ldh, M, c.Nout, p("dW"), 4, p("db"), c.dh_bf16, s)
        elif e == "clift_wgrad_narrow":
            L.call(e, p("dY"), c.ldd, c.no, p("X"), c.ldx, c.ni, M, p("gW"), c.ldw, p("gb"), c.x_bf16, s)
        elif e == "clift_colsum":
            L.call(e, p("dY"), c.ld, M, c.N, p("db"), s)
        elif e == "clift_rows_act_fwd":
            L.call(e, p("pre", row0, c.ldp), c.ldp, M, c.C, c.kind, p("out", row0, c.ldo), c.ldo, s)
        elif e == "clift_rows_act_bwd":
            L.call(e, p("out"), c.ldo, p("dout"), c.lddo, M, c.C, c.kind, p("dpre"), c.ldd, s)
        elif e == "clift_out_layer_fwd":
            L.call(e, p("H", row0, c.ldh), c.ldh, p("W"), c.ldw, p("b"), c.no, M, p("out", row0, c.ldo), c.ldo, c.act, s)
        elif e == "clift_out_layer_bwd":
            L.call(e, p("dOut"), c.ldd, c.no, p("W"), c.nh + 4, p("H"), c.ldh, M, p("dX"), c.ldx, p("gW"), c.nh + 4, p("gb"), s)
        elif e == "clift_out_layer_bwd_nh":
            L.call(e, p("dOut"), c.ldd, c.no, p("W"), c.nh + 4, p("H"), c.ldh, c.nh, M, p("dX"), c.ldx, p("gW"), c.nh + 4, p("gb"), c.h_bf16, s)
        elif e == "clift_out_layer_bwd_n128_bf16":
            L.call(e, p("dOut"), c.ldd, c.no, p("W"), c.nh + 4, p("H"), c.ldh, M, p("dX"), c.ldx, p("gW"), c.nh + 4, p("gb"), s)
        elif e == "clift_xyz_head_first2_fwd":
            L.call(e, p("x4", row0, 4), p("W0"), 4, p("b0"), p("W1"), 260, p("b1"), M, p("h1", row0, c.ldh1), c.ldh1, p("h2", row0, c.ldh2), c.ldh2, s)
        elif e == "clift_xyz_head_last2_fwd":
            L.call(e, p("A", row0, c.lda), c.lda, p("W"), 260, p("b"), p("Wout"), 260, p("bout"), c.E, M, p("hidden", row0, c.ldh), c.ldh,
                   p("out", row0, c.ldo), c.ldo, s)
        elif e == "clift_app_head_last2_fwd":
            L.call(e, p("A", row0, c.lda), c.lda, p("W"), 132, p("b"), p("Wout"), 132, p("bout"), c.E, M, p("hidden", row0, c.ldh), c.ldh,
                   p("pre", row0, c.ldo + 1), c.ldo + 1, p("out", row0, c.ldo), c.ldo, c.sigmoid, s)
        elif e == "clift_xyz_head_first2_x6_fwd":
            self.signs = torch.zeros((int(L.load().clift_sign_bits_bytes(M)),), dtype=torch.uint8, device=DEV) if c.signs else None
            L.call(e, p("x4", row0, 4), p("W0"), 4, p("b0"), p("W1"), 260, p("b1"), M, p("h2", row0, c.ldh2), c.ldh2,
                   self.signs.data_ptr() if c.signs else None, s)
        elif e == "clift_xyz_head_last2_x6_fwd":
            ws = torch.empty((int(L.load().clift_xyz_head_last2_x6_workspace_bytes(M)),), dtype=torch.uint8, device=DEV)
            L.call(e, p("A", row0, c.lda), c.lda, p("W"), 260, p("b"), p("Wout"), 260, p("bout"), c.E, M, p("hidden", row0, c.ldh), c.ldh,
                   p("out", row0, c.ldo), c.ldo, ws.data_ptr(), ws.numel(), s)
        elif e == "clift_app_head_last2_x6_fwd":
            L.call(e, p("A", row0, c.lda), c.lda, p("W"), 132, p("b"), p("Wout"), 132, p("bout"), c.E, M, p("hidden", row0, c.ldh), c.ldh,
                   p("out", row0, c.ldo), c.ldo, c.sigmoid, s)
        elif e == "clift_app_head_last2_bf16_fwd":
            L.call(e, p("A", row0, c.lda), c.lda, p("W"), 132, p("b"), p("Wout"), 132, p("bout"), c.E, M, p("hidden", row0, c.ldh), c.ldh,
                   p("out", row0, c.ldo), c.ldo, c.sigmoid, s)
        elif e == "clift_xyz_head_first2_bf16_bwd":
            L.call(e, p("dH2"), c.ldd, p("W1"), 260, p("h1"), c.ldm, p("x4"), M, p("gW0"), 4, p("gb0"), s)
        elif e == "clift_xyz_head_bf16_fwd":
            L.call(e, p("x4", row0, 4), p("W0"), 4, p("b0"), p("W1"), 260, p("b1"), p("W2"), 260, p("b2"), p("Wout"), 260, p("bout"), c.E, M,
                   p("h1", row0, 256), p("h2", row0, 256), p("h3", row0, 256), p("out", row0, c.ldo), c.ldo, s)
        elif e in ("clift_xyz_head_first2_bwd", "clift_xyz_head_first2_x6_bwd"):
            L.call(e, p("dH2"), c.ldd, p("W1"), 260, p("W0"), 4, p("b0"), p("x4"), M, p("gW0"), 4, p("gb0"), s)
        elif e in ("clift_xyz_head_first2_wgrad", "clift_xyz_head_first2_x6_wgrad"):
            L.call(e, p("dH2"), c.ldd, p("W0"), 4, p("b0"), p("x4"), M, p("gW1"), c.ldg, p("gb1"), s)
        else:
            raise AssertionError(e)
        CALLED.add(e)
        torch.cuda.synchronize()
        return {k: t.float().cpu().numpy().astype(np.float64) for k, t in o.items()}


def _bits_equal(a, b):
    return all(np.array_equal(a[q].view(np.int64), b[q].view(np.int64)) for q in a)


def _stored_chain(la, got, broken):
    """The intermediates a chain of bf16 roundings actually stored.  The two forwards: the case's own hidden activations, or -- where the case
    passes NULL -- those of a launch that stores them all, whose other outputs must then have the bits of the case's launch.
    clift_xyz_head_first2_bf16_bwd: the bf16 dH1 that clift_gemm's masked dgrad stores for the same operands."""
    import ctypes as C
    c, L = la.c, la.L
    if c.entry == "clift_app_head_last2_bf16_fwd":
        if "hidden" in got:
            return got["hidden"][:c.M, :128]
        hidden = torch.full((c.M + 2, c.ldh), hc.SENTINEL, dtype=BF16, device=DEV)
        if not _bits_equal(got, la.run(extra={"hidden": hidden})):
            broken.append(f"{c}: the launch without `hidden` gave other bits than the launch with it")
        return hidden.float().cpu().numpy().astype(np.float64)[:c.M, :128]
    if c.entry == "clift_xyz_head_bf16_fwd":
        hs = {q: torch.full((c.M + 2, 256), hc.SENTINEL, dtype=BF16, device=DEV) for q in ("h1", "h2", "h3")}
        full = la.run(extra=hs)
        imgs = {q: t.float().cpu().numpy().astype(np.float64) for q, t in hs.items()}
        full.update(imgs)
        if not _bits_equal(got, full):
            broken.append(f"{c}: other bits than the launch that stores h1, h2 and h3")
        if not all(np.all(v[c.M:] == hc.SENTINEL) for v in imgs.values()):
            broken.append(f"{c}: an activation was written past its M rows")
        return {q: v[:c.M] for q, v in imgs.items()}
    dH1 = torch.full((c.M + 2, 256), hc.SENTINEL, dtype=BF16, device=DEV)
    g = L.Gemm()
    g.M, g.N, g.K, g.precision, g.split_k = c.M, 256, 256, 1, 1
    g.A, g.lda, g.B, g.ldb, g.b_trans, g.C, g.ldc = la.dev["dH2"].data_ptr(), c.ldd, la.dev["W1"].data_ptr(), 260, 1, dH1.data_ptr(), 256
    g.mask, g.ldmask = la.dev["h1"].data_ptr(), c.ldm
    g.a_bf16, g.c_bf16, g.mask_bf16 = 1, 1, 1
    L.call("clift_gemm", C.byref(g), L.stream())
    torch.cuda.synchronize()
    return dH1.float().cpu().numpy().astype(np.float64)[:c.M]


_ENTRIES = sorted(hc.ENTRIES)
HEAD = "\nentry point             case                                                   | yardstick | dev err/S | bound     | err/bound\n"


@pytest.mark.parametrize("entry", _ENTRIES)
def test_entry_point_against_fp64(entry, capsys):
    L, info, lines, broken = _L(), hc.ENTRIES[entry], [], []
    for c in (c for c in hc.groups()[entry] if not c.p.get("probe")):        # (the refill case has a test of its own)
        with _reserve(L, c):
            la = Launch(L, c)
            got = la.run()
            if entry in hc.CHAINED:
                got["_chain"] = _stored_chain(la, got, broken)
            ok, worst, rel, text = hc.check(got, c)
            got.pop("_chain", None)
            y = max(hc.yardsticks(c).values())
            lines.append(f"{entry[6:]:23s} {c.name:54s} | {y:9.3e} | {rel:9.3e} | {max(hc.factor_for(c, q) for q in got):9.3e} | {worst:6.3f}")
            if not ok:
                broken.append(text)
            if info.fwd:                  # the outputs written with plain stores: the same bits at every launch
                again = la.run()
                if not all(np.array_equal(got[q].view(np.int64), again[q].view(np.int64)) for q in info.fwd if q in got):
                    broken.append(f"{c}: a second launch gave other bits")
    with capsys.disabled():
        print(HEAD + "\n".join(lines))
    assert not broken, "\n".join(broken)


_PERSISTENT_FWD = ("clift_out_layer_fwd", "clift_xyz_head_first2_fwd", "clift_xyz_head_last2_fwd", "clift_app_head_last2_fwd",
                   "clift_xyz_head_first2_x6_fwd", "clift_xyz_head_last2_x6_fwd", "clift_app_head_last2_x6_fwd", "clift_app_head_last2_bf16_fwd",
                   "clift_xyz_head_bf16_fwd")


@pytest.mark.parametrize("entry", _PERSISTENT_FWD)
def test_a_rows_bits_do_not_depend_on_its_launch(entry):
    """The persistent forwards: rows 0, T - 1, T and M - 1 of the M3 launch against the same rows computed in launches of their own."""
    L, T = _L(), hc.ENTRIES[entry].T
    for c in (c for c in hc.groups()[entry] if c.reserve and not c.p.get("probe")):
        with _reserve(L, c):
            la = Launch(L, c)
            whole = la.run()
        for first, n in ((0, 1), (T - 1, 1), (T, 1), (c.M - 1, 1), (T - 1, 2)):
            part = la.run(M=n, row0=first)
            for q, img in part.items():
                pre = hc.inputs(c)[q].astype(np.float64)
                assert np.array_equal(img[first:first + n].view(np.int64), whole[q][first:first + n].view(np.int64)), (c, q, first, n)
                img[first:first + n] = pre[first:first + n]
                assert np.array_equal(img, pre), (c, q, first, n, "rows outside the launch were written")


def test_head_bf16_fwd_past_the_refill_of_its_staged_positions(capsys):
    """128 * 2048 + 64 + 1 rows under a reserve of 128 CUs: every full block walks 2048 staged positions and refills once.  E = 3, no activation
    stored; a second launch that stores h1 / h2 / h3 must give the same `out` bits on every row, and on the probe rows (first and last row of
    each block's first and second stage, the ragged end) `out` is held to the fp64 output layer over the stored h3, h3 over the stored h2, h2
    over the stored h1, h1 to its own reference."""
    L = _L()
    c = next(c for c in hc.groups()["clift_xyz_head_bf16_fwd"] if c.p.get("probe"))
    d = hc.inputs(c)
    rows = d["_rows"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    dev = {k: up(d[k]) for k in ("x4", "W0", "b0", "W1", "b1", "W2", "b2", "Wout", "bout")}
    fresh = lambda: torch.full((c.M + 2, c.ldo), hc.SENTINEL, dtype=F32, device=DEV)
    hs = {q: torch.full((c.M + 2, 256), hc.SENTINEL, dtype=BF16, device=DEV) for q in ("h1", "h2", "h3")}

    def launch(out, h):
        ptr = lambda q: h[q].data_ptr() if h else None
        L.call("clift_xyz_head_bf16_fwd", dev["x4"].data_ptr(), dev["W0"].data_ptr(), 4, dev["b0"].data_ptr(), dev["W1"].data_ptr(), 260, dev["b1"].data_ptr(),
               dev["W2"].data_ptr(), 260, dev["b2"].data_ptr(), dev["Wout"].data_ptr(), 260, dev["bout"].data_ptr(), c.E, c.M,
               ptr("h1"), ptr("h2"), ptr("h3"), out.data_ptr(), c.ldo, L.stream())
        CALLED.add("clift_xyz_head_bf16_fwd")
        torch.cuda.synchronize()

    with _reserve(L, c):
        a, b, again = fresh(), fresh(), fresh()
        launch(a, None)
        launch(again, None)
        launch(b, hs)
    assert torch.equal(a, again), "a second launch gave other bits"
    assert torch.equal(a, b), "the launch that stores the activations gave other `out` bits"
    assert bool((a[c.M:] == hc.SENTINEL).all()) and bool((a[:c.M, c.E:] == hc.SENTINEL).all()) and all(bool((t[c.M:] == hc.SENTINEL).all()) for t in hs.values())
    idx = torch.from_numpy(np.concatenate([rows, [c.M, c.M + 1]])).to(DEV)
    got = {"out": a[idx].cpu().numpy().astype(np.float64), "_chain": {q: t[idx[:-2]].float().cpu().numpy().astype(np.float64) for q, t in hs.items()}}
    ok, worst, rel, text = hc.check(got, c)
    with capsys.disabled():
        print(HEAD + f"{c.entry[6:]:23s} {c.name:54s} | {max(hc.yardsticks(c).values()):9.3e} | {rel:9.3e} | {hc.factor_for(c, 'out'):9.3e} | {worst:6.3f}")
    assert ok, text


def test_h_plus_inf_is_on_in_the_out_layer_backwards():
    """H = +inf is ON (include/clift.h: an entry is on iff > 0).  H is also an operand of gW there, where +inf gives inf - inf, so the tables
    leave it out; here it is put into H and only dX is looked at."""
    L = _L()
    for entry in hc._OB:
        c = next(c for c in hc.groups()[entry] if c.M == 2 * hc.ENTRIES[entry].T + 1 and c.gb)
        d = dict(hc.inputs(c))
        d["H"] = d["H"].copy()
        at = (np.arange(0, c.M, 3), (7 * np.arange(0, c.M, 3)) % c.nh)
        d["H"][at] = np.inf
        got = Launch(L, c, d).run()
        ref = hc.ENTRIES[entry].ref(c, d)
        assert np.all(ref["dX"][0][at] != 0)
        ok, worst, rel, text = hc.check(got, c, ref={"dX": ref["dX"]})
        assert ok, text


def test_first2_fwd_gives_the_bits_of_the_unfused_pair():
    """include/clift.h: "bit-identical to clift_linear_k3_fwd followed by clift_gemm", and the h1 it writes is clift_linear_k3_fwd's."""
    import ctypes as C
    L = _L()
    for c in (c for c in hc.groups()["clift_xyz_head_first2_fwd"] if c.h1 and (c.reserve or c.M == 2 * hc.LF_ROWS + 1)):
        with _reserve(L, c):
            la = Launch(L, c)
            fused = la.run()
            h1 = torch.full((c.M + 2, c.ldh1), hc.SENTINEL, dtype=F32, device=DEV)
            h2 = torch.full((c.M + 2, c.ldh2), hc.SENTINEL, dtype=F32, device=DEV)
            dv = la.dev
            L.call("clift_linear_k3_fwd", dv["x4"].data_ptr(), dv["W0"].data_ptr(), 4, dv["b0"].data_ptr(), c.M, 256, 1, h1.data_ptr(), c.ldh1, 0, L.stream())
            g = L.Gemm()
            g.M, g.N, g.K = c.M, 256, 256
            g.A, g.lda, g.B, g.ldb, g.C, g.ldc = h1.data_ptr(), c.ldh1, dv["W1"].data_ptr(), 260, h2.data_ptr(), c.ldh2
            g.bias, g.act, g.split_k = dv["b1"].data_ptr(), 1, 1
            L.call("clift_gemm", C.byref(g), L.stream())
            torch.cuda.synchronize()
        for q, t in (("h1", h1), ("h2", h2)):
            assert np.array_equal(fused[q].view(np.int64), t.cpu().numpy().astype(np.float64).view(np.int64)), (c, q)


def test_sign_bytes_of_first2_x6_fwd_drive_the_next_dgrad(capsys):
    """The record's layout is private, so it is fed to what reads it: a LAYER_X6 masked dgrad with mask = NULL, held to the fp64 dgrad whose mask
    is ``reference pre-activation > 0``.  Elements whose reference pre-activation lies within its own bound of zero may take either sign and are
    left out: at most 0.1 % of a case."""
    import ctypes as C
    import gemm_cases as gc
    L, lines = _L(), []
    for c in (c for c in hc.groups()["clift_xyz_head_first2_x6_fwd"] if c.signs and c.M > hc.X6_ROWS):
        rng = np.random.default_rng(c.seed)
        dY = (gc._nonzero(rng, (c.M, 256)) * np.exp2(rng.integers(-6, 7, (c.M, 1)))).astype(np.float32)
        Wd = (gc._nonzero(rng, (256, 256)) / 16).astype(np.float32)               # [k][n]: b_trans
        pre, Sp = hc.f2_pre(c)
        unsure = hc.sign_unsure(c)                # (the host test holds their number to the 0.1 % cap)
        v, S = dY.astype(np.float64) @ Wd.astype(np.float64), np.abs(dY.astype(np.float64)) @ np.abs(Wd.astype(np.float64))
        rows = np.arange(min(c.M, 8))
        yard = max(float(np.max(np.abs(hc._layer32(dY[rows], Wd.T, np.zeros(256, np.float32), o, split=True) - v[rows]) / S[rows])) for o in hc.ORDERS)
        with _reserve(L, c):
            la = Launch(L, c)
            la.run()
            A, B = torch.from_numpy(dY).to(DEV), torch.from_numpy(Wd).to(DEV)
            out = torch.full((c.M + 2, 256), hc.SENTINEL, dtype=F32, device=DEV)
            g = L.Gemm()
            g.M, g.N, g.K, g.precision, g.split_k = c.M, 256, 256, 2, 1
            g.A, g.lda, g.B, g.ldb, g.b_trans, g.C, g.ldc = A.data_ptr(), 256, B.data_ptr(), 256, 1, out.data_ptr(), 256
            g.sign_bits = la.signs.data_ptr()
            r = L.load().clift_gemm_route(C.byref(g))
            assert L.load().clift_gemm_route_name(r).decode() == "LAYER_X6"
            L.call("clift_gemm", C.byref(g), L.stream())
            torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        assert np.all(got[c.M:] == hc.SENTINEL)
        err = np.abs(got[:c.M] - np.where(pre > 0, v, 0.0))
        bad = (err > gc.bound_factor(yard) * S) & ~unsure
        lines.append(f"first2_x6_fwd signs     {c.name:54s} | {yard:9.3e} | {float((err / S)[~unsure].max()):9.3e} | {gc.bound_factor(yard):9.3e} | left out {int(unsure.sum())}")
        assert not bad.any(), (c, np.argwhere(bad)[:4])
    with capsys.disabled():
        print(HEAD + "\n".join(lines))


_UNCLAMPED = [e for e in sorted(hc.ENTRIES) if not hc.ENTRIES[e].limit]


@pytest.mark.parametrize("entry", _UNCLAMPED)
def test_bf16_mode_kernels_do_not_clamp_to_the_row_limit(entry):
    """include/clift.h names the entry points that do NOT honour the device row limit (no kernel of layer_bf16.hip, layer_nb16.hip, head_bf16.hip
    calls limit_rows).  With a limit L = M - T - 1 on the device and every row valid: a forward writes all M rows with the bits of the unlimited
    launch, a reduction sums all M rows."""
    L, info = _L(), hc.ENTRIES[entry]
    c = next(c for c in hc.groups()[entry] if c.M == 2 * info.T + 1 and c.p.get("gb", 1))
    la, broken = Launch(L, c), []
    free = la.run()
    with _limit(c.M - info.T - 1):
        got = la.run()
    assert all(np.array_equal(got[q].view(np.int64), free[q].view(np.int64)) for q in info.fwd if q in got), (c, "the limit changed a forward's rows")
    sums = [q for q in got if q not in info.fwd]
    if sums:
        ref = hc.ENTRIES[entry].ref(c, hc.inputs(c), chain=_stored_chain(la, got, broken)) if entry in hc.CHAINED else hc.reference(c)
        ok, worst, rel, text = hc.check(got, c, ref={q: ref[q] for q in sums})
        assert ok and not broken, text


def _limit_cases():
    """Per entry point that honours the device row limit (Entry.limit, read from the kernels: every one of the table but the bf16-mode
    clift_out_layer_bwd_n128_bf16) its largest case without a reserve, and -- the persistent kernels -- the M3 case, whose second limit T + 1
    leaves the trailing blocks of the capacity-sized grid without a row."""
    out = []
    for entry, mine in hc.groups().items():
        if not hc.ENTRIES[entry].limit:
            continue
        plain = [c for c in mine if not c.reserve and c.M < 100000 and c.M > hc.tile(c) + 2]
        forms = {}
        for c in plain:               # one per kernel the entry point launches
            key = (hc.tile(c), c.p.get("dh_bf16"), c.p.get("x_bf16"), c.p.get("kind"), c.p.get("act"), c.p.get("h_bf16"), c.p.get("nh"))
            if key not in forms or c.M >= forms[key].M:
                forms[key] = c
        out += [(c, c.M - hc.tile(c) - 1) for c in forms.values()]
        out += [(c, hc.tile(c) + 1) for c in mine if c.reserve]
    return out


_LIMITED = _limit_cases()


@pytest.mark.parametrize("c,lim", _LIMITED, ids=[f"{c.entry[6:]}-{c.name}-L{lim}" for c, lim in _LIMITED])
def test_entry_point_under_a_device_side_row_limit(c, lim):
    """A sync-free pass sizes a launch by a capacity and leaves the true row count L on the device.  With NaN in every sample row at and past L:
    a reduction equals the reference of the first L rows; a forward gives rows < L the bits of the unlimited launch and writes nothing outside
    its M rows (nothing is asserted of its rows in [L, M))."""
    L, info = _L(), hc.ENTRIES[c.entry]
    d = dict(hc.inputs(c))
    with _reserve(L, c):
        free = Launch(L, c).run() if info.fwd else None
        for name in info.streamed:
            d[name] = d[name].copy()
            d[name][lim:] = np.nan
        la = Launch(L, c, d)
        with _limit(lim):
            got = la.run()
    pre = hc.inputs(c)
    for q in (q for q in info.fwd if q in got):
        g = got[q]
        assert np.array_equal(g[:lim].view(np.int64), free[q][:lim].view(np.int64)), (c, q, "rows below the limit differ from the unlimited launch")
        assert np.array_equal(g[c.M:], pre[q][c.M:].astype(np.float64)), (c, q, "rows past the launch were written")
    sums = {q: v for q, v in hc.reference_of(c, lim).items() if q not in info.fwd}
    if sums:
        ok, worst, rel, text = hc.check(got, c, ref=sums)
        assert ok, text


# ---------------------------------------------------------------------------------------------------------------- gradient shards
def _shard_cases():
    g = hc.groups()
    wn = next(c for c in g["clift_wgrad_narrow"] if c.M == 4097 and not c.x_bf16)
    k3 = next(c for c in g["clift_linear_k3_bwd"] if c.M == 4097 and c.db and not c.dh_bf16)
    plain = next(c for c in g["clift_linear_k3_bwd"] if c.M == 513)
    ob = next(c for c in g["clift_out_layer_bwd"] if c.M == 2 * hc.NS_ROWS + 1 and c.gb and c.no == 22)
    obh = next(c for c in g["clift_out_layer_bwd_nh"] if c.M == 2 * hc.NS_ROWS + 1 and c.gb and c.h_bf16)
    nb = next(c for c in g["clift_out_layer_bwd_n128_bf16"] if c.M == 33 and c.gb and c.no == 3)
    ends = [next(c for c in g[e] if c.M == 2 * hc.ENTRIES[e].T + 1 and c.p.get("gb", 1)) for e in hc._FB + hc._FW + ("clift_xyz_head_first2_bf16_bwd",)]
    cs = next(c for c in g["clift_colsum"] if c.M == 513 and c.ld > c.N)
    wnp = next(c for c in g["clift_wgrad_narrow"] if c.M == 129 and c.gb and c.ni == 260 and not c.x_bf16)
    return [(wn, True), (k3, True), (plain, False), (cs, False), (wnp, False), (ob, True), (obh, True), (nb, True)] + [(c, True) for c in ends]


_SHARDED = _shard_cases()


@pytest.mark.parametrize("c,sharded", _SHARDED, ids=[f"{c.entry[6:]}-{c.name}" for c, _ in _SHARDED])
def test_gradient_shard_bracket(c, sharded, capsys):
    """One launch inside clift_grad_shards_begin ... clift_grad_shards_fold.  The gradients of the case lie in one arena [weight gradient | bias
    gradient], pre-filled with the case's pre-fill.  ``sharded``: the kernel calls grad_target (the matrix-core streams); the plain VALU kernels
    of the same entry points add straight into the gradients inside a bracket too, which the fold then leaves alone.
    The record is the one the engine binds once per process (engine.grad_shard_record).  clift_bind_grad_shards(NULL) unbinds it in the
    ``finally`` -- after which a launch inside a begun bracket adds straight into the gradients -- and the engine's record is bound again at
    once, zeroed: the engine caches that it has bound one, and the tests that follow rely on it."""
    from contrastive_lift_amd import engine
    L = _L()
    d, ref = hc.inputs(c), hc.reference(c)
    if c.entry in hc.CHAINED:                # the sums run over the dH1 that was actually stored
        ref = hc.ENTRIES[c.entry].ref(c, d, chain=_stored_chain(Launch(L, c), {}, []))
    names = [q for q in ref if q not in hc.ENTRIES[c.entry].fwd and not q.startswith("_")]           # the accumulated-into outputs: the gradients
    sizes = [d[q].size for q in names]
    R = sum(sizes) + 3
    fill = np.concatenate([d[q].reshape(-1) for q in names] + [np.full(3, hc.SENTINEL, np.float32)])
    delta = np.concatenate([(np.nan_to_num(ref[q][0]) - np.where(np.isnan(ref[q][0]), 0, d[q])).reshape(-1) for q in names] + [np.zeros(3)])
    Sd = np.concatenate([(ref[q][1] - np.where(np.isnan(ref[q][0]), 0, np.abs(d[q]))).reshape(-1) for q in names] + [np.zeros(3)])
    factor = max(hc.factor_for(c, q) for q in names)
    zero_n = R - 5 - int((R - 5) % 4 == 0)                    # begin's scalar tail: not a multiple of 4, short of the range
    arena = torch.from_numpy(fill).to(DEV)
    shards = torch.zeros((8, R), dtype=F32, device=DEV)
    record = engine.grad_shard_record(torch.device(DEV))
    src = torch.tensor([arena.data_ptr(), 4 * R, shards.data_ptr(), 4 * R, 0], dtype=torch.int64, device=DEV)
    la = Launch(L, c)
    views, at = {}, 0
    for q, n in zip(names, sizes):
        views[q] = arena[at:at + n].view(d[q].shape)
        at += n
    host = lambda t: t.cpu().numpy().astype(np.float64)
    within = lambda g, want, base: np.all(np.abs(g - want) <= factor * (Sd + np.abs(base)))
    s = L.stream()
    try:
        L.call("clift_grad_shards_begin", record.data_ptr(), src.data_ptr(), arena.data_ptr(), zero_n, s)
        CALLED.add("clift_grad_shards_begin")
        base = fill.astype(np.float64)
        base[:zero_n] = 0
        assert np.array_equal(host(arena), base), "begin clears exactly zero_n floats"
        rec = record.cpu().numpy()
        assert np.array_equal(rec[:4], src.cpu().numpy()[:4]) and int(rec[4]) & 0xFFFFFFFF == 1
        la.run(outs=views)
        if sharded:
            assert np.array_equal(host(arena), base), "before the fold the gradient range holds only what begin left"
            before = host(shards)
            assert within(before.sum(0), delta, 0 * base)
            first, n = 5, R // 2
            L.call("clift_grad_shards_fold", record.data_ptr(), first, n, 0, s)
            CALLED.add("clift_grad_shards_fold")
            g, sh = host(arena), host(shards)
            on = np.zeros(R, bool)
            on[first:first + n] = True
            assert np.all(np.abs(g - (base + delta))[on] <= (factor * (Sd + np.abs(base)))[on]), "the folded part misses the bound"
            assert np.array_equal(g[~on], base[~on]), "the fold touched gradients outside [first, first + n)"
            assert np.all(sh[:, on] == 0) and np.array_equal(sh[:, ~on], before[:, ~on])
            L.call("clift_grad_shards_fold", record.data_ptr(), 0, first, 0, s)
            L.call("clift_grad_shards_fold", record.data_ptr(), first + n, R - first - n, 1, s)
        else:
            assert np.all(host(shards) == 0), "a kernel without grad_target wrote a shard"
            L.call("clift_grad_shards_fold", record.data_ptr(), 0, R, 1, s)
            CALLED.add("clift_grad_shards_fold")
        g = host(arena)
        assert within(g, base + delta, base) and np.all(host(shards) == 0)
        assert np.array_equal(g[Sd + np.abs(delta) == 0], base[Sd + np.abs(delta) == 0]), "pad words of the gradient range changed"
        assert int(record.cpu().numpy()[4]) & 0xFFFFFFFF == 0, "disable = 1 ends the bracket"
        la.run(outs=views)                                    # after the bracket: straight into the gradients
        assert within(host(arena), base + 2 * delta, np.abs(base) + np.abs(delta) + Sd) and np.all(host(shards) == 0)
        L.call("clift_grad_shards_begin", record.data_ptr(), src.data_ptr(), None, 0, s)
        assert int(record.cpu().numpy()[4]) & 0xFFFFFFFF == 1
        L.call("clift_grad_shards_fold", record.data_ptr(), 0, 0, 1, s)
        assert int(record.cpu().numpy()[4]) & 0xFFFFFFFF == 0, "fold with n = 0, disable = 1 ends the bracket"
    finally:
        torch.cuda.synchronize()
        L.call("clift_bind_grad_shards", None)
    try:                                  # unbound: a begun bracket has no effect on where a kernel adds
        now = host(arena)
        L.call("clift_grad_shards_begin", record.data_ptr(), src.data_ptr(), None, 0, s)
        la.run(outs=views)
        assert np.all(host(shards) == 0) and not np.array_equal(host(arena), now), "an unbound record still steered a kernel into the shards"
    finally:
        L.call("clift_grad_shards_fold", record.data_ptr(), 0, 0, 1, s)
        torch.cuda.synchronize()
        record.zero_()
        torch.cuda.synchronize()
        L.call("clift_bind_grad_shards", record.data_ptr())


def test_every_entry_point_of_the_table_was_called():
    """Runs last in this file: the launches above reached every entry point of the family, as parsed from include/clift.h."""
    assert CALLED == hc.header_entry_points(), sorted(hc.header_entry_points() ^ CALLED)
