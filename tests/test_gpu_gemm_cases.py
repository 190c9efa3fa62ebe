"""Every route of clift_gemm against the fp64 references of tests/gemm_cases.py, launched through _lib.call("clift_gemm", ...) with raw
pointers.  Per case: the route the real device addresses take is the case's; the result is held element by element to gemm_cases.check;
output pad columns, the two rows past the output and the words in front of a misaligned base keep their sentinel; a second launch gives
the same bits wherever the route does not add with atomics.  Operand rows past the row count are NaN and operand pad columns are NaN or --
where the kernel reads them against zero weights -- 9.5e8, so a kernel that reads what it should not returns a NaN or a wrong number.
Each test prints ``yardstick | device error / S | bound factor | worst error / bound`` per case."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_cases as gc
from test_gpu_march import DEV, _L, _stop_after_a_device_error  # noqa: F401

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _up(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return (t.to(BF16) if bf16 else t).to(DEV).contiguous()


@contextlib.contextmanager
def _setting(L, c):
    """The case's switch word and CU reserve around its launches."""
    from contrastive_lift_amd import engine
    with engine.kernel_switches(tiled_only=bool(c.switches & gc.SW_TILED_ONLY), x6_tiled=bool(c.switches & gc.SW_X6_TILED)):
        if c.reserve:
            L.call("clift_set_cu_reserve", c.reserve)
        try:
            yield
        finally:
            if c.reserve:
                L.call("clift_set_cu_reserve", 0)


@contextlib.contextmanager
def _limit(rows):
    from contrastive_lift_amd import engine
    lim = engine.rows_limit(torch.device(DEV))
    lim[0:1].fill_(rows)
    try:
        yield
    finally:
        engine.reset_rows_limit()


class Launch:
    """The device buffers of a case and its launches."""

    def __init__(self, L, c, d, sign_bits=None):
        self.L, self.c = L, c
        self.A, self.B = _up(d["A"], c.a_bf16), _up(d["B"], c.b_bf16)
        self.bias = _up(d["bias"]) if c.bias else None
        self.mask = _up(d["mask"], c.mask_bf16) if c.mask else None
        self.lead = c.c_mis // 4                                  # (only fp32 outputs are misaligned in the table)
        self.C0 = torch.cat([torch.full((self.lead,), gc.SENTINEL), torch.from_numpy(d["C0"]).reshape(-1)]).to(BF16 if c.c_bf16 else F32).to(DEV)
        self.cs0 = _up(d["colsum0"]) if c.colsum else None
        lib = L.load()
        self.signs = sign_bits if sign_bits is not None else (torch.zeros((int(lib.clift_sign_bits_bytes(c.M)),), dtype=torch.uint8, device=DEV) if c.sign_bits else None)
        self.ws = None
        if c.route == "SPLIT_TILED":
            self.ws = torch.empty((int(lib.clift_gemm_workspace_bytes(c.N, c.K)),), dtype=torch.uint8, device=DEV)

    def run(self, M=None, a_off=0, c_rows_off=0):
        """One launch on fresh copies of the output pre-fills; returns (C logical (M, N) float64, colsum, the whole output buffer, the whole
        colsum buffer).  ``M`` / ``a_off`` / ``c_rows_off``: a launch of M rows of its own from row a_off of A into row c_rows_off of C (forward forms)."""
        L, c = self.L, self.c
        Cb, cs = self.C0.clone(), (self.cs0.clone() if self.cs0 is not None else None)
        es_a, es_c = (2 if c.a_bf16 else 4), (2 if c.c_bf16 else 4)
        ptr = lambda t: t.data_ptr() if t is not None else None
        addr = {"A": self.A.data_ptr() + es_a * a_off * c.lda, "B": self.B.data_ptr(), "C": Cb.data_ptr() + es_c * c_rows_off * c.ldc, "bias": ptr(self.bias),
                "mask": ptr(self.mask), "colsum": ptr(cs), "sign_bits": ptr(self.signs), "workspace": ptr(self.ws),
                "workspace_bytes": self.ws.numel() if self.ws is not None else 0}
        g = gc.descriptor(c, addr)
        if M is not None:
            g.M = M
        r = L.load().clift_gemm_route(C.byref(g))
        name = L.load().clift_gemm_route_name(r).decode() if r >= 0 else "error: " + L.load().clift_last_error().decode()
        assert name == c.route, (c, name)
        L.call("clift_gemm", C.byref(g), L.stream())
        torch.cuda.synchronize()
        flat = Cb.float().cpu().numpy().astype(np.float64)
        body = flat[self.lead:].reshape(c.c_rows + 2, c.ldc)
        logical = body[:c.N, :c.M].T if c.c_trans else body[:c.M, :c.N]
        return logical, (cs.cpu().numpy().astype(np.float64) if cs is not None else None), flat, body

    def untouched(self, flat, body, cs):
        c = self.c
        if not (np.all(flat[:self.lead] == gc.SENTINEL) and np.all(body[:c.c_rows, c.c_cols:] == gc.SENTINEL) and np.all(body[c.c_rows:] == gc.SENTINEL)):
            return "output pad columns / rows past the output were written"
        if cs is not None and not np.all(cs[c.M:] == gc.SENTINEL):
            return "colsum was written past its M entries"
        return None


def _x6_forward_with_signs(L, c):
    """The activation and the sign bytes a LAYER_X6 forward of the same row count writes: what the dgrad-from-sign-bytes form reads."""
    fwd = next(f for f in gc.cases() if f.route == "LAYER_X6" and f.signs == "write" and f.M == c.M and f.reserve == c.reserve)
    with _setting(L, fwd):
        la = Launch(L, fwd, gc.inputs(fwd))
        H, _, _, _ = la.run()
    return H, la.signs


def _report(c, got, ref):
    y = gc.yardsticks(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got["C"] - ref["C"]) / ref["S_C"]
    e = float(np.nanmax(np.where(np.isfinite(e), e, np.nan))) if e.size else 0.0
    return f"{y['C']:9.3e} | {e:9.3e} | {gc.factor_for(c, 'C'):9.3e}"


_GROUPS = sorted(gc.groups())


@pytest.mark.parametrize("route,form", _GROUPS, ids=[f"{r}-{f}" for r, f in _GROUPS])
def test_route_against_fp64(route, form, capsys):
    L, info, lines, broken = _L(), gc.ROUTES[route], [], []
    for c in gc.groups()[(route, form)]:
        d, ref, signs = gc.inputs(c), None, None
        if c.signs == "read":
            H, signs = _x6_forward_with_signs(L, c)
            ref = gc.reference_of(c, mask=H)
        ref = gc.reference(c) if ref is None else ref
        with _setting(L, c):
            la = Launch(L, c, d, signs)
            Cl, cs, flat, body = la.run()
            got = {"C": Cl.copy(), "colsum": None if cs is None else cs[:c.M]}
            ok, worst, text = gc.check(got, c, ref=ref)
            lines.append(f"{route:18s} {form:14s} {c.name:34s} | {_report(c, got, ref)} | {worst:6.3f}")
            if not ok:
                broken.append(text)
            bad = la.untouched(flat, body, cs)
            if bad:
                broken.append(f"{c}: {bad}")
            if not info.atomics and not c.accumulate and not c.colsum:
                again = la.run()[2]
                if not np.array_equal(flat.view(np.int64), again.view(np.int64)):
                    broken.append(f"{c}: a second launch gave other bits")
    with capsys.disabled():
        print("\nroute              form           case                               | yardstick | dev err/S | bound     | err/bound\n" + "\n".join(lines))
    assert not broken, "\n".join(broken)


@pytest.mark.parametrize("route", ["LAYER_F32_FWD", "LAYER_N128", "LAYER_X6", "LAYER_N6"])
def test_a_rows_bits_do_not_depend_on_its_launch(route):
    """csrc/gemm.hip: "every M: a row's bits must not depend on its launch".  Rows 0, T - 1, T and M - 1 of the M3 launch against the same rows
    computed in launches of their own: M = 1 at an offset pointer, and the two-row range [T - 1, T + 1)."""
    L, T = _L(), gc.ROUTES[route].T
    for c in (c for c in gc.cases() if c.route == route and c.form == "fwd" and c.reserve and c.signs is None):
        with _setting(L, c):
            la = Launch(L, c, gc.inputs(c))
            whole = la.run()[0].copy()
        for first, n in ((0, 1), (T - 1, 1), (T, 1), (c.M - 1, 1), (T - 1, 2)):
            part = la.run(M=n, a_off=first, c_rows_off=first)[0]
            assert np.array_equal(part[first:first + n].view(np.int64), whole[first:first + n].view(np.int64)), (c, first, n)
            assert np.all(part[:first] == gc.SENTINEL) and np.all(part[first + n:] == gc.SENTINEL), (c, first, n, "rows outside the launch were written")


def _limit_cases():
    """One case per (route, form) of every precision-0 / -2 route whose kernel calls limit_rows: the largest of its plain row counts (the tiled
    kernels: the forward at 2 T + 1 rows and a weight-gradient form)."""
    out = []
    for (route, form), mine in gc.groups().items():
        info = gc.ROUTES[route]
        if not info.limit:
            continue
        mine = [c for c in mine if not c.reserve and c.signs is None and c.rows > info.T + 1 and not c.c_trans and not c.c_mis]
        if mine:
            out.append(max(mine, key=lambda c: (c.rows, -c.seed)))
    return out


_LIMITED = _limit_cases()


@pytest.mark.parametrize("c", _LIMITED, ids=[f"{c.route}-{c.form}-{c.name}" for c in _LIMITED])
def test_route_under_a_device_side_row_limit(c):
    """A sync-free pass sizes a launch by a capacity and leaves the true row count L on the device.  With L = count - T - 1 and NaN in every
    streamed row at and past L: a weight-gradient form equals the reference of the first L rows; a forward / dgrad form gives rows < L the bits
    of the unlimited launch (nothing is asserted of its rows >= L)."""
    L, T = _L(), gc.ROUTES[c.route].T
    lim = c.rows - T - 1
    d = dict(gc.inputs(c))
    with _setting(L, c):
        free = Launch(L, c, d).run()[0].copy() if not c.a_trans else None
        d["A"] = d["A"].copy()
        d["A"][lim:] = np.nan
        if c.a_trans:
            d["B"] = d["B"].copy()
            if c.b_trans:
                d["B"][lim:] = np.nan
            else:
                d["B"][:, lim:] = np.nan
        la = Launch(L, c, d)
        with _limit(lim):
            Cl, cs, flat, body = la.run()
    assert la.untouched(flat, body, cs) is None
    if c.a_trans:
        ok, worst, text = gc.check({"C": Cl, "colsum": None if cs is None else cs[:c.M]}, c, ref=gc.reference_of(c, rows=lim))
        assert ok, text
    else:
        assert np.array_equal(Cl[:lim].view(np.int64), free[:lim].view(np.int64)), (c, "rows below the limit differ from the unlimited launch")
