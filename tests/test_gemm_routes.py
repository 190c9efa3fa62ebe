"""The clift_gemm routing table (no GPU: clift_gemm_route is host arithmetic on the descriptor, and engine.gemm is run on stand-in tensors with
the launch recorded instead of issued).

``descriptors()`` below enumerates the table: the three precisions; each kernel switch alone, both, and the density switches; N, K over
{3, 22, 27, 32, 128, 144, 160, 256} and the row count over {1, 63, 4095, 4096, 265000} in the four transpose forms, plus the training step's
own shapes under every kernel-switch state, once with drawn options and once with their usual ones; mask / bias / act / accumulate / split_k /
c_trans / colsum / sign_bits present or absent; fp32- and bf16-stored operands; aligned and odd pitches and base addresses (addresses are made
up: nothing reads through them).  tests/golden/gemm_routes.json holds, row for row, what the commit before routing moved into clift_gemm_route
did with them -- recorded with a build of that commit's library whose clift_gemm reported the branch it took instead of launching, and with that
commit's engine.gemm -- and the sha256 of the enumeration, so that the two cannot drift apart.  A route added later gets new rows, recorded
from clift_gemm_route itself; the rows recorded here do not change."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "gemm_routes.json")
BASE = {"A": 0x10000000000, "B": 0x20000000000, "C": 0x30000000000, "mask": 0x40000000000, "bias": 0x50000000000, "colsum": 0x60000000000,
        "sign_bits": 0x70000000000, "workspace": 0x80000000000}
# switches: bit 0 tiled-only, bit 1 x6-tiled, bit 2 density-forward-per-thread, bit 3 density-scatter-walk; *_mis: byte offset of a base
# address from 16-byte alignment; mode: engine.MLP_PRECISION = clift_gemm_t.precision
FIELDS = ["mode", "switches", "M", "N", "K", "a_trans", "b_trans", "lda", "ldb", "ldc", "ldmask", "bias", "act", "mask", "accumulate", "split_k",
          "c_trans", "colsum", "sign_bits", "a_bf16", "b_bf16", "c_bf16", "mask_bf16", "a_mis", "b_mis", "c_mis", "mask_mis"]
DIMS = [3, 22, 27, 32, 128, 144, 160, 256]
ROWS = [1, 63, 4095, 4096, 265000]
# (a_trans, b_trans, M, N, K; None = the row count) of the training step's launches and their neighbours
HOT = [(0, 0, None, 256, 256), (0, 1, None, 256, 256), (1, 1, 256, 256, None), (0, 0, None, 128, 128), (0, 0, None, 128, 160), (0, 1, None, 128, 128),
       (0, 1, None, 160, 128), (1, 1, 128, 128, None), (1, 1, 128, 160, None), (0, 1, None, 256, 3), (0, 1, None, 256, 22), (0, 1, None, 128, 3),
       (0, 1, None, 144, 27), (0, 0, None, 22, 256), (0, 0, None, 3, 256), (0, 0, None, 27, 144), (0, 0, None, 3, 128)]


class _Draw:
    """A fixed 64-bit linear congruential sequence: the enumeration must not depend on the interpreter's generator."""

    def __init__(self, seed):
        self.x = seed

    def u(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 11) / 2.0 ** 53

    def p(self, prob):
        return int(self.u() < prob)

    def choice(self, seq):
        return seq[int(self.u() * len(seq))]


def descriptors():
    d = _Draw(20261017)
    r4, r8 = (lambda x: (x + 3) // 4 * 4), (lambda x: (x + 7) // 8 * 8)

    def pitch(n, bf16, p_odd, natural_ok=False):
        base, u = (r8(n) if bf16 else r4(n)), d.u()
        if u < p_odd:
            return base + 1
        if natural_ok and u < p_odd + 0.15:
            return n
        return base if u < 0.75 else base + (8 if bf16 else 4) if u < 0.9 else max(base, 256)

    def make(mode, sw, at, bt, M, N, K, hot=False):
        # options drawn per form so that most launches are legal (a table of refused launches would say little), faults at a few per cent each
        c = dict.fromkeys(FIELDS, 0)
        c.update(mode=mode, switches=sw, M=M, N=N, K=K, a_trans=at, b_trans=bt, split_k=1)
        x6shape = mode == 2 and N == 256 and K == 256
        if not at and not bt:
            c.update(bias=d.p(0.7), act=d.p(0.6), mask=d.p(0.08), accumulate=d.p(0.03), c_trans=d.p(0.03))
            c["sign_bits"] = d.p(0.4) if (x6shape and not c["mask"]) else d.p(0.01)
        elif not at:
            c.update(mask=d.p(0.6), bias=d.p(0.04), act=d.p(0.04), accumulate=d.p(0.03), c_trans=d.p(0.03))
            c["sign_bits"] = d.p(0.5) if (x6shape and not c["mask"]) else d.p(0.01)
        elif bt:
            c.update(accumulate=d.p(0.93), colsum=d.p(0.5), c_trans=d.p(0.05), bias=d.p(0.02), mask=d.p(0.02), act=d.p(0.02))
            if c["accumulate"]:
                c["split_k"] = d.choice([1, 1, 8, 64])
        else:
            c.update(accumulate=d.p(0.5), colsum=d.p(0.3))
            if c["accumulate"]:
                c["split_k"] = d.choice([1, 8])
        if not at:
            c["colsum"] = d.p(0.005)
        if not c["accumulate"] and d.p(0.005):
            c["split_k"] = 8
        if mode == 1:       # storage: the streamed operands bf16-stored together, the output alone, or drawn flag by flag
            u = d.u()
            if u < 0.45:
                if not at:
                    c.update(a_bf16=1, c_bf16=1, mask_bf16=c["mask"])
                elif bt:
                    c.update(a_bf16=1, b_bf16=1)
            elif u < 0.6 and not at:
                c.update(c_bf16=1, mask_bf16=c["mask"])
            elif u < 0.66:
                c.update(a_bf16=d.p(0.5), b_bf16=d.p(0.3), c_bf16=d.p(0.5), mask_bf16=c["mask"] and d.p(0.5))
        elif d.p(0.01):
            c.update(a_bf16=1, c_bf16=1)
        if c["accumulate"] or c["c_trans"]:
            c["c_bf16"] = c["c_bf16"] and d.p(0.1)
        pf = 0.0 if hot else 0.012
        c["lda"] = pitch(M if at else K, c["a_bf16"], 0.0 if c["a_bf16"] else pf)
        c["ldb"] = pitch(N if bt else K, c["b_bf16"], 0.0 if c["b_bf16"] else pf)
        c["ldc"] = pitch(M if c["c_trans"] else N, c["c_bf16"], 0.08, natural_ok=True)
        c["ldmask"] = pitch(N, c["mask_bf16"], 0.08, natural_ok=True) if c["mask"] else 0
        c["a_mis"], c["b_mis"] = 4 * d.p(pf), 4 * d.p(pf)
        c["c_mis"] = d.choice([4, 8]) * d.p(0.08)
        c["mask_mis"] = d.choice([4, 8]) * d.p(0.08) if c["mask"] else 0
        return c

    def usual(c):        # the options the training step itself uses for the form: aligned rows, bias / mask / accumulate as the chains pass them
        at, bt, M, N, K = c["a_trans"], c["b_trans"], c["M"], c["N"], c["K"]
        c.update(c_trans=0, c_mis=0, mask_mis=0)
        if at:
            c.update(accumulate=1, bias=0, act=0, mask=0)
        elif bt:
            c.update(accumulate=0, split_k=1, colsum=0, bias=0, act=0, mask=int(N == K or K <= 22))
            c["sign_bits"] = 0 if c["mask"] else c["sign_bits"]
        else:
            c.update(accumulate=0, split_k=1, colsum=0, mask=0)
        if c["mode"] == 1 and d.u() < 0.6:
            c.update(a_bf16=1, b_bf16=1) if at else c.update(a_bf16=int(K > 32), c_bf16=1)
        else:
            c.update(a_bf16=0, b_bf16=0, c_bf16=0)
        c["mask_bf16"] = int(c["mask"] and c["c_bf16"])
        c["lda"], c["ldb"] = pitch(M if at else K, c["a_bf16"], 0.0), pitch(N if bt else K, c["b_bf16"], 0.0)
        c["ldc"], c["ldmask"] = pitch(N, c["c_bf16"], 0.0), (pitch(N, c["mask_bf16"], 0.0) if c["mask"] else 0)
        return c

    sw_grid = [0] * 8 + [1] * 4 + [2] * 3 + [3] * 2 + [4, 8, 12, 15, 5, 10]
    cases = []
    for mode in (0, 1, 2):
        for at, bt in ((0, 0), (0, 1), (1, 1), (1, 0)):
            for n in DIMS:
                for k in DIMS:
                    for rows in ROWS:      # (the row count is K in the a_trans forms)
                        cases.append(make(mode, d.choice(sw_grid), at, bt, *((k, n, rows) if at else (rows, n, k))))
    for finish in (lambda c: c, usual):
        for mode in (0, 1, 2):
            for sw in (0, 1, 2, 3):
                for at, bt, m, n, k in HOT:
                    for rows in ROWS:
                        cases.append(finish(make(mode, sw, at, bt, *((m, n, rows) if at else (rows, n, k)), hot=True)))
    for mode in (0, 1, 2):     # empty launches
        cases += [make(mode, 0, 0, 0, 0, 256, 256, hot=True), make(mode, 0, 1, 1, 256, 0, 4096, hot=True)]
    seen, uniq = set(), []
    for c in cases:
        key = tuple(int(c[f]) for f in FIELDS)
        if key not in seen:
            seen.add(key)
            uniq.append({f: v for f, v in zip(FIELDS, key)})
    return uniq


def descriptors_sha256(rows):
    return hashlib.sha256(json.dumps([[c[f] for f in FIELDS] for c in rows]).encode()).hexdigest()


@pytest.fixture(scope="module")
def table():
    """(outcomes, rows): every descriptor with its recorded `library` outcome (index into outcomes: the kernel clift_gemm chose, or its error,
    for precision = mode and -- in mode 2 -- a valid workspace) and what engine.gemm sent for it (sent_precision, sent_workspace) and whether
    the library accepted that launch (sent_accepted)."""
    doc, rows = json.load(open(GOLDEN)), descriptors()
    assert len(rows) == len(doc["library"]) == len(doc["sent"]) and descriptors_sha256(rows) == doc["descriptors_sha256"], \
        "descriptors() no longer enumerates the table the golden file was recorded for"
    for c, lib, sent in zip(rows, doc["library"], doc["sent"]):       # sent = 4 * precision + 2 * workspace + accepted
        c.update(library=lib, sent_precision=sent >> 2, sent_workspace=(sent >> 1) & 1, sent_accepted=sent & 1)
    return doc["outcomes"], rows


@pytest.fixture()
def switches():
    """Sets the library's switch word per row; the word the process started with is back afterwards."""
    from contrastive_lift_amd import _lib, engine
    lib = _lib.load()
    prev = lib.clift_get_switches()

    def put(word):
        lib.clift_set_switches(word)
        engine._switches = word
    yield put
    put(prev)


def test_switch_word_roundtrip():
    from contrastive_lift_amd import _lib, engine
    lib = _lib.load()
    start = lib.clift_get_switches()
    with engine.kernel_switches(tiled_only=True, dens_scatter_walk=True):
        inner = start | engine.SWITCH_TILED_ONLY | engine.SWITCH_DENS_SCATTER_WALK
        assert lib.clift_get_switches() == inner and not engine.persistent_ok()
        with engine.kernel_switches(tiled_only=False, x6_tiled=True):
            assert lib.clift_get_switches() == (inner & ~engine.SWITCH_TILED_ONLY) | engine.SWITCH_X6_TILED
            assert engine.persistent_ok() and not engine.persistent_x6_ok()
        assert lib.clift_get_switches() == inner
    assert lib.clift_get_switches() == start and engine._switches == start
    assert lib.clift_set_switches(start) == start          # the setter returns the previous word


def test_route_names():
    from contrastive_lift_amd import _lib
    routes = _lib.gemm_routes()
    assert routes["NONE"] == 0 and len(set(routes.values())) == len(routes) > 20
    assert _lib.load().clift_gemm_route_name(-1) == b"INVALID" and _lib.load().clift_gemm_route_name(len(routes)) == b"INVALID"


def test_library_routes_match_the_recorded_table(table, switches):
    """clift_gemm_route gives, for every recorded descriptor, the kernel the parent's clift_gemm chose -- or the same error."""
    from contrastive_lift_amd import _lib
    from contrastive_lift_amd._lib import Gemm
    outcomes, rows = table
    lib, routes = _lib.load(), _lib.gemm_routes()
    assert {o for o in outcomes if not o.startswith("error: ")} == set(routes), "the table must reach every route, and only routes the library names"
    seen, bad = set(), []
    for c in rows:
        switches(c["switches"])
        g = Gemm()
        g.M, g.N, g.K = c["M"], c["N"], c["K"]
        g.A, g.lda, g.a_trans = BASE["A"] + c["a_mis"], c["lda"], c["a_trans"]
        g.B, g.ldb, g.b_trans = BASE["B"] + c["b_mis"], c["ldb"], c["b_trans"]
        g.C, g.ldc = BASE["C"] + c["c_mis"], c["ldc"]
        g.bias = BASE["bias"] if c["bias"] else None
        g.act = c["act"]
        g.mask, g.ldmask = (BASE["mask"] + c["mask_mis"] if c["mask"] else None), c["ldmask"]
        g.accumulate, g.split_k, g.c_trans = c["accumulate"], c["split_k"], c["c_trans"]
        g.colsum = BASE["colsum"] if c["colsum"] else None
        g.sign_bits = BASE["sign_bits"] if c["sign_bits"] else None
        g.a_bf16, g.b_bf16, g.c_bf16, g.mask_bf16 = c["a_bf16"], c["b_bf16"], c["c_bf16"], c["mask_bf16"]
        g.precision = c["mode"]
        if c["mode"] == 2:
            g.workspace, g.workspace_bytes = BASE["workspace"], 1 << 40
        r = lib.clift_gemm_route(C.byref(g))
        got = lib.clift_gemm_route_name(r).decode() if r >= 0 else "error: " + lib.clift_last_error().decode()
        seen.add(got)
        if got != outcomes[c["library"]]:
            bad.append((c, got, outcomes[c["library"]]))
    assert not bad, f"{len(bad)} of {len(rows)} descriptors routed differently, e.g. {bad[:3]}"
    assert seen == set(outcomes)


class _Stand:
    """What engine.gemm reads of a tensor: address, element size, dtype, device."""

    def __init__(self, addr, bf16):
        self.addr, self.dtype, self.device = addr, (torch.bfloat16 if bf16 else torch.float32), torch.device("cpu")

    def data_ptr(self):
        return self.addr

    def element_size(self):
        return 2 if self.dtype == torch.bfloat16 else 4


def test_engine_gemm_sends_what_the_parent_sent(table, switches, monkeypatch):
    """engine.gemm sends the recorded precision, with or without a workspace as recorded, for every descriptor whose launch the parent's library
    accepted.  (The rest -- the parent's launch was refused, among them the few on which its Python copy of the predicates disagreed with the
    library -- are compared at the library level only, above; they must stay under 10 % of the table.)"""
    from contrastive_lift_amd import engine
    _, rows = table
    sent = {}

    def record(name, gref, stream):
        assert name == "clift_gemm"
        sent["precision"], sent["workspace"] = int(gref._obj.precision), int(bool(gref._obj.workspace))

    monkeypatch.setattr(engine, "call", record)
    monkeypatch.setattr(engine, "stream", lambda: None)
    rejected, bad = 0, []
    for c in rows:
        if not c["sent_accepted"]:
            rejected += 1
            continue
        switches(c["switches"])
        monkeypatch.setattr(engine, "MLP_PRECISION", c["mode"])
        es_a, es_c = (2 if c["a_bf16"] else 4), (2 if c["c_bf16"] else 4)
        opt = lambda key: _Stand(BASE[key], 0) if c[key] else None
        engine.gemm(c["M"], c["N"], c["K"], _Stand(BASE["A"], c["a_bf16"]), c["lda"], _Stand(BASE["B"] + c["b_mis"], c["b_bf16"]), c["ldb"],
                    _Stand(BASE["C"], c["c_bf16"]), c["ldc"], a_trans=c["a_trans"], b_trans=c["b_trans"], bias=opt("bias"), act=c["act"],
                    mask=_Stand(BASE["mask"] + c["mask_mis"], c["mask_bf16"]) if c["mask"] else None, ldmask=c["ldmask"], accumulate=c["accumulate"],
                    split_k=c["split_k"], a_off=c["a_mis"] // es_a, c_off=c["c_mis"] // es_c, c_trans=c["c_trans"], colsum=opt("colsum"),
                    sign_bits=opt("sign_bits"))
        if (sent["precision"], sent["workspace"]) != (c["sent_precision"], c["sent_workspace"]):
            bad.append((c, dict(sent)))
    print(f"{rejected} of {len(rows)} descriptors were refused at the parent ({100.0 * rejected / len(rows):.1f} %): library-level comparison only")
    assert rejected < 0.1 * len(rows)
    assert not bad, f"{len(bad)} launches sent differently, e.g. {bad[:3]}"
