"""The clift_gemm case table on the CPU (tests/gemm_cases.py; the GPU side is tests/test_gpu_gemm_cases.py): every case's descriptor takes the
route the case names, the table reaches every route and every form the routes' predicates admit, every case is well-conditioned, the
comparison of the GPU tests passes the fp32 restatement in all three orders and fails it with each of the known mistakes built in, and the
M3 row counts do what they are for.  No GPU: clift_gemm_route is host arithmetic on made-up addresses."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as gc
from gemm_cases import ILL_CONDITIONED, ORDERS

BASE = {"A": 0x10000000000, "B": 0x20000000000, "C": 0x30000000000, "mask": 0x40000000000, "bias": 0x50000000000, "colsum": 0x60000000000,
        "sign_bits": 0x70000000000, "workspace": 0x80000000000}


@pytest.fixture()
def switches():
    """Sets the library's switch word; the word the process started with is back afterwards."""
    from contrastive_lift_amd import _lib, engine
    lib = _lib.load()
    prev = lib.clift_get_switches()

    def put(word):
        lib.clift_set_switches(word)
        engine._switches = word
    yield put
    put(prev)


def test_every_case_takes_its_route_and_the_table_reaches_every_route(switches):
    from contrastive_lift_amd import _lib
    lib, reached, bad = _lib.load(), set(), []
    for c in gc.cases():
        switches(c.switches)
        g = gc.descriptor(c, BASE)
        r = lib.clift_gemm_route(C.byref(g))
        got = lib.clift_gemm_route_name(r).decode() if r >= 0 else "error: " + lib.clift_last_error().decode()
        reached.add(got)
        if got != c.route:
            bad.append((c, got))
    assert not bad, f"{len(bad)} cases routed elsewhere, e.g. {bad[:4]}"
    assert reached == set(_lib.gemm_routes()) - {"NONE"}
    assert set(gc.ROUTES) == reached


def test_every_form_of_the_issue_is_present():
    has = lambda route, form, **f: any(c.route == route and c.form == form and all(getattr(c, k) == v for k, v in f.items()) for c in gc.cases())
    assert has("LAYER_X6", "fwd", signs=None) and has("LAYER_X6", "fwd", signs="write")
    assert has("LAYER_X6", "dgrad_masked", signs=None, mask=1) and has("LAYER_X6", "dgrad_masked", signs="read", mask=0)
    for route in ("LAYER_N6", "LAYER_NB16"):
        assert has(route, "fwd", K=128) and has(route, "fwd", K=160) and has(route, "dgrad_masked", N=128, K=128) and has(route, "dgrad_unmasked", N=160, K=128)
    assert has("LAYER_NB16", "dgrad_unmasked", c_bf16=1) and has("LAYER_NB16", "dgrad_unmasked", c_bf16=0)
    assert has("LAYER_N128", "fwd", K=128) and has("LAYER_N128", "fwd", K=160) and has("LAYER_N128", "dgrad_masked")
    assert has("LAYER_BF16", "fwd") and has("LAYER_BF16", "dgrad_masked")
    assert all(has("DGRAD_NARROW", "dgrad_masked", N=n) for n in (128, 256)) and all(has("DGRAD_NARROW", "dgrad_unmasked", N=n) for n in (36, 144, 256))
    assert {(c.K, c.lda) for c in gc.cases() if c.route == "DGRAD_NARROW"} == set(gc.NARROW_KLDA)
    assert {gc.cdiv(k, 8) for k, _ in gc.NARROW_KLDA} == {1, 2, 3, 4}
    for route in ("WGRAD_N128", "WGRAD_N6", "WGRAD_NB16"):
        assert all(has(route, "wgrad", N=n, colsum=cs) for n in (128, 160) for cs in (0, 1))
    assert has("SPLIT_TILED", "fwd", switches=0) and has("SPLIT_TILED", "fwd", N=256, K=256, switches=gc.SW_X6_TILED)
    assert has("SPLIT_TILED", "dgrad_masked", N=256, K=256, switches=gc.SW_X6_TILED)
    tiled = {"TILED_256X32": (32,), "TILED_128X128": (33, 128), "TILED_128X256": (129,)}
    for prefix in ("TILED_", "TILED_BF16_"):
        for suffix, ns in tiled.items():
            route = prefix + suffix[len("TILED_"):]
            mine = [c for c in gc.cases() if c.route == route]
            assert {(c.a_trans, c.b_trans) for c in mine} >= ({(0, 0), (0, 1), (1, 1), (1, 0)} if prefix == "TILED_" else {(0, 0), (0, 1), (1, 1)})
            assert {c.N for c in mine} >= set(ns)
            assert any(c.N % 4 for c in mine) and any(c.ldc % 2 for c in mine) and any(c.c_mis == 4 for c in mine) and any(c.c_trans for c in mine)
            assert {c.split_k for c in mine if c.accumulate} >= {1, 3} and any(c.colsum for c in mine)
            assert any(c.K == 1 for c in mine) and any(c.K % 32 and c.K > 32 for c in mine)
            assert any(c.mask and c.bias and c.act for c in mine)
            if prefix == "TILED_BF16_":       # the storage combinations the router admits
                st = {(c.a_bf16, c.b_bf16, c.c_bf16) for c in mine}
                assert st >= {(0, 0, 0), (1, 0, 1), (0, 0, 1), (1, 1, 0)}
    assert {c.N for c in gc.cases() if c.route.endswith("128X128")} >= {33, 128} and {c.N for c in gc.cases() if c.route.endswith("256X32")} >= {32}


def test_row_counts_follow_the_size_rule():
    for (route, form), mine in gc.groups().items():
        info = gc.ROUTES[route]
        rows = {c.rows for c in mine if not c.reserve}
        T = info.T
        want = {"every": {1, T - 1, T, T + 1, 2 * T + 1}, "m64": {64, 65, 64 + T + 1}, "m4096": {4096, 4097, 4096 + T - 1}}[info.rows]
        if form == "fwd" or info.plan is not None:
            assert rows >= want, (route, form, rows)
        assert max(c.rows for c in mine) <= 50000
        if info.plan is not None:
            assert any(c.reserve == gc.RESERVE and c.rows == gc.m3(route, form) for c in mine), (route, form)


@pytest.mark.parametrize("route", gc.PERSISTENT)
def test_m3_walks_three_tiles_and_ends_on_a_ragged_tile(route):
    """Pushed through the restated row_ranges with the launcher's per_cu and the reserve, M3 gives a block with at least three tiles and a ragged
    last tile; M3 - 1 does not (it is the smallest such count), unless the route's minimum already does."""
    T = gc.ROUTES[route].T
    for form in sorted({c.form for c in gc.cases() if c.route == route}):
        rows = gc.m3(route, form)
        blocks = gc.block_rows(route, form, rows, gc.CUS - gc.RESERVE)
        assert blocks[0][0] == 0 and blocks[-1][1] == rows and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert max(gc.cdiv(e - b, T) for b, e in blocks) >= 3
        assert (blocks[-1][1] - blocks[-1][0]) % T != 0
        assert rows == gc.MIN_ROWS[gc.ROUTES[route].rows] or not gc.walks_three_tiles_and_ends_ragged(route, form, rows - 1)
        assert rows <= 50000


def test_row_ranges_restated_like_the_header():
    """The same expressions as csrc/row_ranges.h on a few values its own host test pins (tests/test_row_ranges_host.py walks all of them)."""
    assert gc.row_ranges(0, 32, 256) == (0, 0, 0)
    assert gc.row_ranges(1, 32, 256) == (1, 32, 1)
    assert gc.row_ranges(8193, 32, 128) == (128, 96, 86)
    assert gc.row_ranges(70000, 64, 256, 2) == (512, 192, 365)


_GROUPS = sorted(gc.groups())


@pytest.mark.parametrize("route,form", _GROUPS, ids=[f"{r}-{f}" for r, f in _GROUPS])
def test_conditioning_and_plain_orders_pass(route, form):
    """Every yardstick is at most ILL_CONDITIONED, and ``check`` passes the fp32 restatement in each of the three orders."""
    for c in gc.groups()[(route, form)]:
        y = gc.yardsticks(c)
        assert max(y.values()) <= ILL_CONDITIONED, (c, y)
        for order in ORDERS:
            ok, worst, text = gc.check(gc.restate(c, order), c)
            assert ok, (order, text)


def _candidates(mistake):
    """Cases a mistake can show on, the cheapest first."""
    T = lambda c: gc.ROUTES[c.route].T
    ragged = lambda c: c.rows > T(c) and c.rows % T(c)
    want = {
        "k_last_chunk_dropped": lambda c: c.form == "fwd" and c.K == 160,
        "ragged_tile_rows_from_previous_tile": ragged,
        "mask_one_tile_late": lambda c: c.mask and c.M > T(c),
        "mask_ge": lambda c: c.mask,
        "bias_missing_on_last_quad": lambda c: c.bias and c.M >= 32,        # (a single row under ReLU may hide it: negative either way)
        "relu_after_mask": lambda c: c.mask and c.bias and c.act,
        "accumulate_overwrites": lambda c: c.accumulate,
        "colsum_overwrites": lambda c: c.colsum,
        "c_trans_ignored": lambda c: c.c_trans,
        "pad_column_contracted": lambda c: not c.a_trans and c.lda > c.K,
        "row_past_count_reduced": lambda c: c.a_trans,
        "x6_middle_term_dropped": lambda c: gc.ROUTES[c.route].split,
    }[mistake]
    return sorted((c for c in gc.cases() if want(c)), key=lambda c: c.M * c.N * c.K)


@pytest.mark.parametrize("mistake", gc.MISTAKES)
def test_check_catches_known_mistakes(mistake):
    """For every mistake there is a case whose ``check`` fails on the restatement with that mistake built in -- and it fails on every kind of
    route the mistake applies to that is tried here (the three cheapest cases of distinct routes)."""
    tried, seen = 0, set()
    for c in _candidates(mistake):
        if c.route in seen:
            continue
        seen.add(c.route)
        ok, worst, text = gc.check(gc.restate(c, "natural", mistake), c)
        assert not ok, f"{mistake} passed on {c}: {text}"
        tried += 1
        if tried == 3:
            break
    assert tried >= 1, f"no case for {mistake}"


def test_times_zero_pads_are_finite_and_unread_pads_are_nan():
    for route, pad in (("DGRAD_NARROW", "times_zero"), ("DGRAD_NARROW_BF16", "times_zero"), ("LAYER_N128", "unread"), ("TILED_128X128", "unread")):
        assert gc.ROUTES[route].pad == pad
        c = next(c for c in gc.cases() if c.route == route and c.lda > c.K and not c.a_trans)
        d = gc.inputs(c)
        padA = d["A"][:c.M, c.K:]
        assert padA.size and (np.all(padA == np.float32(gc.PAD_FINITE)) if pad == "times_zero" else np.all(np.isnan(padA)))
        assert np.all(np.isnan(d["A"][c.M:])) and d["A"].shape[0] == c.M + gc.ROUTES[route].T
        assert np.all(d["A"][:c.M, :c.K] != 0) and np.all(np.isfinite(d["A"][:c.M, :c.K]))


def test_masks_hold_the_special_values():
    c = next(c for c in gc.cases() if c.route == "LAYER_N128" and c.mask and c.M >= 64)
    m = gc.inputs(c)["mask"][:c.M, :c.N]
    assert np.any((m == 0) & ~np.signbit(m)) and np.any((m == 0) & np.signbit(m)) and np.any(np.isposinf(m))
    assert np.any((m > 0) & (m < 1e-38)) and np.any((m < 0) & (m > -1e-38)) and not np.any(np.isnan(m))
    c = next(c for c in gc.cases() if c.route == "LAYER_NB16" and c.mask)
    m = gc.inputs(c)["mask"][:c.M, :c.N]
    assert np.any((m > 0) & (m < 1e-38)) and np.any((m < 0) & (m > -1e-38)) and np.array_equal(gc.bf16r(m), m)
