"""The MLP-head case tables on the CPU (tests/head_cases.py; the GPU side is tests/test_gpu_head_cases.py): the tables name
every entry point of the family in include/clift.h, the tables reach every form the launchers distinguish (asserted from the dispatchers'
predicates restated in head_cases), the inputs meet the conditions the bound relies on, the references agree with torch in fp64, the
comparison of the GPU tests passes the fp32 restatement in all three orders and fails it with each of the known mistakes built in."""
import numpy as np
import pytest
import torch

import head_cases as hc
from head_cases import ILL_CONDITIONED, LF_ROWS, LN_ROWS, N6_ROWS, NS_ROWS, OF_ROWS, ORDERS, RESERVE, X6_ROWS, XW_ROWS

_G = hc.groups()


def _has(entry, **f):
    return any(all(getattr(c, k) == v for k, v in f.items()) for c in _G[entry])


def test_tables_and_pending_list_name_every_entry_point_of_the_header():
    names = hc.header_entry_points()
    assert len(names) == 25, sorted(names)
    assert hc.TABLE == names
    assert set(_G) == set(hc.ENTRIES) and all(_G[e] for e in hc.ENTRIES)
    assert hc.WIDENED == {}


def test_linear_k3_forms():
    fwd = _G["clift_linear_k3_fwd"]
    assert {c.Nout for c in fwd if hc.k3_fwd_kernel(c.Nout) == "main"} >= {4, 64, 256}
    assert {c.Nout for c in fwd if hc.k3_fwd_kernel(c.Nout) == "any"} >= {12, 1028}
    for Nout in (4, 64, 256, 12, 1028):
        assert {(c.relu, c.out_bf16) for c in fwd if c.Nout == Nout} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        T = hc.tile(next(c for c in fwd if c.Nout == Nout))
        assert {c.M for c in fwd if c.Nout == Nout} >= {1, max(T - 1, 1), T, T + 1, 2 * T + 1}
        assert any(c.ldo > c.Nout for c in fwd if c.Nout == Nout) and any(c.ldo == c.Nout for c in fwd if c.Nout == Nout)
    cap = [c for c in fwd if c.Nout == 4 and hc.cdiv(c.M, 256) > 2048]
    assert cap and all(c.M > 3 * 2048 * 256 for c in cap)        # the capped grid, and its four-rows-in-flight loop
    bwd = _G["clift_linear_k3_bwd"]
    route = lambda c: hc.k3_bwd_route(c.M, c.Nout, c.db, c.ldh, c.dh_bf16)
    plain, stream = [c for c in bwd if route(c) == "plain"], [c for c in bwd if route(c) == "stream"]
    assert {c.M % 32 for c in plain} >= {0, 1, 7, 8, 9, 31} and {33, 511, 512, 513} <= {c.M for c in plain}
    assert any(c.M < 4096 and c.Nout == 256 for c in plain) and any(c.M >= 4096 and not c.db for c in plain)
    assert any(c.Nout == 64 for c in plain) and any(c.Nout == 260 for c in plain)
    for bf in (0, 1):
        assert {c.M for c in stream if c.dh_bf16 == bf and not c.reserve} >= {4096, 4097, 4096 + NS_ROWS - 1}
        assert any(c.reserve == RESERVE and c.M == hc.m3_rows(NS_ROWS, first=4096) for c in stream if c.dh_bf16 == bf)
        assert any(c.dh_bf16 == bf for c in plain)


def test_wgrad_narrow_forms():
    wn = _G["clift_wgrad_narrow"]
    route = lambda c: hc.wgrad_narrow_route(c.M, c.no, c.ni, c.ldd, c.ldx, c.x_bf16)
    plain, stream = [c for c in wn if route(c)[0] == "plain"], [c for c in wn if route(c)[0] == "stream"]
    assert {c.no for c in plain} >= {1, 4, 5, 8, 9, 16, 22, 24, 25, 32} and {route(c)[1] for c in plain} == {4, 8, 16, 24, 32}
    assert {(c.ni, c.x_bf16) for c in plain} >= {(ni, bf) for ni in (3, 36, 256, 260, 515) for bf in (0, 1)}
    assert {c.M for c in plain} >= {1, 63, 64, 65, 71, 129} and any(not c.gb for c in plain) and any(not c.gb for c in stream)
    # both sides of every term of the stream predicate
    assert any(c.M == 4095 and c.ni == 256 for c in plain) and any(c.M == 4096 and c.ni == 256 and not c.x_bf16 for c in stream)
    assert any(c.M == 4096 and c.ni == 28 for c in plain) and any(c.M == 4096 and c.ni == 32 for c in stream)
    assert any(c.M == 4096 and c.ni == 34 for c in plain) and any(c.M == 4096 and c.ni == 128 and c.x_bf16 for c in plain)
    assert any(c.M == 4096 and c.ldd > 32 for c in plain) and any(c.x_bf16 and c.ni == 256 for c in stream)
    for bf in (0, 1):
        assert {c.M for c in stream if c.x_bf16 == bf and not c.reserve} >= {4096, 4097, 4096 + NS_ROWS - 1}
        assert any(c.reserve == RESERVE and c.M == hc.m3_rows(NS_ROWS, first=4096) for c in stream if c.x_bf16 == bf)


def test_colsum_rows_act_and_out_layer_forms():
    cs = _G["clift_colsum"]
    assert {c.N for c in cs} >= {1, 255, 256, 257} and {c.M for c in cs} >= {1, 255, 256, 257} and any(c.ld > c.N for c in cs)
    Cs = {1, 2, 3, 5, 22, 32, 33, 64}
    assert {(c.C, c.kind) for c in _G["clift_rows_act_fwd"]} == {(C_, k) for C_ in Cs for k in (1, 2)}
    assert {(c.C, c.kind) for c in _G["clift_rows_act_bwd"]} == {(C_, k) for C_ in Cs for k in (0, 1, 2)}
    for C_ in Cs:
        ldds = {c.ldd for c in _G["clift_rows_act_bwd"] if c.C == C_}
        assert C_ in ldds and (C_ == 64 or any(l > C_ and l % 4 == 0 for l in ldds))
    for c in _G["clift_rows_act_fwd"] + _G["clift_rows_act_bwd"]:
        lg = int(np.ceil(np.log2(max(getattr(c, "ldd", c.C), 1))))
        assert (c.M << lg) % 256 != 0
    of = _G["clift_out_layer_fwd"]
    for no in (1, 3, 4, 5, 22, 29, 32):
        mine = [c for c in of if c.no == no]
        assert {c.act for c in mine} == {0, 2} and {c.ldh for c in mine} == {256, 260} and {c.ldw for c in mine} == {256, 260}
        assert any(c.ldo == no for c in mine) and any(c.ldo > no for c in mine)
        assert {c.M for c in mine} >= {1, OF_ROWS - 1, OF_ROWS, OF_ROWS + 1, 2 * OF_ROWS + 1}
    assert {c.act for c in of if c.reserve == RESERVE and c.M == hc.m3_rows(OF_ROWS)} == {0, 2}


def test_out_layer_bwd_forms():
    ob, nh, nb = _G["clift_out_layer_bwd"], _G["clift_out_layer_bwd_nh"], _G["clift_out_layer_bwd_n128_bf16"]
    assert {hc.cdiv(c.no, 8) for c in ob} == {1, 2, 3, 4} and all(c.nh == 256 and not c.h_bf16 for c in ob)
    for no in (3, 9, 22, 29):
        assert {c.ldd for c in ob if c.no == no} >= {hc.r4(no), 32}
    assert {(c.nh, c.h_bf16) for c in nh} == {(32, 0), (128, 0), (256, 1)} and {c.ldd for c in nh if c.h_bf16} >= {24, 32}
    assert {c.no for c in nb} == {1, 3, 4} and {c.ldd for c in nb} == {4, 8} and all(c.nh == 128 and c.h_bf16 for c in nb)
    for mine, T, per_cu in ((ob, NS_ROWS, 1), (nh, NS_ROWS, 1), (nb, 16, 4)):
        assert {c.M for c in mine} >= {1, T - 1, T, T + 1, 2 * T + 1} and any(not c.gb for c in mine)
        assert any(c.reserve == RESERVE and c.M == hc.m3_rows(T, per_cu) for c in mine)
        for c in mine[:6]:                  # dOut's pad columns: zeros where the header demands them, NaN where it says "ignored"
            pad = hc.inputs(c)["dOut"][:c.M, c.no:]
            assert pad.size == 0 or (np.all(np.isnan(pad)) if hc.ob_kind(c)[2] == "nan" else np.all(pad == 0))
    c = next(c for c in nh if c.h_bf16 and c.M >= 65)
    H = hc.inputs(c)["H"][:c.M, :c.nh]
    assert np.any((H == 0) & ~np.signbit(H)) and np.any((H == 0) & np.signbit(H)) and np.any((H > 0) & (H < 1e-38)) and np.any((H < 0) & (H > -1e-38))
    assert not np.any(np.isnan(H)) and np.array_equal(hc.bf16r(H), H) and 0.3 <= np.mean(H > 0) <= 0.7


def test_fused_forward_forms():
    f2, x2, a2 = _G["clift_xyz_head_first2_fwd"], _G["clift_xyz_head_last2_fwd"], _G["clift_app_head_last2_fwd"]
    assert {c.h1 for c in f2} == {0, 1} and {c.ldh2 for c in f2} == {256, 264} and {c.ldh1 for c in f2 if c.h1} == {256, 264}
    assert {(c.E, c.hid) for c in x2} >= {(E, h) for E in (1, 2, 3, 4) for h in (0, 1)} and any(c.ldo > c.E for c in x2) and any(c.ldo == c.E for c in x2)
    assert {c.E for c in a2} == {1, 3, 4} and {(c.hid, c.pre, c.sigmoid) for c in a2} >= {(0, 0, 1), (1, 1, 1), (1, 0, 0), (0, 1, 0)}
    assert {c.lda for c in a2} == {128, 160} and {c.ldh for c in a2 if c.hid} == {128, 160}
    for mine, T in ((f2, LF_ROWS), (x2, LF_ROWS), (a2, LN_ROWS)):
        assert {c.M for c in mine} >= {1, T - 1, T, T + 1, 2 * T + 1}
        assert any(c.reserve == RESERVE and c.M == hc.m3_rows(T) for c in mine)
    for c in (next(c for c in x2 if c.M == 2 * LF_ROWS + 1 and c.hid), next(c for c in a2 if c.M == 2 * LN_ROWS + 1 and c.hid)):
        h = hc.reference(c)["hidden"][0][:c.M, :hc.l2_kind(c)[0]]
        assert 0.3 <= np.mean(h > 0) <= 0.7
    for c in a2:
        if c.sigmoid and c.M <= 200:          # (the M3 cases: test_inputs_meet_the_conditions... looks at every sigmoid output)
            o = hc.reference(c)["out"][0][:c.M, :c.E].astype(np.float32)
            assert np.all(o > 0) and np.all(o < 1), (c, "saturated")


def test_x6_forward_and_first2_backward_forms():
    """The fp32x6 forwards and the four backward ends of the first two layers: forms, row counts, and the dyadic first layer -- every
    pre-activation is exact in fp32 (so never within round-off of zero) and the hand-built units land on 0, on a tiny positive value and on -0."""
    f6, x6, a6 = _G["clift_xyz_head_first2_x6_fwd"], _G["clift_xyz_head_last2_x6_fwd"], _G["clift_app_head_last2_x6_fwd"]
    ab = _G["clift_app_head_last2_bf16_fwd"]
    assert {c.E for c in ab} == {1, 3, 4} and {(c.hid, c.sigmoid) for c in ab} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c.lda for c in ab} == {128, 160}
    assert {c.M for c in ab} >= {1, hc.NB_ROWS - 1, hc.NB_ROWS, hc.NB_ROWS + 1, 2 * hc.NB_ROWS + 1, hc.m3_rows(hc.NB_ROWS, 2)} and hc.m3_rows(hc.NB_ROWS, 2) <= 32769
    A = hc.inputs(ab[4])["A"]
    assert np.array_equal(hc.bf16r(A[:ab[4].M, :128]), A[:ab[4].M, :128]), "A is bf16-stored"
    assert {c.signs for c in f6} == {0, 1} and {c.ldh2 for c in f6} == {256, 264}
    assert {(c.E, c.hid) for c in x6} >= {(E, h) for E in (1, 2, 3, 4) for h in (0, 1)} and any(c.ldo > c.E for c in x6)
    assert {c.E for c in a6} == {1, 3, 4} and {(c.hid, c.sigmoid) for c in a6} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c.lda for c in a6} == {128, 160}
    for mine, T, big in ((f6, X6_ROWS, hc.m3_x6()), (x6, X6_ROWS, hc.m3_x6()), (a6, N6_ROWS, hc.m3_rows(N6_ROWS, 2)),
                         (_G["clift_xyz_head_first2_bwd"], LF_ROWS, hc.m3_rows(LF_ROWS)), (_G["clift_xyz_head_first2_x6_bwd"], X6_ROWS, hc.m3_x6()),
                         (_G["clift_xyz_head_first2_wgrad"], 64, hc.m3_fixed(64, 64)),
                         (_G["clift_xyz_head_first2_x6_wgrad"], XW_ROWS, hc.m3_fixed((hc.CUS - RESERVE) // 4, XW_ROWS))):
        assert {c.M for c in mine} >= {1, T - 1, T, T + 1, 2 * T + 1} and any(c.reserve == RESERVE and c.M == big for c in mine), mine[0].entry
        assert big <= 32769
    for entry in hc._FB + hc._FW:
        assert {c.ldd for c in _G[entry]} == {256, 260}
        assert entry in hc._FB or ({c.gb for c in _G[entry]} == {0, 1} and {c.ldg for c in _G[entry]} == {256, 264})
        for c in _G[entry][1:4]:
            d = hc.inputs(c)
            p32, p64 = hc.k3_pre(d, c.M), hc.k3_pre(d, c.M, np.float64)
            assert np.array_equal(p32.astype(np.float64), p64), (c, "the first layer's chain is not exact in fp32")
            x, W, b = np.abs(d["x4"][:c.M, :3].astype(np.float64)), np.abs(d["W0"][:, :3].astype(np.float64)), np.abs(d["b0"].astype(np.float64))
            largest = np.maximum(b[None, :], (x[:, :, None] * W.T[None, :, :]).max(1))
            away = np.abs(p64) > 16 * 2.0 ** -23 * largest
            assert np.all(away | (p64 == 0)), (c, "a pre-activation within 16 ulps of its largest term of zero")
            assert np.all(p32[:, 0] == 0) and p32[0, 1] == 0 and 0 < p32[0, 2] < 1e-17 and p32[0, 3] == 0 and np.signbit(p32[0, 3])
            assert 0.3 <= np.mean(p32[:, 4:] > 0) <= 0.7, (c, np.mean(p32[:, 4:] > 0))
    big = _G[hc._FB[0]][-1]                               # an M3 case: the draw itself lands on exact zeros outside the hand-built units
    assert np.any(hc.k3_pre(hc.inputs(big), big.M)[:, 4:] == 0)


def test_sign_byte_exclusions_stay_under_the_cap():
    """The elements the sign-byte comparison of clift_xyz_head_first2_x6_fwd leaves out -- reference pre-activation within its own bound of zero --
    are at most 0.1 % of a case, from the reference alone; nothing is redrawn to get there."""
    for c in (c for c in _G["clift_xyz_head_first2_x6_fwd"] if c.signs):
        unsure = hc.sign_unsure(c)
        assert unsure.mean() <= hc.SIGN_CAP, (c, int(unsure.sum()), unsure.size)


def test_bf16_chain_forms():
    bb, hb = _G["clift_xyz_head_first2_bf16_bwd"], _G["clift_xyz_head_bf16_fwd"]
    T = hc.LY_ROWS
    assert {c.M for c in bb} >= {1, T - 1, T, T + 1, 2 * T + 1, hc.gc.m3("LAYER_BF16", "dgrad_masked")} and {c.ldd for c in bb} == {256, 264} == {c.ldm for c in bb}
    m = hc.inputs(bb[4])["h1"][:bb[4].M, :256]
    assert np.any((m == 0) & ~np.signbit(m)) and np.any((m == 0) & np.signbit(m)) and np.any(np.isposinf(m)) and not np.any(np.isnan(m))
    assert np.any((m > 0) & (m < 1e-38)) and np.any((m < 0) & (m > -1e-38)) and np.array_equal(hc.bf16r(m), m)
    T = hc.HB_ROWS
    assert {c.E for c in hb} == {0, 1, 2, 3, 4} and all(c.h3 for c in hb if c.E == 0) and any(not c.bout for c in hb)
    assert {(c.h1, c.h2, c.h3) for c in hb if c.E} == {(a, b, c_) for a in (0, 1) for b in (0, 1) for c_ in (0, 1)}
    assert {c.M for c in hb} >= {1, T - 1, T, T + 1, 2 * T + 1, hc.m3_rows(T)}
    big = next(c for c in hb if c.p.get("probe"))
    assert big.M == 128 * 2048 + 64 + 1 and big.reserve == RESERVE and big.E == 3 and not (big.h1 or big.h2 or big.h3)
    rows = hc.inputs(big)["_rows"]
    rpb = hc.row_ranges(big.M, T, hc.CUS - RESERVE)[1]
    assert rpb > hc.HB_XROWS and {0, hc.HB_XROWS - 1, hc.HB_XROWS, rpb - 1, rpb, rpb + hc.HB_XROWS, big.M - 1} <= set(rows.tolist()) and (big.M % rpb) % T != 0


def test_m3_walks_three_tiles_and_ends_on_a_ragged_tile():
    for T, first, per_cu in ((NS_ROWS, 4096, 1), (OF_ROWS, 1, 1), (LN_ROWS, 1, 1), (16, 1, 4)):
        rows = hc.m3_rows(T, per_cu, first)
        blocks, rpb, grid = hc.row_ranges(rows, T, hc.CUS - RESERVE, per_cu)
        assert hc.cdiv(min(rpb, rows), T) >= 3 and (rows - (grid - 1) * rpb) % T != 0 and rows <= 32769
        if rows > first:
            prev = hc.row_ranges(rows - 1, T, hc.CUS - RESERVE, per_cu)[1]
            assert not (hc.cdiv(min(prev, rows - 1), T) >= 3 and (rows - 1 - (hc.cdiv(rows - 1, prev) - 1) * prev) % T != 0)


@pytest.mark.parametrize("entry", sorted(hc.ENTRIES))
def test_inputs_meet_the_conditions_and_plain_orders_pass(entry):
    """Contracted columns nonzero in both operands, rows of scale 2^+-6, operand pads and rows past the count NaN, gradients nonzero, ReLU
    layers 30 - 70 % active, no saturated sigmoid / softmax, yardsticks at most 1e-5 -- and ``check`` passes the fp32 restatement in each of
    the three orders (in the same walk over the cases: a case's inputs are drawn once)."""
    e = hc.ENTRIES[entry]
    for c in _G[entry]:
        if c.M > 100000 and entry != "clift_linear_k3_fwd":
            continue
        d = hc.inputs(c)
        assert max(hc.yardsticks(c).values()) <= ILL_CONDITIONED, c
        for order in ORDERS:
            ok, worst, _, text = hc.check(hc.restate(c, order), c)
            assert ok, (order, text)
        for name in e.streamed:
            x = d[name]
            assert np.all(np.isnan(x[c.M:])) and x.shape[0] > c.M and not np.any(np.isnan(x[:c.M, :1])), (c, name)
        for q, (r, S) in hc.reference(c).items():
            on = ~np.isnan(r)
            if not (entry == "clift_rows_act_bwd" and c.kind == 2 and c.C == 1):        # (the derivative of a softmax over one class is 0)
                assert on.any() and np.any(r[on] != 0), (c, q)
            assert np.all(np.isnan(r[-2:])), (c, q, "two rows past the output are held to the sentinel")
        lefts = {"clift_linear_k3_bwd": ("dH", c.p.get("Nout")), "clift_wgrad_narrow": ("dY", c.p.get("no")), "clift_colsum": ("dY", c.p.get("N")),
                 "clift_out_layer_fwd": ("H", 256), "clift_out_layer_bwd": ("dOut", c.p.get("no")), "clift_out_layer_bwd_nh": ("dOut", c.p.get("no")),
                 "clift_out_layer_bwd_n128_bf16": ("dOut", c.p.get("no")), "clift_xyz_head_last2_fwd": ("A", 256), "clift_app_head_last2_fwd": ("A", 128),
                 "clift_xyz_head_last2_x6_fwd": ("A", 256), "clift_app_head_last2_x6_fwd": ("A", 128), "clift_app_head_last2_bf16_fwd": ("A", 128),
                 "clift_xyz_head_first2_bwd": ("dH2", 256),
                 "clift_xyz_head_first2_x6_bwd": ("dH2", 256), "clift_xyz_head_first2_wgrad": ("dH2", 256), "clift_xyz_head_first2_x6_wgrad": ("dH2", 256)}
        if c.M >= 63 and entry in lefts:
            left = lefts[entry]
            x = d[left[0]][:c.M, :left[1]]
            assert np.all(np.any(x != 0, 0)), (c, "a contracted column is zero")
            scale = np.log2(np.abs(x).max(1) + 1e-300)
            assert scale.max() - scale.min() >= 6, (c, "rows do not differ in scale")
            if left[0] in ("dH", "dY", "A", "dH2") and d[left[0]].shape[1] > left[1]:
                assert np.all(np.isnan(d[left[0]][:c.M, left[1]:])), (c, "operand pad columns are NaN")
        if entry == "clift_linear_k3_fwd" and c.relu and c.M * c.Nout >= 256:
            r = hc.reference(c)["out"][0][:c.M, :c.Nout]
            assert 0.3 <= np.mean(r > 0) <= 0.7, (c, np.mean(r > 0))
        if entry == "clift_out_layer_fwd" and c.M >= 32:
            H = d["H"][:c.M, :256]
            assert 0.3 <= np.mean(H > 0) <= 0.7
        if c.p.get("sigmoid") and "E" in c.p:
            v = hc.reference(c)["out"][0][:c.M, :c.E].astype(np.float32)
            assert np.all(v > 0) and np.all(v < 1), (c, "saturated")
        if entry == "clift_rows_act_fwd" or (entry == "clift_out_layer_fwd" and c.act == 2):
            n = c.C if entry == "clift_rows_act_fwd" else c.no
            v = hc.reference(c)["out"][0][:c.M, :n].astype(np.float32)
            if n >= 3 or getattr(c, "kind", 2) == 1:         # (softmax over one class is 1 by construction; over two, the spread rows are not drawn)
                assert np.all(v > 0) and np.all(v < 1), (c, "saturated")
        if entry == "clift_rows_act_fwd" and c.kind == 2 and c.C >= 3 and c.M >= 6:
            x = d["pre"][:c.M, :c.C]
            assert np.any(x.max(1) - x.min(1) == hc.SPREAD) and np.any(x.max(1) == x.min(1)) and x.max() > 89


def test_references_agree_with_torch_fp64():
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    # (elementwise relative; the reductions are compared after their pre-fill is taken off again, so relative to the largest entry)
    close = lambda a, b, whole=False: float(np.max(np.abs(a - b.numpy()) / (np.abs(a).max() if whole else np.maximum(np.abs(a), 1e-300)))) <= 1e-12
    for entry in ("clift_linear_k3_fwd", "clift_linear_k3_bwd", "clift_wgrad_narrow", "clift_colsum", "clift_rows_act_fwd", "clift_rows_act_bwd",
                  "clift_out_layer_fwd", "clift_xyz_head_first2_fwd", "clift_xyz_head_first2_x6_fwd") + hc._L2 + hc._OB + hc._FB + hc._FW + (
                      "clift_xyz_head_first2_bf16_bwd", "clift_xyz_head_bf16_fwd"):
        for c in [c for c in _G[entry] if c.M <= 1100][-2:]:
            d = hc.inputs(c)
            ref = {q: r for q, (r, _) in hc.reference(c).items()}
            if entry == "clift_linear_k3_fwd":
                v = torch.nn.functional.linear(t(d["x4"][:c.M, :3]), t(d["W"][:, :3]), t(d["b"]))
                assert close(ref["out"][:c.M, :c.Nout], torch.relu(v) if c.relu else v)
            elif entry in ("clift_linear_k3_bwd", "clift_wgrad_narrow"):
                ln, rn, n, k, o, b = ("dH", "x4", c.p.get("Nout"), 3, "dW", "db") if entry == "clift_linear_k3_bwd" else ("dY", "X", c.p.get("no"), c.p.get("ni"), "gW", "gb")
                W = torch.zeros(n, k, dtype=torch.float64, requires_grad=True)
                bias = torch.zeros(n, dtype=torch.float64, requires_grad=True)
                (torch.nn.functional.linear(t(d[rn][:c.M, :k]), W, bias) * t(d[ln][:c.M, :n])).sum().backward()
                assert close(ref[o][:n, :k] - d[o][:n, :k], W.grad, True)
                if d[b] is not None:
                    assert close(ref[b][:n, 0] - d[b][:n, 0], bias.grad, True)
            elif entry == "clift_colsum":
                assert close(ref["db"][:c.N, 0] - d["db"][:c.N, 0], t(d["dY"][:c.M, :c.N]).sum(0), True)
            elif entry == "clift_rows_act_fwd":
                x = t(d["pre"][:c.M, :c.C])
                assert close(ref["out"][:c.M, :c.C], torch.sigmoid(x) if c.kind == 1 else torch.softmax(x, 1))
            elif entry == "clift_rows_act_bwd" and c.kind:
                # autograd through the activation at a pre-activation that gives exactly the stored `out` is not available; the derivative formulas
                # are checked on torch's own forward instead
                x = t(hc._logits(hc._rng(c.seed), c.M, c.C, c.kind)).requires_grad_(True)
                o = torch.sigmoid(x) if c.kind == 1 else torch.softmax(x, 1)
                g = t(d["dout"][:c.M, :c.C])
                (o * g).sum().backward()
                dd = dict(d, out=np.pad(o.detach().numpy(), ((0, 8), (0, c.ldo - c.C))))
                mine = hc._rab_ref(c, dd)["dpre"][0][:c.M, :c.C]
                assert float(np.max(np.abs(mine - x.grad.numpy()))) <= 1e-12 * float(g.abs().max())
            elif entry == "clift_out_layer_fwd":
                v = torch.nn.functional.linear(t(d["H"][:c.M, :256]), t(d["W"][:c.no, :256]), t(d["b"]))
                assert close(ref["out"][:c.M, :c.no], torch.softmax(v, 1) if c.act == 2 else v)
            elif entry in hc._OB:
                H = t(d["H"][:c.M, :c.nh]).requires_grad_(True)                 # dX: the gradient of sum(dOut . (relu(H) W^T)) with respect to H
                W = t(d["W"][:c.no, :c.nh]).requires_grad_(True)
                bias = torch.zeros(c.no, dtype=torch.float64, requires_grad=True)
                (torch.nn.functional.linear(torch.relu(H), W, bias) * t(d["dOut"][:c.M, :c.no])).sum().backward()
                assert close(ref["dX"][:c.M, :c.nh], H.grad, True)
                assert close(ref["gW"][:c.no, :c.nh] - d["gW"][:c.no, :c.nh], (t(d["dOut"][:c.M, :c.no]).T @ t(d["H"][:c.M, :c.nh])), True)
                if d["gb"] is not None:
                    assert close(ref["gb"][:c.no, 0] - d["gb"][:c.no, 0], bias.grad, True)
            elif entry == "clift_xyz_head_first2_bf16_bwd":
                dH1 = torch.where(t(d["h1"][:c.M, :256]) > 0, t(d["dH2"][:c.M, :256]) @ t(hc.bf16r(d["W1"][:, :256])), torch.zeros((), dtype=torch.float64))
                ch = t(hc.bf16r(dH1.numpy()))
                assert close(ref["gW0"][:256, :3] - d["gW0"][:256, :3], ch.T @ t(d["x4"][:c.M, :3]), True)
                assert close(ref["gb0"][:256, 0] - d["gb0"][:256, 0], ch.sum(0), True)
            elif entry == "clift_xyz_head_bf16_fwd":
                lin, rb = torch.nn.functional.linear, lambda v: t(hc.bf16r(v.numpy()))
                h = rb(torch.relu(lin(t(d["x4"][d["_rows"], :3]), t(d["W0"][:, :3]), t(d["b0"]))))
                for W, b in (("W1", "b1"), ("W2", "b2")):
                    h = rb(torch.relu(lin(h, t(hc.bf16r(d[W][:, :256])), t(d[b]))))
                if c.E:
                    o = lin(h, t(hc.bf16r(d["Wout"][:c.E, :256])), t(d["bout"]) if d["bout"] is not None else None)
                    assert close(ref["out"][:len(d["_rows"]), :c.E], o, True)
                if d["h3"] is not None:
                    assert float(np.max(np.abs(hc.bf16r(ref["h3"][:len(d["_rows"]), :256]) - h.numpy()))) == 0
            elif entry in ("clift_xyz_head_first2_fwd", "clift_xyz_head_first2_x6_fwd"):
                h1 = torch.relu(torch.nn.functional.linear(t(d["x4"][:c.M, :3]), t(d["W0"][:, :3]), t(d["b0"])))
                assert close(ref["h2"][:c.M, :256], torch.relu(torch.nn.functional.linear(h1, t(d["W1"][:, :256]), t(d["b1"]))), True)
            elif entry in hc._L2:
                n = hc.l2_kind(c)[0]
                bf = entry == "clift_app_head_last2_bf16_fwd"
                h = torch.relu(torch.nn.functional.linear(t(d["A"][:c.M, :n]), t(hc.bf16r(d["W"][:, :n]) if bf else d["W"][:, :n]), t(d["b"])))
                h = t(hc.bf16r(h.numpy())) if bf else h
                v = torch.nn.functional.linear(h, t(d["Wout"][:, :n]), t(d["bout"]))
                assert close(ref["out"][:c.M, :c.E], torch.sigmoid(v) if c.p.get("sigmoid") else v, True)
            elif entry in hc._FB + hc._FW:
                # autograd through the two layers with dH2 as the cotangent of the second layer's PRE-activation (dH2 is "already masked")
                W0, b0 = t(d["W0"][:, :3]).requires_grad_(True), t(d["b0"]).requires_grad_(True)
                W1 = (t(d["W1"][:, :256]) if entry in hc._FB else torch.zeros(256, 256, dtype=torch.float64)).requires_grad_(True)
                b1 = torch.zeros(256, dtype=torch.float64, requires_grad=True)
                h1 = torch.relu(torch.nn.functional.linear(t(d["x4"][:c.M, :3]), W0, b0))
                (torch.nn.functional.linear(h1, W1, b1) * t(d["dH2"][:c.M, :256])).sum().backward()
                pairs = (("gW0", W0.grad), ("gb0", b0.grad[:, None])) if entry in hc._FB else (("gW1", W1.grad), ("gb1", b1.grad[:, None]))
                for q, g in pairs:
                    if d[q] is not None:
                        assert close(ref[q][:256, :g.shape[1]] - d[q][:256, :g.shape[1]], g, True), (c, q)


def _candidates(mistake, entry):
    T = hc.tile
    want = {
        "x4_pad_contracted": lambda c: True,
        "mask_ge": lambda c: c.M >= 15,
        "mask_from_second_layer": lambda c: c.M >= 15,
        "first_layer_sign_without_b0": lambda c: c.M >= 15,
        "x6_middle_term_dropped": lambda c: c.M >= 15,
        "gb_from_masked_dout": lambda c: c.gb and c.M >= 15,
        "dout_pad_column_contracted": lambda c: c.ldd > c.no,
        "bout_of_column_0_for_all": lambda c: c.E > 1,
        "relu_missing_before_output_layer": lambda c: c.M >= 15,
        "hidden_stored_before_relu": lambda c: c.hid,
        "bf16_hidden_rounded_after_output_layer": lambda c: c.M >= 15,
        "last_m_mod_8_rows_dropped": lambda c: c.M % 8 and c.M > 8,
        "last_m_mod_64_rows_dropped": lambda c: c.M % 64 and c.M > 64,
        "ragged_tile_rows_from_previous_tile": lambda c: c.M > T(c) and c.M % T(c),
        "row_past_count_reduced": lambda c: True,
        "gb_missing_on_last_quad": lambda c: bool(c.p.get("gb", c.p.get("db", 1))) and c.M >= 8,
        "accumulate_overwrites": lambda c: True,
        "ni_tail_beyond_256_dropped": lambda c: c.ni > 256,
        "out_bias_added_per_column_group": lambda c: True,
        "column_group_share_dropped": lambda c: True,
        "columns_no_ldo_written": lambda c: c.ldo > c.p.get("no", c.p.get("E")),
        "sigmoid_of_minus_pre": lambda c: c.p.get("kind") == 1 or c.p.get("sigmoid"),
        "softmax_without_max": lambda c: c.kind == 2 and c.C >= 3,
        "softmax_pad_lanes_exp0": lambda c: c.kind == 2 and c.C % 4,
        "softmax_bwd_dot_over_c_minus_1": lambda c: c.kind == 2 and c.C >= 2,
        "identity_pad_columns_unwritten": lambda c: c.kind == 0 and c.ldd > c.C,
    }[mistake]
    one_class_softmax = lambda c: entry == "clift_out_layer_fwd" and c.act == 2 and c.no == 1        # 1.0 whatever the logit
    return sorted((c for c in _G[entry] if want(c) and not one_class_softmax(c)), key=lambda c: c.M)


@pytest.mark.parametrize("mistake", sorted(hc.MISTAKES))
def test_check_catches_known_mistakes(mistake):
    """Every mistake breaks the bound on the two cheapest cases of every entry point it applies to."""
    for entry in hc.MISTAKES[mistake]:
        tried = 0
        for c in _candidates(mistake, entry)[:2]:
            ok, worst, _, text = hc.check(hc.restate(c, "natural", mistake), c)
            assert not ok, f"{mistake} passed on {c}: {text}"
            tried += 1
        assert tried >= 1, f"no case of {entry} for {mistake}"


def test_mistakes_that_change_no_bit_by_construction():
    """The pad lanes of a softmax whose class count is a multiple of 4 do not exist, and an identity backward with ldd = C has no pad."""
    c = next(c for c in _G["clift_rows_act_fwd"] if c.kind == 2 and c.C == 32)
    assert np.array_equal(hc.restate(c, "natural", "softmax_pad_lanes_exp0")["out"], hc.restate(c)["out"])
    c = next(c for c in _G["clift_rows_act_bwd"] if c.kind == 0 and c.ldd == c.C)
    assert np.array_equal(hc.restate(c, "natural", "identity_pad_columns_unwritten")["dpre"], hc.restate(c)["dpre"])


def test_shard_fold_model_and_its_mistakes():
    """clift_grad_shards_fold restated: a gradient range whose per-XCD partials lie in eight shards; fold(first, n) completes [first, first + n),
    leaves the rest, clears exactly the folded part of the shards.  Each fold mistake breaks the plain bound."""
    rng = np.random.default_rng(5)
    R, first, n = 203, 5, 101
    parts = rng.standard_normal((8, R)).astype(np.float32)
    g0 = rng.standard_normal(R).astype(np.float32)
    ref = g0.astype(np.float64) + parts.astype(np.float64).sum(0)
    S = np.abs(g0.astype(np.float64)) + np.abs(parts.astype(np.float64)).sum(0)
    yard = 0.0

    def ok(g, sh):
        on = slice(first, first + n)
        inside = np.all(np.abs(g[on] - ref[on]) <= (8 * yard + 4 * hc.HALF_ULP) * S[on]) and np.all(sh[:, on] == 0)
        rest = np.ones(R, bool)
        rest[on] = False
        return bool(inside and np.array_equal(g[rest], g0[rest]) and np.array_equal(sh[:, rest], parts[:, rest]))

    g, sh = hc.shards_fold(g0, parts, first, n)
    yard = float(np.max(np.abs(g[first:first + n] - ref[first:first + n]) / S[first:first + n]))
    assert yard <= ILL_CONDITIONED and ok(g, sh)
    for m in hc.FOLD_MISTAKES:
        assert not ok(*hc.shards_fold(g0, parts, first, n, m)), m
    g, sh = hc.shards_fold(*hc.shards_fold(g, sh, 0, first), first + n, R - first - n)
    assert np.all(sh == 0) and np.all(np.abs(g - ref) <= (8 * yard + 4 * hc.HALF_ULP) * S)
