"""What tests/heads_io_cases.py promises, checked without a GPU: the references themselves (the lookup and its gradients against torch's
grid_sample, the encode column map against a literal restatement of the reference implementation, the explicit backward forms and the
activation formulas against autograd), the conditions on the inputs, that the cases reach every launch path of clift_app_gather_bwd and both
sample forms of clift_composite_bwd_act, and the mistakes table: each known mistake, built into the fp32 restatement, breaks the bound on at
least one case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import heads_io_cases as hc
import march_cases as mc

F64 = torch.float64
SMALL = 400              # rows up to which a case takes part in the fp64 cross-checks and the mistakes table


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) if b.numel() else 0.0


def _small(kernel):
    return [c for c in hc.CASES[kernel]() if kernel == "composite" or getattr(c, "M", getattr(c, "n", 0)) <= SMALL]


# ---------------------------------------------------------------------------------------------------------------- conditions on the inputs
def test_ray_derived_samples_keep_off_the_box_faces():
    n = 0
    for kernel in ("scatter", "gather", "front"):
        for c in hc.CASES[kernel]():
            if c.ray_derived:
                assert mc.face_margin_ulps(c) > mc.FACE_ULPS, c
                g = mc.geometry(c)
                assert bool(g.mask.reshape(-1)[c.act].all()) and bool((np.diff(c.act) > 0).all()), c
                assert np.array_equal(c.xn, g.xn.reshape(-1, 3)[c.act])
                n += 1
    assert n >= 30


def test_active_lists_have_runs_and_jumps():
    for c in hc.scatter_cases():
        if c.ray_derived and c.M >= 31:
            step = np.diff(c.act)
            same_ray = (c.act[1:] // c.S) == (c.act[:-1] // c.S)
            assert (step == 1).any() and (~same_ray).any() and ((step > 1) & same_ray).any(), c


def test_explicit_positions_sit_on_nodes_and_faces_and_step_one_texel_at_a_time():
    cases = [c for c in hc.scatter_cases() if not c.ray_derived]
    assert {c.comps for c in cases} == {16, 72}
    for c in cases:
        taps = [mc._tap(c.xn[:, a], c.res[a], None) for a in range(3)]
        for a in range(3):                                         # the fp32 tap position IS the texel position the case was built from
            fpos = ((c.xn[:, a] + np.float32(1.0)) / np.float32(2.0)) * np.float32(c.res[a] - 1)
            assert np.array_equal(fpos[:c.n_exact].astype(np.float64), c.texel_pos[:c.n_exact, a]), (c, a)
            assert (c.xn[:, a] == -1.0).any() and (c.xn[:, a] == 1.0).any(), "on both faces"
            t = taps[a]
            on_node = (t.w1 == 0.0) & (t.w0 == 1.0)
            assert on_node.any() and ((t.w0 > 0) & (t.w1 > 0)).any()
            top = c.xn[:, a] == 1.0
            assert (t.i0.numpy()[top] == c.res[a] - 1).all() and (t.w1[top] == 0.0).all(), "at +1 the far tap is out of range and weighs 0"
        dx, dy = np.diff(taps[0].i0.numpy()[:8]), np.diff(taps[1].i0.numpy()[:8])
        moves = set(zip(dx.tolist(), dy.tolist()))
        assert {(1, 0), (0, 1), (1, 1), (-1, -1), (-1, 0), (0, -1)} <= moves, moves
        assert (np.abs(c.xn) <= 1.0).all()


def test_row_counts_cover_the_segment_edges():
    ms = {c.M for c in hc.scatter_cases()}
    assert ms >= {1, 3, 31, 32, 33}
    assert {m % hc.AU_SEG for m in ms if m > hc.AU_SEG} >= {1, 2, 3, 5} and {m % hc.APP_SEG for m in ms if m > hc.APP_SEG} >= {1, 2, 3, 5}
    assert {c.comps for c in hc.scatter_cases()} == {4, 16, 48, 64, 72}
    assert {c.comps for c in hc.gather_cases()} == {4, 16, 48} and {c.jitter is None for c in hc.gather_cases()} == {True, False}
    assert any(c.n == 1 for c in hc.points_cases()) and all(c.ldx >= 3 for c in hc.points_cases()) and any(c.ldx > 3 for c in hc.points_cases())
    assert all(bool((np.abs(c.xn) > 1).any()) for c in hc.points_cases() if c.n > 1), "zero padding is exercised"
    assert {(c.nf, c.pef, c.pev) for c in hc.encode_cases()} == {(1, 1, 1), (27, 2, 2), (28, 2, 2), (5, 4, 3)}
    assert {c.M for c in hc.encode_cases() if c.dirs is None} == {1, 255, 257}
    assert any(c.ldx == c.width for c in hc.encode_cases()) and any(c.ldx > c.width for c in hc.encode_cases())
    assert any(c.ldf > c.nf for c in hc.encode_cases()) and any(c.lddf > c.nf for c in hc.encode_cases())
    assert any(c.dirs is not None and c.dirs.shape[1] > 3 for c in hc.encode_cases())
    fr = hc.front_cases()
    assert {c.comps for c in fr} == {16, 32, 48} and {c.M for c in fr} == {1, 63, 64, 65, 128, 64 * 1024 + 3} and {c.nf for c in fr} >= {1, 27, 28}
    assert {(c.want_F, c.want_xa) for c in fr} == {(True, True), (True, False), (False, True), (False, False)}
    assert all(c.ldb > 3 * c.comps and np.isnan(c.Wb[:, 3 * c.comps:]).all() and np.isnan(c.Wb[c.nf:]).all() for c in fr)


def test_scatter_cases_leave_texels_untouched_and_no_gradient_is_zero():
    for c in hc.scatter_cases():
        ref, tch = hc.reference(c), hc.touched(c)
        total = sum(t.numel() for t in tch.values())
        free = sum(int((~t).sum()) for t in tch.values())
        assert free >= 0.25 * total, (c, free / total)
        for q in hc.GRADS:
            assert bool(tch[q].any()), (c, q)
            assert float((ref[q] - torch.from_numpy(dict(zip(hc.GRADS, list(c.prefill_plane) + list(c.prefill_line)))[q]).to(F64)).abs().max()) > 0
        assert not np.isnan(c.dF[:c.M]).any() and (c.cap == c.M or np.isnan(c.dF[c.M:]).all())
    assert sum(c.cap > c.M for c in hc.scatter_cases()) == 2


def test_every_checked_gradient_is_nonzero():
    for c in hc.encode_cases():
        assert float(hc.reference(c)["dfeat"].abs().max()) > 0, c
    for c in hc.composite_cases():
        ref = hc.reference(c)
        if c.M == 0:
            continue
        for q, given in (("d_rgb", c.g_rgb is not None), ("d_sem", c.g_sem is not None and c.C > 0), ("d_inst", c.g_inst is not None and c.D > 0)):
            assert (hc.scale_of(ref[q]) > 0) == given, (c, q)
        assert float(ref["g_w"].abs().max()) > 0 or (c.g_rgb is None and c.stop_grad), c


def test_composite_cases_cover_the_list():
    cases = hc.composite_cases()
    assert {c.N for c in cases} == {1, 255, 257}
    counts = set()
    for c in cases:
        counts |= set(np.diff(c.start).tolist())
        assert c.start[-1] == c.M and c.ld_rgb >= 3 and c.ld_sem >= c.C and c.ld_inst >= c.E and 2 * c.E >= c.D
        if c.softmax_mode and c.C > 0:                            # no softmax-mode ray with samples has a class sum below 1e-3
            has = np.diff(c.start) > 0
            assert float(c.sem_raw_in.sum(1)[has].min() if has.any() else 1.0) >= 1e-3, c
        raw = c.rgb_raw_in.reshape(-1)
        if c.N > 1:
            assert (raw == 0).any() and (raw == 1).any() and (raw < 0).any() and (raw > 1).any()
    assert counts >= {0, 1, 7, 8, 9, 17}
    assert any(c.empty and c.M == 0 for c in cases)
    forms = {}
    for c in cases:
        forms.setdefault(hc.composite_form(c.C, c.D, c.ld_sem), []).append(c)
    assert set(forms) == {"lanes16", "scalar"}
    assert {(c.C, c.D) for c in forms["lanes16"]} >= {(0, 0), (1, 3), (5, 6), (22, 6), (48, 8)}
    assert {(c.C, c.D, c.E) for c in forms["scalar"]} >= {(49, 6, 3), (22, 10, 5)} and any(c.ld_sem == 52 and c.C <= 48 and c.D <= 8 for c in forms["scalar"])
    for form, cs in forms.items():
        assert any(c.E < c.D < 2 * c.E for c in cs) and any(c.D < c.E for c in cs), form
        assert {(c.softmax_mode, c.white_bg, c.stop_grad) for c in cs} >= {(a, b, s) for a in (0, 1) for b in (0, 1) for s in (0, 1)} or form == "scalar"
        assert {c.sem_kind for c in cs} == {0, 2}
    assert {(c.softmax_mode, c.white_bg, c.stop_grad) for c in cases} == {(a, b, s) for a in (0, 1) for b in (0, 1) for s in (0, 1)}
    assert {c.softmax_mode for c in forms["scalar"]} == {0, 1} and {c.stop_grad for c in forms["scalar"]} == {0, 1}
    assert any(c.ld_sem > c.C for c in cases) and any(c.ld_inst > c.E for c in cases) and all(c.ld_rgb > 3 for c in cases)


def test_every_launch_path_of_the_scatter_is_reached():
    cases = hc.scatter_cases()
    with_xa = {hc.gather_bwd_branch(c.comps, c.res, True) for c in cases}
    without = {hc.gather_bwd_branch(c.comps, c.res, False) for c in cases if c.ray_derived}
    assert with_xa | without == hc.ALL_BRANCHES
    assert {b for b in with_xa if b[0] == "wave"} == {("wave", 3), ("wave", 2), ("wave", 1), ("wave", 0)}
    assert without == {("lane", 256), ("lane", 512), ("lane", 1024), ("lane", 0)}
    assert any(c.comps > 64 and hc.gather_bwd_branch(c.comps, c.res, True)[0] == "lane" for c in cases), "the lane walk with xa"
    trips = [c for c in cases if c.second_trip]
    assert {hc.gather_bwd_branch(c.comps, c.res, True) for c in trips} == {("wave", 3), ("wave", 1), ("lane", 512)}
    for c in trips:
        assert c.M > hc.gather_bwd_rows_per_trip(c.comps, c.res, True, 256 - hc.RESERVE), c
    # the thresholds the dispatcher's formulas give at comps = 16: the longest axis that still fits each tier
    edges = [max(r for r in range(1, 4000) if hc.gather_bwd_branch(16, (r, 5, 6), True) == ("wave", b)) for b in (3, 2, 1)]
    assert edges == [589, 888, 2040]
    assert hc.gather_bwd_rows_per_trip(16, (20, 28, 36), True, 128) == 32768 and hc.gather_bwd_rows_per_trip(16, (2000, 5, 6), True, 128) == 21504


def test_every_entry_point_of_heads_io_is_called_by_the_gpu_test():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "contrastive_lift_amd", "csrc", "heads_io.hip")).read()
    gpu = open(os.path.join(root, "tests", "test_gpu_heads_io.py")).read()
    entries = set(re.findall(r'extern "C" int (clift_\w+)\(', src))
    assert len(entries) == 12 and {"clift_app_gather_bwd", "clift_composite_bwd_act", "clift_app_front_fwd_x"} <= entries
    for name in entries:
        assert f'L.call("{name}"' in gpu, name


# ---------------------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("kernel", list(hc.CASES))
def test_every_case_is_well_conditioned(kernel):
    for c in hc.CASES[kernel]():
        ref = hc.reference(c)
        for q in hc.checked(c):
            assert hc.yardstick(c, q) <= hc.ILL_CONDITIONED * hc.scale_of(ref[q]), (c, q, hc.yardstick(c, q), hc.scale_of(ref[q]))


# ---------------------------------------------------------------------------------------------------------------- the references themselves
def _grid_sample_products(c, xn, planes, lines):
    """The appearance products with torch's own sampler: planes as (1, C, H, W), lines as (1, C, R, 1), fp64."""
    x = torch.from_numpy(xn).to(F64)
    out = []
    for i, (a, b, v) in enumerate(mc.AXES):
        grid = torch.stack([x[:, a], x[:, b]], 1).reshape(1, -1, 1, 2)
        lgrid = torch.stack([torch.zeros_like(x[:, v]), x[:, v]], 1).reshape(1, -1, 1, 2)
        P = F.grid_sample(planes[i].permute(2, 0, 1)[None], grid, mode="bilinear", align_corners=True, padding_mode="zeros")
        L = F.grid_sample(lines[i].permute(1, 0)[None, :, :, None], lgrid, mode="bilinear", align_corners=True, padding_mode="zeros")
        out.append((P * L)[0, :, :, 0].permute(1, 0))
    return torch.cat(out, 1)


def test_products_and_their_gradients_agree_with_grid_sample():
    for c in _small("scatter") + list(hc.points_cases()):
        n = c.xn.shape[0]
        cot = torch.from_numpy(np.random.default_rng(5).standard_normal((n, 3 * c.comps)))
        res = []
        for fn in ("ours", "torch"):
            planes, lines = mc._tables(c, F64, True)
            if fn == "ours":
                _, Ps, Ls, _ = mc._lookup(c, c.xn, planes, lines, F64, "natural", mc.INDEX_FP64)
                Fp = torch.cat([Ps[i] * Ls[i] for i in range(3)], 1)
            else:
                Fp = _grid_sample_products(c, c.xn, planes, lines)
            res.append([Fp.detach()] + list(torch.autograd.grad((Fp * cot).sum(), planes + lines)))
        for a, b in zip(*res):
            assert _rel(a, b) <= 1e-12, (c, _rel(a, b))


def test_explicit_scatter_form_equals_autograd():
    for c in _small("scatter"):
        a, m = hc._eval_scatter(c, F64, "natural", None, manual=False), hc._eval_scatter(c, F64, "natural", None, manual=True)
        for q in hc.GRADS:
            assert _rel(m[q], a[q]) <= 1e-12, (c, q)
            assert torch.equal(m["touched_" + q], a["touched_" + q]), (c, q)


def test_encode_column_map_is_the_reference_implementation_s():
    for c in hc.encode_cases():
        feat, dirs = mc._t(c.feat[:c.M, :c.nf], F64), hc._dirs_of(c, F64, None)
        assert torch.equal(hc.encode_row(feat, dirs, c.pef, c.pev, F64), hc.literal_encode(feat, dirs, c.pef, c.pev)), c
        assert hc.reference(c)["X"].shape == (c.M, c.width)
        m = hc._eval_encode(c, F64, "natural", None, manual=True)
        assert _rel(m["dfeat"], hc.reference(c)["dfeat"]) <= 1e-12, c
        if c.pef == 1 and c.pev == 1:                               # the invisible mistake: no bit changes
            assert torch.equal(hc._eval_encode(c, F64, "natural", "pe_p_major")["X"], hc.reference(c)["X"])


def test_front_end_is_gather_then_basis_then_encode():
    for c in _small("front"):
        ref = hc.reference(c)
        assert _rel(ref["feat"], ref["F"] @ mc._t(c.Wb[:c.nf, :3 * c.comps], F64).T) <= 1e-13, c
        assert torch.equal(ref["X"], hc.literal_encode(ref["feat"], hc._dirs_of(c, F64, None), c.pef, c.pev)), c


def test_compositing_backward_forms_equal_autograd():
    for c in hc.composite_cases():
        a, m = hc._eval_composite(c, F64, "natural", None, manual=False), hc._eval_composite(c, F64, "natural", None, manual=True)
        for q in a:
            assert _rel(m[q], a[q]) <= 1e-12, (c, q, _rel(m[q], a[q]))
        # the forward against a plain loop over the rays
        ref = hc.reference(c)
        w = c.w.reshape(-1).astype(np.float64)
        for r in range(0, c.N, 37):
            sl = slice(int(c.start[r]), int(c.start[r + 1]))
            raw = (w[c.act[sl]][:, None] * c.rgb_s[sl].astype(np.float64)).sum(0) + ((1.0 - float(c.ray_out[r, 0])) if c.white_bg else 0.0)
            assert np.allclose(ref["rgb_raw"][r].numpy(), raw, rtol=0, atol=1e-14)
            assert np.array_equal(ref["rgb_map"][r].numpy(), np.clip(ref["rgb_raw"][r].numpy(), 0.0, 1.0))
            s = (w[c.act[sl]][:, None] * c.sem_s[sl].astype(np.float64)).sum(0)
            want = np.log(s / (s.sum() + 1e-8) + 1e-8) if (c.softmax_mode and c.C) else s
            assert np.allclose(ref["sem_map"][r].numpy(), want, rtol=0, atol=1e-13)


def test_activation_formulas_equal_autograd_through_sigmoid_and_softmax():
    seen = set()
    for c in hc.composite_cases():
        if c.M == 0:
            continue
        ref, chk = hc.reference(c), hc.activation_check(c)
        assert _rel(chk["o_rgb"], mc._t(c.rgb_s, F64)) <= 1e-12
        assert _rel(ref["dpre_rgb"], chk["dpre_rgb"]) <= 1e-12, c
        if c.sem_kind == 2:
            assert _rel(chk["dpre_sem_formula"], chk["dpre_sem"]) <= 1e-12, c
            assert _rel(ref["dpre_sem"], chk["dpre_sem"]) <= 1e-6, c        # (the case's fp32 rows sum to 1 within an ulp or two)
        else:
            assert torch.equal(ref["dpre_sem"], ref["d_sem"])
        E, D = c.E, c.D
        assert ref["dpre_i0"].shape[1] == E and ref["dpre_i1"].shape[1] == E
        assert torch.equal(ref["dpre_i0"][:, :min(D, E)], ref["d_inst"][:, :min(D, E)]) and float(ref["dpre_i0"][:, min(D, E):].abs().sum()) == 0.0
        n1 = max(min(D, 2 * E) - E, 0)
        assert torch.equal(ref["dpre_i1"][:, :n1], ref["d_inst"][:, E:E + n1]) and float(ref["dpre_i1"][:, n1:].abs().sum()) == 0.0
        seen.add(c.sem_kind)
    assert seen == {0, 2}


# ---------------------------------------------------------------------------------------------------------------- the bound has teeth
def _breaks(c, mistake):
    r, ref = hc.restate(c, "natural", mistake), hc.reference(c)
    return any(hc.exceeds(hc.max_error(r[q], ref[q]), hc.bound_for(c, q)) for q in hc.checked(c))


@pytest.mark.parametrize("kernel,mistake", [(k, m) for k, ms in hc.MISTAKES.items() for m in ms])
def test_bounds_catch_known_mistakes(kernel, mistake):
    assert any(_breaks(c, mistake) for c in _small(kernel)), f"{kernel}: no case notices {mistake}"


def test_the_mistakes_table_is_complete():
    assert len({m for ms in hc.MISTAKES.values() for m in ms}) >= 26
    for kernel in hc.CASES:                                        # and without a mistake the restatement is inside the bound
        for c in _small(kernel):
            assert not _breaks(c, None), c
