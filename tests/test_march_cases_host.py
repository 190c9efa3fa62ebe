"""What tests/march_cases.py promises, checked without a GPU: the conditions its inputs have to meet, every case well-conditioned, the table
lookup against torch's grid_sample, the prefix / suffix-sum forms of the distortion loss and of dsigma against the pairwise definition and
autograd, and the mistakes table: each known mistake, built into the fp32 restatement, breaks the bound on at least one case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import march_cases as mc

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------- conditions on the inputs
def test_samples_keep_off_the_box_faces_except_in_the_on_face_case():
    faced = 0
    for c in mc.march_cases():
        g = mc.geometry(c)
        if not c.on_face:
            assert mc.face_margin_ulps(c) > mc.FACE_ULPS, c
            continue
        faced += 1
        for r, (face, sign) in enumerate(((c.hi, 1.0), (c.lo, -1.0))):
            hit = g.p[r, :, 2] == face[2]
            assert hit.sum() == 1 and bool(g.mask[r][hit][0]), "the mask is inclusive on a face"
            assert float(g.xn[r][hit][0, 2]) == sign
        tz = mc._tap(g.xn[0, :, 2], c.res[2], None)
        k = int(np.nonzero(g.p[0, :, 2] == c.hi[2])[0][0])
        assert tz.w1[k] == 0.0 and tz.w0[k] == 1.0 and int(tz.i0[k]) == c.res[2] - 1, "at xn == 1 the far tap is out of range"
    assert faced == 1


def test_thresholds_sit_in_a_gap_of_the_weights():
    for c in mc.march_cases():
        g, w = mc.geometry(c), mc.reference(c)["w"].numpy()
        assert g.mask.mean() >= 0.25, c
        if c.only is None:
            assert mc.thres_margin(c) > 0.0, (c, mc.thres_margin(c))
        if c.S > 1:                                            # (S == 1: the only sample has delta = 0, every weight is 0)
            active = float((w > c.thres)[g.mask].mean())
            assert 0.2 <= active <= 0.8, (c, active)
        else:
            assert float(np.abs(w).max()) == 0.0
        n_act = mc.extras(c)["n_active"].numpy()
        assert (n_act == (w > np.float32(c.thres)).sum(1)).all()
        assert (w[~g.mask] == 0).all() and (mc.reference(c)["sigma"].numpy()[~g.mask] == 0).all()


def test_cases_cover_what_they_are_there_for():
    cases = mc.march_cases()
    seen = {"miss": 0, "inside": 0, "zero1": 0, "zero2": 0, "early": 0, "jitter": 0, "nojitter": 0, "untouched": 0}
    for c in cases:
        g, ex = mc.geometry(c), mc.extras(c)
        d = c.rays[:, 3:6]
        seen["miss"] += int((~g.mask.any(1)).sum())
        seen["inside"] += int((g.tmin == c.rays[:, 6]).sum())
        seen["zero1"] += int(((d == 0).sum(1) == 1).sum())
        seen["zero2"] += int(((d == 0).sum(1) == 2).sum())
        seen["early"] += int((g.mask[:, 0] & ~g.mask[:, -1]).sum()) if c.S > 1 else 0
        seen["jitter" if c.jitter is not None else "nojitter"] += 1
        for i in range(3):
            assert bool(ex[f"touched_p{i}"].any()) and bool(ex[f"touched_l{i}"].any()), (c, i)
            seen["untouched"] += int(not bool(ex[f"touched_p{i}"].all())) + int(not bool(ex[f"touched_l{i}"].all()))
        if c.S >= 2 * mc.DU_SEG and c.N > 1:
            assert (c.ds_in[1, mc.DU_SEG:2 * mc.DU_SEG] == 0).all(), "a whole chunk of zeros"
        if c.S >= 8:
            assert ((c.ds_in == 0) & g.mask).any() and ((c.ds_in != 0) & g.mask).any()
    assert all(v > 0 for v in seen.values()), seen
    by = {c.name: c for c in cases}
    x = mc.extras(by["softplus_span_N5_S64_C16"])["x"]
    assert float(x.max()) > 25.0 and float(x.min()) < -25.0 and bool(((x > 0) & (x < 20)).any())
    big = by["N2100_S65_C16_20x28x36"]           # more work items than 256 persistent blocks hold: 16 waves each, or 4 x 256 threads in groups
    assert big.N * -(-big.S // mc.DU_SEG) > 256 * 16 and big.N * -(-big.S // mc.DENS_SEG) > 256 * 4 * 256 // big.comps
    sat = by["saturated_N3_S33_C16"]
    assert bool((mc.reference(sat)["alpha"].float() == 1.0).any()) and sat.only == ("alpha", "T", "w")
    assert {c.S for c in cases} >= {1, 2, 4, 5, 31, 32, 33, 63, 64, 65, 129, 200} and {c.N for c in cases} >= {1, 3, 4, 5, 257}
    assert {c.S for c in cases if c.N == 257} >= {33, 64, 65, 129, 200}
    assert {c.comps for c in cases} == {4, 8, 16, 32, 64}


def test_every_branch_of_the_density_backward_dispatch_is_reached():
    got = {mc.density_bwd_branch(c, sw) for c in mc.march_cases() for sw in (False, True)}
    assert got == mc.ALL_BRANCHES, mc.ALL_BRANCHES - got
    for comps in (4, 8, 16):                                   # the wave walk meets each width with and without its LDS lines
        assert {mc.density_bwd_branch(c, False) for c in mc.march_cases() if c.comps == comps} == {("wave", True), ("wave", False)}, comps


def test_no_pooled_alpha_lies_within_its_bound_of_the_threshold():
    kinds = set()
    for c in mc.bbox_cases():
        pooled, box = mc.pool_box(mc.reference(c)["alpha"].numpy(), c.dims, c.thr)
        assert float(np.abs(pooled - c.thr).min()) > mc.bound_for(c, "alpha"), c
        kinds.add("none" if box[6] == 0 else "all" if box[6] == int(np.prod(c.dims)) else "some")
        if box[6] == 0:
            assert box == [0x7fffffff] * 3 + [-1] * 3 + [0]
    assert kinds == {"none", "all", "some"}
    assert any(1 in c.dims for c in mc.bbox_cases()) and any(2 in c.dims for c in mc.bbox_cases())


# ---------------------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("kernel", ["march", "points", "bbox", "fold"])
def test_every_case_is_well_conditioned(kernel):
    for c in mc.CASES[kernel]():
        ref = mc.reference(c)
        for q in mc.checked(c):
            assert mc.yardstick(c, q) <= mc.ILL_CONDITIONED * mc.scale_of(ref[q]), (c, q, mc.yardstick(c, q), mc.scale_of(ref[q]))


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def _grid_sample_feature(c, xn, planes, lines):
    """TensoRF's density feature with torch's own sampler: planes as (1, C, H, W), lines as (1, C, R, 1), fp64."""
    x = torch.from_numpy(xn).to(F64)
    feat = 0
    for i, (a, b, v) in enumerate(mc.AXES):
        grid = torch.stack([x[:, a], x[:, b]], 1).reshape(1, -1, 1, 2)
        lgrid = torch.stack([torch.zeros_like(x[:, v]), x[:, v]], 1).reshape(1, -1, 1, 2)
        P = F.grid_sample(planes[i].permute(2, 0, 1)[None], grid, mode="bilinear", align_corners=True, padding_mode="zeros")
        L = F.grid_sample(lines[i].permute(1, 0)[None, :, :, None], lgrid, mode="bilinear", align_corners=True, padding_mode="zeros")
        feat = feat + (P * L).sum(1).reshape(-1)
    return feat


def test_lookup_and_its_gradients_agree_with_grid_sample():
    cases = [c for c in mc.march_cases() if c.N <= 5] + list(mc.points_cases())
    for c in cases:
        xn = mc.geometry(c).xn.reshape(-1, 3) if c.kernel == "march" else c.xn
        cot = torch.from_numpy(np.random.default_rng(5).standard_normal(xn.shape[0]))
        out = []
        for fn in ("ours", "torch"):
            planes, lines = mc._tables(c, F64, True)
            feat = mc._lookup(c, xn, planes, lines, F64, "natural", mc.INDEX_FP64)[0] if fn == "ours" else _grid_sample_feature(c, xn, planes, lines)
            out.append([feat.detach()] + list(torch.autograd.grad((feat * cot).sum(), planes + lines)))
        for a, b in zip(*out):
            assert _rel(a, b) <= 1e-12, (c, _rel(a, b))
        if c.kernel == "points" and c.n > 1:
            assert bool((np.abs(c.xn) > 1).any()), "zero padding is exercised"


def test_prefix_sum_forms_equal_the_pairwise_definition_and_autograd():
    for c in mc.march_cases():
        if c.N > 5 and c.S > 70:
            continue
        ref = mc._eval_march(c, F64, "natural", None, manual=False)
        man = mc._eval_march(c, F64, "natural", None, manual=True)
        assert float((man["dist"] - ref["dist"]).abs().max()) <= 1e-12 * max(float(ref["dist"].abs().max()), 1e-30), c
        assert float((man["dsigma"] - ref["dsigma"]).abs().max()) <= 1e-11 * max(float(ref["dsigma"].abs().max()), 1e-30), c


# ---------------------------------------------------------------------------------------------------------------- the bound has teeth
def _breaks(c, mistake):
    if c.kernel == "scan":
        good, bad = mc.scan_reference(c.cnt), mc.scan_reference(c.cnt, mistake=mistake)
        return not np.array_equal(good[0], bad[0])
    if c.kernel == "compact":
        good, bad = mc.compact_reference(c), mc.compact_reference(c, mistake=mistake)
        return not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    r, ref = mc.restate(c, "natural", mistake), mc.reference(c)
    return any(mc.exceeds(mc.max_error(r[q], ref[q]), mc.bound_for(c, q)) for q in mc.checked(c))


@pytest.mark.parametrize("kernel,mistake", [(k, m) for k, ms in mc.MISTAKES.items() for m in ms])
def test_bounds_catch_known_mistakes(kernel, mistake):
    cases = [c for c in mc.CASES[kernel]() if not (kernel == "march" and c.N > 5 and mistake not in ("T_restart_64",))]
    assert any(_breaks(c, mistake) for c in cases), f"{kernel}: no case notices {mistake}"


def test_the_mistakes_table_is_complete():
    assert len({m for ms in mc.MISTAKES.values() for m in ms}) >= 25
    for c in mc.CASES["march"]():                              # and without a mistake the restatement is inside the bound
        if c.N <= 5:
            assert not _breaks(c, None), c


def test_the_last_midpoint_cannot_show():
    """delta = 0 on the last sample makes alpha and w exactly 0 there: the last midpoint is multiplied by zero in every sum, and the last
    dsigma carries the factor delta.  Taking z_{S-1} for it changes no output by a single bit."""
    for c in mc.march_cases():
        if c.N > 5:
            continue
        a = mc._eval_march(c, F64, "natural", None, manual=True)
        b = mc._eval_march(c, F64, "natural", "last_mid_z_last", manual=True)
        for q in mc.MARCH_QUANTITIES:
            assert torch.equal(a[q], b[q]), (c, q)
