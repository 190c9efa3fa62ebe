"""What tests/meanshift_cases.py promises, checked without a GPU: the cases cover what they are there for, they do not hang on the order of a
sum or on the last bit of a square root, and the mistakes table: each known mistake, built into ``ordered_shift``, changes a centre bit, a
count or an iteration number on at least one case."""
import numpy as np
import pytest

import meanshift_cases as mc

f32, f64 = np.float32, np.float64


def _dist2(c, m):
    d2 = np.zeros(c.n, f64)
    for k in range(c.d):
        t = c.points[:, k].astype(f64) - f64(m[k])
        d2 = d2 + t * t
    return d2


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_widths_point_counts_and_strides():
    cases = mc.cases()
    assert {c.d for c in cases} >= {1, 2, 3, 4, 5, 8, 9, 16, 17, 32}
    assert {c.n for c in cases} >= {1, 63, 64, 255, 256, 257, 1000}
    assert max(c.n for c in cases) == 1000 and max(c.ldx for c in cases) == 32
    for group in (3, 4, 8, 16, 32):
        mine = [c for c in cases if mc.width_group(c.d) == group]
        assert len(mine) >= 2, group                                         # every instantiation runs in at least two cases
        assert any(c.ldx == c.d + 3 for c in mine) and any(c.ldx == c.d for c in mine), group
    for c in cases:
        assert 1 <= c.S <= 12 and c.why
        assert np.isnan(c.X[:, c.d:]).all() and c.X[:, c.d:].size == c.n * (c.ldx - c.d)


def test_every_width_group_has_a_real_climb():
    """A seed with at least 4 completed iterations whose neighbour count changes between steps, stopped by the norm."""
    for group in (3, 4, 8, 16, 32):
        found = 0
        for c in mc.cases():
            if mc.width_group(c.d) != group:
                continue
            _, _, iters, trace = mc.reference(c.name)
            climbs = [s for s, rec in enumerate(trace) if iters[s] >= 4 and len(set(rec["counts"])) >= 3 and rec["end"] == "norm"]
            assert bool(climbs) or not c.climb, c
            found += len(climbs)
        assert found >= 1, group


def test_seed_kinds():
    kinds = {"empty": 0, "lone": 0, "shared": 0}
    for c in mc.cases():
        centers, counts, iters, trace = mc.reference(c.name)
        for s, rec in enumerate(trace):
            assert len(rec["counts"]) == len(rec["norms"]) + (rec["end"] == "empty")
            if rec["counts"] == [0]:                                          # no neighbour at the first step: the seed comes back
                assert counts[s] == 0 and iters[s] == 0 and np.array_equal(centers[s].view(np.int32), c.seeds[s].view(np.int32))
                kinds["empty"] += 1
            on_point = (c.points == c.seeds[s]).all(1)
            if rec["counts"] == [1] and on_point.sum() == 1:                   # a data point alone in its ball
                assert counts[s] == 1 and iters[s] == 0 and rec["nb"][on_point].all() and rec["norms"][0] == 0
                assert np.array_equal(centers[s].view(np.int32), c.seeds[s].view(np.int32))
                kinds["lone"] += 1
        groups = mc.shared_sets(c.name)
        assert bool(groups) or not c.shared, c
        for g in groups:
            kinds["shared"] += 1
            assert all(np.array_equal(centers[g[0]].view(np.int32), centers[s].view(np.int32)) and counts[s] == counts[g[0]] for s in g)
            assert len({c.seeds[s].tobytes() for s in g}) == len(g), "the seeds of a group start at different places"
    assert kinds["empty"] >= 10 and kinds["lone"] >= 10 and kinds["shared"] >= 10, kinds


def test_max_iter_values_and_both_ways_to_stop():
    assert {c.max_iter for c in mc.cases()} == {0, 1, 2, 300}
    for limit in (0, 1, 2):
        ends = set()
        for c in mc.cases():
            if c.max_iter != limit:
                continue
            _, _, iters, trace = mc.reference(c.name)
            assert iters.max() <= limit
            for s, rec in enumerate(trace):
                ends.add(rec["end"])
                if rec["end"] == "max_iter":
                    assert iters[s] == limit and len(rec["norms"]) == limit + 1 and f64(rec["norms"][-1]) > 1e-3 * c.bandwidth
        assert ends >= {"max_iter", "norm"}, (limit, ends)
    for c in mc.cases():
        if c.max_iter == 300:
            _, _, iters, trace = mc.reference(c.name)
            assert iters.max() < 300 and all(rec["end"] != "max_iter" for rec in trace), c


def test_boundary_points_sit_exactly_on_the_ball():
    c = mc.case("boundary_lattice_d3")
    centers, counts, iters, trace = mc.reference(c.name)
    assert c.bandwidth == 5 * 2.0 ** -6 and np.array_equal(c.points * 64, np.round(c.points * 64))
    d2 = _dist2(c, c.seeds[0])
    bw2 = c.bandwidth * c.bandwidth
    on = d2 == bw2
    offsets = sorted(map(tuple, np.round((c.points[on] - c.seeds[0]) * 64).astype(int).tolist()))
    assert offsets == [(-3, -4, 0), (0, 0, -5), (0, 0, 5), (3, 4, 0)]
    assert counts[0] == 7 and iters[0] == 0 and np.array_equal(centers[0], c.seeds[0]) and (trace[0]["nb"] >= on).all()
    assert int((d2 < bw2).sum()) == 3 and int(((d2 > bw2) & (d2 < 1.05 * bw2)).sum()) == 2      # 3 inside, 4 on, 2 just outside
    wrong = mc.ordered_shift(c.X, c.seeds, c.bandwidth, c.max_iter, mistake="ball_exclusive")
    assert wrong[1][0] == 3


def test_ball_rounding_cases_split_fp64_from_fp32():
    for name, inside64 in (("ball_fp64_inside_fp32_outside_d3", True), ("ball_fp64_outside_fp32_inside_d3", False)):
        c = mc.case(name)
        _, counts, iters, _ = mc.reference(name)
        wrong = mc.ordered_shift(c.X, c.seeds, c.bandwidth, c.max_iter, mistake="d2_fp32")
        assert (counts[0], wrong[1][0]) == ((3, 1) if inside64 else (1, 3)) and iters[0] == 0 and wrong[2][0] == 0


def test_offset_cloud_and_zero_stop():
    c = mc.case("offset_cloud_d3_n1000")
    assert np.abs(c.points - 100).max() < 0.2 and np.abs(c.points - 100).max() > 0.05
    c = mc.case("zero_stop_d3")
    assert c.bandwidth > 0 and c.bandwidth * c.bandwidth == 0 and 1e-3 * c.bandwidth == 0
    _, counts, iters, trace = mc.reference(c.name)
    assert counts.tolist() == [3, 2, 1, 0] and iters.tolist() == [0, 0, 0, 0] and all(rec["norms"] == [0] for rec in trace[:3])


# ---------------------------------------------------------------------------------------------------------------- order-independence
@pytest.mark.parametrize("name", mc.case_names())
def test_cases_do_not_hang_on_the_order_of_the_sum(name):
    """Conditions on the inputs: with NumPy's order of the neighbour sum the climb has the same counts and iterations and ends within one
    fp32 ulp; the centre is within one ulp of the exactly summed mean of the last neighbour set."""
    c = mc.case(name)
    centers, counts, iters, trace = mc.reference(name)
    plain = mc.numpy_shift(c.points, c.seeds, c.bandwidth, c.max_iter)
    assert np.array_equal(plain[1], counts) and np.array_equal(plain[2], iters)
    worst = mc.ulps_apart(plain[0], centers)
    assert worst <= 1, worst
    for s, rec in enumerate(trace):
        if counts[s] == 0:
            continue
        assert int(rec["nb"].sum()) == counts[s]
        assert mc.ulps_apart(mc.fsum_mean(c.points, rec["nb"]), centers[s]) <= 1, s


@pytest.mark.parametrize("name", mc.case_names())
def test_stop_margin(name):
    """At every step of every seed the fp32 norm is more than 4 ulps of the stop value away from it, or exactly 0: a device sqrtf one ulp
    off cannot change a decision."""
    c = mc.case(name)
    stop = 1e-3 * c.bandwidth
    ulp = f64(np.spacing(f32(stop)))
    closest = np.inf
    for rec in mc.reference(name)[3]:
        for norm in rec["norms"]:
            if norm != 0:
                closest = min(closest, abs(f64(norm) - stop) / ulp)
    assert closest > 4, closest


# ---------------------------------------------------------------------------------------------------------------- mistakes
@pytest.mark.parametrize("mistake", list(mc.MISTAKES))
def test_every_mistake_is_caught(mistake):
    caught = []
    for c in mc.cases():
        centers, counts, iters, _ = mc.reference(c.name)
        wrong = mc.ordered_shift(c.X, c.seeds, c.bandwidth, c.max_iter, mistake=mistake)
        if not (np.array_equal(wrong[0].view(np.int32), centers.view(np.int32)) and np.array_equal(wrong[1], counts)
                and np.array_equal(wrong[2], iters)):
            caught.append(c.name)
    print(mistake, "caught by", caught)
    assert caught, mc.MISTAKES[mistake]


def test_mistakes_table_matches_the_issue_and_helpers():
    assert len(mc.MISTAKES) == 8
    with pytest.raises(AssertionError):
        mc.ordered_shift(np.zeros((2, 2), f32), np.zeros((1, 2), f32), 0.1, 3, mistake="none")
    empty = mc.ordered_shift(np.zeros((2, 2), f32), np.zeros((0, 2), f32), 0.1, 3)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    # the documented split: 256 partials by i % 256, butterfly per 64, waves in order -- spelled out with scalars for one odd input
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((700, 1)) * 10.0 ** rng.integers(-6, 6, (700, 1))
    nb = rng.random(700) < 0.7
    part = [0.0] * 256
    for i in range(700):
        if nb[i]:
            part[i % 256] += float(rows[i, 0])
    waves = []
    for w in range(4):
        a = part[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            a = [a[lane] + a[lane ^ off] for lane in range(64)]
        assert len(set(a)) == 1                                               # every lane holds the same bits
        waves.append(a[0])
    assert mc.ordered_sum(rows, nb)[0] == ((waves[0] + waves[1]) + waves[2]) + waves[3]
