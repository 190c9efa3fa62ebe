"""What tests/rays_cases.py promises, checked without a GPU: the cameras meet their conditions (well-conditioned discriminants, one miss set in
fp32 and fp64, odd ray counts), the reference agrees with the reference-named functions of contrastive_lift_amd/rays.py, the fp32
restatement passes every assertion the GPU test makes, and each known mistake breaks one of them.  Prints the measured yardsticks."""
import numpy as np
import pytest
import torch

import rays_cases as rc

f32, f64 = np.float32, np.float64


def test_conditions_on_the_cameras():
    names = rc.case_names()
    assert names == ["inside_1x1", "inside_7x37_offcentre", "inside_near_surface_33x8", "outside_narrow_16x17", "outside_wide_20x13_misses"]
    counts = [c.N for c in rc.cases()]
    assert counts == [1, 259, 264, 272, 260] and 1 in counts and sum(n % 256 != 0 for n in counts) == 5 and sum(n > 256 for n in counts) >= 3
    for c in rc.cases():
        r64, r32 = rc.reference(c.name), rc.ray_reference(c, f32)
        if c.misses:
            assert float(np.abs(r64["disc"]).min()) > rc.MIN_DISC_MISS and float(np.abs(r32["disc"]).min()) > rc.MIN_DISC_MISS
            assert np.array_equal(r64["miss"], r32["miss"]) and 0 < r64["miss"].sum() < c.N
        else:
            assert float(r64["disc"].min()) >= rc.MIN_DISC_ACCURACY, (c, float(r64["disc"].min()))
            assert not r64["miss"].any() and not r32["miss"].any()
    c = rc.case("outside_wide_20x13_misses")
    disc = rc.reference(c.name)["disc"]
    assert int(rc.reference(c.name)["miss"].sum()) == 206 and abs(float(np.abs(disc).min()) - 6.2e-3) < 0.5e-3
    c = rc.case("inside_7x37_offcentre")
    assert c.K[0, 0] != c.K[1, 1] and c.K[0, 2] != c.W / 2 and c.K[1, 2] != c.H / 2 and c.H != c.W
    R = c.c2w[:3, :3].astype(f64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R - np.eye(3)).max() > 0.5 and np.linalg.norm(c.c2w[:3, 3]) < 0.75
    assert abs(np.linalg.norm(rc.case("inside_near_surface_33x8").c2w[:3, 3]) - 0.98) < 1e-6


@pytest.mark.parametrize("name", rc.case_names())
def test_reference_is_the_reference_named_functions(name):
    """The fp64 restatement against get_ray_directions_with_intrinsics / get_rays / rays_intersect_sphere (the reference's formulas in
    torch) evaluated in fp64."""
    from contrastive_lift_amd import rays as R
    c = rc.case(name)
    ref = rc.reference(name)
    K, M = torch.from_numpy(c.K).double(), torch.from_numpy(c.c2w).double()
    i, j = R.create_grid(c.H, c.W)
    dirs = torch.stack([(i.double() - K[0, 2]) / K[0, 0], (j.double() - K[1, 2]) / K[1, 1], torch.ones_like(i).double()], -1)
    o, d = R.get_rays(dirs, M)
    assert float((d - torch.from_numpy(ref["d"].copy())).abs().max()) < 1e-14 and np.array_equal(o.numpy(), ref["o"])
    od, dd, oo = (o * d).sum(1), (d * d).sum(1), (o * o).sum(1)
    disc = od ** 2 + (1 - oo) * dd
    far = ((torch.sqrt(disc) - od) / dd).numpy()
    hit = ~ref["miss"]
    assert np.array_equal(~(disc.numpy() >= 0), ref["miss"])
    assert np.abs(far[hit] / ref["far"][hit] - 1).max() < 1e-12
    if not c.misses:
        assert np.abs(R.rays_intersect_sphere(o, d).numpy() / ref["far"] - 1).max() < 1e-12
        on_sphere = np.linalg.norm(ref["o"] + ref["far"][:, None] * ref["d"], axis=1)
        assert np.abs(on_sphere - 1).max() < 1e-12 and (ref["far"] > 0).all()


def _records(c, r32):
    rays = np.empty((c.N, 8), f32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = r32["o"], r32["d"], f32(c.near), r32["far"]
    return rays


def test_yardsticks_and_the_restatement_passes_the_gpu_checks():
    for c in rc.cases():
        y_d, y_far = rc.yardstick(c.name)
        b_d, b_far = rc.bounds(c.name)
        hits = int((~rc.reference(c.name)["miss"]).sum())
        print(f"yardstick {c.name:28s} d {y_d / rc.EPS:5.2f}  far {y_far / rc.EPS:5.2f}  x 2^-24   ({hits} hits of {c.N})")
        assert b_d == max(4 * y_d, 2 * 2.0 ** -24) and b_far == max(4 * y_far, 2 * 2.0 ** -24)
        if not c.misses:                                                      # (the miss case has grazing rays: sqrt(disc) amplifies there)
            assert y_d <= 3 * rc.EPS and y_far <= 6 * rc.EPS, "fp32 error of a well-conditioned camera: a few units of 2^-24"
        rc.check_rays(c, _records(c, rc.ray_reference(c, f32)))


@pytest.mark.parametrize("mistake", list(rc.MISTAKES))
def test_every_mistake_is_caught(mistake):
    caught = []
    for c in rc.cases():
        try:
            rc.check_rays(c, _records(c, rc.ray_reference(c, f32, mistake=mistake)))
        except AssertionError:
            caught.append(c.name)
    print(mistake, "caught by", caught)
    assert caught, rc.MISTAKES[mistake]
