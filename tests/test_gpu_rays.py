"""clift_gen_rays (csrc/rays.hip) on the GPU against the fp64 reference of tests/rays_cases.py: non-square images, ray counts that are no
multiple of the block, an off-centre principal point, fx != fy, rotated cameras, a camera just under the sphere's surface and one outside it.
The origin and near columns are held bit for bit; the direction (absolutely) and far (relatively) to 4 x the error of the fp32 restatement
on the same case (rays_cases.bounds: computed on the CPU, never from the device); bad_count to the reference's count of missing rays."""
import ctypes as C

import numpy as np
import pytest
import torch

import rays_cases as rc
from contrastive_lift_amd import _lib
from contrastive_lift_amd.rays import generate_ray_table

pytestmark = pytest.mark.gpu


def raw(c, bad_before=0):
    """Raw call with prefilled outputs: ((N, 8) records, bad_count)."""
    K, M = np.ascontiguousarray(c.K), np.ascontiguousarray(c.c2w)
    rays = torch.full((c.N, 8), -7.0, dtype=torch.float32, device="cuda")
    bad = torch.full((1,), bad_before, dtype=torch.int32, device="cuda")
    _lib.call("clift_gen_rays", c.H, c.W, K.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), float(c.near), _lib.ptr(rays), _lib.ptr(bad),
              _lib.stream())
    torch.cuda.synchronize()
    return rays.cpu().numpy(), int(bad.item())


@pytest.mark.parametrize("name", rc.case_names())
def test_rays_against_fp64(name):
    c = rc.case(name)
    table = generate_ray_table(c.H, c.W, c.K, c.c2w, near=c.near, check=not c.misses)
    rays = table.cpu().numpy()
    rc.check_rays(c, rays)
    again, bad = raw(c, bad_before=5)                                         # *bad_count is incremented, one per missing ray
    assert bad == 5 + int(rc.reference(name)["miss"].sum())
    assert np.array_equal(again.view(np.int32), rays.view(np.int32))


def test_missing_rays_are_counted_and_raise():
    c = rc.case("outside_wide_20x13_misses")
    miss = rc.reference(c.name)["miss"]
    assert int(miss.sum()) == 206
    rays = generate_ray_table(c.H, c.W, c.K, c.c2w, near=c.near, check=False).cpu().numpy()
    _, bad = raw(c)
    assert bad == 206
    assert np.array_equal(np.isnan(rays[:, 7]), miss) and not np.isnan(rays[:, :7]).any()
    _, e_far = rc.errors(c, rays[:, 3:6], rays[:, 7])
    assert e_far <= rc.bounds(c.name)[1]
    with pytest.raises(AssertionError, match="unit sphere"):
        generate_ray_table(c.H, c.W, c.K, c.c2w, near=c.near, check=True)
    K, M = np.ascontiguousarray(c.K), np.ascontiguousarray(c.c2w)              # a NULL bad_count: the rays are written, nothing is counted
    out = torch.full((c.N, 8), -7.0, dtype=torch.float32, device="cuda")
    _lib.call("clift_gen_rays", c.H, c.W, K.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), float(c.near), _lib.ptr(out), None, _lib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), rays.view(np.int32))


def test_bad_image_size_launches_nothing():
    c = rc.case("inside_1x1")
    lib = _lib.load()
    K, M = np.ascontiguousarray(c.K), np.ascontiguousarray(c.c2w)
    rays = torch.full((4, 8), -7.0, dtype=torch.float32, device="cuda")
    bad = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    for H, W in ((0, 2), (2, 0), (-1, 2)):
        rc_ = lib.clift_gen_rays(H, W, K.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), 0.01, _lib.ptr(rays), _lib.ptr(bad), _lib.stream())
        assert rc_ != 0 and "image size" in lib.clift_last_error().decode()
    torch.cuda.synchronize()
    assert bool((rays == -7.0).all()) and int(bad.item()) == -7
