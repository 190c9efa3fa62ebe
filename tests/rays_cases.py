"""Shared inputs of the ray-generation tests (test_rays_cases_host.py on the CPU, test_gpu_rays.py on the GPU): cameras for clift_gen_rays
(csrc/rays.hip) and ``ray_reference``, which restates the kernel once.  Evaluated in fp64 it is the reference; evaluated in fp32, operation
by operation with the kernel's grouping, it is the yardstick: its own error against the fp64 reference says what fp32 can deliver on a case.
A device result is held to 4 x that error (a different but legitimate grouping of the three-term sums), with a floor of 2 * 2^-24: the
direction absolutely (its components are at most 1), ``far`` relatively.

  pixel p = j * W + i -> dx = (i - cx) / fx, dy = (j - cy) / fy, dz = 1            (no half-pixel offset, +z forward)
  d_a = (dx * R[a][0] + dy * R[a][1]) + dz * R[a][2];  d /= sqrt((d0^2 + d1^2) + d2^2)
  od = (t0 d0 + t1 d1) + t2 d2, dd = (d0^2 + d1^2) + d2^2, oo = (t0^2 + t1^2) + t2^2
  disc = od * od + (1 - oo) * dd;  far = (sqrt(disc) - od) / dd;  a ray with disc < 0 misses the unit sphere: far is NaN, *bad_count += 1
  record (8 floats): t, d, near, far

Measured yardsticks (fp32 restatement against fp64, in units of 2^-24; printed by test_rays_cases_host.py):

  case                          max |d32 - d64|    max |far32 / far64 - 1|
  inside_1x1                         1.32                2.00
  inside_7x37_offcentre              2.07                4.41
  inside_near_surface_33x8           1.54                2.82
  outside_narrow_16x17               1.59                4.88
  outside_wide_20x13_misses          1.21               13.52  (54 hits of 260; the grazing rays, disc down to 6.2e-3, lose digits in sqrt)

Nothing here touches the GPU."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24
FLOOR = 2 * EPS
FACTOR = 4
DEFAULT_F, DEFAULT_NEAR = 40.0, 0.01
MIN_DISC_ACCURACY, MIN_DISC_MISS = 0.2, 1e-3

MISTAKES = {
    "half_pixel": "pixel centres at i + 0.5",
    "transposed_rotation": "world-to-camera rotation applied",
    "swapped_focal": "fx and fy exchanged",
    "swapped_centre": "cx and cy exchanged",
    "row_major_by_height": "p split by H instead of W",
    "near_root": "the near root (-sqrt(disc) - od) / dd",
    "not_normalised": "od and dd formed from the direction before it is normalised",
}


def rotation(axis, angle):
    """Rodrigues rotation matrix, fp64."""
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


class Case:
    """One camera: H x W pixels, intrinsics K (3, 3) and camera-to-world c2w (4, 4) as the fp32 arrays the entry point receives."""

    def __init__(self, name, H, W, fx=DEFAULT_F, fy=None, cx=None, cy=None, origin=(0.0, 0.0, 0.0), R=None, near=DEFAULT_NEAR, misses=False):
        self.name, self.H, self.W, self.N, self.near, self.misses = name, H, W, H * W, near, misses
        fy = fx if fy is None else fy
        cx, cy = (W - 0.5) / 2 if cx is None else cx, (H - 0.5) / 2 if cy is None else cy          # by default a quarter pixel off a pixel centre
        self.K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
        M = np.eye(4)
        M[:3, :3] = np.eye(3) if R is None else R
        M[:3, 3] = origin
        self.c2w = M.astype(f32)

    def __repr__(self):
        return f"Case({self.name}: {self.H}x{self.W})"


@functools.lru_cache(maxsize=None)
def cases():
    return (
        Case("inside_1x1", 1, 1),
        Case("inside_7x37_offcentre", 7, 37, fx=31.5, fy=17.0, cx=11.25, cy=5.5, origin=(0.5, 0.4, -0.3), R=rotation((1, -1, 0.5), 2.1), near=0.05),
        Case("inside_near_surface_33x8", 33, 8, origin=(0.0, 0.0, -0.98), R=rotation((0, 1, 0), 0.3)),
        Case("outside_narrow_16x17", 16, 17, fx=200.0, origin=(0.0, 0.0, -3.0)),
        Case("outside_wide_20x13_misses", 20, 13, fx=12.0, origin=(0.0, 0.0, -3.0), misses=True),
    )


def case(name):
    return next(c for c in cases() if c.name == name)


def case_names():
    return [c.name for c in cases()]


def ray_reference(c, dtype, mistake=None):
    """rays.hip in NumPy, every operation in ``dtype`` and grouped as the kernel groups it: dict of o (N, 3), d (N, 3), far (N,), disc (N,),
    miss (N,) bool.  ``mistake`` selects a wrong variant (``MISTAKES``)."""
    assert mistake is None or mistake in MISTAKES, mistake
    T = np.dtype(dtype).type
    K, M = c.K.astype(T), c.c2w.astype(T)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if mistake == "swapped_focal":
        fx, fy = fy, fx
    if mistake == "swapped_centre":
        cx, cy = cy, cx
    R, t = M[:3, :3], M[:3, 3]
    if mistake == "transposed_rotation":
        R = R.T
    p = np.arange(c.N)
    j = p // (c.H if mistake == "row_major_by_height" else c.W)
    i = p - j * (c.H if mistake == "row_major_by_height" else c.W)
    fi, fj = i.astype(T), j.astype(T)
    if mistake == "half_pixel":
        fi, fj = fi + T(0.5), fj + T(0.5)
    dx, dy, dz = (fi - cx) / fx, (fj - cy) / fy, T(1)
    d = [(dx * R[a, 0] + dy * R[a, 1]) + dz * R[a, 2] for a in range(3)]
    raw = d
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    d = [d[a] / n for a in range(3)]
    e = raw if mistake == "not_normalised" else d
    od = (t[0] * e[0] + t[1] * e[1]) + t[2] * e[2]
    dd = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    oo = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    disc = od * od + (T(1) - oo) * dd
    with np.errstate(invalid="ignore"):
        root = np.sqrt(disc)
        far = ((-root if mistake == "near_root" else root) - od) / dd
    out = dict(o=np.broadcast_to(t, (c.N, 3)).copy(), d=np.stack(d, 1), far=far, disc=disc, miss=~(disc >= 0))
    for k in ("o", "d", "far", "disc"):
        assert out[k].dtype == np.dtype(dtype), (k, out[k].dtype)
    return out


def errors(c, got_d, got_far):
    """(max |d - d64|, max |far / far64 - 1| over the rays that hit) of a result against the fp64 reference."""
    ref = reference(c.name)
    hit = ~ref["miss"]
    e_d = float(np.abs(np.asarray(got_d, f64) - ref["d"]).max())
    e_far = float((np.abs(np.asarray(got_far, f64)[hit] - ref["far"][hit]) / np.abs(ref["far"][hit])).max()) if hit.any() else 0.0
    return e_d, e_far


@functools.lru_cache(maxsize=None)
def reference(name):
    out = ray_reference(case(name), f64)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """The fp32 restatement's own error on a case: (absolute in d, relative in far)."""
    c = case(name)
    r32 = ray_reference(c, f32)
    return errors(c, r32["d"], r32["far"])


def bounds(name):
    """What a device result is held to: FACTOR x the yardstick, at least FLOOR.  Never taken from the device."""
    y_d, y_far = yardstick(name)
    return max(FACTOR * y_d, FLOOR), max(FACTOR * y_far, FLOOR)


def check_rays(c, rays):
    """Every assertion the GPU test makes on a (N, 8) record array, so that the host test can prove the fp32 restatement passes them."""
    ref = reference(c.name)
    b_d, b_far = bounds(c.name)
    rays = np.asarray(rays)
    assert rays.shape == (c.N, 8) and rays.dtype == f32
    assert np.array_equal(rays[:, 0:3].view(np.int32), np.broadcast_to(c.c2w[:3, 3], (c.N, 3)).view(np.int32)), "o is the translation, bit for bit"
    assert np.array_equal(rays[:, 6].view(np.int32), np.full(c.N, c.near, f32).view(np.int32)), "column 6 is near, bit for bit"
    d, far = rays[:, 3:6], rays[:, 7]
    length = np.sqrt((d.astype(f64) ** 2).sum(1))
    e_d, e_far = errors(c, d, far)
    print(f"{c.name}: |d| - 1 max {np.abs(length - 1).max() / EPS:.2f}, d {e_d / EPS:.2f} (bound {b_d / EPS:.2f}), far {e_far / EPS:.2f} "
          f"(bound {b_far / EPS:.2f}) x 2^-24")
    assert np.abs(length - 1).max() <= b_d
    assert e_d <= b_d
    assert np.array_equal(np.isnan(far), ref["miss"]), "far is NaN on exactly the rays that miss"
    assert e_far <= b_far
