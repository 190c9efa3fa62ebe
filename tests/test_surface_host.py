"""Surface outputs of the ray route, host side: the references of tests/surface_cases.py against independent arithmetic, the
behaviour the feature exists for on a hand-made two-surface ray, the edge cases of the median hit, and the two new names at the boundary."""
import os

import numpy as np
import torch

import surface_cases as sc
from conftest import REPO
from oracle import field as fld
from oracle import params as op

RES, SHIFT = (9, 13, 17), -3.0


def test_gradient_reference_agrees_with_central_differences():
    """Central differences (h = 1e-7, fp64) of the same explicit lookup on random points that keep 1e-4 texels away from every texel line, so
    that both probes stay in the cell.  Truncation is zero per axis (the function is linear in each coordinate inside a cell); what is left
    is the cancellation 2^-53 |sigma_raw| / h ~ 1e-9 per unit of sigma_raw."""
    P = op.make_params(3, RES, 4, 3)
    rng = np.random.default_rng(0)
    xn = rng.uniform(-1.2, 1.2, (400, 3))
    xn = xn[~sc.near_texel_line(xn, RES)]
    assert xn.shape[0] > 380
    g, raw = sc.grad_reference(P, xn, SHIFT)
    P64 = {k: v.double() for k, v in P.items() if k.startswith("density_")}
    h = 1e-7
    fd = np.zeros_like(g)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        up = fld.density_raw(P64, torch.from_numpy(xn + e), SHIFT, explicit=True).numpy()
        dn = fld.density_raw(P64, torch.from_numpy(xn - e), SHIFT, explicit=True).numpy()
        fd[:, a] = (up - dn) / (2 * h)
    err = np.abs(fd - g).max()
    print(f"gradient reference against central differences: max error {err:.3g}, gradients up to {np.abs(g).max():.3g}")
    assert np.abs(g).max() > 0.1 and err < 1e-7
    outside = (np.abs(sc.texel_coordinates(xn, RES) - (np.asarray(RES) - 1) / 2.0) > (np.asarray(RES) - 1) / 2.0 + 1).any(1)
    assert outside.sum() > 5 and (g[outside] == 0).all() and (raw[outside] == SHIFT).all()       # farther than a texel outside: the padding


def test_gradient_reference_sees_the_step_to_the_padding():
    """A point exactly on the box face x = +1 sits on the last texel line: the cell floor selects reaches into the padding, so the
    derivative along x is -(R_x - 1)/2 times the plane value (times the line value), not the interior slope."""
    P = op.make_params(5, RES, 4, 3)
    xn = np.array([[1.0, 0.1, -0.2]])
    g, raw = sc.grad_reference(P, xn, SHIFT)
    inside = np.array([[1.0 - 1e-6, 0.1, -0.2]])
    gi, _ = sc.grad_reference(P, inside, SHIFT)
    P64 = {k: v.double() for k, v in P.items() if k.startswith("density_")}
    parts = fld.vm_products_explicit(P64, "density", torch.from_numpy(xn))          # planes 0 and 1 span x; plane 2's line runs along x
    expect = -(RES[0] - 1) / 2.0 * float(parts.sum())
    assert abs(g[0, 0] - expect) < 1e-12 and abs(g[0, 0] - gi[0, 0]) > 1e-3


def test_two_surface_ray_median_is_on_the_wall():
    T, w, z, delta = sc.two_surface_ray()
    ref = sc.ray_surface_reference(T, w, z, delta, np.zeros(2, np.int32), np.zeros(0, np.int32), None, 0.5)
    assert ref["k_med"][0] == 40
    assert z[0, 40] <= ref["z_med"][0] <= z[0, 40] + delta[0, 40]
    expected = float((w[0].astype(np.float64) * z[0]).sum())                       # ray_out[:, 1] of the march: sum_k w_k z_k
    print(f"two surfaces at z = {z[0, 5]:.2f} and {z[0, 40]:.2f}: expected distance {expected:.3f}, median {ref['z_med'][0]:.3f}")
    assert z[0, 5] + delta[0, 5] < expected < z[0, 40]                             # in empty space, strictly between the two surfaces
    # prev = 0.6, rem = 0: f = (0.6 - 0.5) / 0.6
    assert abs(ref["f"][0] - (np.float64(np.float32(0.6)) - 0.5) / np.float64(np.float32(0.6))) < 1e-7
    # q = 0.3 stops in the shell: rem_5 = 0.6 <= 0.7
    ref3 = sc.ray_surface_reference(T, w, z, delta, np.zeros(2, np.int32), np.zeros(0, np.int32), None, 0.3)
    assert ref3["k_med"][0] == 5


def test_median_edge_cases():
    S = 8
    z, delta = sc.deltas((2.0 + 0.1 * np.arange(S + 1)).astype(np.float32)[None].repeat(5, 0))
    T, w = np.ones((5, S), np.float32), np.zeros((5, S), np.float32)
    w[1, 0] = 0.9                                          # 1: hit at k = 0
    T[1, 1:] = 0.1
    w[2, S - 1] = 1.0                                      # 2: hit at k = S - 1, delta = 0
    T[3, 3], w[3, 3] = 0.75, 0.25                          # 3: rem_3 == 1 - q exactly
    T[3, 4:] = 0.5
    T[4, 2:] = 0.5                                         # 4: T falls to thr between samples (w = 0 there): den > 0 from the stored arrays
    ref = sc.ray_surface_reference(T, w, z, delta, np.arange(6, dtype=np.int32) * 0, np.zeros(0, np.int32), None, 0.5)
    assert ref["k_med"].tolist() == [-1, 0, S - 1, 3, 2]
    assert ref["z_med"][0] == 0.0
    assert ref["prev"][1] == 1.0 and abs(ref["f"][1] - 0.5 / 0.9) < 1e-7 and z[1, 0] < ref["z_med"][1] < z[1, 1]
    assert delta[2, S - 1] == 0 and ref["z_med"][2] == np.float64(z[2, S - 1])
    assert ref["f"][3] == 1.0 and ref["z_med"][3] == np.float64(z[3, 3]) + np.float64(delta[3, 3])
    assert ref["f"][4] == 1.0
    # the normal map: two active samples on ray 1, one zero gradient among them
    G = np.array([[0.0, 0.0, -2.0, 9.0], [0.0, 0.0, 0.0, 9.0], [3.0, 0.0, 4.0, 9.0]], np.float32)
    w[1, 1], w[1, 2] = 0.05, 0.02
    start = np.array([0, 0, 3, 3, 3, 3], np.int32)
    ref = sc.ray_surface_reference(T, w, z, delta, start, np.array([S, S + 1, S + 2], np.int32), G, 0.5)
    want = np.float64(w[1, 0]) * np.array([0, 0, 1.0]) + np.float64(w[1, 2]) * np.array([-0.6, 0, -0.8])
    assert np.abs(ref["normal"][1] - want).max() < 1e-12 and (ref["normal"][[0, 2, 3, 4]] == 0).all()


def test_made_up_marches_hold_their_cases():
    """The generator of the GPU test: every forced case is what it says, and no hit has den < 2^-12."""
    for S in (1, 63, 64, 65, 130):
        for q in (0.5, 0.9):
            m = sc.made_up_march(130, S, q, seed=S)
            z, delta = sc.deltas((1.0 + 0.03 * np.arange(S + 1)).astype(np.float32)[None].repeat(130, 0))
            ref = sc.ray_surface_reference(m["T"], m["w"], z, delta, m["ray_start"], m["act_idx"], m["G"], q)
            k, f = ref["k_med"], m["forced"]
            assert k[f["no hit"]] == -1 and k[f["empty"]] == -1 and k[f["hit at 0"]] == 0 and k[f["hit at S-1"]] == S - 1
            assert (S <= 64) == ("hit at 64" not in f) and (S < 67) == ("hit above 64" not in f)
            if "hit at 64" in f:
                assert k[f["hit at 64"]] == 64
            if "hit above 64" in f:
                assert k[f["hit above 64"]] == S - 2
            if "equality" in f:
                r = f["equality"]
                assert (m["T"][r, k[r]] - m["w"][r, k[r]]) == np.float32(1.0) - np.float32(q) and k[r] == 2
            hit = k >= 0
            assert (hit.sum() > 100 or S == 1) and (~hit).sum() >= 2 and (ref["den"][hit] >= 2.0 ** -12).all()
            n = np.diff(m["ray_start"])
            assert n[7] == 0 and n[8] == min(1, S) and n[9] == min(64, S) and n[10] == min(65, S) and n[11] == S
            assert (m["G"][::7, :3] == 0).all() and (np.diff(m["T"], axis=1) <= 0).all()


def test_the_new_entry_points_are_declared_exported_and_bound():
    import ctypes
    from contrastive_lift_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(REPO, "include", "clift.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("clift_density_grad_points", "clift_ray_surface"):
        assert f"int {name}(" in header and hasattr(lib, name) and name in _lib.exported_symbols()
