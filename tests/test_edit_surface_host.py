"""Surface outputs of an edited scene, host side: the fp64 reference of tests/edit_surface_cases.py against central differences
of the edited density, the exact and the algebraic cases of the chain J, the generator of the GPU test, and the two new entry points at the
boundary (declared, exported, bound; their argument checks return before anything is launched)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import edit_cases as ec
import edit_surface_cases as esc
import surface_cases as sc
from conftest import REPO
from contrastive_lift_amd import edit as ed
from oracle import params as op

RES, SHIFT = (9, 13, 17), -3.0
LO, HI = ec.AABB[0].double().numpy(), ec.AABB[1].double().numpy()
H = 1e-7                                                    # the step of tests/test_surface_host.py's central differences


def _field():
    return op.make_params(3, RES, 4, 3)


def _clean_points(prog, n, seed):
    """World points in 1.2 x the box that keep 1e-4 texels from every texel line where they are looked up and more than 10 h from every
    box face at every stage of their walk: both probes of a central difference then see the cell and the chain of the point itself."""
    pts = esc.world_points(n, LO, HI, seed).astype(np.float64)
    src, _, state = prog.jacobians(pts)
    keep = (esc.face_distance(prog, pts) > 10 * H) & ~sc.near_texel_line(esc.normalise(src, LO, HI), RES)
    return pts[keep]


def _central_differences(P, prog, pts):
    fd = np.zeros_like(pts)
    for a in range(3):
        e = np.zeros(3)
        e[a] = H
        fd[:, a] = (esc.edited_density(P, prog, pts + e, LO, HI, SHIFT) - esc.edited_density(P, prog, pts - e, LO, HI, SHIFT)) / (2 * H)
    return fd


@pytest.mark.parametrize("name", ["delete", "extract", "copy", "move", "mixed3", "full8", "nonrigid", "sheared", "kill_all"])
def test_reference_agrees_with_central_differences(name):
    """J^T g' against central differences (h = 1e-7, the bound 1e-7 of the unedited field's test) of the fp64 edited density sigma_raw(p'),
    0 where killed.  Inside a cell the field is linear in each coordinate, and the chain is constant between box faces."""
    P, prog = _field(), esc.programs(LO, HI)[name]
    pts = _clean_points(prog, 600, 11)
    assert pts.shape[0] > 560
    ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
    fd = _central_differences(P, prog, pts)
    err = np.abs(fd - ref["g"]).max()
    print(f"{name}: max error {err:.3g}, gradients up to {np.abs(ref['g']).max():.3g}; hops {np.bincount(ref['hops'][~ref['killed']], minlength=1).tolist()}, "
          f"{int(ref['killed'].sum())} killed")
    assert err < 1e-7
    assert (ref["g"][ref["killed"]] == 0).all() and (ref["raw"][ref["killed"]] == 0).all()
    if name == "kill_all":
        assert ref["killed"].all()
    else:
        assert np.abs(ref["g"]).max() > 0.1
    if name in ("copy", "move", "nonrigid", "sheared"):
        assert ((ref["hops"] == 1) & ~ref["killed"]).sum() > 10


def test_the_transpose_not_the_inverse_and_not_the_map_itself():
    """On the rows an edit remapped: a map that is no rotation (scale and shear) tells J^T from J^-1, the reference-faithful manipulate with a
    rotation (an orthogonal M in a motion that is not rigid) tells J^T from J.  Central differences side with J^T in both."""
    P, progs = _field(), esc.programs(LO, HI)
    for name, other in (("sheared", lambda J: np.linalg.inv(J)), ("nonrigid", lambda J: J)):
        prog = progs[name]
        pts = _clean_points(prog, 600, 12)
        ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
        sel = (ref["hops"] == 1) & ~ref["killed"]
        assert sel.sum() > 10
        src, J, _ = prog.jacobians(pts)
        assert np.abs(J[sel] - prog[0].M).max() == 0 and np.abs(src[sel] - (pts[sel] @ prog[0].M.T + prog[0].t)).max() < 1e-15
        gw = sc.grad_reference(P, esc.normalise(src, LO, HI), SHIFT)[0] * (2.0 / (HI - LO))
        wrong = np.einsum("nij,nj->ni", other(J), gw)                  # J^-1 g' resp. J g' in the place of J^T g'
        fd = _central_differences(P, prog, pts)
        assert np.abs(fd - ref["g"])[sel].max() < 1e-7 and np.abs(fd - wrong)[sel].max() > 1e-3


def test_identity_moves_give_the_unedited_gradient_exactly():
    P = _field()
    c, u = (LO + HI) / 2, HI - LO
    box = lambda f: ed.EditBox(np.eye(3), c + np.asarray(f) * u, -0.3 * u, 0.3 * u)
    prog = ed.EditProgram([ed.copy(box((-0.1, 0.0, 0.1)), np.zeros(3), np.eye(3)), ed.move(box((0.2, 0.1, -0.1)), None, None),
                           ed.copy(box((0.0, -0.2, 0.0)))])
    pts = esc.world_points(500, LO, HI, 5).astype(np.float64)
    src, J, state = prog.jacobians(pts)
    assert (state & ed.STATE_KILLED).sum() == 0 and set((state & ed.STATE_REMAPS).tolist()) == {0, 1, 2, 3}
    assert np.array_equal(src, pts) and (J == np.eye(3)).all()
    ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
    g, raw = sc.grad_reference(P, esc.normalise(pts, LO, HI), SHIFT)
    assert np.array_equal(ref["g"], g * (2.0 / (HI - LO))) and np.array_equal(ref["raw"], raw) and np.array_equal(ref["bound"], np.abs(ref["g"]))


def test_a_quarter_turn_permutes_and_negates_the_components():
    """The content of a cube turned by 90 degrees about the cube's centre (z axis): inside the cube the edited scene shows the field at
    p' = R^-1 (p - c) + c, and its gradient is R g': (gx, gy, gz) = (-g'y, g'x, g'z)."""
    P = _field()
    c = (LO + HI) / 2
    cube = ed.EditBox(np.eye(3), c, -np.full(3, 0.3), np.full(3, 0.3))
    prog = ed.EditProgram([ed.move(cube, None, ed.rotation_from_euler_deg(0, 0, 90))])
    pts = c + np.random.default_rng(9).uniform(-0.29, 0.29, (300, 3))
    ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
    assert (ref["hops"] == 1).all() and not ref["killed"].any()
    src = np.stack([c[0] + (pts[:, 1] - c[1]), c[1] - (pts[:, 0] - c[0]), pts[:, 2]], 1)
    assert np.abs(ref["xn"] - esc.normalise(src, LO, HI)).max() < 1e-14
    gw = sc.grad_reference(P, esc.normalise(src, LO, HI), SHIFT)[0] * (2.0 / (HI - LO))
    want = np.stack([-gw[:, 1], gw[:, 0], gw[:, 2]], 1)
    assert np.abs(want).max() > 0.1 and np.abs(ref["g"] - want).max() < 1e-12


@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene
    finally:
        sys.path.pop(0)
    return edit_scene


def test_a_two_hop_chain_is_the_product_of_its_maps(tool):
    """Move the object, then move the moved object again ("at": "moved"): a point of the final place is looked up at
    M_1 (M_2 p + t_2) + t_1 -- the walk meets edit 2 first -- and its chain is J = M_1 M_2."""
    boxes = {4: {"bbox": (np.array([-0.2, -0.15, -0.1]), np.array([0.2, 0.15, 0.1])), "orientation": ec.rot_xyz(0.1, 0.2, 0.3).double().numpy(),
                 "position": np.array([-0.4, -0.2, 0.0])}}
    prog = tool.resolve_program(boxes, [{"instance": 4, "op": "move", "translate": [0.5, 0.1, 0.0], "rotate_deg": [0, 20, 30]},
                                        {"instance": 4, "op": "move", "translate": [0.1, 0.5, 0.1], "rotate_deg": [40, 0, -25], "at": "moved"}])
    e1, e2 = prog
    q = np.random.default_rng(2).uniform(-1, 1, (200, 3)) * np.array([0.19, 0.14, 0.09])
    pts = q @ e2.dst.axes + e2.dst.centre                              # inside the final box
    src, J, state = prog.jacobians(pts)
    assert (state == 2).all()
    assert np.abs(J - e1.M @ e2.M).max() < 1e-15 and np.abs(src - ((pts @ e2.M.T + e2.t) @ e1.M.T + e1.t)).max() < 1e-15
    assert np.abs(e1.M @ e2.M - e2.M @ e1.M).max() > 0.05              # the order matters here
    assert e1.src.contains(src).all()                                 # ... and the chain ends in the box as fitted
    P = _field()
    ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
    gw = sc.grad_reference(P, esc.normalise(src, LO, HI), SHIFT)[0] * (2.0 / (HI - LO))
    assert np.abs(ref["g"] - gw @ (e1.M @ e2.M)).max() < 1e-13


def test_the_generator_of_the_gpu_test_holds_its_cases():
    """The seeds of tests/test_gpu_edit_surface.py, from the reference alone: at most 1 % of the rows of every case are left out (none among
    the first 65), every remap count 0 .. 3 and the kill state occur in the full eight, every point dies in kill_all."""
    P = op.make_params(216, RES, 4, 3)
    progs = esc.programs(LO, HI)
    pts = esc.world_points(4097, LO, HI, esc.POINT_SEED)
    for name, prog in progs.items():
        ref = esc.reference(P, prog, pts, LO, HI, SHIFT)
        out = esc.left_out(ref, prog, pts, RES)
        for n in (1, 3, 63, 64, 65, 4097):
            assert out[:n].sum() <= 0.01 * n, (name, n, int(out[:n].sum()))
        live = ~ref["killed"]
        counts = np.bincount(ref["hops"][live], minlength=4).tolist()
        print(f"{name}: {int(out.sum())} rows left out, {int(ref['killed'].sum())} killed, live rows by remap count {counts}")
        if name == "full8":
            assert min(counts[:4]) >= 8 and ref["killed"].sum() > 100
        elif name == "kill_all":
            assert ref["killed"].all() and (ref["hops"] > 0).any()
        elif name in ("delete", "extract"):
            assert ref["killed"].sum() > 100 and counts[0] > 100 and sum(counts[1:]) == 0
        else:
            assert counts[0] > 100 and counts[1] > 30
        if name == "move":
            assert ref["killed"].sum() > 10
    src, _, state = progs["copy"].jacobians(pts)
    outside = (np.abs(esc.normalise(src, LO, HI)) > 1.0).any(1)
    assert outside.sum() > 100 and (outside & (state > 0)).sum() > 10      # points that read padding, remapped ones among them


def test_the_new_entry_points_are_declared_exported_and_bound():
    from contrastive_lift_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(REPO, "include", "clift.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in (("clift_edit_list_density_grad_points", 12), ("clift_edit_list_density_grad_active", 9)):
        assert f"int {name}(" in header and hasattr(lib, name) and name in _lib.exported_symbols()
        assert len(_lib._SIGNATURES[name][0]) == n_args


def test_the_new_entry_points_check_their_arguments():
    """Every refusal comes before anything touches a device: callable without one."""
    from contrastive_lift_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    prog = esc.programs(LO, HI)["mixed3"]
    nine = (_lib.EditRec * 9)(*(prog[i % 3].record() for i in range(9)))
    ms, vm = _lib.March(), _lib.VM()
    ms.n_samples, vm.comps = 38, 16
    for i in range(3):
        vm.res[i] = RES[i]
    lo3, inv3 = (C.c_float * 3)(*LO), (C.c_float * 3)(*(2.0 / (HI - LO)))
    fake = C.c_void_p(4096)                                            # a non-NULL address that is never followed
    points = lambda recs, n, vm=vm, ldp=3, rows=10, out=fake: ("clift_edit_list_density_grad_points", recs, n, C.byref(vm), fake, ldp, rows, lo3,
                                                                 inv3, 0.0, out, None, None)
    active = lambda recs, n, vm=vm, M=10, out=fake: ("clift_edit_list_density_grad_active", C.byref(ms), recs, n, C.byref(vm), fake, fake, M, out,
                                                     None)
    for args in (points, active):
        name = args(nine, 3)[0]
        for n in (0, 9):
            with pytest.raises(_lib.CliftError, match=f"{name}: .*1 to 8 edits.*n_edits = {n}"):
                _lib.call(*args(nine, n))
        bad = _lib.VM()
        bad.comps = 6
        for i in range(3):
            bad.res[i] = RES[i]
        with pytest.raises(_lib.CliftError, match=f"{name}: comps must be a positive multiple of 4 .got 6"):
            _lib.call(*args(nine, 3, vm=bad))
        with pytest.raises(_lib.CliftError, match=f"{name}: NULL"):
            _lib.call(*args(nine, 3, out=None))
    with pytest.raises(_lib.CliftError, match="clift_edit_list_density_grad_points: ldp must be >= 3"):
        _lib.call(*points(nine, 3, ldp=2))
    with pytest.raises(_lib.CliftError, match=r"clift_edit_list_density_grad_points: .*\[0, 2\^36\)"):
        _lib.call(*points(nine, 3, rows=1 << 36))
    assert _lib.call(*points(nine, 3, rows=0, out=None)) in (0, None)   # nothing to do: no launch, no complaint about the buffers
    assert _lib.call(*active(nine, 3, M=0, out=None)) in (0, None)
