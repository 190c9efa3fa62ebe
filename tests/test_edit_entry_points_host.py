"""The refusals of the edit entry points (csrc/edit.hip), message by message, without a GPU: every refusal returns before anything touches
a device, so the thirteen functions are called here with valid host records (``March``, ``VM``) and NULL or stand-in device pointers.

Per entry point the cases are
  * the program's own faults: n_edits of 0, -1 and 9, NULL records, mode 7 in edit 1, a NaN in edit 2 (the single-edit names: no record, mode 7,
    a NaN); for the shaped names also the six shape faults of test_gpu_edit_shape._bad_shaped_programs, and h_shapes = NULL with n_edits = 0;
  * the function's own faults, one at a time, in the order in which the function checks them (``ENTRY``);
  * double faults that pin the order: the program's first fault together with the function's first, and every two neighbouring faults of
    the function together (comps = 6 with n_samples = 0, ...).
The full message of every case is compared with tests/golden/edit_entry_point_refusals.json, recorded from a build of the commit BEFORE the
entry points were gathered over one checked body per walk kernel (``CLIFT_LIB_PATH=<that build's libclift.so> python
tests/test_edit_entry_points_host.py --golden``): the wrappers reproduce every text, the name it starts with included, and the order of
the checks.  A call that is not refused returns 0 without a launch for N = 0, M = 0 and n = 0 (the last field of ``ENTRY``)."""
import ctypes as C
import json
import os
import sys

import pytest

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "edit_entry_point_refusals.json")
DEV = C.c_void_p(0x1000)        # stands for a device buffer: every call here returns before anything could read it
F3 = (C.c_float * 3)(0.0, 0.5, 1.0)


def _march(n_samples):
    from contrastive_lift_amd import _lib
    ms = _lib.March()
    ms.n_samples = n_samples
    return C.byref(ms)


def _vm(comps, res0=16):
    from contrastive_lift_amd import _lib
    vm = _lib.VM()
    vm.comps, vm.res[0], vm.res[1], vm.res[2] = comps, res0, 16, 16
    return C.byref(vm)


# ----------------------------------------------------------------------------- the argument lists (p: the program's arguments)
def density_fwd(p, comps=16, n_samples=38, N=10):
    return (_march(n_samples), *p, _vm(comps), DEV, N, DEV, None)


def active(p, n_samples=38, M=10, xa=DEV, dirs=DEV):
    return (_march(n_samples), *p, DEV, DEV, M, xa, dirs, None)


def active_origin(p, n_samples=38, M=10, xa=DEV, origin=DEV):
    return (_march(n_samples), *p, DEV, DEV, M, xa, origin, None, None)


def points(p, pts=DEV, ldp=3, dirs=None, ldd=3, n=256, out_pts=DEV, out_dirs=None):
    return (*p, pts, ldp, dirs, ldd, n, out_pts, out_dirs, None, None)


def dense_sigma(p, dens=True, comps=16, lo=F3, inv=F3, n0=4, n1=5, n2=6, s0=DEV, out=DEV):
    return (_vm(comps) if dens else None, *p, lo, F3, inv, s0, DEV, DEV, n0, n1, n2, 0.0, out, None, None)


def grad_points(p, dens=True, comps=16, res0=16, lo=F3, pts=DEV, ldp=3, n=256, out=DEV):
    return (*p, _vm(comps, res0) if dens else None, pts, ldp, n, lo, F3, 0.0, out, None, None)


def grad_active(p, dens=True, comps=16, res0=16, march=True, n_samples=38, rays=DEV, M=10, out=DEV):
    return (_march(n_samples) if march else None, *p, _vm(comps, res0) if dens else None, rays, DEV, M, out, None)


COMPS6, NO_SAMPLES = ("comps = 6", dict(comps=6)), ("n_samples = 0", dict(n_samples=0))
_DENSITY = (density_fwd, [COMPS6, NO_SAMPLES], dict(N=0))
_ACTIVE = (active, [NO_SAMPLES, ("NULL xa", dict(xa=None)), ("NULL dirs", dict(dirs=None))], dict(M=0))
_POINTS = (points, [("ldp = 2", dict(ldp=2)), ("ldd = 2", dict(dirs=DEV, out_dirs=DEV, ldd=2)), ("n = -1", dict(n=-1)), ("n = 2^36", dict(n=1 << 36)),
                    ("NULL pts", dict(pts=None)), ("NULL out_pts", dict(out_pts=None)), ("dirs without out_dirs", dict(dirs=DEV))], dict(n=0))
_LATTICE = (dense_sigma, [("NULL table record", dict(dens=False)), ("NULL lo", dict(lo=None)), ("NULL inv_ext2", dict(inv=None)), COMPS6,
                          ("n0 = 0", dict(n0=0)), ("n2 = -3", dict(n2=-3)), ("2^36 lattice points", dict(n0=4096, n1=4096, n2=4096)),
                          ("NULL ticks", dict(s0=None)), ("NULL out", dict(out=None))], None)
_TABLE = [("NULL table record", dict(dens=False)), COMPS6, ("comps = 0", dict(comps=0)), ("res[0] = 0", dict(res0=0))]
# entry point -> (tier of its program, argument list, its own faults in the order of its checks, what returns 0 without a launch)
ENTRY = {
    "clift_edit_density_fwd": ("single",) + _DENSITY,
    "clift_edit_list_density_fwd": ("list",) + _DENSITY,
    "clift_edit_shaped_density_fwd": ("shaped",) + _DENSITY,
    "clift_edit_active": ("single",) + _ACTIVE,
    "clift_edit_list_active": ("list",) + _ACTIVE,
    "clift_edit_shaped_active": ("shaped",) + _ACTIVE,
    "clift_edit_list_points": ("list",) + _POINTS,
    "clift_edit_shaped_points": ("shaped",) + _POINTS,
    "clift_edit_list_dense_sigma": ("list",) + _LATTICE,
    "clift_edit_shaped_dense_sigma": ("shaped",) + _LATTICE,
    "clift_edit_list_active_origin": ("list", active_origin, [NO_SAMPLES, ("NULL xa", dict(xa=None)), ("NULL origin", dict(origin=None))], dict(M=0)),
    "clift_edit_list_density_grad_points": ("list", grad_points, _TABLE + [("NULL lo", dict(lo=None)), ("ldp = 2", dict(ldp=2)), ("n = -1", dict(n=-1)),
                                                                          ("n = 2^36", dict(n=1 << 36)), ("NULL pts", dict(pts=None)),
                                                                          ("NULL out", dict(out=None))], dict(n=0)),
    "clift_edit_list_density_grad_active": ("list", grad_active, _TABLE + [("NULL march record", dict(march=False)), NO_SAMPLES,
                                                                          ("NULL rays", dict(rays=None)), ("NULL out", dict(out=None))], dict(M=0)),
}


# ----------------------------------------------------------------------------- the programs
def _edits():
    from contrastive_lift_amd import edit
    box = edit.EditBox([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [0.125, -0.25, 0.0625], [-0.375, -0.25, -0.1875], [0.375, 0.25, 0.1875])
    t, R = [0.25, 0.0, -0.125], [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    return [edit.move(box, t, R), edit.delete(box), edit.copy(box, t)]


def _records(n=3):
    from contrastive_lift_amd import _lib
    es = _edits()
    return (_lib.EditRec * n)(*(es[i % 3].record() for i in range(n)))


def _shapes():
    """Three host shape records, (5, 6, 7) cells each, the words a stand-in device pointer (a record with NULL words is not looked at)."""
    from contrastive_lift_amd import _lib
    sh = (_lib.EditShapeRec * 3)()
    for i in range(3):
        sh[i].words = DEV.value
        sh[i].dims[0], sh[i].dims[1], sh[i].dims[2] = 5, 6, 7
        sh[i].inv_cell[0], sh[i].inv_cell[1], sh[i].inv_cell[2] = 4.0, 8.0, 16.0
    return sh


SHAPE_FAULTS = (("dims 0", 1, "dims", 2, 0), ("dims 1025", 2, "dims", 0, 1025), ("inv_cell 0", 0, "inv_cell", 1, 0.0), ("inv_cell < 0", 1, "inv_cell", 0, -3.0),
                ("inv_cell inf", 2, "inv_cell", 2, float("inf")), ("inv_cell nan", 0, "inv_cell", 0, float("nan")))


def programs(tier):
    """-> (the arguments of a good program, [(what, the arguments of a faulty one)]), the program's first check first."""
    mode7, nan2 = _records(), _records()
    mode7[1].mode = 7
    nan2[2].dst.centre[1] = float("nan")
    if tier == "single":
        return (C.byref(_records()[0]),), [("no record", (None,)), ("mode 7", (C.byref(mode7[1]),)), ("NaN", (C.byref(nan2[2]),))]
    faults = [("n_edits = 0", _records(), 0), ("n_edits = -1", _records(), -1), ("n_edits = 9", _records(9), 9), ("NULL records", None, 3),
              ("mode 7 in edit 1", mode7, 3), ("NaN in edit 2", nan2, 3)]
    if tier == "list":
        return (_records(), 3), [(what, (recs, n)) for what, recs, n in faults]
    some = _shapes()
    some[1].words = None
    out = [(what, (recs, _shapes(), n)) for what, recs, n in faults] + [("h_shapes = NULL, n_edits = 0", (_records(), None, 0))]
    for what, i, field, k, value in SHAPE_FAULTS:
        sh = _shapes()
        getattr(sh[i], field)[k] = value
        out.append((what, (_records(), sh, 3)))
    two = _shapes()                                                 # the records are checked before the shapes, the shapes edit by edit
    two[0].dims[1], two[2].inv_cell[0] = 0, -1.0
    out += [("mode 7 in edit 1 + dims 0 in edit 0", (mode7, two, 3)), ("dims 0 in edit 0 + inv_cell < 0 in edit 2", (_records(), two, 3))]
    return (_records(), some, 3), out


def cases(name):
    """[(what, arguments)] of every refusal of entry point ``name``."""
    tier, args, own, _ = ENTRY[name]
    good, bad = programs(tier)
    out = [(what, args(p)) for what, p in bad]
    out += [(what, args(good, **kw)) for what, kw in own]
    out.append((f"{bad[0][0]} + {own[0][0]}", args(bad[0][1], **own[0][1])))
    out.append((f"{bad[-1][0]} + {own[0][0]}", args(bad[-1][1], **own[0][1])))
    for (wa, a), (wb, b) in zip(own, own[1:]):
        if not set(a) & set(b):
            out.append((f"{wa} + {wb}", args(good, **a, **b)))
    assert len({what for what, _ in out}) == len(out)
    return out


@pytest.fixture(scope="module")
def lib():
    from contrastive_lift_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def refusals(lib, name):
    """{what: message} of ``cases(name)``; every one must be a refusal (rc 1: an argument check, not a failed launch)."""
    out = {}
    for what, a in cases(name):
        rc = getattr(lib, name)(*a)
        msg = lib.clift_last_error().decode()
        assert rc == 1 and "launch failed" not in msg, f"{name} / {what}: rc = {rc}, {msg!r}"
        out[what] = msg
    return out


def test_every_edit_entry_point_is_listed():
    from contrastive_lift_amd import _lib
    assert set(ENTRY) == {n for n in _lib._SIGNATURES if n.startswith("clift_edit_")} and len(ENTRY) == 13


@pytest.mark.parametrize("name", list(ENTRY))
def test_refusals_have_the_recorded_text(lib, name):
    want = json.load(open(GOLDEN))[name]
    got = refusals(lib, name)
    assert list(got) == list(want), "cases() no longer enumerates what the golden file was recorded for"
    bad = [f"{what}: {got[what]!r}, recorded {want[what]!r}" for what in want if got[what] != want[what]]
    assert not bad, f"{name}: {len(bad)} of {len(want)} messages differ:\n" + "\n".join(bad)
    assert all(m.startswith(name + ": ") for m in got.values())


@pytest.mark.parametrize("name", [n for n in ENTRY if ENTRY[n][3]])
def test_nothing_to_do_returns_zero(lib, name):
    tier, args, _, early = ENTRY[name]
    good = programs(tier)[0]
    assert getattr(lib, name)(*args(good, **early)) == 0
    if tier == "shaped":                                            # h_shapes = NULL: the list entry point's behaviour
        assert getattr(lib, name)(*args((good[0], None, good[2]), **early)) == 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--golden"]:
        sys.exit("usage: test_edit_entry_points_host.py --golden   (rewrites the golden file from the library CLIFT_LIB_PATH names)")
    from contrastive_lift_amd import _lib
    doc = {name: refusals(_lib.load(), name) for name in ENTRY}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{sum(len(v) for v in doc.values())} messages of {_lib.LIB_PATH} -> {GOLDEN}")
