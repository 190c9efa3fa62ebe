"""The placement map without a GPU: the numpy backend of contrastive_lift_amd/placement.py against the brute force of
tests/placement_cases.py on every integer, hand lattices, the identities against the HOST clearance and ``distance.placement_from_keys``,
the summary, every error of the module and of the entry point, its declarations, and the refusals of ``edit_scene.py --snap_placement``."""
import ctypes
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

import clearance_cases as cc
import placement_cases as pc
from conftest import REPO

from contrastive_lift_amd import _lib, clearance, distance, placement

LOOPED = (pc.SMALL, "(9, 3, 5) object (9, 1, 1)", "solid names key 0 too", "rejected keys") + pc.NONE_CASES


def host(key, shape, *a, **kw):
    return pc.to_numpy(placement.placement_tables(key, shape, *a, backend="host", **kw))


# ----------------------------------------------------------------------------- the brute force
@pytest.mark.parametrize("name", LOOPED)
def test_host_backend_against_the_brute_force(name):
    case = pc.cases()[name]
    T = tuple(case["key"].shape[a] - case["shape"].shape[a] + 1 for a in range(3))
    target = tuple(min(max(case["target"][a], 0), T[a] - 1) for a in range(3))
    for d in pc.DIRECTIONS:
        got = pc.host_tables()[(name, d)]
        want = pc.brute(case["key"], case["n_keys"], case["solid"], case["shape"], d, target, case["min_support"])
        assert pc.same(got, want) == "", (name, d, pc.same(got, want))
        assert got["overlap"].shape == T and got["best"].dtype == np.int64 and got["count"].dtype == np.int32


def test_the_none_cases_say_none():
    tables = pc.host_tables()
    for d in pc.DIRECTIONS:
        one = tables[("a single translation", d)]
        assert one["overlap"].shape == (1, 1, 1) and one["overlap"].item() > 0 and one["count"].tolist() == [0, 0] and one["best"].tolist() == [pc.NONE_WORD] * 2
        full = tables[("all solid", d)]
        case = pc.cases()["all solid"]
        assert (full["overlap"] == int(case["shape"].sum())).all() and full["count"].tolist() == [0, 0] and full["best"].tolist() == [pc.NONE_WORD] * 2
        empty = tables[("an empty lattice", d)]                              # everything is free, nothing is supported: the border is no floor
        assert not empty["overlap"].any() and not empty["support"].any() and empty["count"].tolist() == [empty["overlap"].size, 0]
        assert empty["best"][1] == pc.NONE_WORD and empty["best"][0] != pc.NONE_WORD


# ----------------------------------------------------------------------------- hand lattices
def test_the_object_with_a_foot_by_hand():
    key = pc.hover_room()
    shape, origin = placement.object_of(key, 2)
    assert origin == (3, 3, 7) and shape.shape == (2, 2, 2) and shape.dtype == torch.uint8
    assert shape[:, :, 1].all() and shape[:, :, 0].reshape(-1).tolist() == [1, 0, 0, 0]          # the plate and the one foot
    t = host(key, shape, 3, solid=1, direction="-z", target=origin)
    assert t["overlap"].shape == (5, 5, 13) and int(t["rejected"][0]) == 0
    assert (t["overlap"][:, :, 0] > 0).all()                                                     # the foot or the plate inside the floor
    assert t["overlap"][3, 3, 1] == 0 and t["support"][3, 3, 1] == 1                              # it stands on its foot alone
    assert t["overlap"][0, 0, 1] == 1 and t["overlap"][1, 1, 1] == 5 and t["overlap"][0, 0, 2] == 1     # a corner of the plate, or all of it, in the block
    assert t["overlap"][1, 1, 3] == 1 and t["support"][1, 1, 4] == 1 and t["overlap"][1, 1, 4] == 0     # the foot in the block, then on its top
    assert t["support"][0, 0, 3] == 1 and t["overlap"][0, 0, 3] == 0                              # the plate's face (1, 1) on the block's top at z 3
    assert t["support"][2, 2, 4] == 1 and t["overlap"][2, 2, 4] == 0
    assert not t["support"][:, :, 5:].any() and not t["overlap"][:, :, 4:].any()
    assert placement.split_best(t["best"][0], t["overlap"].shape) == (0, origin)                  # where it hovers it is free
    assert placement.split_best(t["best"][1], t["overlap"].shape) == (11, (2, 2, 4))              # the foot on the block's nearest corner
    up = host(key, shape, 3, solid=1, direction="+z", target=origin)                             # under the block is only the block: no free place
    assert np.array_equal(up["overlap"], t["overlap"]) and up["support"][0, 0, 0] == 1 and up["count"].tolist() == [int(t["count"][0]), 0]
    assert up["best"][1] == pc.NONE_WORD
    assert pc.same(t, pc.brute(key, 3, 1, shape.numpy(), "-z", origin)) == ""


def test_of_two_translations_at_one_distance_the_smaller_lin_wins():
    key = np.zeros((1, 1, 9), np.int32)
    key[0, 0, 4] = 1
    one = np.ones((1, 1, 1), np.uint8)
    t = host(key, one, 2, direction="-z", target=(0, 0, 4))
    assert t["overlap"].reshape(-1).tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and t["support"].reshape(-1).tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert t["best"].tolist() == [(1 << 31) | 3, (1 << 31) | 5] and t["count"].tolist() == [8, 1]  # 3 and 5 tie on distance: 3 wins
    assert placement.split_best(t["best"][0], (1, 1, 9)) == (1, (0, 0, 3)) and placement.split_best(pc.NONE_WORD, (1, 1, 9)) is None
    t = host(key, one, 2, direction="+z", target=(0, 0, 4))
    assert t["best"].tolist() == [(1 << 31) | 3, (1 << 31) | 3]
    plane = np.zeros((3, 3, 1), np.int32)
    plane[1, 1, 0] = 1
    t = host(plane, one, 2, direction="-x", target=(1, 1, 0))                                     # four free neighbours at distance 1
    assert t["best"].tolist() == [(1 << 31) | 1, (1 << 31) | 7] and placement.split_best(t["best"][1], (3, 3, 1)) == (1, (2, 1, 0))


def test_a_target_outside_is_clamped_and_none_is_the_corner():
    case = pc.cases()[pc.SMALL]
    T = (4, 4, 6)
    for target, clamped in (((100, -4, 3), (3, 0, 3)), ((-1, -1, -1), (0, 0, 0)), (None, (0, 0, 0)), ((2, 9, 99), (2, 3, 5))):
        got = host(case["key"], case["shape"], case["n_keys"], target=target)
        want = host(case["key"], case["shape"], case["n_keys"], target=clamped)
        assert pc.same(got, want) == "" and got["overlap"].shape == T
    assert pc.same(host(case["key"], case["shape"], case["n_keys"], target=(3, 0, 3)), pc.brute(case["key"], case["n_keys"], None, case["shape"], "-z", (3, 0, 3))) == ""


def test_min_support_one_against_two():
    key = np.zeros((4, 1, 3), np.int32)
    key[0:2, 0, 0] = 1                                                      # a floor under x 0..1 only
    bar = np.ones((2, 1, 1), np.uint8)
    one, two = host(key, bar, 2, min_support=1), host(key, bar, 2, min_support=2)
    assert one["support"][:, 0, 1].tolist() == [2, 1, 0] and np.array_equal(one["support"], two["support"]) and np.array_equal(one["overlap"], two["overlap"])
    assert one["count"].tolist() == [7, 2] and two["count"].tolist() == [7, 1]
    assert placement.split_best(one["best"][1], (3, 1, 3)) == (1, (0, 0, 1)) and placement.split_best(two["best"][1], (3, 1, 3)) == (1, (0, 0, 1))
    far = host(key, bar, 2, min_support=1, target=(2, 0, 1))
    assert placement.split_best(far["best"][1], (3, 1, 3)) == (1, (1, 0, 1))
    assert placement.split_best(host(key, bar, 2, min_support=2, target=(2, 0, 1))["best"][1], (3, 1, 3)) == (4, (0, 0, 1))
    assert host(key, bar, 2, min_support=3)["best"][1] == pc.NONE_WORD


def test_every_form_of_solid():
    case = pc.cases()["solid names key 0 too"]
    key, shape = case["key"], case["shape"]
    forms = {"none": (None, [1, 2, 3, 4]), "int": (2, [2]), "list": ([0, 2], [0, 2]), "bool": (np.array([False, True, False, False, True]), [1, 4]),
             "tensor": (torch.tensor([True, False, False, True, False]), [0, 3])}
    for name, (solid, keys) in forms.items():
        got = host(key, shape, 5, solid=solid, direction="+y")
        assert pc.same(got, pc.brute(key, 5, keys, shape, "+y")) == "", name
    assert pc.same(host(key == 2, shape), host(key, shape, 5, solid=2)) == ""                   # a bool lattice: n_keys = 2, key 1 solid


def test_a_rejected_key_is_not_solid():
    key = np.zeros((1, 1, 6), np.int32)
    key[0, 0, [1, 3]] = [7, -2]
    key[0, 0, 5] = 1
    t = host(key, np.ones((1, 1, 1), np.uint8), 2, direction="+z")
    assert int(t["rejected"][0]) == 2 and t["overlap"].reshape(-1).tolist() == [0, 0, 0, 0, 0, 1] and t["support"].reshape(-1).tolist() == [0, 0, 0, 0, 1, 0]
    with pytest.raises(_lib.CliftError, match=r"lattice_placement: 2 lattice points carry a key outside \[0, 2\)"):
        placement.lattice_placement(key, np.ones((1, 1, 1), np.uint8), 2, backend="host")
    case = pc.cases()["rejected keys"]
    assert int(pc.host_tables()[("rejected keys", "-z")]["rejected"][0]) == int(((case["key"] < 0) | (case["key"] >= 3)).sum()) > 50


# ----------------------------------------------------------------------------- the identities
def two_keys(key, u):
    """A lattice of clearance_cases reduced to two keys: 2 = key ``u``, 1 = every other key >= 1."""
    return np.where(key == u, 2, np.where(key > 0, 1, 0)).astype(np.int32)


def clearance_identity(key, tables_of, clr):
    """The three identities between the placement map of object 2 over solid 1 and the clearance tables ``clr`` of the same lattice; ->
    the number of (direction, step) checks made."""
    shape, origin = placement.object_of(key, 2)
    checks = 0
    for d, name in enumerate(pc.DIRECTIONS):
        s = int(clr["travel"][2, d])
        if s == cc.NONE:
            continue
        t = tables_of(key, shape, name, origin)
        T = t["overlap"].shape
        e = np.zeros(3, np.int64)
        e[d // 2] = 1 if d % 2 == 0 else -1
        at = lambda k: tuple(int(x) for x in np.asarray(origin) + k * e)
        inside = lambda p: all(0 <= p[a] < T[a] for a in range(3))
        for k in range(s + 1):
            if inside(at(k)):
                assert t["overlap"][at(k)] == 0, (name, k)
                checks += 1
        if inside(at(s)):
            assert t["support"][at(s)] == clr["landing"][2, 1, d], name
            checks += 1
        if inside(at(s + 1)):
            assert t["overlap"][at(s + 1)] > 0, name
            checks += 1
    return checks


def identity_lattices():
    out = {"the object with a foot": pc.hover_room(), "cup": two_keys(cc.cup_room(), 3), "table": two_keys(cc.cup_room(), 2),
           "slack steps": cc.slack_steps(), "C shape": two_keys(cc.c_shape(), 2)}
    for j, shape in enumerate([(5, 6, 7), (17, 9, 70)]):
        out[f"random {shape}"] = two_keys(cc.random_key(shape, 4, 0.9, 40 + j), 2)
    return out


def test_the_identity_with_the_host_clearance():
    checks = 0
    for name, key in identity_lattices().items():
        clr = cc.to_numpy(clearance.lattice_clearance(key, 3, 0, backend="host"))
        checks += clearance_identity(key, lambda k, shape, d, origin: host(k, shape, 3, solid=1, direction=d, target=origin), clr)
    assert checks > 60
    key = pc.hover_room()
    clr = cc.to_numpy(clearance.lattice_clearance(key, 3, 0, backend="host"))
    assert int(clr["travel"][2, 5]) == 6 and int(clr["landing"][2, 1, 5]) == 1                    # the foot: 6 steps down onto one face
    t = host(key, placement.object_of(key, 2)[0], 3, solid=1)
    assert t["overlap"][3, 3, 1:8].tolist() == [0] * 7 and t["support"][3, 3, 1] == 1 and t["overlap"][3, 3, 0] > 0


def test_the_identity_with_placement_from_keys():
    rest = np.zeros((8, 8, 8), np.int32)
    rest[:, :, :2] = 1
    rest[2:5, 2:5, 2:4] = 1
    moved = np.zeros((8, 8, 8), np.int32)
    moved[3:6, 4:7, 3:6] = 1
    moved[3, 4, 3] = 0
    key = rest + 2 * moved
    ticks = [np.linspace(0.0, 0.7, 8), np.linspace(0.0, 1.4, 8), np.linspace(-0.35, 0.0, 8)]
    shape, origin = placement.object_of(key >= 2, 1)
    assert origin == (3, 4, 3) and int(shape.sum()) == 26
    t = host(key, shape, 4, solid=[1, 3], target=origin)
    found = distance.placement_from_keys(key, ticks, backend="host")
    assert int(t["overlap"][origin]) == int((key == 3).sum()) == found["overlap"] == 1
    snap = placement.snap_from_keys(key, ticks, backend="host")
    assert snap["found"] and snap["overlap_before"] == 1 and snap["n_moved"] == 26 and snap["steps"].tolist() == [0, 0, 1]
    assert snap["dist2"] == 1 and snap["support"] == 1 and np.allclose(snap["offset"], [0.0, 0.0, 0.05]) and np.allclose(snap["spacing"], [0.1, 0.2, 0.05])
    assert snap["n_free"] == int(t["count"][0]) and snap["n_supported"] == int(t["count"][1]) and snap["direction"] == "-z"
    key2 = key.copy()
    key2[key2 == 1] = 0
    key2[key2 == 3] = 2
    none = placement.snap_from_keys(key2, ticks, backend="host")                                 # nothing else in the scene: nothing to stand on
    assert not none["found"] and none["steps"].tolist() == [0, 0, 0] and none["offset"].tolist() == [0.0, 0.0, 0.0] and none["support"] is None
    with pytest.raises(_lib.CliftError, match="moved set is empty"):
        placement.snap_from_keys(rest, ticks, backend="host")


# ----------------------------------------------------------------------------- the summary and the helpers
def test_the_summary_object_of_and_node_placement():
    key = cc.cup_room()
    shape, origin = placement.object_of(key, 3)
    assert origin == (4, 4, 8) and shape.shape == (3, 3, 2) and bool(shape.all())
    with pytest.raises(ValueError, match="no lattice point carries key 5"):
        placement.object_of(key, 5)
    tables, at = placement.node_placement(key, 4, 3, backend="host")
    assert at == origin
    want = host(key, shape, 4, solid=[1, 2], target=origin)
    assert pc.same(pc.to_numpy(tables), want) == ""
    assert placement.split_best(tables["best"][0], (10, 10, 11)) == (0, origin)                   # where it stands it is free
    assert placement.split_best(tables["best"][1], (10, 10, 11)) == (9, (4, 4, 5))                # 3 points down: on the table
    assert int(tables["support"][4, 4, 5]) == 9
    with pytest.raises(ValueError, match=r"node key 4 lies outside \[1, 4\)"):
        placement.node_placement(key, 4, 4, backend="host")
    summary = placement.PlacementMap.from_tables(tables, origin, cc.CUP_TICKS)
    d = summary.to_dict()
    assert d["n_translations"] == 1100 and d["n_free"] == int(tables["count"][0]) and d["n_supported"] == int(tables["count"][1]) and d["origin"] == [4, 4, 8]
    assert d["best_free"] == dict(translation=[4, 4, 8], steps=[0, 0, 0], offset=[0.0, 0.0, 0.0], overlap=0, support=0, dist2=0)
    best = d["best_supported"]
    assert best["translation"] == [4, 4, 5] and best["steps"] == [0, 0, -3] and best["overlap"] == 0 and best["support"] == 9 and best["dist2"] == 9
    assert np.allclose(best["offset"], [0.0, 0.0, -0.3])
    assert json.loads(summary.to_json()) == d and summary == placement.PlacementMap.from_tables(want, origin, cc.CUP_TICKS)
    none = placement.PlacementMap.from_tables(pc.host_tables()[("an empty lattice", "-z")], (0, 0, 0), [np.arange(5.0), np.arange(4.0), np.arange(70.0)])
    assert none.best_supported is None and none.best_free["translation"] == list(pc.cases()["an empty lattice"]["target"])


# ----------------------------------------------------------------------------- the errors of the module
def test_argument_errors_come_before_any_launch():
    key = cc.cup_room()
    one = np.ones((2, 2, 2), np.uint8)
    for kw, msg in ((dict(n_keys=0), "n_keys must be 1 .. 1024"), (dict(n_keys=1025), "n_keys must be 1 .. 1024"), (dict(backend="cpu"), "backend"),
                    (dict(solid=4), r"site key 4 lies outside \[0, 4\)"), (dict(solid=np.array([True, False])), "a bool site table holds n_keys = 4 entries"),
                    (dict(direction="down"), "direction must be one of"), (dict(direction=5), "direction must be one of"),
                    (dict(min_support=0), r"min_support must be >= 1 \(got 0\)"), (dict(target=(1, 2)), "target must be three indices"),
                    (dict(shape=np.zeros((2, 2, 2), np.uint8)), "the shape holds no cell"), (dict(shape=one[0]), r"shape must be \(m0, m1, m2\)"),
                    (dict(shape=one.astype(np.float32)), "shape must be bool or integer"),
                    (dict(shape=np.ones((13, 2, 2), np.uint8)), r"every shape dimension must be 1 .. the lattice's \(got 13 x 2 x 2 in 12 x 12 x 12\)"),
                    (dict(shape=np.ones((2, 0, 2), np.uint8)), "every shape dimension must be 1 .. the lattice's")):
        with pytest.raises(ValueError, match=msg):
            placement.placement_tables(key, **{"shape": one, "n_keys": 4, "backend": "host", **kw})
    with pytest.raises(ValueError, match=r"\(n0, n1, n2\)"):
        placement.placement_tables(key[0], one, 4, backend="host")
    with pytest.raises(ValueError, match="bool or integer"):
        placement.placement_tables(key.astype(np.float32), one, 4, backend="host")
    with pytest.raises(ValueError, match="1 .. 16384"):
        placement.placement_tables(np.zeros((1, 1, 16385), np.int32), np.ones((1, 1, 1), np.uint8), 2, backend="host")
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        placement.placement_tables(key, one, 4)                                                   # a host tensor: no quiet fall-back
    assert placement.placement_tables(key, one, backend="host")["overlap"].shape == (11, 11, 11)  # n_keys = max + 1
    assert placement.work_words((128, 128, 128), (24, 24, 32)) == 130 * 130 * 3 + 2 * 26 * 26 * 1


# ----------------------------------------------------------------------------- the entry point's declarations
NAMES = ["key", "n0", "n1", "n2", "n_keys", "solid", "shape", "m0", "m1", "m2", "direction", "min_support", "t0", "t1", "t2", "overlap", "support", "count",
         "best", "rejected", "work", "s"]


def test_the_entry_point_is_declared_exported_and_documented():
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    m = re.search(r"\bint\s+clift_lattice_placement\s*\(([^)]*)\)\s*;", src)
    assert m, "clift_lattice_placement is not declared in include/clift.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    argtypes, restype = _lib._SIGNATURES["clift_lattice_placement"]
    assert len(args) == len(argtypes) == 22 and restype is ctypes.c_int
    ints = [i for i, a in enumerate(args) if re.fullmatch(r"int\s+\w+", a)]
    assert ints == [i for i, t in enumerate(argtypes) if t is ctypes.c_int] == [1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14]
    assert all("*" in a or a.startswith("clift_stream_t") for i, a in enumerate(args) if i not in ints)
    assert [a.split()[-1].lstrip("*") for a in args] == NAMES
    assert re.search(r"#define\s+CLIFT_PM_NONE\s+CLIFT_DT_NONE", src) and placement.NONE_WORD == distance.NONE_WORD
    assert "the lattice border is not a floor" in src and "CLIFT_PM_WORK_WORDS" in src
    assert _lib.ABI_VERSION == 27
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clift_lattice_placement"), "clift_lattice_placement is not exported by libclift.so"
    assert "clift_lattice_placement" in _lib.exported_symbols()
    assert "placement.hip" in open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "Makefile")).read()
    for doc in ("DESIGN.md", "README.md"):
        assert "clift_lattice_placement" in open(os.path.join(REPO, doc)).read(), doc


def test_errors_of_the_entry_point_need_no_device():
    """Every check of the entry point comes before the device is touched: made-up addresses stand in for device memory."""
    lib = _lib.load()
    p = {name: ctypes.c_void_p(64 * (i + 1)) for i, name in enumerate(("key", "solid", "shape", "overlap", "support", "count", "best", "rejected", "work"))}
    good = dict(p, n=(4, 5, 6), n_keys=3, m=(2, 2, 2), direction=5, min_support=1, target=(0, 0, 0))
    bad = [(dict(n=(0, 4, 4)), r"clift_lattice_placement: lattice dimensions must be 1 .. 16384 \(got 0 x 4 x 4\)"),
           (dict(n=(4, -1, 4)), r"lattice dimensions must be 1 .. 16384 \(got 4 x -1 x 4\)"),
           (dict(n=(4, 4, 16385)), r"lattice dimensions must be 1 .. 16384 \(got 4 x 4 x 16385\)"),
           (dict(m=(0, 2, 2)), r"clift_lattice_placement: shape dimensions must be 1 .. the lattice's \(got 0 x 2 x 2 in 4 x 5 x 6\)"),
           (dict(m=(5, 2, 2)), r"shape dimensions must be 1 .. the lattice's \(got 5 x 2 x 2 in 4 x 5 x 6\)"),
           (dict(m=(2, 2, 7)), r"shape dimensions must be 1 .. the lattice's \(got 2 x 2 x 7 in 4 x 5 x 6\)"),
           (dict(n=(2048, 1024, 1024)), r"clift_lattice_placement: 2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           (dict(n_keys=0), r"clift_lattice_placement: n_keys must be 1 .. 1024 \(got 0\)"), (dict(n_keys=1025), r"n_keys must be 1 .. 1024 \(got 1025\)"),
           (dict(direction=6), r"clift_lattice_placement: direction must be 0 .. 5 \(got 6\)"), (dict(direction=-1), r"direction must be 0 .. 5 \(got -1\)"),
           (dict(min_support=0), r"clift_lattice_placement: min_support must be >= 1 \(got 0\)"),
           (dict(target=(3, 0, 0)), r"clift_lattice_placement: target must lie inside the 3 x 4 x 5 translations \(got 3, 0, 0\)"),
           (dict(target=(0, -1, 0)), r"target must lie inside the 3 x 4 x 5 translations \(got 0, -1, 0\)"),
           (dict(target=(0, 0, 5)), r"target must lie inside the 3 x 4 x 5 translations \(got 0, 0, 5\)")]
    bad += [({name: None}, "clift_lattice_placement: NULL device buffer") for name in p]
    for kw, msg in bad:
        a = {**good, **kw}
        with pytest.raises(_lib.CliftError, match=msg):
            _lib.call("clift_lattice_placement", a["key"], *a["n"], a["n_keys"], a["solid"], a["shape"], *a["m"], a["direction"], a["min_support"],
                      *a["target"], a["overlap"], a["support"], a["count"], a["best"], a["rejected"], a["work"], None)
    assert lib is not None


# ----------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def es():
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene
    finally:
        sys.path.pop(0)
    return edit_scene


def test_refusals_of_snap_placement(es, capsys, tmp_path, monkeypatch):
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", "b.pkl", "--instance", "3"]
    for op in ("delete", "extract"):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", op, "--snap_placement"])
        assert "--snap_placement moves the object that a move or a copy places" in capsys.readouterr().err
    for extra, msg in ((["--snap_placement", "--settle"], "--snap_placement cannot be combined with --settle"),
                       (["--settle", "+x", "--snap_placement", "-y"], "--snap_placement cannot be combined with --settle"),
                       (["--snap_placement", "--snap_upsample", "0"], "--snap_upsample must be >= 1"),
                       (["--snap_placement", "--snap_min_support", "0"], "--snap_min_support must be >= 1"),
                       (["--snap_upsample", "2"], "--snap_upsample needs --snap_placement"),
                       (["--snap_min_support", "2"], "--snap_min_support needs --snap_placement"),
                       (["--snap_placement=up"], "--snap_placement: AXIS is one of")):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", "move"] + extra)
        assert msg in capsys.readouterr().err, extra
    a = es.parse_args(common + ["--op", "move", "--snap_placement"])
    assert a.snap_placement == "-z" and a.snap_upsample == 1 and a.snap_min_support == 1 and a.settle is None and not a.check_placement
    a = es.parse_args(common + ["--op", "copy", "--snap_placement", "-y", "--snap_upsample", "2", "--snap_min_support", "4", "--check_placement"])
    assert a.snap_placement == "-y" and a.snap_upsample == 2 and a.snap_min_support == 4 and a.check_placement
    a = es.parse_args(common + ["--op", "copy", "--settle", "-x"])                                # the other flag parses as before
    assert a.settle == "-x" and a.snap_placement is None and a.snap_upsample is None
    boxes = {3: {"bbox": (-np.ones(3), np.ones(3)), "orientation": np.eye(3), "position": np.zeros(3)}}
    good = [{"instance": 3, "op": "delete"}, {"instance": 3, "op": "copy", "translate": [0.5, 0, 0]}]
    es.check_snap(es.resolve_program(boxes, good))
    es.check_snap(es.resolve_edit(boxes, 3, "move", [0.1, 0, 0]))
    for bad in (es.resolve_program(boxes, good[::-1]), es.resolve_edit(boxes, 3, "extract")):
        with pytest.raises(SystemExit, match="--snap_placement moves the object that a move or a copy places"):
            es.check_snap(bad)
    monkeypatch.setattr(es, "load_run_config", lambda p: type("Cfg", (), {})())
    path = tmp_path / "ends_in_delete.json"
    path.write_text(json.dumps(good[::-1]))
    pkl = tmp_path / "b.pkl"
    with open(pkl, "wb") as f:
        pickle.dump(boxes, f)
    with pytest.raises(SystemExit, match="--snap_placement moves the object that a move or a copy places"):
        es.main(["--ckpt_path", str(tmp_path / "runs" / "x" / "checkpoints" / "y.ckpt"), "--bboxes", str(pkl), "--script", str(path), "--snap_placement"])
    found = dict(found=True, steps=np.array([0, -2, 3]), offset=np.array([0.0, -0.2, 0.3]), overlap_before=140, support_before=0, support=7, dist2=13)
    assert es.snap_line(found) == "snapped by (0, -2, 3) steps = 0.3606 onto 7 faces (was: collides on 140 cells)"
    assert es.snap_line(dict(found, overlap_before=0)) == "snapped by (0, -2, 3) steps = 0.3606 onto 7 faces (was: free on 0 faces)"
    assert es.snap_line(dict(found, found=False)) == "not snapped: no free supported position"
    moved = es.settled_edit(es.resolve_edit(boxes, 3, "move", [0.1, 0, 0]), found["offset"])
    assert np.allclose(moved.dst.centre - moved.src.centre, [0.1, -0.2, 0.3])
