"""The lattice distance transform without a GPU: ``distance.distance_tables(backend="host")`` against a brute force over all
(point, site) pairs and against scipy, the tie rule by hand, the site tables, rejected keys, ``key_min`` and ``separation`` against plain
loops, the two identities with the host relations and clearance tables, ``Separation``, every error of the module, the declarations of the
new entry point, and the refusals of the two command lines.  Exact integers throughout."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import clearance_cases as cc
import distance_cases as dc
import relations_cases as rc
from conftest import REPO

from contrastive_lift_amd import _lib, clearance, distance, relations


def host(key, n_keys=None, sites=None, key_min=False):
    return dc.to_numpy(distance.distance_tables(key, n_keys, sites, key_min, backend="host"))


# ----------------------------------------------------------------------------- the host backend against the brute force and scipy
@pytest.mark.parametrize("density", dc.DENSITIES)
@pytest.mark.parametrize("shape", dc.BRUTE_SHAPES)
def test_host_backend_against_the_brute_force(shape, density):
    key = dc.random_sites(shape, density, sum(shape) + int(100 * density))
    got = host(key, 2, key_min=True)
    want = dc.brute_packed(key, 2, dc.table_of(None, 2))
    assert got["packed"].dtype == np.int64 and got["packed"].shape == shape and np.array_equal(got["packed"], want)
    assert dc.check_nearest(key, 2, dc.table_of(None, 2), got["packed"]) == ""
    assert np.array_equal(got["key_min"], dc.loop_key_min(key, 2, want)) and got["key_min"].dtype == np.int64
    assert got["rejected"].dtype == np.int32 and got["rejected"].tolist() == [0]
    if key.any():
        assert np.array_equal(got["packed"] >> 31, dc.scipy_dist2(key != 0))


@pytest.mark.parametrize("shape", dc.SCIPY_SHAPES)
def test_dist2_against_scipy(shape):
    for density in (0.002, 0.1):
        key = dc.random_sites(shape, density, sum(shape))
        key[0, 0, 0] = 1                                                    # (scipy wants a site)
        packed = host(key, 2)["packed"]
        dist2, nearest = distance.split(packed)
        assert dist2.dtype == np.int32 and nearest.dtype == np.int32 and np.array_equal(dist2, dc.scipy_dist2(key != 0))
        assert dc.check_nearest(key, 2, dc.table_of(None, 2), packed) == ""


def test_of_two_sites_at_one_distance_the_lower_index_wins():
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = 5
        key = np.zeros(shape, np.int32)
        key.reshape(-1)[[0, 4]] = 1
        dist2, nearest = distance.split(host(key, 2)["packed"])
        assert dist2.reshape(-1).tolist() == [0, 1, 4, 1, 0] and nearest.reshape(-1).tolist() == [0, 0, 0, 4, 4]
    key = np.zeros((3, 3, 3), np.int32)                                     # the eight corners around the centre: lin 0 wins
    key[::2, ::2, ::2] = 1
    dist2, nearest = distance.split(host(key, 2)["packed"])
    assert dist2[1, 1, 1] == 3 and nearest[1, 1, 1] == 0 and dist2[1, 1, 2] == 2 and nearest[1, 1, 2] == 2
    key = np.zeros((3, 3, 1), np.int32)                                     # a tie between two axes: (0, 1) lin 1 and (1, 0) lin 3
    key[0, 1, 0] = key[1, 0, 0] = 1
    assert distance.split(host(key, 2)["packed"])[1][1, 1, 0] == 1 and distance.split(host(key, 2)["packed"])[1][0, 0, 0] == 1


def test_site_tables():
    key = cc.random_key((5, 6, 7), 5, 0.4, 3)
    every = host(key, 5)["packed"]
    assert np.array_equal(every, dc.brute_packed(key, 5, dc.table_of(None, 5)))
    for sites, table in ((3, dc.table_of(3, 5)), ([3], dc.table_of(3, 5)), ((1, 2, 4), dc.table_of([1, 2, 4], 5)), (np.int64(2), dc.table_of(2, 5)),
                         (np.array([False, True, True, False, True]), dc.table_of([1, 2, 4], 5)), (torch.tensor([True, False, False, False, True]), dc.table_of([0, 4], 5)),
                         (range(1, 5), dc.table_of(None, 5)), ([], np.zeros(5, bool))):
        assert np.array_equal(host(key, 5, sites)["packed"], dc.brute_packed(key, 5, table)), sites
    # background as the site: the distance to the nearest empty point, scipy on the complement
    free = host(key, 5, 0)["packed"]
    assert np.array_equal(free >> 31, dc.scipy_dist2(key == 0)) and dc.check_nearest(key, 5, dc.table_of(0, 5), free) == ""
    # no site at all
    none = host(key, 5, [], key_min=True)
    dist2, nearest = distance.split(none["packed"])
    assert (none["packed"] == dc.NONE_WORD).all() and (dist2 == dc.NONE).all() and (nearest == -1).all() and (none["key_min"] == dc.NONE_WORD).all()
    dist2, nearest = distance.split(torch.from_numpy(none["packed"]))
    assert dist2.dtype == torch.int32 and bool((dist2 == dc.NONE).all()) and bool((nearest == -1).all())
    assert distance.NONE == dc.NONE and distance.NONE_WORD == dc.NONE_WORD and distance.MAX_DIM == dc.MAX_DIM


def test_a_rejected_key_is_no_site_and_in_no_minimum():
    key = np.asarray([1, 0, 9, 0, 0, 2, -1, 0, 1], np.int32).reshape(1, 1, 9)
    got = host(key, 3, None, key_min=True)
    table = dc.table_of(None, 3)
    assert got["rejected"].tolist() == [2] and np.array_equal(got["packed"], dc.brute_packed(key, 3, table))
    dist2, nearest = distance.split(got["packed"])
    assert dist2.reshape(-1).tolist() == [0, 1, 4, 4, 1, 0, 1, 1, 0] and nearest.reshape(-1).tolist() == [0, 0, 0, 5, 5, 5, 5, 8, 8]
    assert np.array_equal(got["key_min"], dc.loop_key_min(key, 3, got["packed"])) and got["key_min"].tolist() == [dc.NONE_WORD, 0, 5]
    key, n_keys, _ = rc.cases()["rejected keys"]
    got = host(key, n_keys, [1, 2], key_min=True)
    assert int(got["rejected"][0]) == int(((key < 0) | (key >= n_keys)).sum()) > 100
    assert dc.check_nearest(key, n_keys, dc.table_of([1, 2], n_keys), got["packed"]) == ""
    assert np.array_equal(got["key_min"], dc.loop_key_min(key, n_keys, got["packed"]))
    with pytest.raises(_lib.CliftError, match="outside"):
        distance.lattice_distance(key, n_keys, backend="host")
    with pytest.raises(_lib.CliftError, match="outside"):
        distance.separation(key, n_keys, backend="host")


# ----------------------------------------------------------------------------- key_min, voronoi_keys and separation against loops
@pytest.mark.parametrize("name", sorted(dc.separation_lattices()))
def test_key_min_and_separation_against_the_loops(name):
    key, n_keys = dc.separation_lattices()[name]
    for v in sorted(set(np.unique(key).tolist()) - {0})[:3]:
        got = host(key, n_keys, v, key_min=True)
        assert np.array_equal(got["packed"], dc.brute_packed(key, n_keys, dc.table_of(v, n_keys))), v
        assert np.array_equal(got["key_min"], dc.loop_key_min(key, n_keys, got["packed"])), v
    sep = dc.to_numpy(distance.separation(key, n_keys, backend="host"))
    want = dc.loop_separation(key, n_keys)
    assert dc.same(sep, want, ("gap2", "at", "to")) == "", dc.same(sep, want, ("gap2", "at", "to"))
    assert np.array_equal(sep["gap2"], sep["gap2"].T) and (np.diag(sep["gap2"]) == dc.NONE).all() and (sep["gap2"][0] == dc.NONE).all()
    found = sep["gap2"] != dc.NONE
    flat = key.reshape(-1)
    u, v = np.nonzero(found)
    assert np.array_equal(flat[sep["at"][found]], u) and np.array_equal(flat[sep["to"][found]], v) and (sep["at"][~found] == -1).all()


def test_the_cup_and_the_table_by_hand():
    sep = dc.to_numpy(distance.separation(cc.cup_room(), 4, backend="host"))
    assert sep["gap2"][3, 2] == 16 and sep["gap2"][2, 3] == 16                                     # 3 empty points: 4 steps
    assert sep["gap2"][2, 1] == 1 and sep["gap2"][3, 1] == 4                                      # on the floor; the ceiling one empty point above
    assert sep["at"][3, 2] == (4 * 12 + 4) * 12 + 8 and sep["to"][3, 2] == (4 * 12 + 4) * 12 + 4
    diag = np.zeros((4, 4, 4), np.int32)                                                          # diagonal neighbours: no axis look sees them
    diag[0, 0, 0], diag[1, 1, 1], diag[3, 3, 1] = 1, 2, 3
    sep = dc.to_numpy(distance.separation(diag, backend="host"))
    assert sep["gap2"][1, 2] == 3 and sep["gap2"][2, 3] == 8 and sep["gap2"][1, 3] == 19
    assert (dc.to_numpy(clearance.clearance_tables(diag, 4, backend="host"))["pair"] == cc.NONE).all()


def test_voronoi_keys():
    key = cc.random_key((5, 6, 7), 5, 0.7, 4)
    packed = distance.distance_tables(key, 5, backend="host")["packed"]
    owner = distance.voronoi_keys(key, packed).numpy()
    near = dc.brute_packed(key, 5, dc.table_of(None, 5)) & dc.MASK
    assert owner.dtype == np.int32 and np.array_equal(owner, key.reshape(-1)[near]) and np.array_equal(owner[key > 0], key[key > 0]) and (owner > 0).all()
    capped = distance.voronoi_keys(key, packed.numpy(), max_dist2=1).numpy()
    assert np.array_equal(capped, np.where((packed.numpy() >> 31) <= 1, owner, 0)) and (capped == 0).any()
    empty = distance.distance_tables(key, 5, sites=[], backend="host")["packed"]
    assert not distance.voronoi_keys(key, empty).any()
    with pytest.raises(ValueError, match="one lattice"):
        distance.voronoi_keys(key, packed[:2])


# ----------------------------------------------------------------------------- the identities with relations and clearance
def test_the_identities_with_the_host_relations_and_clearance():
    ones = bounded = 0
    for name, (key, n_keys) in dc.identity_lattices().items():
        sep = dc.to_numpy(distance.separation(key, n_keys, backend="host"))
        clr = dc.to_numpy(clearance.clearance_tables(key, n_keys, 0, backend="host"))
        rel = rc.to_numpy(relations.relation_tables(key, n_keys, 0, backend="host"))
        assert dc.identities(sep, clr, rel) == "", name
        ones += int((sep["gap2"] == 1).sum())
        bounded += int((clr["pair"][1:, 1:] != cc.NONE).sum())
    assert ones > 100 and bounded > 100                                                           # (the identities were not vacuous)


# ----------------------------------------------------------------------------- the summary
def test_the_summary_of_the_cup():
    key = cc.cup_room()
    tables = distance.separation(key, 4, backend="host")
    js = json.loads(distance.Separation.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS).to_json())
    assert js["max_cells"] is None and [n["key"] for n in js["nodes"]] == [1, 2, 3] and [(p["a"], p["b"]) for p in js["pairs"]] == [(1, 2), (1, 3), (2, 3)]
    cup = js["nodes"][2]
    assert (cup["semantic"], cup["instance"]) == (2, 1) and cup["nearest"]["key"] == 1 and cup["nearest"]["cells"] == 2.0
    assert abs(cup["nearest"]["distance"] - 0.2) < 1e-12                                          # the ceiling: two steps of 0.1 along z
    pair = js["pairs"][2]
    assert pair["gap2"] == 16 and pair["cells"] == 4.0 and abs(pair["distance"] - 0.4) < 1e-12
    t = cc.CUP_TICKS
    assert pair["point_a"] == [float(t[0][4]), float(t[1][4]), float(t[2][4])] and pair["point_b"] == [float(t[0][4]), float(t[1][4]), float(t[2][8])]
    assert js["nodes"][1]["nearest"] == dict(key=1, cells=1.0, distance=js["pairs"][0]["distance"])
    near = distance.Separation.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS, max_cells=2)
    assert [(p["a"], p["b"]) for p in near.pairs] == [(1, 2), (1, 3)] and near.max_cells == 2.0 and near.nodes == js["nodes"]
    assert near == distance.Separation.from_tables(dc.to_numpy(tables), cc.CUP_NODES, cc.CUP_TICKS, max_cells=2.0) and near != js
    alone = distance.separation(np.where(key == 3, 1, 0), 2, backend="host")
    assert distance.Separation.from_tables(alone, [(2, 1)], cc.CUP_TICKS).to_dict() == dict(max_cells=None, nodes=[dict(key=1, semantic=2, instance=1, nearest=None)], pairs=[])
    diag = np.zeros((12, 12, 12), np.int32)                                                       # a diagonal pair: the world distance over uneven steps
    diag[1, 1, 1], diag[2, 3, 4] = 1, 2
    p = distance.Separation.from_tables(distance.separation(diag, backend="host"), [(0, 0), (1, 1)], cc.CUP_TICKS).pairs[0]
    assert p["gap2"] == 14 and abs(p["distance"] - math.sqrt(0.2 ** 2 + 0.6 ** 2 + 0.3 ** 2)) < 1e-12
    with pytest.raises(ValueError, match="node list"):
        distance.Separation.from_tables(tables, cc.CUP_NODES[:2], cc.CUP_TICKS)
    with pytest.raises(ValueError, match="max_cells"):
        distance.Separation.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS, max_cells=-1)


def test_placement_from_keys_by_hand():
    ticks = cc.CUP_TICKS
    key = np.zeros((12, 12, 12), np.int32)
    key[:, :, 0:3] = 1                                                                            # a slab
    key[4:7, 4:7, 5:8] = 2                                                                        # the object, 2 empty points above it
    got = distance.placement_from_keys(key, ticks, backend="host")
    assert got["verdict"] == "clear" and got["overlap"] == 0 and got["depth2"] == 0 and got["gap2"] == 9 and got["n_moved"] == 27
    assert got["moved_point"] == [float(ticks[0][4]), float(ticks[1][4]), float(ticks[2][5])] and got["rest_point"][2] == float(ticks[2][2])
    assert np.allclose(got["spacing"], [0.2, 0.3, 0.1], atol=1e-12)
    key[4:7, 4:7, 3] = 2
    key[4:7, 4:7, 4] = 2
    assert distance.placement_from_keys(key, ticks, backend="host")["verdict"] == "touches"
    key[4:7, 4:7, 0:3] = 3                                                                        # sunk through the slab
    got = distance.placement_from_keys(key, ticks, backend="host")
    assert got["verdict"] == "collides" and got["overlap"] == 27 and got["gap2"] == 0 and got["depth2"] == 9 and got["n_moved"] == 72
    assert got["moved_point"] == got["rest_point"] == [float(ticks[0][4]), float(ticks[1][4]), float(ticks[2][0])]
    alone = distance.placement_from_keys(np.where(key >= 2, 2, 0), ticks, backend="host")
    assert alone["verdict"] == "clear" and alone["gap2"] is None and alone["rest_point"] is None
    with pytest.raises(_lib.CliftError, match="moved set is empty"):
        distance.placement_from_keys(np.where(key == 1, 1, 0), ticks, backend="host")


def test_scene_before():
    from contrastive_lift_amd import edit
    box = edit.EditBox(np.eye(3), [0.0, 0.0, 0.0], [-0.1, -0.1, -0.1], [0.1, 0.1, 0.1])
    assert distance.scene_before(edit.copy(box, [0.5, 0, 0])) is None
    mv = edit.move(box, [0.5, 0, 0])
    before = distance.scene_before(mv)
    assert len(before) == 1 and before[0].mode == edit.DELETE and before[0].src is mv.src and before[0].shape is None
    prog = edit.EditProgram([edit.delete(box), edit.copy(box, [0.5, 0, 0])])
    assert len(distance.scene_before(prog)) == 1 and distance.scene_before(prog)[0] is prog[0]
    for bad in (edit.delete(box), edit.EditProgram([mv, edit.extract(box)])):
        with pytest.raises(ValueError, match="copy or a move"):
            distance.scene_before(bad)


# ----------------------------------------------------------------------------- the errors of the module
def test_argument_errors_come_before_any_launch():
    key = cc.cup_room()
    for kw, msg in ((dict(n_keys=0), "n_keys must be 1 .. 1024"), (dict(n_keys=1025), "n_keys must be 1 .. 1024"), (dict(backend="cpu"), "backend"),
                    (dict(sites=4), r"site key 4 lies outside \[0, 4\)"), (dict(sites=[1, -1]), "site key -1 lies outside"),
                    (dict(sites=np.array([True, False])), "a bool site table holds n_keys = 4 entries"), (dict(sites=[1.5]), "sites is None, a key"),
                    (dict(sites=[True]), "sites is None, a key")):
        with pytest.raises(ValueError, match=msg):
            distance.distance_tables(key, **{"n_keys": 4, "backend": "host", **kw})
    with pytest.raises(ValueError, match=r"\(n0, n1, n2\)"):
        distance.distance_tables(key[0], 4, backend="host")
    with pytest.raises(ValueError, match="bool or integer"):
        distance.distance_tables(key.astype(np.float32), 4, backend="host")
    with pytest.raises(ValueError, match="at least one point"):
        distance.distance_tables(key[:, :0], 4, backend="host")
    with pytest.raises(ValueError, match="1 .. 16384"):
        distance.distance_tables(np.zeros((1, 1, 16385), np.int32), 2, backend="host")
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        distance.distance_tables(key, 4)                                                          # a host tensor: no quiet fall-back
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        distance.separation(key, 4)
    with pytest.raises(ValueError, match="--min_component"):
        distance.separation(key, 257, backend="host")
    assert distance.distance_tables(key, backend="host", key_min=True)["key_min"].shape == (4,)  # n_keys = max + 1
    assert distance.separation(key == 3, backend="host")["gap2"].tolist() == [[dc.NONE, dc.NONE], [dc.NONE, dc.NONE]]
    assert distance.separation(np.zeros((2, 2, 2), np.int32), 3, backend="host")["at"].tolist() == [[-1] * 3] * 3


# ----------------------------------------------------------------------------- the entry point's declarations
def test_the_entry_point_is_declared_exported_and_documented():
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    m = re.search(r"\bint\s+clift_lattice_distance\s*\(([^)]*)\)\s*;", src)
    assert m, "clift_lattice_distance is not declared in include/clift.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    argtypes, restype = _lib._SIGNATURES["clift_lattice_distance"]
    assert len(args) == len(argtypes) == 11 and restype is ctypes.c_int
    ints = [i for i, a in enumerate(args) if re.fullmatch(r"int\s+\w+", a)]
    assert ints == [i for i, t in enumerate(argtypes) if t is ctypes.c_int] == [1, 2, 3, 4]
    assert all("*" in a or a.startswith("clift_stream_t") for i, a in enumerate(args) if i not in ints)
    assert [a.split()[-1].lstrip("*") for a in args] == ["key", "n0", "n1", "n2", "n_keys", "site", "out", "work", "key_min", "rejected", "s"]
    for name, value in (("CLIFT_DT_MAX_DIM", distance.MAX_DIM), ("CLIFT_DT_NONE", distance.NONE_WORD)):
        m = re.search(rf"#define\s+{name}\s+(\w+)", src)
        assert m and int(m.group(1).rstrip("L"), 0) == value, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clift_lattice_distance"), "clift_lattice_distance is not exported by libclift.so"
    assert "clift_lattice_distance" in _lib.exported_symbols()
    assert "distance.hip" in open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "Makefile")).read()
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "clift_lattice_distance" in open(os.path.join(REPO, doc)).read(), doc


def test_errors_of_the_entry_point_need_no_device():
    """Every check of the entry point comes before the device is touched: made-up addresses stand in for device memory."""
    lib = _lib.load()
    key, site, rej = ctypes.c_void_p(8), ctypes.c_void_p(16), ctypes.c_void_p(24)
    out, work = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    good = dict(key=key, n=(4, 4, 4), n_keys=3, site=site, out=out, work=work, key_min=None, rejected=rej)
    bad = [(dict(n=(0, 4, 4)), r"clift_lattice_distance: lattice dimensions must be 1 .. 16384 \(got 0 x 4 x 4\)"),
           (dict(n=(4, -1, 4)), r"lattice dimensions must be 1 .. 16384 \(got 4 x -1 x 4\)"),
           (dict(n=(4, 4, 16385)), r"lattice dimensions must be 1 .. 16384 \(got 4 x 4 x 16385\)"),
           (dict(n=(2048, 1024, 1024)), r"clift_lattice_distance: 2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           (dict(n_keys=0), r"clift_lattice_distance: n_keys must be 1 .. 1024 \(got 0\)"), (dict(n_keys=1025), r"n_keys must be 1 .. 1024 \(got 1025\)"),
           (dict(work=out), "clift_lattice_distance: out and work overlap"),
           (dict(work=ctypes.c_void_p((1 << 20) + 8 * 63)), "out and work overlap"), (dict(work=ctypes.c_void_p((1 << 20) - 8 * 63)), "out and work overlap")]
    bad += [({name: None}, "clift_lattice_distance: NULL device buffer") for name in ("key", "site", "out", "work", "rejected")]
    for kw, msg in bad:
        a = {**good, **kw}
        with pytest.raises(_lib.CliftError, match=msg):
            _lib.call("clift_lattice_distance", a["key"], *a["n"], a["n_keys"], a["site"], a["out"], a["work"], a["key_min"], a["rejected"], None)
    assert lib is not None


# ----------------------------------------------------------------------------- the command lines
@pytest.fixture(scope="module")
def tools():
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene
        import extract_mesh
    finally:
        sys.path.pop(0)
    return edit_scene, extract_mesh


def test_refusals_of_check_placement(tools, capsys, tmp_path, monkeypatch):
    es, _ = tools
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", "b.pkl", "--instance", "3"]
    for op in ("delete", "extract"):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", op, "--check_placement"])
        assert "--check_placement checks the object that a move or a copy places" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        es.parse_args(common + ["--op", "move", "--check_placement", "--placement_upsample", "0"])
    assert "--placement_upsample" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        es.parse_args(common + ["--op", "move", "--placement_upsample", "2"])
    assert "--placement_upsample needs --check_placement" in capsys.readouterr().err
    a = es.parse_args(common + ["--op", "move", "--check_placement"])
    assert a.check_placement and a.placement_upsample == 1 and a.settle is None
    a = es.parse_args(common + ["--op", "copy", "--check_placement", "--placement_upsample", "2", "--settle"])
    assert a.check_placement and a.placement_upsample == 2 and a.settle == "-z"
    assert not es.parse_args(common + ["--op", "delete"]).check_placement
    boxes = {3: {"bbox": (-np.ones(3), np.ones(3)), "orientation": np.eye(3), "position": np.zeros(3)}}
    good = [{"instance": 3, "op": "delete"}, {"instance": 3, "op": "copy", "translate": [0.5, 0, 0]}]
    es.check_placement_edit(es.resolve_program(boxes, good))
    es.check_placement_edit(es.resolve_edit(boxes, 3, "move", [0.1, 0, 0]))
    for bad in (es.resolve_program(boxes, good[::-1]), es.resolve_edit(boxes, 3, "extract")):
        with pytest.raises(SystemExit, match="--check_placement checks the object that a move or a copy places"):
            es.check_placement_edit(bad)
    monkeypatch.setattr(es, "load_run_config", lambda p: type("Cfg", (), {})())
    path = tmp_path / "ends_in_delete.json"
    path.write_text(json.dumps(good[::-1]))
    pkl = tmp_path / "b.pkl"
    import pickle
    with open(pkl, "wb") as f:
        pickle.dump(boxes, f)
    with pytest.raises(SystemExit, match="--check_placement checks the object that a move or a copy places"):
        es.main(["--ckpt_path", str(tmp_path / "runs" / "x" / "checkpoints" / "y.ckpt"), "--bboxes", str(pkl), "--script", str(path), "--check_placement"])
    assert es.placement_line(dict(verdict="collides", overlap=12, depth2=9, gap2=0, spacing=[0.1, 0.1, 0.1], moved_point=[0, 0, 0], rest_point=[0, 0, 0])) \
        == "placement: collides on 12 cells, depth 3.00"
    assert es.placement_line(dict(verdict="clear", overlap=0, depth2=0, gap2=16, spacing=[0.1, 0.1, 0.1], moved_point=[0, 0, 0.5], rest_point=[0, 0, 0.1])) \
        == "placement: clear, gap 4.00 cells = 0.4000"
    assert es.placement_line(dict(verdict="clear", overlap=0, depth2=0, gap2=None, spacing=[0.1] * 3, moved_point=None, rest_point=None)) \
        == "placement: clear, nothing else in the scene"


def test_refusals_of_the_separation_flags_of_the_mesh_tool(tools, capsys):
    _, xm = tools
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt"]
    with pytest.raises(SystemExit):
        xm.build_parser().parse_args(common + ["--separation_max_cells", "3"])
    assert "--separation_max_cells needs --separation" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        xm.build_parser().parse_args(common + ["--separation", "--separation_max_cells", "-1"])
    assert "--separation_max_cells" in capsys.readouterr().err
    a = xm.build_parser().parse_args(common + ["--separation"])
    assert a.separation and a.separation_max_cells is None and xm.separation_options(a) == dict(max_cells=None) and not a.relations and not a.clearance
    a = xm.build_parser().parse_args(common + ["--separation", "--separation_max_cells", "6", "--relations", "--clearance"])
    assert xm.separation_options(a) == dict(max_cells=6.0) and xm.relations_options(a) is not None and xm.clearance_options(a) == dict(slack=0)
    assert xm.separation_options(xm.build_parser().parse_args(common)) is None
    assert xm.separation_stem(None) == "separation" and xm.separation_stem("move_3") == "separation_edit_move_3"
