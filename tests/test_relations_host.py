"""Lattice relations without a GPU: backend="host" against the triple-loop restatement of tests/relations_cases.py on every case, the
hand-checked numbers of the room and its scene graph under +z and, flipped, under -z, node_keys, the errors, the new library entry declared /
exported / bound at ABI 27 and refusing bad arguments before it touches the device, and the command line's new flags."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import relations_cases as rc


@pytest.fixture(scope="module")
def looped():
    """case name -> the triple loop's tables: computed once, left unchanged."""
    return {name: rc.loop_relations(*case) for name, case in rc.cases().items()}


def host(key, n_keys, gap):
    from contrastive_lift_amd import relations
    return rc.to_numpy(relations.relation_tables(key, n_keys, gap, backend="host"))


# ============================================================================ the host backend
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_host_backend_equals_the_triple_loop(looped, name):
    key, n_keys, gap = rc.cases()[name]
    got = host(key, n_keys, gap)
    assert got["count"].dtype == np.int64 and got["isum"].shape == (n_keys, 3) and got["ibox"].shape == (n_keys, 6)
    assert got["faces"].shape == (n_keys, n_keys, 3) and (got["near"] is None) == (gap == 0)
    assert rc.same_tables(got, looped[name]) == "", (name, rc.same_tables(got, looped[name]))
    assert int(got["count"].sum()) + int(got["rejected"][0]) == key.size
    assert not got["faces"][np.arange(n_keys), np.arange(n_keys)].any()                      # the diagonal stays 0


def test_the_large_skewed_case_on_the_host():
    key, n_keys, gap = rc.skew_case()
    assert key.size == 64 ** 3 and (key == 1).mean() > 0.985
    assert rc.same_tables(host(key, n_keys, gap), rc.loop_relations(key, n_keys, gap)) == ""


@pytest.mark.parametrize("name", sorted(rc.long_cases()))
def test_the_long_cases_on_the_host(name):
    key, n_keys, gap = rc.long_cases()[name]
    tiles = np.prod([-(-n // t) for n, t in zip(key.shape, rc.TILE)])
    assert tiles > 2048 and key.size < 140000
    assert rc.same_tables(host(key, n_keys, gap), rc.loop_relations(key, n_keys, gap)) == ""


def test_the_cases_are_what_their_names_say(looped):
    """A check of the FIXTURES: the look-throughs of ``looks`` really end where their comments say, at every gap."""
    from contrastive_lift_amd import relations
    assert tuple(relations.TILE) == rc.TILE and relations.LDS_KEYS == rc.LDS_KEYS and relations.MAX_KEYS == rc.MAX_KEYS
    for a in range(3):
        near = {gap: looped[f"looks along {a} gap {gap}"]["near"] for gap in (1, 2, 4)}
        assert looped[f"looks along {a} gap 0"]["near"] is None and looped[f"looks along {a} gap 0"]["rejected"][0] == 4
        # 1 0..0 2 across the tile border with 1, 2, 3, 4 and 5 background points: seen at gap >= that many, at most 4
        assert [int(near[g][1, 2, a]) for g in (1, 2, 4)] == [1, 2, 4]
        assert [int(near[g][3, 4, a]) for g in (1, 2, 4)] == [1, 1, 1] and int(near[1][5, 6, a]) == 1
        assert int(near[4][4, 4, a]) == 0 and int(near[4][5, 5, a]) == 0                      # holes add nothing
        assert [int(near[g][6, 7, a]) for g in (1, 2, 4)] == [1, 1, 1] and int(near[4][4, 7, a]) == 0
        assert int(near[4][7, 1, a]) == 0 and int(near[4][8, 1, a]) == 0                      # a look stops at a rejected key
    skew = rc.cases()["skewed, table in LDS"][0]
    assert (skew == 1).mean() > 0.98
    many = rc.many_keys_in_a_wave()
    assert all(len(np.unique(many[i0, 2 * w:2 * w + 2])) == 64 for i0 in range(2) for w in range(4))


def test_room_numbers():
    for gap in (0, 1):
        got = host(rc.room(), 4, gap)
        assert got["count"].tolist() == rc.ROOM_COUNT and got["rejected"][0] == 0
        for (u, v, a), n in rc.ROOM_FACES.items():
            assert int(got["faces"][u, v, a]) == n, (u, v, a)
        assert got["ibox"][2].tolist() == [2, 2, 2, 9, 9, 5] and got["ibox"][3].tolist() == [4, 4, 7, 6, 6, 8]
        assert got["isum"][3].tolist() == [18 * 5, 18 * 5, 9 * 7 + 9 * 8]
    for (u, v, a), n in rc.ROOM_NEAR_GAP1.items():
        assert int(got["near"][u, v, a]) == n, (u, v, a)
    assert int(got["near"].sum()) == 9 and host(rc.room(), 4, 0)["near"] is None


def room_graph(gap, up="+z", flip=False, **kw):
    from contrastive_lift_amd import relations
    key, ticks = rc.room(), [t.copy() for t in rc.ROOM_TICKS]
    if flip:
        key, ticks[2] = key[:, :, ::-1].copy(), ticks[2][::-1].copy()
    return relations.SceneGraph.from_counts(relations.lattice_relations(key, 4, gap, backend="host"), rc.ROOM_NODES, ticks, up=up, **kw)


def test_room_graph():
    g = room_graph(1)
    assert g.on() == {2: [(1, 1.0)], 3: [(2, 1.0)]} and g.beside() == set()                  # table on floor, cup on table
    assert room_graph(0).on() == {2: [(1, 1.0)]}                                             # the cup floats at gap 0
    floor, table, cup = g.nodes
    assert (floor["semantic"], floor["instance"], table["instance"], cup["key"]) == (0, 0, 1, 3)
    assert [n["voxels"] for n in g.nodes] == rc.ROOM_COUNT[1:]
    cell = 0.2 * 0.3 * 0.1
    assert table["volume"] == pytest.approx(256 * cell, rel=1e-12)
    assert table["centroid"] == pytest.approx([-1.0 + 0.2 * 5.5, 0.3 * 5.5, 0.5 + 0.1 * 3.5], rel=1e-12)
    assert table["index_box"] == [2, 2, 2, 9, 9, 5]
    assert table["box"] == pytest.approx([-1.0 + 0.4, 0.6, 0.7, -1.0 + 1.8, 2.7, 1.0], rel=1e-12)
    assert table["free_area"]["+z"] == pytest.approx(64 * 0.2 * 0.3, rel=1e-12) and table["free_area"]["-z"] == 0.0
    assert table["free_area"]["+x"] == table["free_area"]["-x"] == pytest.approx(32 * 0.3 * 0.1, rel=1e-12)
    assert floor["free_area"]["+z"] == pytest.approx(80 * 0.2 * 0.3, rel=1e-12)
    pairs = {(p["u"], p["v"]): p for p in g.pairs}
    assert set(pairs) == {(1, 2), (2, 3)} and pairs[(1, 2)]["faces"] == [0, 0, 64] and pairs[(2, 3)]["near"] == [0, 0, 9]
    # the same room upside down, up = -z: the same graph; with the wrong up nothing stands on anything it should
    gf = room_graph(1, up="-z", flip=True)
    assert gf.on() == g.on() and [n["voxels"] for n in gf.nodes] == [n["voxels"] for n in g.nodes]
    assert gf.nodes[1]["centroid"] == pytest.approx(table["centroid"], rel=1e-12) and gf.nodes[1]["free_area"]["-z"] == pytest.approx(64 * 0.06, rel=1e-12)
    assert room_graph(1, up="-z").on() == {1: [(2, 64 / 144)], 2: [(3, 9 / 64)]}             # read upside down: the floor hangs on the table
    assert room_graph(1, up="+x").on() == {} and room_graph(1, up="+x").beside() == {(1, 2), (2, 3)}      # with x as up, contacts along z are sideways
    assert room_graph(1, min_faces=10).on() == {2: [(1, 1.0)]} and room_graph(1, min_faces=9).on() == g.on()
    d = json.loads(g.to_json())
    assert d["up"] == "+z" and d["min_faces"] == 4 and len(d["nodes"]) == 3 and d["relations"][0]["relation"] == "on"
    assert d == g.to_dict() and g == room_graph(1) and g != room_graph(0)


def test_beside():
    from contrastive_lift_amd import relations
    key = np.zeros((8, 8, 6), np.int32)
    key[:, :, 0] = 1                                                                         # floor
    key[1:3, 2:6, 1:4] = 2
    key[3:5, 2:6, 1:4] = 3                                                                   # touches 2 along x: 4 x 3 faces
    key[6:8, 2:6, 1:4] = 4                                                                   # one empty point from 3
    for gap, want in ((0, {(2, 3)}), (1, {(2, 3), (3, 4)})):
        g = relations.SceneGraph.from_counts(relations.lattice_relations(key, gap=gap, backend="host"), [(0, 0), (1, 1), (1, 2), (1, 3)],
                                             [np.arange(8.0), np.arange(8.0), np.arange(6.0)])
        assert g.beside() == want and set(g.on()) == {2, 3, 4}


def test_node_keys():
    from contrastive_lift_amd import relations
    sem = np.full((2, 3, 4), -1, np.int64)
    inst = np.zeros((2, 3, 4), np.int64)
    sem[0, 0, :], inst[0, 0, :] = 5, [2, 2, 7, 7]
    sem[1, 1, :2], inst[1, 1, :2] = 3, 0                                                     # a stuff class: one node
    sem[1, 2, 1:], inst[1, 2, 1:] = 3, [4, 0, 4]
    inst[0, 1, 0] = 9                                                                        # outside: ignored
    key, nodes = relations.node_keys(sem, inst)
    assert nodes == [(3, 0), (3, 4), (5, 2), (5, 7)] and key.dtype == torch.int32 and tuple(key.shape) == (2, 3, 4)
    k = key.numpy()
    assert k[0, 0].tolist() == [3, 3, 4, 4] and k[1, 1].tolist() == [1, 1, 0, 0] and k[1, 2].tolist() == [0, 2, 1, 2] and k[0, 1, 0] == 0
    assert ((k > 0) == (sem >= 0)).all()
    key, nodes = relations.node_keys(torch.from_numpy(sem).int(), torch.from_numpy(inst).int())
    assert nodes == [(3, 0), (3, 4), (5, 2), (5, 7)] and np.array_equal(key.numpy(), k)
    key, nodes = relations.node_keys(np.full((2, 2, 2), -1), np.zeros((2, 2, 2), np.int64))
    assert nodes == [] and not key.any()
    with pytest.raises(ValueError):
        relations.node_keys(sem, inst[0])
    with pytest.raises(ValueError):
        relations.node_keys(sem.astype(np.float32), inst)
    with pytest.raises(ValueError, match=">= 0"):
        relations.node_keys(sem, -inst)


def test_errors():
    from contrastive_lift_amd import _lib, relations
    key = rc.room()
    with pytest.raises(_lib.CliftError, match="outside"):
        relations.lattice_relations(key, 3, 1, backend="host")                              # the cup's key 3 is no key of a table of 3
    with pytest.raises(_lib.CliftError, match="outside"):
        relations.lattice_relations(-key, backend="host")
    assert relations.relation_tables(key, 3, 1, backend="host")["rejected"].tolist() == [18]
    assert relations.lattice_relations(key, backend="host")["count"].shape[0] == 4          # n_keys = max + 1
    for bad in (dict(n_keys=0), dict(n_keys=1025), dict(gap=-1), dict(gap=5), dict(backend="numpy")):
        with pytest.raises(ValueError):
            relations.lattice_relations(key, **{"backend": "host", **bad})
    with pytest.raises(ValueError):
        relations.lattice_relations(key[0], backend="host")
    with pytest.raises(ValueError):
        relations.lattice_relations(key.astype(np.float32), backend="host")
    with pytest.raises(ValueError):
        relations.lattice_relations(np.zeros((0, 3, 3), np.int32), backend="host")
    with pytest.raises(_lib.CliftError, match="wants the key on the GPU"):                  # the device backend never falls back to the host
        relations.lattice_relations(torch.from_numpy(key), backend="device")
    rel = relations.lattice_relations(key, backend="host")
    with pytest.raises(ValueError):
        relations.SceneGraph.from_counts(rel, rc.ROOM_NODES, rc.ROOM_TICKS, up="z")
    with pytest.raises(ValueError):
        relations.SceneGraph.from_counts(rel, rc.ROOM_NODES[:2], rc.ROOM_TICKS)
    src = open(os.path.join(REPO, "contrastive_lift_amd", "relations.py")).read()
    assert "oracle" not in src


# ============================================================================ the library entry
def test_abi_27_declares_exports_and_binds_the_relations_entry():
    from contrastive_lift_amd import _lib, relations
    raw = open(os.path.join(REPO, "include", "clift.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bclift_lattice_relations\s*\(", src), "clift_lattice_relations is not declared in include/clift.h"
    for name, value in (("CLIFT_REL_LDS_KEYS", relations.LDS_KEYS), ("CLIFT_REL_MAX_KEYS", relations.MAX_KEYS), ("CLIFT_REL_MAX_GAP", relations.MAX_GAP)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1)) == value, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clift_lattice_relations"), "clift_lattice_relations is not exported by libclift.so"
    assert "clift_lattice_relations" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 27 and _lib.load().clift_version() == 27
    hip = open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "relations.hip")).read()
    assert tuple(int(re.search(rf"#define\s+REL_T{a}\s+(\d+)", hip).group(1)) for a in range(3)) == tuple(relations.TILE)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "clift_lattice_relations" in open(os.path.join(REPO, doc)).read(), doc


def test_bad_arguments_are_refused_without_a_gpu():
    from contrastive_lift_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                    # never followed: every call below returns before it touches a buffer
    call = lambda n=(4, 4, 4), n_keys=4, gap=1, key=p, count=p, isum=p, ibox=p, faces=p, near=p, rejected=p: \
        lib.clift_lattice_relations(key, *n, n_keys, gap, count, isum, ibox, faces, near, rejected, None)
    err = lambda: lib.clift_last_error().decode()
    for n in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert call(n=n) != 0 and "positive" in err(), n
    assert call(n=(2048, 1024, 1024)) != 0 and "2^31" in err() and "lattice points" in err()
    for n_keys in (0, -1, 1025):
        assert call(n_keys=n_keys) != 0 and "n_keys" in err(), n_keys
    for gap in (-1, 5):
        assert call(gap=gap) != 0 and "gap" in err(), gap
    assert call(gap=0) != 0 and "near" in err()                # near without gap
    assert call(gap=2, near=None) != 0 and "near" in err()     # gap without near
    for name in ("key", "count", "isum", "ibox", "faces", "rejected"):
        assert call(**{name: None}) != 0 and "NULL" in err(), name
        assert call(gap=0, near=None, **{name: None}) != 0 and "NULL" in err(), name


def test_extract_mesh_cli_relations_flags():
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_rel", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    a = ap.parse_args(["--ckpt_path", "x.ckpt"])
    assert a.relations is False and a.relations_gap == 1 and a.up_axis == "+z" and a.relations_min_faces == 4 and cli.relations_options(a) is None
    a = ap.parse_args(["--ckpt_path", "x.ckpt", "--relations", "--relations_gap", "2", "--up_axis", "-y", "--relations_min_faces", "9"])
    assert cli.relations_options(a) == dict(gap=2, up="-y", min_faces=9)
    for bad in (["--relations_gap", "5"], ["--up_axis", "z"], ["--up_axis", "up"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--ckpt_path", "x.ckpt", "--relations"] + bad)
    assert cli.relations_stem() == "relations" and cli.relations_stem("move_3") == "relations_edit_move_3"
