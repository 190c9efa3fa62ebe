"""Lattice clearance without a GPU: ``clearance.clearance_tables(backend="host")`` against the per-column loop of
tests/clearance_cases.py, constructed lattices whose numbers are known by hand, the two identities that tie the tables to those of
``relations``, ``offset_of`` and ``Clearance``, the declarations of the new entry point, and the refusals of the two command lines."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import clearance_cases as cc
import relations_cases as rc
from conftest import REPO

from contrastive_lift_amd import _lib, clearance, relations

SHAPES = [(1, 1, 1), (1, 1, 70), (3, 4, 5), (9, 10, 67)]


def host(key, n_keys, slack=0):
    return cc.to_numpy(clearance.clearance_tables(key, n_keys, slack, backend="host"))


# ----------------------------------------------------------------------------- the host backend against the loop
@pytest.mark.parametrize("background", [0.3, 0.9])
@pytest.mark.parametrize("n_keys", [2, 3, 33])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_backend_against_the_column_loop(shape, n_keys, background):
    key = cc.random_key(shape, n_keys, background, 11 * n_keys + sum(shape))
    for slack in (0, 1, 4):
        got, want = host(key, n_keys, slack), cc.loop_clearance(key, n_keys, slack)
        assert cc.same_tables(got, want) == "", (slack, cc.same_tables(got, want))
    assert all(v.dtype == np.int32 for v in got.values())
    assert got["pair"].shape == (n_keys, n_keys, 6) and got["travel"].shape == (n_keys, 6) and got["landing"].shape == (n_keys, n_keys, 6)
    assert (got["pair"][0] == cc.NONE).all() and (got["pair"][:, 0] == cc.NONE).all() and (got["landing"][got["pair"] == cc.NONE] == 0).all()


def test_host_backend_with_rejected_keys_against_the_loop():
    key, n_keys, _ = rc.cases()["rejected keys"]
    got, want = host(key, n_keys, 1), cc.loop_clearance(key, n_keys, 1)
    assert cc.same_tables(got, want) == "" and int(got["rejected"][0]) > 100
    with pytest.raises(_lib.CliftError, match="outside"):
        clearance.lattice_clearance(key, n_keys, backend="host")


# ----------------------------------------------------------------------------- values known by hand
def test_the_cup_hovers_three_points_over_the_table():
    t = host(cc.cup_room(), 4)
    assert t["travel"][3, cc.MZ] == 3 and t["landing"][3, 2, cc.MZ] == 9 and t["pair"][2, 3, cc.PZ] == 3 and t["pair"][3, 2, cc.MZ] == 3
    assert t["travel"][3, cc.PZ] == 1 and t["landing"][3, 1, cc.PZ] == 9                          # the ceiling, one empty point above the cup
    assert t["travel"][3, cc.PX] == 4 and t["landing"][3, 1, cc.PX] == 6 and t["travel"][3, cc.MX] == 3     # the walls at x 11 and x 0
    assert t["travel"][2, cc.MZ] == 0 and t["landing"][2, 1, cc.MZ] == 64                         # the table stands on the floor
    assert t["pair"][1, 3, cc.PZ] == cc.NONE                                                      # the table is between the floor and the cup
    assert cc.same_tables(t, cc.loop_clearance(cc.cup_room(), 4, 0)) == ""


def test_a_c_shape_does_not_stop_on_itself():
    t = host(cc.c_shape(), 3)
    want = np.full((3, 3, 6), cc.NONE, np.int32)
    want[1, 2, cc.PY] = want[2, 1, cc.MY] = 2                                                     # from the second arm; the first is 7 away
    assert np.array_equal(t["pair"], want)
    assert t["landing"][1, 2, cc.PY] == 1 and t["landing"][2, 1, cc.MY] == 1 and int(t["landing"].sum()) == 2
    alone = np.where(cc.c_shape() == 1, 1, 0).astype(np.int32)
    t = host(alone, 2)
    assert (t["pair"] == cc.NONE).all() and (t["travel"] == cc.NONE).all() and not t["landing"].any()


def test_no_event_crosses_a_rejected_point():
    t = host(cc.rejected_between(), 4)
    assert int(t["rejected"][0]) == 1
    assert (t["pair"][1] == cc.NONE).all() and (t["pair"][:, 1] == cc.NONE).all()                 # 1 sees nothing, nothing sees 1
    assert t["pair"][2, 3, cc.PZ] == 2 and t["pair"][3, 2, cc.MZ] == 2 and t["travel"][2, cc.MZ] == cc.NONE


@pytest.mark.parametrize("key,n_keys", [(np.zeros((4, 5, 6), np.int32), 3), (np.ones((4, 5, 6), np.int32), 2), (np.zeros((2, 2, 2), np.int32), 1)])
def test_nothing_to_meet(key, n_keys):
    t = host(key, n_keys, 4)
    assert (t["pair"] == cc.NONE).all() and (t["travel"] == cc.NONE).all() and not t["landing"].any() and int(t["rejected"][0]) == 0


def test_slack_counts_the_faces_one_step_further():
    key = cc.slack_steps()
    t0, t1 = host(key, 3, 0), host(key, 3, 1)
    assert t0["travel"][2, cc.MZ] == 1 and t0["landing"][2, 1, cc.MZ] == 1 and t1["landing"][2, 1, cc.MZ] == 2
    assert t0["landing"][1, 2, cc.PZ] == 1 and t1["landing"][1, 2, cc.PZ] == 2
    assert np.array_equal(t0["pair"], t1["pair"]) and np.array_equal(t0["travel"], t1["travel"])


# ----------------------------------------------------------------------------- the identities with relations
@pytest.mark.parametrize("gap", [0, 1, 2, 4])
def test_the_identities_with_the_relations_tables(gap):
    lattices = [(cc.random_key(shape, n_keys, bg, 5 + n_keys), n_keys) for shape in SHAPES for n_keys in (3, 33) for bg in (0.3, 0.9)]
    lattices.append((rc.room(), 4))
    lattices.append((cc.cup_room(), 4))
    holds = 0
    for key, n_keys in lattices:
        clr = host(key, n_keys)
        rel = rc.to_numpy(relations.relation_tables(key, n_keys, gap, backend="host"))
        assert cc.identities(clr, rel, gap) == "", (key.shape, n_keys)
        holds += int((clr["pair"][1:, 1:, 0::2] <= gap).sum())
    assert holds > 100                                                                            # (the identities were not vacuous)


# ----------------------------------------------------------------------------- offsets and the summary
def test_offset_of_on_uneven_spacings():
    ticks = cc.CUP_TICKS
    assert np.allclose(clearance.offset_of(3, ticks, "-z"), [0.0, 0.0, -0.3], atol=1e-12)
    assert np.allclose(clearance.offset_of(2, ticks, "+y"), [0.0, 0.6, 0.0], atol=1e-12)
    assert np.allclose(clearance.offset_of(5, [torch.from_numpy(t) for t in ticks], "-x"), [-1.0, 0.0, 0.0], atol=1e-12)
    assert clearance.offset_of(0, ticks, "+x").tolist() == [0.0, 0.0, 0.0] and clearance.offset_of(1, ticks, "+x").dtype == np.float64
    with pytest.raises(ValueError, match="direction"):
        clearance.offset_of(1, ticks, "z")


def test_the_summary_of_the_cup():
    key = cc.cup_room()
    tables = clearance.lattice_clearance(key, 4, backend="host")
    summary = clearance.Clearance.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS, key=key)
    js = json.loads(summary.to_json())
    assert js["directions"] == list(clearance.DIRECTIONS) and [n["key"] for n in js["nodes"]] == [1, 2, 3]
    cup = js["nodes"][2]
    assert (cup["semantic"], cup["instance"]) == (2, 1)
    down = cup["directions"]["-z"]
    assert down["steps"] == 3 and abs(down["distance"] - 0.3) < 1e-12 and down["onto"] == [{"key": 2, "faces": 9}] and down["border_steps"] == 8
    assert cup["directions"]["+z"]["border_steps"] == 2 and cup["directions"]["+x"]["border_steps"] == 5 and cup["directions"]["-y"]["border_steps"] == 4
    assert abs(cup["directions"]["+x"]["distance"] - 4 * 0.2) < 1e-12 and abs(cup["directions"]["-y"]["distance"] - 3 * 0.3) < 1e-12
    room = js["nodes"][0]["directions"]["+x"]                                                    # the wall at x 0 looks at the table and, beside it, at the cup
    assert room["steps"] == 1 and room["onto"] == [{"key": 2, "faces": 32}]
    rel = relations.lattice_relations(key, 4, backend="host")                                    # the box from a relations dict: the same summary
    assert clearance.Clearance.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS, relations=rel) == summary
    bare = clearance.Clearance.from_tables(tables, cc.CUP_NODES, cc.CUP_TICKS)
    assert bare.nodes[2]["directions"]["-z"]["border_steps"] is None and bare.nodes[2]["directions"]["-z"]["steps"] == 3
    free = clearance.Clearance.from_tables(clearance.lattice_clearance(np.where(key == 3, 1, 0), 2, backend="host"), [(2, 1)], cc.CUP_TICKS, key=key == 3)
    assert free.nodes[0]["directions"]["-z"] == dict(steps=None, distance=None, onto=[], border_steps=8)
    with pytest.raises(ValueError, match="node list"):
        clearance.Clearance.from_tables(tables, cc.CUP_NODES[:2], cc.CUP_TICKS)


def test_argument_errors_come_before_any_launch():
    key = cc.cup_room()
    for kw, msg in ((dict(n_keys=0), "n_keys must be 1 .. 1024"), (dict(n_keys=1025), "n_keys must be 1 .. 1024"), (dict(slack=-1), "slack must be 0 .. 4"),
                    (dict(slack=5), "slack must be 0 .. 4"), (dict(backend="cpu"), "backend")):
        with pytest.raises(ValueError, match=msg):
            clearance.clearance_tables(key, **{"n_keys": 4, "backend": "host", **kw})
    with pytest.raises(ValueError, match=r"\(n0, n1, n2\)"):
        clearance.clearance_tables(key[0], 4, backend="host")
    with pytest.raises(ValueError, match="bool or integer"):
        clearance.clearance_tables(key.astype(np.float32), 4, backend="host")
    with pytest.raises(ValueError, match="at least one point"):
        clearance.clearance_tables(key[:, :0], 4, backend="host")
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        clearance.clearance_tables(key, 4)                                                        # a host tensor: no quiet fall-back
    assert clearance.clearance_tables(key, backend="host")["travel"].shape == (4, 6)             # n_keys = max + 1
    assert clearance.MAX_SLACK == cc.MAX_SLACK and clearance.NONE == cc.NONE and clearance.DIRECTIONS == relations.UP_AXES


# ----------------------------------------------------------------------------- the entry point's declarations
def test_the_entry_point_is_declared_exported_and_documented():
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    assert re.search(r"\bclift_lattice_clearance\s*\(", src), "clift_lattice_clearance is not declared in include/clift.h"
    for name, value in (("CLIFT_CLR_MAX_SLACK", clearance.MAX_SLACK), ("CLIFT_CLR_NONE", clearance.NONE)):
        m = re.search(rf"#define\s+{name}\s+(\w+)", src)
        assert m and int(m.group(1), 0) == value, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clift_lattice_clearance"), "clift_lattice_clearance is not exported by libclift.so"
    assert "clift_lattice_clearance" in _lib.exported_symbols()
    assert "clearance.hip" in open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "Makefile")).read()
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "clift_lattice_clearance" in open(os.path.join(REPO, doc)).read(), doc


def test_errors_of_the_entry_point_need_no_device():
    """Every check of the entry point comes before the device is touched: NULL buffers stand in for device memory."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)
    bad = [((0, 4, 4), 3, 0, one, r"lattice dimensions must be positive \(got 0 x 4 x 4\)"), ((4, -1, 4), 3, 0, one, "lattice dimensions must be positive"),
           ((2048, 1024, 1024), 3, 0, one, r"2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           ((4, 4, 4), 0, 0, one, r"n_keys must be 1 .. 1024 \(got 0\)"), ((4, 4, 4), 1025, 0, one, r"n_keys must be 1 .. 1024 \(got 1025\)"),
           ((4, 4, 4), 3, -1, one, r"slack must be 0 .. 4 \(got -1\)"), ((4, 4, 4), 3, 5, one, r"slack must be 0 .. 4 \(got 5\)"),
           ((4, 4, 4), 3, 0, None, "NULL device buffer")]
    for n, n_keys, slack, buf, msg in bad:
        with pytest.raises(_lib.CliftError, match=msg):
            _lib.call("clift_lattice_clearance", one, *n, n_keys, slack, buf, one, one, one, None)
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


def test_refusals_of_settle(tools, capsys):
    es, _ = tools
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", "b.pkl", "--instance", "3"]
    for op in ("delete", "extract"):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", op, "--settle"])
        assert "--settle drops the object that a move or a copy places" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        es.parse_args(common + ["--op", "move", "--settle", "up"])
    assert "--settle" in capsys.readouterr().err
    for flag, value in (("--settle_slack", "5"), ("--settle_slack", "-1"), ("--settle_upsample", "0")):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", "move", "--settle", flag, value])
        assert flag in capsys.readouterr().err
    for flag in ("--settle_slack", "--settle_upsample"):
        with pytest.raises(SystemExit):
            es.parse_args(common + ["--op", "move", flag, "1"])
        assert "needs --settle" in capsys.readouterr().err
    a = es.parse_args(common + ["--op", "move", "--settle"])
    assert a.settle == "-z" and a.settle_upsample == 1 and a.settle_slack == 0
    a = es.parse_args(common + ["--op", "copy", "--follow_shape", "--settle", "-x", "--settle_slack", "2", "--settle_upsample", "2"])
    assert a.settle == "-x" and a.settle_slack == 2 and a.settle_upsample == 2 and a.follow_shape
    a = es.parse_args(common + ["--op", "copy", "--settle", "+y", "--translate", "0", "0", "-1"])
    assert a.settle == "+y" and a.translate == [0.0, 0.0, -1.0]
    assert es.parse_args(common + ["--op", "delete"]).settle is None
    text = " ".join(es.build_parser().format_help().split())                                      # the help names the companion flag
    assert "carries a slab of its surroundings along" in text and "--follow_shape is the intended companion" in text


def test_settle_refuses_a_script_that_ends_in_no_move(tools, tmp_path, monkeypatch):
    es, _ = tools
    monkeypatch.setattr(es, "load_run_config", lambda p: type("Cfg", (), {})())
    boxes = {3: {"bbox": (-np.ones(3), np.ones(3)), "orientation": np.eye(3), "position": np.zeros(3)}}
    good = [{"instance": 3, "op": "delete"}, {"instance": 3, "op": "copy", "translate": [0.5, 0, 0]}]
    es.check_settle(es.resolve_program(boxes, good))
    es.check_settle(es.resolve_edit(boxes, 3, "move", [0.1, 0, 0]))
    for bad in (es.resolve_program(boxes, good[::-1]), es.resolve_edit(boxes, 3, "extract")):
        with pytest.raises(SystemExit, match="--settle drops the object that a move or a copy places"):
            es.check_settle(bad)
    path = tmp_path / "ends_in_delete.json"
    path.write_text(json.dumps(good[::-1]))
    pkl = tmp_path / "b.pkl"
    import pickle
    with open(pkl, "wb") as f:
        pickle.dump(boxes, f)
    with pytest.raises(SystemExit, match="--settle drops the object that a move or a copy places"):
        es.main(["--ckpt_path", str(tmp_path / "runs" / "x" / "checkpoints" / "y.ckpt"), "--bboxes", str(pkl), "--script", str(path), "--settle"])
    moved = es.settled_edit(es.resolve_edit(boxes, 3, "move", [0.1, 0, 0]), np.array([0.0, 0.0, -0.25]))
    assert np.allclose(moved.dst.centre, [0.1, 0.0, -0.25]) and moved.mode == es.ed.MANIPULATE
    prog = es.settled_edit(es.resolve_program(boxes, good), np.array([0.0, 0.0, -0.25]))
    assert len(prog) == 2 and np.allclose(prog[1].dst.centre, [0.5, 0.0, -0.25]) and prog[0].record_bytes() == es.resolve_program(boxes, good)[0].record_bytes()


def test_refusals_of_the_clearance_flags_of_the_mesh_tool(tools, capsys):
    _, xm = tools
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt"]
    with pytest.raises(SystemExit):
        xm.build_parser().parse_args(common + ["--clearance_slack", "1"])
    assert "--clearance_slack needs --clearance" in capsys.readouterr().err
    for value in ("5", "-1"):
        with pytest.raises(SystemExit):
            xm.build_parser().parse_args(common + ["--clearance", "--clearance_slack", value])
        assert "--clearance_slack" in capsys.readouterr().err
    a = xm.build_parser().parse_args(common + ["--clearance"])
    assert a.clearance and a.clearance_slack == 0 and xm.clearance_options(a) == dict(slack=0) and not a.relations
    a = xm.build_parser().parse_args(common + ["--clearance", "--clearance_slack", "2", "--relations"])
    assert xm.clearance_options(a) == dict(slack=2) and xm.relations_options(a) is not None
    assert xm.clearance_options(xm.build_parser().parse_args(common)) is None
    assert xm.clearance_stem(None) == "clearance" and xm.clearance_stem("move_3") == "clearance_edit_move_3"
    with pytest.raises(SystemExit, match=r"alpha_level must lie in \(0, 1\)"):                    # default_level lives in the package now
        xm.default_level(None, 1.0)
