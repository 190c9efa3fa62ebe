"""Edit programs on the host (CPU only): ``edit.EditProgram`` / ``as_program``, the header and the ctypes table, the argument checks of the
list entry points (they return before anything is launched) and ``resolve_program`` / ``--script`` of inference/edit_scene.py."""
import ctypes as C
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import edit_cases as ec
from conftest import REPO

HEADER = os.path.join(REPO, "include", "clift.h")
TOOL = os.path.join(REPO, "inference", "edit_scene.py")


def _box(rot, centre, lo, hi):
    from contrastive_lift_amd import edit
    return edit.EditBox(ec.rot_xyz(*rot).double().numpy(), centre, lo, hi)


def _three():
    """[move(A), delete(B), copy(A's destination)]: the copy's destination feeds the move's, B cuts into both A and the copy."""
    from contrastive_lift_amd import edit
    A = _box((0.2, 0.1, -0.7), [0.1, -0.2, 0.05], [-0.4, -0.3, -0.2], [0.5, 0.25, 0.3])
    mv = edit.move(A, [0.3, 0.15, -0.1], ec.rot_xyz(0.5, -0.3, 0.9).double().numpy())
    B = _box((0.0, 0.3, 0.1), [0.0, 0.1, 0.0], [-0.3, -0.2, -0.6], [0.2, 0.3, 0.6])
    cp = edit.copy(mv.dst, [-0.5, 0.2, 0.1], ec.rot_xyz(-0.2, 0.4, 0.3).double().numpy())
    return [mv, edit.delete(B), cp]


def test_constructor_limits():
    from contrastive_lift_amd import edit
    e = _three()[1]
    assert edit.MAX_EDITS == 8
    for n in (0, 9):
        with pytest.raises(ValueError, match="8"):
            edit.EditProgram([e] * n)
    assert len(edit.EditProgram([e] * 8)) == 8 and len(edit.EditProgram([e])) == 1
    with pytest.raises(TypeError):
        edit.EditProgram([e, "delete"])


def test_records_are_the_members_records_in_order():
    from contrastive_lift_amd import _lib, edit
    es = _three()
    prog = edit.EditProgram(es)
    assert prog.record_bytes() == b"".join(e.record_bytes() for e in es)
    recs = prog.records()
    assert len(recs) == 3 and C.sizeof(recs) == 3 * C.sizeof(_lib.EditRec)
    assert C.string_at(C.addressof(recs), C.sizeof(recs)) == prog.record_bytes()            # contiguous, nothing between the records
    assert [r.mode for r in recs] == [edit.MANIPULATE, edit.DELETE, edit.DUPLICATE]
    assert list(prog) == es and prog[2] is es[2]


def _apply(e, scene):
    """scene -> scene: one edit as a function composition.  A scene maps fp64 (points, dirs) to (where each is looked up in the TRAINED field,
    with which direction, whether it is empty)."""
    from contrastive_lift_amd import edit

    def edited(p, d):
        src, dst = e.src.contains(p), e.dst.contains(p)
        if e.mode == edit.DELETE:
            kill, mov = src, np.zeros_like(src)
        elif e.mode == edit.EXTRACT:
            kill, mov = ~src, np.zeros_like(src)
        elif e.mode == edit.DUPLICATE:
            kill, mov = np.zeros_like(src), dst
        else:
            kill, mov = src & ~dst, dst
        q = np.where(mov[:, None], p @ e.M.T + e.t, p)
        v = np.where(mov[:, None], d @ e.dir_inv.T, d)
        q2, v2, empty = scene(q, v)                                  # the scene this edit was applied to, at the point the content came from
        # (where this edit kills, what the earlier scene holds at q is of no account: the row reports the point at which it was killed)
        return np.where(kill[:, None], p, q2), np.where(kill[:, None], d, v2), kill | empty
    return edited


def test_walk_is_the_composition_of_the_edits():
    """source_points / killed of a three-edit program against scene_3 = e_3(e_2(e_1(field))) built by brute force, on 10 000 points."""
    from contrastive_lift_amd import edit
    es = _three()
    prog = edit.EditProgram(es)
    rng = np.random.default_rng(11)
    p, d = rng.uniform(-1.0, 1.0, (10000, 3)), rng.standard_normal((10000, 3))
    scene = lambda q, v: (q, v, np.zeros(q.shape[0], dtype=bool))    # scene_0: the trained field
    for e in es:
        scene = _apply(e, scene)
    want_p, want_d, want_dead = scene(p, d)
    got_p, got_d = prog.source_points(p, d)
    dead = prog.killed(p)
    assert np.array_equal(dead, want_dead) and 100 < dead.sum() < 5000
    live = ~dead
    assert np.array_equal(got_p[live], want_p[live]) and np.array_equal(got_d[live], want_d[live])
    assert np.array_equal(prog.source_points(p)[live], want_p[live])
    once = es[2].source_points(p)
    twice = es[2].dst.contains(p) & es[0].dst.contains(once) & live
    assert twice.sum() > 50                                          # points that two edits remap, one after the other
    assert np.abs(got_p[twice] - es[0].source_points(once)[twice]).max() < 1e-12
    # one edit: the program is that edit
    for e in es:
        one = edit.EditProgram([e])
        assert np.array_equal(one.killed(p), e.killed(p))
        assert np.array_equal(one.source_points(p)[~e.killed(p)], e.source_points(p)[~e.killed(p)])


def test_as_program_takes_an_edit_a_program_or_a_sequence():
    from contrastive_lift_amd import edit
    es = _three()
    prog = edit.EditProgram(es)
    assert edit.as_program(prog) is prog
    assert edit.as_program(es[0]).record_bytes() == es[0].record_bytes() and len(edit.as_program(es[0])) == 1
    assert edit.as_program(es).record_bytes() == prog.record_bytes()
    assert edit.as_program(tuple(es[:2])).record_bytes() == b"".join(e.record_bytes() for e in es[:2])
    with pytest.raises(ValueError):
        edit.as_program([])


def _prototype_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    return [a.strip() for a in args.split(",")]


def test_header_and_binding_agree():
    from contrastive_lift_amd import _lib, edit
    src = open(HEADER).read()
    assert int(re.search(r"#define\s+CLIFT_EDIT_MAX\s+(\d+)", src).group(1)) == edit.MAX_EDITS == 8
    for name, n_args in (("clift_edit_list_density_fwd", 8), ("clift_edit_list_active", 9)):
        args = _prototype_args(name)
        assert len(args) == n_args == len(_lib._SIGNATURES[name][0])
        assert args[1].startswith("const clift_edit_t*") and args[2].startswith("int ")
        ints = [i for i, a in enumerate(args) if a.startswith("int ")]
        assert [i for i, t in enumerate(_lib._SIGNATURES[name][0]) if t is C.c_int] == ints
    for name, n_args in (("clift_edit_density_fwd", 7), ("clift_edit_active", 8)):            # the single-edit entry points keep their signatures
        assert len(_prototype_args(name)) == n_args == len(_lib._SIGNATURES[name][0])
    assert int(re.search(r"clift_version\(void\) \{ return (\d+); \}", open(os.path.join(_lib.CSRC, "core.hip")).read()).group(1)) == _lib.ABI_VERSION >= 24


def test_list_entry_points_check_their_arguments():
    """n_edits out of range, an unknown mode and a non-finite value are refused before anything touches a device: callable without one."""
    from contrastive_lift_amd import _lib, edit
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    es = _three()
    ms, vm = _lib.March(), _lib.VM()
    ms.n_samples, vm.comps = 38, 16
    calls = {"clift_edit_list_density_fwd": lambda recs, n: (C.byref(ms), recs, n, C.byref(vm), None, 10, None, None),
             "clift_edit_list_active": lambda recs, n: (C.byref(ms), recs, n, None, None, 10, None, None, None)}
    nine = (_lib.EditRec * 9)(*(es[i % 3].record() for i in range(9)))
    for name, args in calls.items():
        for n in (0, -1, 9):
            with pytest.raises(_lib.CliftError, match=f"1 to 8 edits.*n_edits = {n}"):
                _lib.call(name, *args(nine, n))
        recs = edit.EditProgram(es).records()
        recs[2].dst.hi[0] = float("inf")
        with pytest.raises(_lib.CliftError, match=r"edit 2: .*not finite"):
            _lib.call(name, *args(recs, 3))
        recs = edit.EditProgram(es).records()
        recs[1].mode = 4
        with pytest.raises(_lib.CliftError, match=r"edit 1: unknown edit mode 4"):
            _lib.call(name, *args(recs, 3))
        with pytest.raises(_lib.CliftError, match="no edit records"):
            _lib.call(name, *args(None, 3))


# ----------------------------------------------------------------------------- inference/edit_scene.py
@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import edit_scene
    finally:
        sys.path.pop(0)
    return edit_scene


def _boxes():
    entry = lambda c, a: {"bbox": (np.array([-0.2, -0.15, -0.1]), np.array([0.25, 0.1, 0.15])), "orientation": ec.rot_xyz(0.1, a, 0.3).double().numpy(),
                          "position": np.array(c)}
    return {3: entry([0.1, 0.0, -0.05], 0.2), 7: entry([-0.4, 0.2, 0.1], -0.5), 12: entry([0.3, -0.3, 0.0], 0.9)}


def test_resolve_program_keeps_the_order_and_the_fitted_boxes(tool):
    from contrastive_lift_amd import edit
    boxes = _boxes()
    entries = [{"instance": 7, "op": "delete"}, {"instance": 3, "op": "move", "translate": [0.3, 0.0, 0.1], "rotate_deg": [0, 0, 30]},
               {"instance": 12, "op": "copy", "translate": [0.0, 0.4, 0.0], "pad": 0.02}, {"instance": 3, "op": "extract"}]
    prog = tool.resolve_program(boxes, entries)
    assert isinstance(prog, edit.EditProgram) and [e.mode for e in prog] == [edit.DELETE, edit.MANIPULATE, edit.DUPLICATE, edit.EXTRACT]
    want = [tool.resolve_edit(boxes, 7, "delete"), tool.resolve_edit(boxes, 3, "move", [0.3, 0.0, 0.1], [0, 0, 30]),
            tool.resolve_edit(boxes, 12, "copy", [0.0, 0.4, 0.0], pad=0.02), tool.resolve_edit(boxes, 3, "extract")]
    assert prog.record_bytes() == b"".join(e.record_bytes() for e in want)
    # without "at": "moved" the last entry addresses the box as fitted, although entry 1 moved the instance
    assert np.array_equal(prog[3].src.centre, boxes[3]["position"])


def test_at_moved_picks_the_earlier_destination_box(tool):
    from contrastive_lift_amd import edit
    boxes = _boxes()
    t1, t2 = [0.3, 0.0, 0.1], [0.0, -0.2, 0.0]
    entries = [{"instance": 3, "op": "move", "translate": t1, "rotate_deg": [0, 0, 30]}, {"instance": 7, "op": "move", "translate": [0.1, 0.1, 0.1]},
               {"instance": 3, "op": "move", "translate": t2, "at": "moved"}, {"instance": 3, "op": "move", "rotate_deg": [0, 0, 45], "at": "moved"}]
    prog = tool.resolve_program(boxes, entries)
    for later, earlier in ((2, 0), (3, 2)):                          # the most recent earlier move of the instance, not the first
        for f in ("axes", "centre", "lo", "hi"):
            assert np.array_equal(getattr(prog[later].src, f), getattr(prog[earlier].dst, f)), (later, f)
    assert np.allclose(prog[3].dst.centre, boxes[3]["position"] + np.array(t1) + np.array(t2))
    # the motions compose: a point of the fitted box, carried by the three moves one after the other, is looked up where it started
    x = boxes[3]["position"] + np.array([0.05, -0.03, 0.02])
    y = x[None]
    for i in (0, 2, 3):
        b, R = prog[i].src, np.linalg.inv(prog[i].dir_inv)
        y = (y - b.centre) @ R.T + prog[i].dst.centre
    assert np.abs(prog.source_points(y) - x).max() < 1e-12 and not prog.killed(y).any()
    for bad, msg in (([{"instance": 3, "op": "delete", "at": "moved"}], "earlier move"),
                     ([{"instance": 7, "op": "move"}, {"instance": 3, "op": "copy", "at": "moved"}], "earlier move"),
                     ([{"instance": 99, "op": "delete"}], "instance 99 has no box"), ([{"instance": 3, "op": "shrink"}], "unknown op"),
                     ([{"instance": 3}], "needs"), ([{"instance": 3, "op": "move", "translation": [0, 0, 1]}], "may hold"),
                     ([{"instance": 3, "op": "move", "at": "there"}], '"at"'), ([], "1 to 8"), ([{"instance": 3, "op": "delete"}] * 9, "1 to 8")):
        with pytest.raises(SystemExit, match=msg):
            tool.resolve_program(boxes, bad)


def _run_tool(*args):
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True)


def test_script_flag_on_the_command_line(tmp_path):
    r = _run_tool("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--script", "--instance", "--op"):
        assert flag in r.stdout
    script, boxes = tmp_path / "tidy_up.json", tmp_path / "bboxes.pkl"
    script.write_text(json.dumps([{"instance": 3, "op": "delete"}]))
    boxes.write_bytes(pickle.dumps(_boxes()))
    common = ("--ckpt_path", str(tmp_path / "run" / "checkpoints" / "x.ckpt"), "--bboxes", str(boxes))
    r = _run_tool(*common, "--script", str(script), "--op", "delete")
    assert r.returncode == 2 and "--script" in r.stderr and "--op" in r.stderr
    r = _run_tool(*common, "--instance", "3")
    assert r.returncode == 2 and "required without --script" in r.stderr
