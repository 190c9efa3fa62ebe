"""Shaped edits on the host (CPU only): the numpy packing of ``edit.EditShape`` against a plain loop, the fp64 host walk with
shapes against a per-point loop, what all-ones and all-zero shapes do, ``resolve_program`` with ``"shape"`` and the refusals of the two
command lines.  No device is touched."""
import os
import sys

import numpy as np
import pytest

import edit_cases as ec
import edit_shape_cases as sc
from conftest import REPO


def _box(rot, centre, lo, hi):
    from contrastive_lift_amd import edit
    return edit.EditBox(ec.rot_xyz(*rot).double().numpy(), centre, lo, hi)


def _program():
    """move(A), delete(B), copy of A's destination, extract of a wide box: every mode, up to two remaps, boxes that cut into each other."""
    from contrastive_lift_amd import edit
    A = _box((0.2, 0.1, -0.7), [0.1, -0.2, 0.05], [-0.4, -0.3, -0.2], [0.5, 0.25, 0.3])
    mv = edit.move(A, [0.3, 0.15, -0.1], ec.rot_xyz(0.5, -0.3, 0.9).double().numpy())
    B = _box((0.0, 0.3, 0.1), [0.0, 0.1, 0.0], [-0.3, -0.2, -0.6], [0.2, 0.3, 0.6])
    cp = edit.copy(mv.dst, [-0.5, 0.2, 0.1], ec.rot_xyz(-0.2, 0.4, 0.3).double().numpy())
    W = _box((0.1, 0.0, 0.0), [0.0, 0.0, 0.0], [-0.9, -0.9, -0.8], [0.9, 0.9, 0.8])
    return edit.EditProgram([mv, edit.delete(B), cp, edit.extract(W)])


# ----------------------------------------------------------------------------- packing
@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (8, 8, 33)])
@pytest.mark.parametrize("grow", [0, 1, 2])
def test_host_pack_against_a_loop(dims, grow):
    from contrastive_lift_amd import edit
    for seed, p in ((0, 0.1), (1, 0.5), (2, 0.0), (3, 1.0)):
        flags = np.random.default_rng(seed).random(dims) < p
        sh = edit.EditShape.from_flags(flags, grow=grow, backend="host")
        want = sc.pack_loop(flags, grow)
        assert sh.words.dtype == np.uint32 and sh.dims == dims and np.array_equal(sh.words, want), (seed, p)
        total = dims[0] * dims[1] * dims[2]
        assert sh.n_cells == total and sh.words.shape[0] == (total + 31) // 32
        if total % 32:
            assert int(sh.words[-1]) >> (total % 32) == 0                  # the unused high bits of the last word
        back = sh.flags()
        assert back.shape == dims and back.dtype == bool and sh.n_set == int(back.sum())
        if grow == 0:
            assert np.array_equal(back, flags)                             # the round trip
        else:
            assert (back | ~flags).all()                                   # growing only adds
        assert np.array_equal(edit.EditShape(sh.words, dims).words, sh.words) and np.array_equal(edit.EditShape.from_flags(back, backend="host").words, sh.words)


def test_shape_constructor_refusals():
    from contrastive_lift_amd import edit
    with pytest.raises(ValueError, match="1 .. 1024"):
        edit.EditShape(np.zeros(1, np.uint32), (0, 1, 1))
    with pytest.raises(ValueError, match="1 .. 1024"):
        edit.EditShape.from_flags(np.zeros((1, 1025, 1), bool), backend="host")
    with pytest.raises(ValueError, match="words"):
        edit.EditShape(np.zeros(3, np.uint32), (3, 5, 7))
    with pytest.raises(ValueError, match="high bits"):
        edit.EditShape(np.full(1, 0xffffffff, np.uint32), (1, 1, 1))
    with pytest.raises(ValueError, match="grow"):
        edit.EditShape.from_flags(np.ones((2, 2, 2), bool), grow=5, backend="host")
    with pytest.raises(TypeError, match="EditShape"):
        edit.delete(_box((0, 0, 0), [0, 0, 0], [-1, -1, -1], [1, 1, 1]), shape=np.ones((2, 2, 2), bool))


# ----------------------------------------------------------------------------- the host walk
@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 6, 7), (16, 16, 16)])
def test_host_walk_against_a_per_point_loop(dims):
    from contrastive_lift_amd import edit
    base = _program()
    shapes = sc.bernoulli_shapes(len(base), dims)
    shapes[1] = None                                                       # the two kinds mix in one program
    prog = sc.with_shapes(base, shapes)
    assert prog.is_shaped and not base.is_shaped and prog.record_bytes() == base.record_bytes()
    pts = sc.box_points(base, per_box=48).astype(np.float64)
    want_p, want_s = sc.brute_walk(prog, pts)
    p, d, s = prog.apply_to_points(pts, backend="host")
    same = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-14)              # (M p as a matrix product and as a loop's: another summation order)
    assert d is None and np.array_equal(s, want_s) and same(p, want_p)
    assert np.array_equal(prog.killed(pts), (want_s & edit.STATE_KILLED) != 0) and same(prog.source_points(pts), want_p)
    pj, J, sj = prog.jacobians(pts)
    po, org, so = prog.origins(pts)
    assert same(pj, want_p) and np.array_equal(sj, want_s) and same(po, want_p) and np.array_equal(so, want_s)
    moved = (want_s & edit.STATE_REMAPS) > 0
    assert moved.sum() >= 10 and not np.allclose(J[moved], np.eye(3))
    assert ((org > 0) <= moved).all()                                      # a copy's origin only where something remapped the point
    if dims != (1, 1, 1):
        assert (want_s != base.apply_to_points(pts, backend="host")[2]).sum() >= 20       # the shapes matter


def test_full_and_empty_shapes():
    """All ones: the plain box edit.  All zeros: a delete kills nothing, a move neither takes anything away nor brings anything, an extract
    kills everything."""
    from contrastive_lift_amd import edit
    base = _program()
    pts = sc.box_points(base, per_box=64).astype(np.float64)
    ones = sc.with_shapes(base, [edit.EditShape.full((4, 3, 5)) for _ in base])
    assert ones.is_shaped and ones[0].shape.n_set == 60
    for a, b in zip(ones.apply_to_points(pts, backend="host"), base.apply_to_points(pts, backend="host")):
        assert (a is None and b is None) or np.array_equal(a, b)
    none = edit.EditShape.full((4, 3, 5), False)
    assert none.n_set == 0
    for e in (base[0], base[1], base[2]):                                  # move, delete, copy
        p, _, s = edit.EditProgram([e.with_shape(none)]).apply_to_points(pts, backend="host")
        assert not s.any() and np.array_equal(p, pts)
    assert (edit.EditProgram([base[3].with_shape(none)]).apply_to_points(pts, backend="host")[2] == edit.STATE_KILLED).all()
    assert edit.Edit.with_shape(ones[0], None).shape is None and base.shapes("cpu") is None


def test_a_moved_object_is_addressed_with_the_same_words():
    """A rigid move keeps lo, hi and the local frame: deleting the moved object at its destination with the SAME shape kills exactly the
    points the move brought there."""
    from contrastive_lift_amd import edit
    mv = _program()[0]
    sh = sc.bernoulli_shapes(1, (6, 5, 4))[0]
    moved = mv.with_shape(sh)
    pts = sc.box_points([mv], per_box=400).astype(np.float64)
    arrived = (edit.EditProgram([moved]).apply_to_points(pts, backend="host")[2] & edit.STATE_REMAPS) == 1
    both = edit.EditProgram([moved, edit.delete(mv.dst, shape=sh)])
    state = both.apply_to_points(pts, backend="host")[2]
    assert arrived.sum() >= 50 and np.array_equal((state & edit.STATE_KILLED) != 0, arrived | edit.EditProgram([moved]).killed(pts))
    assert (state[arrived] == edit.STATE_KILLED).all()                     # killed where they stand: the delete is met first


def test_majority_slot():
    from contrastive_lift_amd import edit
    assert edit.majority_slot([-1, 3, 3, 2, 2, -1, -1, -1]) == 2           # a tie goes to the lower slot; -1 is no slot
    assert edit.majority_slot(np.array([5, 0, 5, 0, 5])) == 5
    with pytest.raises(ValueError, match="no occupied cell"):
        edit.majority_slot([-1, -1])
    with pytest.raises(ValueError, match="no occupied cell"):
        edit.majority_slot([])


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


def _boxes():
    entry = lambda c, a: {"bbox": (np.array([-0.2, -0.15, -0.1]), np.array([0.25, 0.1, 0.15])), "orientation": ec.rot_xyz(0.1, a, 0.3).double().numpy(),
                          "position": np.array(c)}
    return {3: entry([0.1, 0.0, -0.05], 0.2), 7: entry([-0.4, 0.2, 0.1], -0.5)}


def test_resolve_program_with_shapes(tools):
    from contrastive_lift_amd import edit
    es, _ = tools
    made = []

    def shape_of(box):
        made.append(box)
        return edit.EditShape.full((2, 3, 4))
    entries = [{"instance": 3, "op": "move", "translate": [0.3, 0.0, 0.1], "rotate_deg": [0, 0, 30], "pad": 0.02},
               {"instance": 7, "op": "delete", "shape": False},
               {"instance": 3, "op": "copy", "translate": [0.0, 0.4, 0.0], "at": "moved"},
               {"instance": 7, "op": "extract"}]
    prog = es.resolve_program(_boxes(), entries, follow_shape=True, shape_of=shape_of)
    assert [e.shape is not None for e in prog] == [True, False, True, True] and len(made) == 2
    assert prog[2].shape is prog[0].shape and prog[3].shape is not prog[0].shape          # "at": "moved" reuses the move's object
    assert made[0] is prog[0].src and np.array_equal(prog[2].src.lo, prog[0].dst.lo)
    plain = es.resolve_program(_boxes(), entries)                                          # the default is the flag
    assert not plain.is_shaped and plain.record_bytes() == prog.record_bytes()
    only = es.resolve_program(_boxes(), [dict(entries[0], shape=True), entries[1]], shape_of=shape_of)
    assert [e.shape is not None for e in only] == [True, False]
    bad = [(entries[:2] + [dict(entries[2], pad=0.01)], "pad"),                            # the reused shape was made over the box as it is
           ([dict(entries[0], shape=False), entries[2]], "follows none"),
           ([dict(entries[0], shape="yes")], "true or false")]
    for ents, msg in bad:
        with pytest.raises(SystemExit, match=msg):
            es.resolve_program(_boxes(), ents, follow_shape=True, shape_of=shape_of)
    with pytest.raises(SystemExit, match="trained field"):
        es.resolve_program(_boxes(), [dict(entries[0], shape=True)])
    one = es.resolve_edit(_boxes(), 3, "move", [0.1, 0, 0], shape=shape_of)
    assert one.shape is not None and one.mode == edit.MANIPULATE


def test_command_line_refusals(tools):
    es, xm = tools
    common = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", "b.pkl", "--instance", "3", "--op", "move", "--follow_shape"]
    for flag in ("--save_surface", "--save_layers"):
        with pytest.raises(SystemExit, match="cannot be combined with --save_surface or --save_layers"):
            es.main(common + [flag])
    a = xm.build_parser().parse_args(common + ["--shape_grid", "48"])
    assert a.follow_shape and a.shape_grid == 48 and a.shape_grow == 1 and a.shape_alpha == 0.5
    assert xm.edit_tag_of(a) == "move_3_shape" and xm.mesh_stem(xm.edit_tag_of(a)) == "mesh_edit_move_3_shape"
    assert callable(xm.cli_edit_of(a))                                     # resolved once the field is loaded
    with pytest.raises(SystemExit, match="--follow_shape shapes an edit"):
        xm.build_parser().parse_args(["--ckpt_path", "x", "--follow_shape"])
    b = xm.build_parser().parse_args(common[:-1])
    assert not b.follow_shape and xm.edit_tag_of(b) == "move_3"

    class NoCentroids:
        instance_loss_mode = "contrastive"
    with pytest.raises(SystemExit, match="--cached_centroids_path"):

        class Scene:
            class segmentation_data:
                fg_classes, bg_classes = [1], [0]
        es.shape_table(NoCentroids(), Scene(), None)
