"""Scene edits on the host (CPU only): the torch restatement of the reference's four edit forwards against the reference's own outputs
(tests/golden/g25_scene_edit.npz, made by tests/golden/make_edit_golden.py), and the box / record logic of contrastive_lift_amd/edit.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import edit_cases as ec
from conftest import REPO, T, load_golden, rel_close
from oracle import render as orender

OPS = ("delete", "extract", "duplicate", "manipulate")


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_scene_edit")


@pytest.mark.parametrize("mode", ["softmax", "none"])
@pytest.mark.parametrize("white", [False, True])
def test_restatement_matches_the_reference(g25, mode, white):
    """All 96 rays, the one with a sample on a box face included: the restatement classifies with the reference's own 4 x 4 inverse."""
    g = g25
    P = ec.golden_params(g)
    cfg = orender.RenderCfg(T(g["aabb"]), tuple(int(x) for x in g["res"]), density_shift=float(g["shift"]), semantic_weight_mode=mode)
    assert cfg.n_samples == int(g["n_samples"]) == 38
    tag = f"{mode}_{'w' if white else 'b'}"
    for op in OPS:
        spec = ec.reference_edit(op, ec.golden_bbox(g), T(g["translation"]), T(g["rotation"]))
        (rgb, sem, inst, depth), _ = ec.render_edit(P, T(g["rays"]), cfg, spec, white)
        for name, got in (("rgb", rgb), ("sem", sem), ("inst", inst), ("depth", depth)):
            rel_close(got, g[f"{tag}.{op}.{name}"], 1e-3, what=f"{tag} {op} {name}")


def test_golden_mask_and_edit_strength(g25):
    on_face = g25["on_face"]
    assert on_face.dtype == np.bool_ and on_face.shape == (96,) and int(on_face.sum()) <= 4
    for op in OPS:          # the four edits differ from each other where it matters: no case is a copy of another
        for other in OPS:
            if op < other:
                assert float(np.abs(g25[f"softmax_b.{op}.depth"] - g25[f"softmax_b.{other}.depth"]).max()) > 0.01, (op, other)


def _cloud(seed, n=20000):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, (n, 3))


def test_editbox_from_reference_classifies_like_the_definition():
    from contrastive_lift_amd import edit
    O = ec.rot_xyz(0.3, -0.5, 0.6).double().numpy()
    d = {"extent": torch.tensor([0.9, 0.8, 0.7]), "position": torch.tensor([0.05, -0.02, 0.03]), "orientation": torch.tensor(O, dtype=torch.float32)}
    pts = _cloud(1)
    O32 = d["orientation"].double().numpy()
    q = np.linalg.solve(O32, (pts - d["position"].double().numpy()).T).T                 # world = O local + position
    for pad in (0.0, 0.07):
        want = np.all(np.abs(q) <= d["extent"].double().numpy() / 2 + pad, axis=1)
        got = edit.EditBox.from_reference(d, pad=pad).contains(pts)
        assert 0.02 < want.mean() < 0.6
        assert int((got != want).sum()) == 0
    assert np.array_equal(edit.EditBox.from_reference(d).axes, O32.T)                    # axes = COLUMNS of orientation


def test_editbox_from_fitted_classifies_like_the_definition():
    from contrastive_lift_amd import edit
    A = ec.rot_xyz(-0.2, 0.4, 1.1).double().numpy()                                      # rows are the axes (PCA.components_)
    entry = {"bbox": (np.array([-0.5, -0.2, -0.1]), np.array([0.3, 0.45, 0.2])), "orientation": A, "position": np.array([0.1, 0.0, -0.05])}
    pts = _cloud(2)
    q = (pts - entry["position"]) @ A.T
    for pad in (0.0, 0.05):
        want = np.all((entry["bbox"][0] - pad <= q) & (q <= entry["bbox"][1] + pad), axis=1)
        got = edit.EditBox.from_fitted(entry, pad=pad).contains(pts)
        assert 0.01 < want.mean() < 0.6
        assert int((got != want).sum()) == 0
    corner = entry["position"] + entry["bbox"][1] @ A                                     # the box's own extreme points (axes orthonormal to fp32 round-off)
    lo_corner = entry["position"] + entry["bbox"][0] @ A
    box = edit.EditBox(np.eye(3), np.zeros(3), [-1, -1, -1], [1, 1, 1])
    assert box.contains(np.array([[1.0, -1.0, 1.0], [1.0, 1.0, 1.0 + 1e-12]])).tolist() == [True, False]
    assert edit.EditBox.from_fitted(entry, pad=1e-6).contains(np.stack([corner, lo_corner])).all()


def test_rigid_edits_move_the_box_with_its_content():
    """copy / move: a point x of the source box lands at y = R (x - pos) + pos + t, y is in the destination box, and y is looked up at x."""
    from contrastive_lift_amd import edit
    A = ec.rot_xyz(0.2, 0.1, -0.7).double().numpy()
    box = edit.EditBox(A, [0.1, -0.2, 0.05], [-0.4, -0.3, -0.2], [0.5, 0.25, 0.3])
    R, t = ec.rot_xyz(0.5, -0.3, 0.9).double().numpy(), np.array([0.3, 0.15, -0.1])
    x = _cloud(3, 4000)
    x = x[box.contains(x)]
    assert x.shape[0] > 50
    y = (x - box.centre) @ R.T + box.centre + t
    for e in (edit.copy(box, t, R), edit.move(box, t, R)):
        assert e.dst.contains(y).all()
        assert np.abs(e.source_points(y) - x).max() < 1e-12
        assert np.abs(e.dir_inv @ R - np.eye(3)).max() < 1e-12
    far = np.array([[5.0, 5.0, 5.0]])
    assert not edit.move(box, t, R).dst.contains(far).any() and np.array_equal(edit.move(box, t, R).source_points(far), far)
    assert edit.copy(box, t, R).killed(x).sum() == 0
    k = edit.move(box, t, R).killed(x)
    assert np.array_equal(k, ~edit.move(box, t, R).dst.contains(x))


def test_move_without_rotation_is_forward_manipulate(g25):
    from contrastive_lift_amd import edit
    bbox = ec.golden_bbox(g25)
    t = T(g25["translation"])
    a = edit.move(bbox, t, torch.eye(3))
    b = edit.reference_manipulate(bbox, t, torch.eye(3))
    assert a.record_bytes() == b.record_bytes()
    assert a.mode == b.mode == edit.MANIPULATE
    # ... and with a rotation the two are different edits (the reference's maps are no rigid motion)
    R = T(g25["rotation"])
    assert edit.move(bbox, t, R).record_bytes() != edit.reference_manipulate(bbox, t, R).record_bytes()


def test_reference_named_records_restate_the_reference_formulas(g25):
    from contrastive_lift_amd import edit
    bbox, t, R = ec.golden_bbox(g25), T(g25["translation"]).double().numpy(), T(g25["rotation"]).double().numpy()
    O, pos = bbox["orientation"].double().numpy(), bbox["position"].double().numpy()
    p = _cloud(4, 2000)
    dup = edit.reference_duplicate(bbox, t, R)
    man = edit.reference_manipulate(bbox, t, R)
    assert np.allclose(dup.dst.centre, R @ pos + t) and np.allclose(dup.dst.axes, (R @ O).T) and dup.mode == edit.DUPLICATE
    assert np.allclose(man.dst.centre, pos + t) and np.allclose(man.dst.axes, (R @ O).T) and man.mode == edit.MANIPULATE
    assert np.abs((p @ dup.M.T + dup.t) - (p - t)).max() < 1e-12
    assert np.abs((p @ man.M.T + man.t) - ((p - pos) @ R.T + pos - t)).max() < 1e-12
    for e in (dup, man):
        assert np.abs(e.dir_inv - np.linalg.inv(R)).max() < 1e-12
    assert edit.reference_delete(bbox).mode == edit.DELETE and edit.reference_extract(bbox).mode == edit.EXTRACT


def _header_struct(name):
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(1), m.group(2), int(m.group(3) or 1)) for m in re.finditer(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_record_packs_to_the_header_layout(g25):
    """ctypes mirror == include/clift.h: field names, order and sizes; the mode constants; and a packed record read back field by field."""
    from contrastive_lift_amd import _lib, edit
    box_fields = _header_struct("clift_edit_box_t")
    assert box_fields == [("float", "axes", 9), ("float", "centre", 3), ("float", "lo", 3), ("float", "hi", 3)]
    assert [(n, ctypes.sizeof(t) // 4) for n, t in _lib.EditBoxRec._fields_] == [(n, k) for _, n, k in box_fields]
    rec_fields = _header_struct("clift_edit_t")
    assert [n for _, n, _ in rec_fields] == [n for n, _ in _lib.EditRec._fields_] == ["mode", "src", "dst", "map_m", "map_t", "dir_inv"]
    assert ctypes.sizeof(_lib.EditBoxRec) == 72 and ctypes.sizeof(_lib.EditRec) == 4 + 2 * 72 + 4 * (9 + 3 + 9)
    assert _lib.EditRec.src.offset == 4 and _lib.EditRec.dst.offset == 76 and _lib.EditRec.map_m.offset == 148
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    for name, val in (("DELETE", edit.DELETE), ("EXTRACT", edit.EXTRACT), ("DUPLICATE", edit.DUPLICATE), ("MANIPULATE", edit.MANIPULATE)):
        assert int(re.search(rf"CLIFT_EDIT_{name} = (\d+)", src).group(1)) == val
    e = edit.reference_manipulate(ec.golden_bbox(g25), T(g25["translation"]), T(g25["rotation"]))
    raw = np.frombuffer(e.record_bytes(), dtype=np.float32)
    assert np.frombuffer(e.record_bytes(), dtype=np.int32)[0] == edit.MANIPULATE
    want = np.concatenate([e.src.axes.reshape(-1), e.src.centre, e.src.lo, e.src.hi, e.dst.axes.reshape(-1), e.dst.centre, e.dst.lo, e.dst.hi,
                           e.M.reshape(-1), e.t, e.dir_inv.reshape(-1)]).astype(np.float32)
    assert np.array_equal(raw[1:], want)
    with pytest.raises(ValueError):
        edit.EditBox(np.eye(3), [0, 0, float("nan")], [0, 0, 0], [1, 1, 1])


def test_edit_scene_cli_parses():
    r = subprocess.run([sys.executable, os.path.join(REPO, "inference", "edit_scene.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--ckpt_path", "--bboxes", "--instance", "--op", "--translate", "--rotate_deg", "--pad", "--render_trajectory", "--image_dim",
                 "--weight_thres"):
        assert flag in r.stdout
    for op in ("delete", "extract", "copy", "move"):
        assert op in r.stdout
