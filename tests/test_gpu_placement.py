"""The placement map on the GPU: clift_lattice_placement / backend="device" against backend="host", integer for integer, for
all six directions on every case of tests/placement_cases.py -- windows that straddle the 64-bit words of a row (n2 and m2 at 63, 64, 65 and
above 128), objects longer than 64 along x and y, T2 = 1, a single translation, sparse shapes with empty rows, 1024 keys with a mixed solid
table, rejected keys --, the buffers filled by the call itself, determinism, every refusal of the entry point, the identity against the
DEVICE clearance, ``snap_offset`` on the scene130 field of the shaped-edit suite, and ``edit_scene.py --snap_placement`` end to end."""
import importlib
import json
import pickle
import types

import numpy as np
import pytest
import torch

import clearance_cases as cc
import edit_cases as ec
import placement_cases as pc
from test_gpu_clearance import _table, hover_translation
from test_gpu_edit_mesh import LEVEL, UP, cli, scene  # noqa: F401  (cli and scene are that module's fixtures, used here as they are)
from test_gpu_edit_program import box_C
from test_placement_host import clearance_identity, identity_lattices

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = pc.cases()


def device(case, direction):
    from contrastive_lift_amd import placement
    out = placement.placement_tables(torch.from_numpy(case["key"]).to(DEV), torch.from_numpy(case["shape"]).to(DEV), case["n_keys"], case["solid"],
                                     direction, case["target"], case["min_support"])
    assert all(v.is_cuda for v in out.values()) and out["best"].dtype == torch.int64 and all(out[k].dtype == torch.int32 for k in pc.NAMES if k != "best")
    return pc.to_numpy(out)


# ============================================================================ 1. parity, seams, determinism
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host(name):
    for d in pc.DIRECTIONS:
        got, want = device(CASES[name], d), pc.host_tables()[(name, d)]
        assert pc.same(got, want) == "", (name, d, pc.same(got, want))


def test_the_cases_cannot_be_met_by_zeros():
    tables = pc.host_tables()
    for name in CASES:
        if name not in pc.NONE_CASES:
            assert all(tables[(name, d)]["count"][0] >= 1 for d in pc.DIRECTIONS) and any(tables[(name, d)]["count"][1] >= 1 for d in pc.DIRECTIONS), name
    assert tables[("a single translation", "-z")]["overlap"].shape == (1, 1, 1) and tables[("T2 = 1: (4, 5, 66) object (2, 2, 66)", "-z")]["overlap"].shape[2] == 1
    assert int(tables[("rejected keys", "-z")]["rejected"][0]) > 50 and CASES["1024 keys, a mixed solid table"]["n_keys"] == 1024


def raw_call(case, along, out, work, null=None, **kw):
    """The raw entry point on the buffers ``out`` and ``work``; ``kw`` replaces arguments, ``null`` names a buffer to pass as NULL."""
    from contrastive_lift_amd import _lib, distance
    key, shape = case["key"], case["shape"]
    T = tuple(key.shape[a] - shape.shape[a] + 1 for a in range(3))
    a = dict(key=torch.from_numpy(key).to(DEV), n=key.shape, n_keys=case["n_keys"], shape=torch.from_numpy(shape).to(DEV), m=shape.shape,
             solid=torch.from_numpy(distance.site_table(case["solid"], case["n_keys"]).astype(np.uint8)).to(DEV), direction=pc.DIRECTIONS.index(along),
             min_support=case["min_support"], target=tuple(min(max(case["target"][i], 0), T[i] - 1) for i in range(3)), work=work, **out)
    a.update(kw)
    if null is not None:
        a[null] = None
    _lib.call("clift_lattice_placement", _lib.ptr(a["key"]), *a["n"], a["n_keys"], _lib.ptr(a["solid"]), _lib.ptr(a["shape"]), *a["m"], a["direction"],
              a["min_support"], *a["target"], _lib.ptr(a["overlap"]), _lib.ptr(a["support"]), _lib.ptr(a["count"]), _lib.ptr(a["best"]),
              _lib.ptr(a["rejected"]), _lib.ptr(a["work"]), _lib.stream())


def junk_buffers(case, value=12345):
    from contrastive_lift_amd import placement
    key, shape = case["key"], case["shape"]
    T = tuple(key.shape[a] - shape.shape[a] + 1 for a in range(3))
    junk = lambda size, dtype: torch.full(size, value, dtype=dtype, device=DEV)
    out = dict(overlap=junk(T, torch.int32), support=junk(T, torch.int32), count=junk((2,), torch.int32), best=junk((2,), torch.int64),
               rejected=junk((1,), torch.int32))
    return out, junk((placement.work_words(key.shape, shape.shape),), torch.int64)


@pytest.mark.parametrize("name", ["(6, 5, 65) object (2, 2, 64)", "(40, 33, 70) object (7, 9, 33)", "1024 keys, a mixed solid table", "rejected keys", "all solid",
                                  "an empty lattice"])
def test_the_call_fills_its_buffers_and_two_runs_give_the_same_bits(name):
    """The raw entry on buffers full of other numbers: the call itself fills every output, on its stream; the second call starts from the
    first one's results and scratch."""
    case = CASES[name]
    for d in ("+x", "-z"):
        out, work = junk_buffers(case)
        for _ in range(2):
            raw_call(case, d, out, work)
            assert pc.same(pc.to_numpy(out), pc.host_tables()[(name, d)]) == "", (name, d)


# ============================================================================ 2. the errors of the entry point
def test_every_error_of_the_entry_point():
    from contrastive_lift_amd import _lib
    case = CASES[pc.SMALL]                                                   # (5, 6, 7) with (2, 3, 2): T = (4, 4, 6)
    out, work = junk_buffers(case, 0x55)
    bad = [(dict(n=(0, 6, 7)), r"clift_lattice_placement: lattice dimensions must be 1 .. 16384 \(got 0 x 6 x 7\)"),
           (dict(n=(5, -3, 7)), r"lattice dimensions must be 1 .. 16384 \(got 5 x -3 x 7\)"),
           (dict(n=(16385, 6, 7)), r"lattice dimensions must be 1 .. 16384 \(got 16385 x 6 x 7\)"),
           (dict(m=(2, 0, 2)), r"clift_lattice_placement: shape dimensions must be 1 .. the lattice's \(got 2 x 0 x 2 in 5 x 6 x 7\)"),
           (dict(m=(6, 3, 2)), r"shape dimensions must be 1 .. the lattice's \(got 6 x 3 x 2 in 5 x 6 x 7\)"),
           (dict(m=(2, 3, 8)), r"shape dimensions must be 1 .. the lattice's \(got 2 x 3 x 8 in 5 x 6 x 7\)"),
           (dict(n=(2048, 1024, 1024)), r"clift_lattice_placement: 2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           (dict(n_keys=0), r"clift_lattice_placement: n_keys must be 1 .. 1024 \(got 0\)"), (dict(n_keys=1025), r"n_keys must be 1 .. 1024 \(got 1025\)"),
           (dict(direction=6), r"clift_lattice_placement: direction must be 0 .. 5 \(got 6\)"), (dict(direction=-1), r"direction must be 0 .. 5 \(got -1\)"),
           (dict(min_support=0), r"clift_lattice_placement: min_support must be >= 1 \(got 0\)"),
           (dict(target=(4, 0, 0)), r"clift_lattice_placement: target must lie inside the 4 x 4 x 6 translations \(got 4, 0, 0\)"),
           (dict(target=(0, 0, -1)), r"target must lie inside the 4 x 4 x 6 translations \(got 0, 0, -1\)")]
    bad += [(dict(null=name), "clift_lattice_placement: NULL device buffer") for name in ("key", "solid", "shape", "overlap", "support", "count", "best", "rejected", "work")]
    for kw, msg in bad:
        with pytest.raises(_lib.CliftError, match=msg):
            raw_call(case, "-z", out, work, **kw)
    torch.cuda.synchronize()
    assert all(bool((v == 0x55).all()) for v in out.values()) and bool((work == 0x55).all())                  # nothing was launched
    raw_call(case, "-z", out, work)
    assert pc.same(pc.to_numpy(out), pc.host_tables()[(pc.SMALL, "-z")]) == ""
    from contrastive_lift_amd import placement
    with pytest.raises(_lib.CliftError, match="outside"):
        placement.lattice_placement(torch.from_numpy(CASES["rejected keys"]["key"]).to(DEV), CASES["rejected keys"]["shape"], 3)
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        placement.lattice_placement(case["key"], case["shape"], backend="device")                            # a host tensor: no quiet fall-back


# ============================================================================ 3. the identity against the device clearance
def test_the_identity_with_the_device_clearance():
    from contrastive_lift_amd import clearance, placement
    checks = 0
    for name, key in identity_lattices().items():
        k = torch.from_numpy(key).to(DEV)
        clr = cc.to_numpy(clearance.lattice_clearance(k, 3, 0))
        checks += clearance_identity(k, lambda kk, shape, d, origin: pc.to_numpy(placement.lattice_placement(kk, shape, 3, 1, d, origin)), clr)
    assert checks > 60
    tables, origin = placement.node_placement(torch.from_numpy(cc.cup_room()).to(DEV), 4, 3)
    want = placement.node_placement(cc.cup_room(), 4, 3, backend="host")[0]
    assert origin == (4, 4, 8) and pc.same(pc.to_numpy(tables), pc.to_numpy(want)) == "" and placement.split_best(tables["best"][1], (10, 10, 11)) == (9, (4, 4, 5))


# ============================================================================ 4. snap_offset on scene130's field
@pytest.fixture(scope="module")
def blob_moves(scene):
    """The two moves of tests/test_gpu_distance.py, rebuilt: ``free`` sets the blob 3 empty lattice points above everything else;
    ``occupied`` is a copy to that place followed by a MOVE of the original to the very same place."""
    from contrastive_lift_amd import edit
    _, m, r = scene
    sh = edit.EditShape.from_field(m, r, box_C(), _table(m), dims=(12, 12, 12), grow=0, sigma_min=LEVEL)
    tz, _, _ = hover_translation(scene, edit.copy(box_C(), shape=sh), LEVEL)
    up = edit.copy(box_C(), [0.0, 0.0, tz], shape=sh)
    return dict(free=edit.move(box_C(), [0.0, 0.0, tz], shape=sh), occupied=edit.EditProgram([up, edit.move(box_C(), [0.0, 0.0, tz], shape=sh)]))


def same_snap(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


@pytest.mark.parametrize("which", ["free", "occupied"])
def test_snap_offset_equals_its_recomposition(cli, scene, blob_moves, which):
    from contrastive_lift_amd import distance, placement
    es = importlib.import_module("edit_scene")                                                    # (the cli fixture has put inference/ on the path)
    _, m, r = scene
    e = blob_moves[which]
    got = placement.snap_offset(m, r, e, upsample=UP, level=LEVEL)
    key, ticks = distance.placement_key(m, r, e, UP, LEVEL)
    want = placement.snap_from_keys(key.cpu(), [t.cpu() for t in ticks], backend="host")
    print(f"snap_offset ({which}): {got}")
    assert same_snap(got, want), (got, want)
    assert got["n_moved"] == int((key >= 2).sum()) > 20 and got["steps"].dtype == np.int64 and got["offset"].dtype == np.float64
    shape, origin = placement.object_of(key >= 2, 1)
    tables = placement.lattice_placement(key, shape, 4, [1, 3], "-z", origin)
    assert got["overlap_before"] == int(tables["overlap"][origin]) == int((key == 3).sum())
    assert got["found"] and got["n_supported"] == int(tables["count"][1]) >= 1
    at = tuple(int(origin[a] + got["steps"][a]) for a in range(3))
    assert int(tables["overlap"][at]) == 0 and int(tables["support"][at]) == got["support"] >= 1 and got["dist2"] == int((got["steps"] ** 2).sum())
    if which == "occupied":
        assert got["overlap_before"] > 0 and got["dist2"] > 0
    else:
        assert got["overlap_before"] == 0 and got["support_before"] == 0 and got["dist2"] > 0     # it hovers: free, and unsupported
    after = distance.placement(m, r, es.settled_edit(e, got["offset"]), upsample=UP, level=LEVEL)
    print(f"placement of the snapped edit ({which}): {after['verdict']}, overlap {after['overlap']}, gap2 {after['gap2']}")   # recorded, not asserted


def test_snap_offset_refusals(scene):
    from contrastive_lift_amd import _lib, edit, placement
    _, m, r = scene
    with pytest.raises(ValueError, match="copy or a move"):
        placement.snap_offset(m, r, edit.delete(box_C()), upsample=UP, level=LEVEL)
    with pytest.raises(ValueError, match="copy or a move"):
        placement.snap_offset(m, r, edit.EditProgram([edit.move(box_C(), [0.1, 0, 0]), edit.extract(box_C())]), upsample=UP, level=LEVEL)
    with pytest.raises(_lib.CliftError, match="moved set is empty"):
        placement.snap_offset(m, r, edit.copy(box_C(), [0.0, 0.0, 5.0]), upsample=UP, level=LEVEL)
    with pytest.raises(ValueError, match="direction must be one of"):
        placement.snap_offset(m, r, edit.copy(box_C(), [0.0, 0.0, 0.1]), direction="down", upsample=UP, level=LEVEL)


# ============================================================================ 5. the command line
def tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_edit_scene_snap_placement(cli, scene, tmp_path, monkeypatch, capsys):
    """inference/edit_scene.py --op copy --follow_shape --snap_placement on scene130's field (the loader, the frames and the output folder
    are stubbed, the rest is the tool's own): the one line, snap.json = ``placement.snap_offset``, the folder name, --check_placement on the
    snapped edit; a snap that finds no position renders the edit as given, byte for byte the tree of the run without the flag."""
    from contrastive_lift_amd import distance, edit, placement
    es = importlib.import_module("edit_scene")                                                    # (the cli fixture has put inference/ on the path)
    _, m, r = scene
    E = int(m.render_instance_mlp.output_channels)
    cfg = types.SimpleNamespace(instance_loss_mode="linear_assignment", max_instances=E, use_delta=False, chunk=0)
    H, W = 10, 13
    data = types.SimpleNamespace(segmentation_data=types.SimpleNamespace(fg_classes=[0], bg_classes=[1, 2, 3]), image_dim=(H, W), white_bg=False)
    K = np.array([[20.0, 0.0, W / 2], [0.0, 20.0, H / 2], [0.0, 0.0, 1.0]])
    frames = [("around", ec.scene130()[1].to(DEV), K)]
    monkeypatch.setattr(es, "load_run_config", lambda p: cfg)
    monkeypatch.setattr(es.rp, "distributed_device", lambda device: (torch.device(DEV), 0))
    monkeypatch.setattr(es.rp, "load_for_inference", lambda config, device: (data, m, r))
    monkeypatch.setattr(es.rp, "scene_frames", lambda sc_, traj, test_only: iter(frames))
    monkeypatch.setattr(es.rp, "output_dirname", lambda *a: tmp_path / "runs" / "scene130_test")
    box = edit.EditBox(np.eye(3), [-0.05, 0.0, 0.05], [-0.15, -0.15, -0.15], [0.15, 0.15, 0.15])  # the blob's core
    boxes = {1: {"bbox": (box.lo, box.hi), "orientation": box.axes, "position": box.centre}}
    path = tmp_path / "bboxes.pkl"
    with open(path, "wb") as f:
        pickle.dump(boxes, f)
    t = ["0.05", "0", "0.05"]                                                                     # the copy collides with the original
    argv = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", str(path), "--instance", "1", "--op", "copy", "--translate", *t,
            "--follow_shape", "--shape_grid", "12", "--shape_grow", "0"]
    plain_dir, snapped_dir = (tmp_path / "runs" / f"scene130_test_edit_copy_1_shape{tail}" for tail in ("", "_snapped"))
    es.main(argv)
    plain = tree(plain_dir)
    assert "rgb/around.png" in plain and "snap.json" not in plain and not snapped_dir.exists()
    capsys.readouterr()
    es.main(argv + ["--snap_placement", "--snap_upsample", str(UP), "--snap_min_support", "100000000"])      # nobody has that many faces
    text = capsys.readouterr().out
    assert [ln for ln in text.splitlines() if "snapped" in ln and not ln.startswith("/")] == ["not snapped: no free supported position"], text
    not_snapped = tree(snapped_dir)
    assert sorted(set(not_snapped) - set(plain)) == ["snap.json"] and all(not_snapped[k] == v for k, v in plain.items())     # rendered as given
    assert json.loads(not_snapped["snap.json"])["found"] is False and tree(plain_dir) == plain
    es.main(argv + ["--snap_placement", "-z", "--snap_upsample", str(UP), "--check_placement", "--placement_upsample", str(UP)])
    text = capsys.readouterr().out
    shape_of = es.field_shapes(m, r, es.shape_table(cfg, data, None), 12, 0, 0.5)
    e = es.resolve_edit(boxes, 1, "copy", [float(x) for x in t], shape=shape_of)
    capsys.readouterr()
    want = placement.snap_offset(m, r, e, upsample=UP)
    line = [ln for ln in text.splitlines() if ln.startswith("snapped by ")]
    print(line, [ln for ln in text.splitlines() if ln.startswith("placement: ")])
    assert line == [es.snap_line(want)] and want["found"] and want["overlap_before"] > 0, text
    assert f"(was: collides on {want['overlap_before']} cells)" in line[0] and f" onto {want['support']} faces" in line[0]
    snapped = tree(snapped_dir)
    assert json.loads(snapped["snap.json"]) == json.loads(json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in want.items()}))
    assert sorted(set(snapped) - set(plain)) == ["placement.json", "snap.json"] and tree(plain_dir) == plain   # the other folder is left alone
    checked = distance.placement(m, r, es.settled_edit(e, want["offset"]), upsample=UP)          # --check_placement saw the snapped edit
    assert json.loads(snapped["placement.json"]) == json.loads(json.dumps(checked))
    assert [ln for ln in text.splitlines() if ln.startswith("placement: ")] == [es.placement_line(checked)]
