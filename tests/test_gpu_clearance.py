"""Lattice clearance on the GPU: clift_lattice_clearance / backend="device" against backend="host" on every case of
tests/clearance_cases.py (exact integers, every table, no tolerances), long carries, the tables filled by the call itself, determinism, the
two identities against the DEVICE relations, every error of the entry point, ``settle_offset`` and ``inference/edit_scene.py --settle`` on
the scene130 field of the shaped-edit suite, and the clearance stage of inference/extract_mesh.py."""
import importlib
import json
import math
import pickle
import types

import numpy as np
import pytest
import torch

import clearance_cases as cc
import edit_cases as ec
import edit_shape_cases as sc
import relations_cases as rc
from test_gpu_edit_mesh import LEVEL, THINGS, UP, cli, scene, stages  # noqa: F401  (cli and scene are that module's fixtures, used here as they are)
from test_gpu_edit_program import box_C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = cc.device_cases()
SLACKS = (0, 1, 4)


@pytest.fixture(scope="module")
def host_tables():
    """(case name, slack) -> the tables of backend="host": computed once, left unchanged."""
    from contrastive_lift_amd import clearance
    return {(name, slack): cc.to_numpy(clearance.clearance_tables(key, n_keys, slack, backend="host"))
            for name, (key, n_keys) in CASES.items() for slack in SLACKS}


def device(key, n_keys, slack=0):
    from contrastive_lift_amd import clearance
    out = clearance.clearance_tables(torch.from_numpy(key).to(DEV), n_keys, slack)
    assert all(v.is_cuda and v.dtype == torch.int32 for v in out.values())
    return cc.to_numpy(out)


# ============================================================================ 1. parity, carries, determinism
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host(host_tables, name):
    key, n_keys = CASES[name]
    for slack in SLACKS:
        got = device(key, n_keys, slack)
        assert cc.same_tables(got, host_tables[name, slack]) == "", (name, slack, cc.same_tables(got, host_tables[name, slack]))


def test_long_carries_give_the_run_itself():
    """Two keys 199 background points apart along every axis (three 64-point chunks of a row lie between them), and columns that are
    non-zero at their two ends only: the numbers by hand."""
    for a, (name, key) in enumerate((n, k) for n, k in cc.long_carries().items() if n.startswith("two keys")):
        t = device(key, 3)
        assert t["pair"][1, 2, 2 * a] == 198 and t["pair"][2, 1, 2 * a + 1] == 198 and t["travel"][1, 2 * a] == 198, name
        assert t["landing"][1, 2, 2 * a] == 4 and t["landing"][2, 1, 2 * a + 1] == 4 and int(t["landing"].sum()) == 8, name
        assert int((t["pair"] != cc.NONE).sum()) == 2, name
    for a, (name, key) in enumerate((n, k) for n, k in cc.long_carries().items() if n.startswith("the two ends")):
        t = device(key, 3)
        assert t["pair"][1, 2, 2 * a] == key.shape[a] - 2 and t["travel"][2, 2 * a + 1] == key.shape[a] - 2 and t["landing"][2, 1, 2 * a + 1] == 4, name


def test_hand_checked_cases_on_the_device():
    t = device(cc.cup_room(), 4)
    assert t["travel"][3, cc.MZ] == 3 and t["landing"][3, 2, cc.MZ] == 9 and t["pair"][2, 3, cc.PZ] == 3
    t = device(cc.c_shape(), 3)
    assert int((t["pair"] != cc.NONE).sum()) == 2 and t["pair"][1, 2, cc.PY] == 2 and int(t["landing"].sum()) == 2
    t = device(cc.rejected_between(), 4)
    assert int(t["rejected"][0]) == 1 and (t["pair"][1] == cc.NONE).all() and (t["pair"][:, 1] == cc.NONE).all() and t["pair"][2, 3, cc.PZ] == 2
    t0, t1 = device(cc.slack_steps(), 3, 0), device(cc.slack_steps(), 3, 1)
    assert t0["landing"][2, 1, cc.MZ] == 1 and t1["landing"][2, 1, cc.MZ] == 2
    for name in ("all background", "one key", "n_keys 1"):
        t = device(*CASES[name], 4)
        assert (t["pair"] == cc.NONE).all() and (t["travel"] == cc.NONE).all() and not t["landing"].any() and int(t["rejected"][0]) == 0, name


@pytest.mark.parametrize("name", ["skewed, table in LDS", "skewed, table in memory", "1024 keys, many in a wave", "(33, 31, 95) n_keys 33", "rejected keys"])
def test_two_runs_give_the_same_bits(name):
    key, n_keys = CASES[name]
    a, b = device(key, n_keys, 1), device(key, n_keys, 1)
    assert cc.same_tables(a, b) == ""


@pytest.mark.parametrize("name", ["(17, 9, 70) n_keys 3", "(17, 9, 70) n_keys 33", "cup"])
def test_the_call_fills_its_tables(host_tables, name):
    """The raw entry on buffers full of other numbers: the call itself fills them, on its stream."""
    from contrastive_lift_amd import _lib
    key, n_keys = CASES[name]
    k = torch.from_numpy(key).to(DEV)
    junk = lambda shape: torch.full(shape, 12345, dtype=torch.int32, device=DEV)
    out = dict(pair=junk((n_keys, n_keys, 6)), travel=junk((n_keys, 6)), landing=junk((n_keys, n_keys, 6)), rejected=junk((1,)))
    for _ in range(2):                                         # the second call starts from the first one's results
        _lib.call("clift_lattice_clearance", _lib.ptr(k), *key.shape, n_keys, 1, _lib.ptr(out["pair"]), _lib.ptr(out["travel"]),
                  _lib.ptr(out["landing"]), _lib.ptr(out["rejected"]), _lib.stream())
        assert cc.same_tables(cc.to_numpy(out), host_tables[name, 1]) == ""


def test_rejected_keys_and_the_python_raise(host_tables):
    from contrastive_lift_amd import _lib, clearance
    key, n_keys = CASES["rejected keys"]
    got = device(key, n_keys)
    assert int(got["rejected"][0]) == int(((key < 0) | (key >= n_keys)).sum()) > 100
    with pytest.raises(_lib.CliftError, match="outside"):
        clearance.lattice_clearance(torch.from_numpy(key).to(DEV), n_keys)
    with pytest.raises(_lib.CliftError, match="outside"):
        clearance.lattice_clearance(torch.from_numpy(cc.cup_room()).to(DEV), 3)
    out = clearance.lattice_clearance(torch.from_numpy(cc.cup_room()).to(DEV))                    # n_keys = max + 1
    assert cc.same_tables(cc.to_numpy(out), host_tables["cup", 0]) == ""
    with pytest.raises(_lib.CliftError):
        clearance.lattice_clearance(torch.from_numpy(cc.cup_room()), backend="device")           # a host tensor: no quiet fall-back
    with pytest.raises(ValueError):
        clearance.lattice_clearance(torch.from_numpy(cc.cup_room()).to(DEV), slack=5)


# ============================================================================ 2. the identities against the device relations
@pytest.mark.parametrize("gap", [0, 4])
def test_the_identities_against_the_device_relations(gap):
    from contrastive_lift_amd import relations
    holds = 0
    for name in ("(17, 9, 70) n_keys 3", "(33, 31, 95) n_keys 32", "(33, 31, 95) n_keys 33", "skewed and sparse", "1024 keys at random", "cup"):
        key, n_keys = CASES[name]
        rel = rc.to_numpy(relations.lattice_relations(torch.from_numpy(key).to(DEV), n_keys, gap))
        clr = device(key, n_keys)
        assert cc.identities(clr, rel, gap) == "", name
        holds += int((clr["pair"][1:, 1:, 0::2] <= gap).sum())
    assert holds > 100


# ============================================================================ 3. the errors of the entry point
def test_every_error_of_the_entry_point():
    from contrastive_lift_amd import _lib
    key = torch.from_numpy(cc.cup_room()).to(DEV)
    n = tuple(key.shape)
    pair, travel, landing = (torch.full(s, 0x55, dtype=torch.int32, device=DEV) for s in ((4, 4, 6), (4, 6), (4, 4, 6)))
    rejected = torch.full((1,), 0x55, dtype=torch.int32, device=DEV)
    good = dict(key=key, n=n, n_keys=4, slack=0, pair=pair, travel=travel, landing=landing, rejected=rejected)

    def call(**kw):
        a = {**good, **kw}
        _lib.call("clift_lattice_clearance", _lib.ptr(a["key"]), *a["n"], a["n_keys"], a["slack"], _lib.ptr(a["pair"]), _lib.ptr(a["travel"]),
                  _lib.ptr(a["landing"]), _lib.ptr(a["rejected"]), _lib.stream())
    bad = [(dict(n=(0, 12, 12)), r"clift_lattice_clearance: lattice dimensions must be positive \(got 0 x 12 x 12\)"),
           (dict(n=(12, -3, 12)), r"lattice dimensions must be positive \(got 12 x -3 x 12\)"),
           (dict(n=(12, 12, 0)), r"lattice dimensions must be positive \(got 12 x 12 x 0\)"),
           (dict(n=(2048, 1024, 1024)), r"clift_lattice_clearance: 2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           (dict(n_keys=0), r"clift_lattice_clearance: n_keys must be 1 .. 1024 \(got 0\)"), (dict(n_keys=1025), r"n_keys must be 1 .. 1024 \(got 1025\)"),
           (dict(slack=-1), r"clift_lattice_clearance: slack must be 0 .. 4 \(got -1\)"), (dict(slack=5), r"slack must be 0 .. 4 \(got 5\)")]
    bad += [({name: None}, "clift_lattice_clearance: NULL device buffer") for name in ("key", "pair", "travel", "landing", "rejected")]
    for kw, msg in bad:
        with pytest.raises(_lib.CliftError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == 0x55).all()) for t in (pair, travel, landing, rejected))               # nothing was launched
    call()
    assert int(travel[3, cc.MZ]) == 3 and int(rejected[0]) == 0                                   # and the good call does write


# ============================================================================ 4. settling an edit on scene130's field
def _table(m):
    from contrastive_lift_amd.layers import SlotTable
    return SlotTable.from_scores([0], ec.C_CLS, int(m.render_instance_mlp.output_channels))


def hover_translation(scene, e0, level, up=UP):
    """The +z translation that sets the content of the copy ``e0`` (a copy with zero translation: what its source selects) 3 empty lattice
    points above the highest point of the unedited inside set, on the lattice of ``up``: (tz, points (N, 3) fp32 numpy, shape of the
    lattice).  The content spans the blob in z, so this is its extent plus 3 steps."""
    _, m, r = scene
    sigma = r.get_dense_sigma(m, up)
    ticks = [t.cpu().numpy() for t in r.lattice_ticks(sigma.shape)]
    pts = np.stack(np.meshgrid(*ticks, indexing="ij"), -1).reshape(-1, 3)
    inside = (sigma >= level).cpu().numpy()
    top = int(np.nonzero(inside.any((0, 1)))[0].max())
    content = inside & e0.in_src(pts).reshape(inside.shape)
    low = int(np.nonzero(content.any((0, 1)))[0].min())
    n2 = inside.shape[2]
    assert content.sum() > 100 and top + 4 <= n2 - 2, "the hovering copy must keep two layers on the lattice"
    h = (float(ticks[2][-1]) - float(ticks[2][0])) / (n2 - 1)
    return (top + 4 - low) * h, pts.astype(np.float32), tuple(inside.shape)


@pytest.fixture(scope="module")
def hovering_copy(scene):
    """A shaped copy of the blob (the shape read from the field in box C at LEVEL) that hovers over the original."""
    from contrastive_lift_amd import edit
    _, m, r = scene
    sh = edit.EditShape.from_field(m, r, box_C(), _table(m), dims=(12, 12, 12), grow=0, sigma_min=LEVEL)
    tz, pts, shape = hover_translation(scene, edit.copy(box_C(), shape=sh), LEVEL)
    return edit.copy(box_C(), [0.0, 0.0, tz], shape=sh), pts, shape


def test_settle_offset_on_the_hovering_copy(scene, hovering_copy):
    from contrastive_lift_amd import clearance, edit
    _, m, r = scene
    e, pts, shape = hovering_copy
    out = clearance.settle_offset(m, r, e, "-z", upsample=UP, level=LEVEL, slack=1)
    key, ticks, n_moved = clearance.settle_key(m, r, e, UP, LEVEL)
    assert tuple(key.shape) == shape and n_moved == out["n_moved"] == int((key == 2).sum()) > 20
    ref = cc.to_numpy(clearance.lattice_clearance(key.cpu(), 3, 1, backend="host"))
    print(f"settle: steps {out['steps']}, faces {out['faces']}, n_moved {n_moved}, spacing {out['spacing']:.5f}, offset {out['offset'].tolist()}")
    assert out["found"] and out["steps"] == int(ref["travel"][2, cc.MZ]) >= 3 and out["faces"] == int(ref["landing"][2, 1, cc.MZ]) > 0
    assert out["direction"] == "-z" and out["offset"].dtype == np.float64 and out["offset"][:2].tolist() == [0.0, 0.0]
    assert abs(out["offset"][2] + out["steps"] * out["spacing"]) < 1e-12 and abs(out["spacing"] - 1.1 / (shape[2] - 1)) < 1e-6
    # n_moved against the fp64 host walk, up to the rows the face rule of 6k leaves out
    keep = sc.ref_walk(edit.EditProgram([e]), pts)["keep"]
    inside = (key > 0).cpu().numpy().reshape(-1)
    host_moved = e.in_dst(pts) & inside
    dev_moved = (key == 2).cpu().numpy().reshape(-1)
    left = int((~keep).sum())
    print(f"settle: {left} of {pts.shape[0]} rows left out by the face rule; host walk {int(host_moved.sum())} moved rows, device {n_moved}")
    assert left <= 0.01 * pts.shape[0] and np.array_equal(dev_moved[keep], host_moved[keep]) and abs(int(host_moved.sum()) - n_moved) <= left
    # settled: a second look finds the object resting (the lattice is resampled: a face may fall either side of the level)
    again = clearance.settle_offset(m, r, edit.copy(box_C(), e.dst.centre - e.src.centre + out["offset"], shape=e.shape), "-z", upsample=UP, level=LEVEL)
    print(f"settle: after adding the offset, steps {again['steps']}, faces {again['faces']}")
    assert again["found"] and again["steps"] in (0, 1) and again["faces"] > 0
    # the refusals
    with pytest.raises(ValueError, match="copy or a move"):
        clearance.settle_offset(m, r, edit.delete(box_C()), upsample=UP, level=LEVEL)
    with pytest.raises(ValueError, match="copy or a move"):
        clearance.settle_offset(m, r, edit.EditProgram([e, edit.extract(box_C())]), upsample=UP, level=LEVEL)
    with pytest.raises(ValueError, match="direction"):
        clearance.settle_offset(m, r, e, "down", upsample=UP, level=LEVEL)
    from contrastive_lift_amd import _lib
    with pytest.raises(_lib.CliftError, match="moved set is empty"):
        clearance.settle_offset(m, r, edit.copy(box_C(), [0.0, 0.0, 5.0], shape=e.shape), upsample=UP, level=LEVEL)
    up = clearance.settle_offset(m, r, e, "+z", upsample=UP, level=LEVEL)                         # nothing above the copy: the border is no obstacle
    assert not up["found"] and up["steps"] is None and up["offset"].tolist() == [0.0, 0.0, 0.0] and up["faces"] == 0


def test_edit_scene_settle(cli, scene, tmp_path, monkeypatch, capsys):
    """inference/edit_scene.py --op copy --follow_shape --settle on scene130's field (the loader, the frames and the output folder are
    stubbed, the rest is the tool's own): it runs, prints its line, writes into ..._settled, and its frames differ from the unsettled ones."""
    from contrastive_lift_amd import edit
    es = importlib.import_module("edit_scene")                                                    # (the cli fixture has put inference/ on the path)
    _, m, r = scene
    E = int(m.render_instance_mlp.output_channels)
    cfg = types.SimpleNamespace(instance_loss_mode="linear_assignment", max_instances=E, use_delta=False, chunk=0)
    H, W = 10, 13
    data = types.SimpleNamespace(segmentation_data=types.SimpleNamespace(fg_classes=[0], bg_classes=[1, 2, 3]), image_dim=(H, W), white_bg=False)
    zz, yy = np.meshgrid(np.linspace(0.2, 0.59, H), np.linspace(-0.3, 0.3, W), indexing="ij")     # a side view of the space over the blob
    side = np.stack([np.full(H * W, -0.89), yy.reshape(-1), zz.reshape(-1), np.ones(H * W), np.zeros(H * W), np.zeros(H * W),
                     np.full(H * W, 0.01), np.full(H * W, 1.68)], 1).astype(np.float32)
    K = np.array([[20.0, 0.0, W / 2], [0.0, 20.0, H / 2], [0.0, 0.0, 1.0]])
    frames = [("around", ec.scene130()[1].to(DEV), K), ("side", torch.from_numpy(side).to(DEV), K)]
    monkeypatch.setattr(es, "load_run_config", lambda p: cfg)
    monkeypatch.setattr(es.rp, "distributed_device", lambda device: (torch.device(DEV), 0))
    monkeypatch.setattr(es.rp, "load_for_inference", lambda config, device: (data, m, r))
    monkeypatch.setattr(es.rp, "scene_frames", lambda sc_, traj, test_only: iter(frames))
    monkeypatch.setattr(es.rp, "output_dirname", lambda *a: tmp_path / "runs" / "scene130_test")
    box = edit.EditBox(np.eye(3), [-0.05, 0.0, 0.05], [-0.15, -0.15, -0.15], [0.15, 0.15, 0.15])  # the blob's core: the copy keeps layers on the lattice
    boxes = {1: {"bbox": (box.lo, box.hi), "orientation": box.axes, "position": box.centre}}
    path = tmp_path / "bboxes.pkl"
    with open(path, "wb") as f:
        pickle.dump(boxes, f)
    level = cli.default_level(r, 0.5)                                                             # what --settle and --shape_alpha 0.5 both mean
    shape_of = es.field_shapes(m, r, es.shape_table(cfg, data, None), 12, 0, 0.5)
    tz, _, _ = hover_translation(scene, es.resolve_edit(boxes, 1, "copy", shape=shape_of), level)
    capsys.readouterr()
    argv = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", str(path), "--instance", "1", "--op", "copy", "--translate", "0", "0", repr(tz),
            "--follow_shape", "--shape_grid", "12", "--shape_grow", "0"]
    es.main(argv)
    es.main(argv + ["--settle", "--settle_upsample", str(UP)])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("settled by ")]
    assert len(line) == 1, text
    found = line[0].split()
    steps, dist, faces = int(found[2]), float(found[5]), int(found[9])                           # settled by N steps = D along -z onto F faces
    print(line[0])
    assert found[3:5] == ["steps", "="] and found[6:9] == ["along", "-z", "onto"] and found[10:] == ["faces"]
    assert steps >= 3 and faces > 0 and abs(dist - steps * 1.1 / (int(r.grid_dim[2]) * UP - 1)) < 1e-4
    plain, settled = tmp_path / "runs" / "scene130_test_edit_copy_1_shape", tmp_path / "runs" / "scene130_test_edit_copy_1_shape_settled"
    assert str(settled) in text
    for out in (plain, settled):
        assert sorted(p.name for p in (out / "rgb").iterdir()) == ["around.png", "side.png"] and (out / "depth" / "side.npy").exists()
    differ = [name for name in ("around", "side") if not np.array_equal(np.load(plain / "depth" / f"{name}.npy"), np.load(settled / "depth" / f"{name}.npy"))]
    assert "side" in differ and open(plain / "rgb" / "side.png", "rb").read() != open(settled / "rgb" / "side.png", "rb").read()
    capsys.readouterr()
    es.main(argv + ["--settle", "+z", "--settle_upsample", str(UP)])                              # nothing above the copy: rendered as given
    text = capsys.readouterr().out
    assert "not settled: nothing stands in the way along +z" in text and "settled by" not in text
    assert open(plain / "rgb" / "side.png", "rb").read() == open(settled / "rgb" / "side.png", "rb").read()


# ============================================================================ 5. the clearance stage of inference/extract_mesh.py
def test_clearance_stage_writes_both_files(cli, scene, tmp_path):
    from contrastive_lift_amd import clearance, relations
    _, m, r = scene
    rel_options = dict(gap=1, up="+z", min_faces=4)
    both = stages(cli, scene, None, relations=rel_options, clearance=dict(slack=1))[0]
    only = stages(cli, scene, None, clearance=dict(slack=1))[0]
    base = stages(cli, scene, None, relations=rel_options)[0]
    assert "clearance" not in base and "relations" not in only
    found = both["clearance"]
    assert found["key"] is both["relations"]["key"] and found["nodes"] == both["relations"]["nodes"] == only["clearance"]["nodes"]      # one labelling
    assert torch.equal(only["clearance"]["key"], found["key"]) and only["clearance"]["summary"] == found["summary"]
    for k, v in base["relations"]["tables"].items():                                              # the relations do not change
        assert v is None or torch.equal(v, both["relations"]["tables"][k]), k
    assert all(torch.equal(both[k], base[k]) for k in ("verts", "faces", "normals", "sem", "inst", "rgb"))
    nodes = found["nodes"]
    ref = cc.to_numpy(clearance.lattice_clearance(found["key"].cpu(), len(nodes) + 1, 1, backend="host"))
    assert cc.same_tables(cc.to_numpy(found["tables"]), ref) == "" and len(nodes) >= 1
    cli.write_clearance(tmp_path, cli.clearance_stem(None), found)
    cli.write_clearance(tmp_path, cli.clearance_stem("move_1"), found)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["clearance.json", "clearance.npz", "clearance_edit_move_1.json", "clearance_edit_move_1.npz"]
    z = np.load(tmp_path / "clearance.npz")
    assert cc.same_tables({k: z[k] for k in ref}, ref) == "" and z["nodes"].tolist() == [list(n) for n in nodes] and int(z["slack"]) == 1
    js = json.load(open(tmp_path / "clearance.json"))
    want = clearance.Clearance.from_tables(ref, nodes, r.lattice_ticks(found["key"].shape), key=found["key"].cpu(), slack=1)
    assert js == json.loads(want.to_json()) and js["slack"] == 1 and len(js["nodes"]) == len(nodes)
    n2 = found["key"].shape[2]
    for node in js["nodes"]:
        d = node["directions"]
        assert 0 <= d["+z"]["border_steps"] < n2 and 0 <= d["-z"]["border_steps"] < n2
    assert not math.isnan(sum(d["distance"] or 0.0 for node in js["nodes"] for d in node["directions"].values()))
