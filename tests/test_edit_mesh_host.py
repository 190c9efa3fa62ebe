"""Edited-scene meshes, the host side: ``EditProgram.apply_to_points(backend="host")`` against the walks that exist already, and the command
line of inference/extract_mesh.py (flags, file names, refusals).  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import edit_mesh_cases as emc
import edit_program_cases as epc
from conftest import REPO


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cli():
    return _load(os.path.join(REPO, "inference", "extract_mesh.py"), "clift_extract_mesh_cli_edit_host")


# ---------------------------------------------------------------------------- apply_to_points on the host
@pytest.mark.parametrize("name", ["chain", "eight"])
def test_host_walk_equals_source_points_and_killed(name):
    from contrastive_lift_amd import edit
    prog = emc.program(name)
    pts, dirs = emc.cloud_points()
    p, d, state = prog.apply_to_points(pts, dirs, backend="host")
    sp, sd = prog.source_points(pts, dirs)
    assert p.dtype == np.float64 and state.dtype == np.uint8 and state.shape == (pts.shape[0],)
    assert np.array_equal(p, sp) and np.array_equal(d, sd)
    killed = (state & edit.STATE_KILLED) != 0
    assert np.array_equal(killed, prog.killed(pts)) and killed.sum() > 50
    hops = state & edit.STATE_REMAPS
    assert hops.max() >= 2 and hops.max() <= len(prog)
    assert np.array_equal(p[hops == 0], pts[hops == 0].astype(np.float64)) and np.array_equal(d[hops == 0], dirs[hops == 0].astype(np.float64))
    p2, d2, state2 = prog.apply_to_points(torch.from_numpy(pts), None, backend="host")            # tensors are taken too; dirs are optional
    assert d2 is None and np.array_equal(p2, p) and np.array_equal(state2, state)
    w = emc.ref_walk(prog, pts, dirs)                   # the tests' fp64 walk over the fp32 records: the same classification off the faces
    assert np.array_equal(state[w["keep"]], w["state"][w["keep"]])
    with pytest.raises(ValueError):
        prog.apply_to_points(pts, backend="cpu")


def test_host_walk_counts_are_the_restatements_hops():
    from contrastive_lift_amd import edit
    from test_gpu_edit_program import chain_case
    prog, specs, _ = chain_case()
    pts, dirs = emc.cloud_points()
    w = emc.ref_walk(prog, pts, dirs)
    assert int((~w["keep"]).sum()) <= 8
    _, _, dead, hops = epc.walk(torch.from_numpy(pts), torch.from_numpy(dirs), specs)          # fp32 torch, from the motion of the object
    _, _, state = prog.apply_to_points(pts, dirs, backend="host")
    keep = w["keep"]
    assert np.array_equal((state & edit.STATE_REMAPS)[keep], hops.numpy()[keep])
    assert np.array_equal(((state & edit.STATE_KILLED) != 0)[keep], dead.numpy()[keep])
    assert (hops.numpy() == 2).sum() > 100


# ---------------------------------------------------------------------------- the command line
BASE = ["--ckpt_path", "runs/x/checkpoints/last.ckpt"]


def test_old_flags_keep_their_defaults(cli):
    a = cli.build_parser().parse_args(BASE)
    assert (a.upsample, a.alpha_level, a.level, a.cached_centroids_path, a.split_instances, a.save_voxel_cloud) == (2, 0.5, None, None, False, False)
    assert (a.min_component, a.keep_largest, a.connectivity, a.split_disconnected, a.image_dim) == (0, None, "kuhn", None, [256, 384])
    assert (a.bboxes, a.instance, a.op, a.script, a.translate, a.rotate_deg, a.pad) == (None, None, None, None, [0.0] * 3, [0.0] * 3, 0.0)
    assert cli.edit_tag_of(a) is None and cli.mesh_stem(cli.edit_tag_of(a)) == "mesh"
    assert cli.resolve_cli_edit(a) == (None, None)
    b = cli.build_parser().parse_args(BASE + ["--upsample", "3", "--split_disconnected", "--save_voxel_cloud", "--keep_largest", "2"])
    assert (b.upsample, b.split_disconnected, b.save_voxel_cloud, b.keep_largest) == (3, 1, True, 2)


def test_edit_flags_and_file_names(cli):
    ap = cli.build_parser()
    a = ap.parse_args(BASE + ["--bboxes", "b.pkl", "--instance", "4", "--op", "move", "--translate", "0.1", "0", "-0.2", "--rotate_deg", "0", "0", "30",
                              "--pad", "0.02", "--split_disconnected", "5"])
    assert (a.bboxes, a.instance, a.op, a.translate, a.rotate_deg, a.pad, a.split_disconnected) == ("b.pkl", 4, "move", [0.1, 0.0, -0.2], [0.0, 0.0, 30.0], 0.02, 5)
    assert cli.mesh_stem(cli.edit_tag_of(a)) + ".ply" == "mesh_edit_move_4.ply"
    s = ap.parse_args(BASE + ["--bboxes", "b.pkl", "--script", "some/dir/tidy_up.json"])
    assert cli.mesh_stem(cli.edit_tag_of(s)) + ".ply" == "mesh_edit_script_tidy_up.ply"
    assert f"{cli.mesh_stem(cli.edit_tag_of(s))}_instance_7.ply" == "mesh_edit_script_tidy_up_instance_7.ply"
    for op in ("delete", "extract", "copy", "move"):
        assert cli.edit_tag_of(ap.parse_args(BASE + ["--bboxes", "b.pkl", "--instance", "2", "--op", op])) == f"{op}_2"


@pytest.mark.parametrize("argv", [
    ["--bboxes", "b.pkl", "--script", "e.json", "--op", "delete", "--instance", "1"],         # --script and --op exclude each other
    ["--bboxes", "b.pkl", "--script", "e.json", "--instance", "1"],
    ["--instance", "1", "--op", "delete"],                                                    # either needs --bboxes
    ["--script", "e.json"],
    ["--bboxes", "b.pkl"],                                                                     # boxes without an edit
    ["--bboxes", "b.pkl", "--op", "delete"],                                                   # an op without its instance
    ["--bboxes", "b.pkl", "--instance", "1"],
    ["--bboxes", "b.pkl", "--instance", "1", "--op", "duplicate"],                             # the tool's ops are the rigid ones
])
def test_edit_flag_combinations_that_are_refused(cli, argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(BASE + argv)
    assert e.value.code == 2 and "error" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--instance", "1", "--op", "delete"], ["--script", "e.json"]])
def test_voxel_cloud_with_an_edit_says_why(cli, argv):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(BASE + ["--bboxes", "b.pkl", "--save_voxel_cloud"] + argv)
    assert "get_instance_clusters" in str(e.value.code) and "model grid" in str(e.value.code)
    from contrastive_lift_amd import edit
    with pytest.raises(SystemExit) as e2:                                    # the function refuses it too, before it loads anything
        cli.extract_mesh(None, save_voxel_cloud=True, edit=edit.delete(edit.EditBox(np.eye(3), np.zeros(3), -np.ones(3), np.ones(3))), edit_tag="delete_1")
    assert str(e2.value.code) == str(e.value.code)


def test_cli_edit_resolves_through_edit_scene(cli, tmp_path):
    """``resolve_cli_edit`` reads the boxes and hands them to inference/edit_scene.py's resolvers: the records are those that tool renders."""
    import json
    import pickle
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_scene_cli_edit_host")
    boxes = {3: {"orientation": np.eye(3), "position": np.array([0.1, 0.0, -0.1]), "bbox": (np.array([-0.2, -0.1, -0.3]), np.array([0.2, 0.1, 0.3]))}}
    bp, sp = str(tmp_path / "bboxes.pkl"), str(tmp_path / "two.json")
    pickle.dump(boxes, open(bp, "wb"))
    entries = [{"instance": 3, "op": "move", "translate": [0.3, 0.0, 0.0]}, {"instance": 3, "op": "copy", "at": "moved", "rotate_deg": [0, 0, 90]}]
    json.dump(entries, open(sp, "w"))
    ap = cli.build_parser()
    e, tag = cli.resolve_cli_edit(ap.parse_args(BASE + ["--bboxes", bp, "--instance", "3", "--op", "copy", "--translate", "0", "0.2", "0", "--pad", "0.01"]))
    assert tag == "copy_3" and e.record_bytes() == es.resolve_edit(boxes, 3, "copy", [0.0, 0.2, 0.0], [0.0, 0.0, 0.0], 0.01).record_bytes()
    p, tag = cli.resolve_cli_edit(ap.parse_args(BASE + ["--bboxes", bp, "--script", sp]))
    assert tag == "script_two" and len(p) == 2 and p.record_bytes() == es.resolve_program(boxes, entries).record_bytes()
