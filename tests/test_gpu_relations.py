"""Lattice relations on the GPU: clift_lattice_relations / backend="device" against backend="host" on every case of tests/relations_cases.py
(exact integers, every table, no tolerances), the tables cleared by the call itself, determinism, the scene graph from device counts, and the
relations stage of inference/extract_mesh.py on the scene130 field of the edited-mesh suite, unedited and under a move."""
import json

import numpy as np
import pytest
import torch

import edit_cases as ec
import edit_mesh_cases as emc
import relations_cases as rc
from test_gpu_edit_mesh import LEVEL, THINGS, UP, cli, scene, stages  # noqa: F401  (cli and scene are that module's fixtures, used here as they are)
from test_gpu_edit_program import box_C

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_CASES = {**rc.cases(), **rc.long_cases(), "skewed, 262144 points": rc.skew_case()}


@pytest.fixture(scope="module")
def host_tables():
    """case name -> the tables of backend="host": computed once, left unchanged."""
    from contrastive_lift_amd import relations
    return {name: rc.to_numpy(relations.relation_tables(key, n_keys, gap, backend="host")) for name, (key, n_keys, gap) in ALL_CASES.items()}


def device(key, n_keys, gap):
    from contrastive_lift_amd import relations
    out = relations.relation_tables(torch.from_numpy(key).to(DEV), n_keys, gap)
    assert all(v is None or v.is_cuda for v in out.values())
    return rc.to_numpy(out)


# ============================================================================ 1. parity and determinism
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_device_equals_host(host_tables, name):
    key, n_keys, gap = ALL_CASES[name]
    got = device(key, n_keys, gap)
    assert rc.same_tables(got, host_tables[name]) == "", (name, rc.same_tables(got, host_tables[name]))
    if name.startswith("room"):
        for (u, v, a), n in rc.ROOM_FACES.items():
            assert int(got["faces"][u, v, a]) == n, (u, v, a)
        assert got["near"] is None or int(got["near"][2, 3, 2]) == 9


@pytest.mark.parametrize("name", ["skewed, 262144 points", "64 keys in a wave", "random density 0.5", "long along 1", "n_keys 1024"])
def test_two_runs_give_the_same_bits(name):
    key, n_keys, gap = ALL_CASES[name]
    a, b = device(key, n_keys, gap), device(key, n_keys, gap)
    assert rc.same_tables(a, b) == ""


@pytest.mark.parametrize("name", ["random density 0.5", "n_keys 33", "room gap 0"])
def test_the_call_clears_its_tables(host_tables, name):
    """The raw entry on buffers full of other numbers: the call itself clears them, on its stream."""
    from contrastive_lift_amd import _lib
    key, n_keys, gap = ALL_CASES[name]
    k = torch.from_numpy(key).to(DEV)
    junk = lambda shape, dtype: torch.full(shape, 12345, dtype=dtype, device=DEV)
    out = dict(count=junk((n_keys,), torch.int64), isum=junk((n_keys, 3), torch.int64), ibox=junk((n_keys, 6), torch.int32),
               faces=junk((n_keys, n_keys, 3), torch.int32), near=junk((n_keys, n_keys, 3), torch.int32) if gap else None,
               rejected=junk((1,), torch.int32))
    for _ in range(2):                                         # the second call starts from the first one's results
        _lib.call("clift_lattice_relations", _lib.ptr(k), *key.shape, n_keys, gap, _lib.ptr(out["count"]), _lib.ptr(out["isum"]), _lib.ptr(out["ibox"]),
                  _lib.ptr(out["faces"]), _lib.ptr(out["near"]), _lib.ptr(out["rejected"]), _lib.stream())
        assert rc.same_tables(rc.to_numpy(out), host_tables[name]) == ""


def test_rejected_keys_and_the_python_raise(host_tables):
    from contrastive_lift_amd import _lib, relations
    key, n_keys, gap = ALL_CASES["rejected keys"]
    got = device(key, n_keys, gap)
    assert int(got["rejected"][0]) == int(((key < 0) | (key >= n_keys)).sum()) > 100
    with pytest.raises(_lib.CliftError, match="outside"):
        relations.lattice_relations(torch.from_numpy(key).to(DEV), n_keys, gap)
    with pytest.raises(_lib.CliftError, match="outside"):
        relations.lattice_relations(torch.from_numpy(rc.room()).to(DEV), 3, 1)
    out = relations.lattice_relations(torch.from_numpy(rc.room()).to(DEV), gap=1)                 # n_keys = max + 1
    assert rc.same_tables(rc.to_numpy(out), host_tables["room gap 1"]) == ""
    with pytest.raises(_lib.CliftError):
        relations.lattice_relations(torch.from_numpy(rc.room()), gap=1, backend="device")         # a host tensor: no quiet fall-back
    with pytest.raises(ValueError):
        relations.lattice_relations(torch.from_numpy(rc.room()).to(DEV), gap=5)
    mask = torch.from_numpy(rc.room() > 0).to(DEV)                                                 # a bool lattice: keys 0 and 1
    assert relations.lattice_relations(mask)["count"].tolist() == [rc.ROOM_COUNT[0], sum(rc.ROOM_COUNT[1:])]


@pytest.mark.parametrize("name", ["room gap 0", "room gap 1", "random density 0.5"])
def test_scene_graph_from_device_counts(name):
    from contrastive_lift_amd import relations
    key, n_keys, gap = ALL_CASES[name]
    nodes = [(k % 3, k) for k in range(1, n_keys)]
    ticks = [np.linspace(-1.0, 1.0, n) for n in key.shape]
    for up in ("+z", "-x"):
        on_device = relations.SceneGraph.from_counts(relations.lattice_relations(torch.from_numpy(key).to(DEV), n_keys, gap), nodes,
                                                     [torch.from_numpy(t).to(DEV) for t in ticks], up=up)
        on_host = relations.SceneGraph.from_counts(relations.lattice_relations(key, n_keys, gap, backend="host"), nodes, ticks, up=up)
        assert on_device == on_host and on_device.to_json() == on_host.to_json()
    if name == "room gap 1":
        assert on_host.nodes[2]["voxels"] == 18
        g = relations.SceneGraph.from_counts(relations.lattice_relations(torch.from_numpy(key).to(DEV), n_keys, gap), rc.ROOM_NODES, rc.ROOM_TICKS)
        assert g.on() == {2: [(1, 1.0)], 3: [(2, 1.0)]}


# ============================================================================ 2. the relations stage of inference/extract_mesh.py
OPTIONS = dict(gap=1, up="+z", min_faces=4)


def host_of_stage(cli, scene, out, edit, ids=None):
    """The tool's rule restated with backend="host": class and id of the inside points of the lattice it meshed, (class, id) -> key,
    the tables in numpy."""
    from contrastive_lift_amd import relations
    _, m, r = scene
    sem, p_ids = cli.lattice_nodes(m, r, out["sigma"], LEVEL, THINGS, None, False, edit=edit)
    key, nodes = relations.node_keys(sem.cpu(), (p_ids if ids is None else ids).cpu())
    return key, nodes, rc.to_numpy(relations.lattice_relations(key, len(nodes) + 1, OPTIONS["gap"], backend="host"))


@pytest.fixture(scope="module")
def plain_stage(cli, scene):
    return stages(cli, scene, None, relations=OPTIONS)[0]


def test_relations_stage_writes_both_files(cli, scene, plain_stage, tmp_path):
    from contrastive_lift_amd import relations
    _, m, r = scene
    out = plain_stage
    found = out["relations"]
    base = stages(cli, scene, None)[0]
    assert "relations" not in base and all(torch.equal(out[k], base[k]) for k in ("verts", "faces", "normals", "sem", "inst", "rgb"))
    inside = out["sigma"] >= LEVEL
    key, nodes, ref = host_of_stage(cli, scene, out, None)
    assert nodes == found["nodes"] and len(nodes) >= 1 and torch.equal(found["key"].cpu(), key) and torch.equal(found["key"] > 0, inside)
    assert rc.same_tables(rc.to_numpy(found["tables"]), ref) == ""
    ids = cli.lattice_ids(m, r, out["sigma"], LEVEL, THINGS, None, False)                        # the sibling keeps lattice_ids' numbers
    assert torch.equal(cli.lattice_nodes(m, r, out["sigma"], LEVEL, THINGS, None, False)[1], ids)
    assert int(ref["count"][1:].sum()) == int(inside.sum()) and int(ref["count"][0]) == int((~inside).sum())
    cli.write_relations(tmp_path, cli.relations_stem(None), found, OPTIONS["gap"])
    cli.write_relations(tmp_path, cli.relations_stem("move_1"), found, OPTIONS["gap"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["relations.json", "relations.npz", "relations_edit_move_1.json", "relations_edit_move_1.npz"]
    z = np.load(tmp_path / "relations.npz")
    assert rc.same_tables({k: z[k] for k in ref}, ref) == "" and z["nodes"].tolist() == [list(n) for n in nodes] and int(z["gap"]) == 1
    graph = json.load(open(tmp_path / "relations.json"))
    want = relations.SceneGraph.from_counts(ref, nodes, r.lattice_ticks(out["sigma"].shape), **{k: OPTIONS[k] for k in ("up", "min_faces")})
    assert graph == json.loads(want.to_json()) and [n["voxels"] for n in graph["nodes"]] == ref["count"][1:].tolist()
    ends = [t.cpu().numpy()[[0, -1]] for t in r.lattice_ticks(out["sigma"].shape)]
    for n in graph["nodes"]:                                   # centroids and boxes are world coordinates inside the scene box
        for a, (t0, t1) in enumerate(ends):
            assert t0 <= n["box"][a] <= n["centroid"][a] <= n["box"][3 + a] <= t1


def test_relations_under_a_move(cli, scene, plain_stage):
    """move(C, t) with --split_disconnected: the tables are the host's on the edited lattice with the split ids, and the nodes whose points
    lie inside the destination box do not have the extent and contacts that any node of the unedited scene has."""
    from contrastive_lift_amd import components, edit
    _, m, r = scene
    Cb = box_C()
    mv = edit.move(Cb, [0.45, -0.3, 0.1], ec.rot_xyz(0.0, 0.0, 0.3))
    out = stages(cli, scene, mv, split_disconnected=1, relations=OPTIONS)[0]
    found = out["relations"]
    assert not torch.equal(out["sigma"], plain_stage["sigma"])
    # the split restated: this call's ids, fresh ones above every id the vertices carried before the split
    base = stages(cli, scene, mv)[0]
    ids = cli.lattice_ids(m, r, out["sigma"], LEVEL, THINGS, None, False, edit=mv)
    new_ids, table = components.split_disconnected(ids, connectivity="kuhn", min_voxels=1, first_fresh=int(base["inst"].max()) + 1)
    assert table == out["table"]
    key, nodes, ref = host_of_stage(cli, scene, out, mv, ids=new_ids)
    assert nodes == found["nodes"] and torch.equal(found["key"].cpu(), key)
    assert rc.same_tables(rc.to_numpy(found["tables"]), ref) == ""
    # the nodes at the destination
    shape = tuple(out["sigma"].shape)
    ticks = [t.cpu().numpy() for t in r.lattice_ticks(shape)]
    at = np.argwhere(key.numpy() > 0)
    xyz = np.stack([ticks[a][at[:, a]] for a in range(3)], 1)
    moved = np.unique(key.numpy()[tuple(at[emc.box_depth(mv.dst, xyz) > 1e-5].T)])
    assert moved.size >= 1
    plain = rc.to_numpy(plain_stage["relations"]["tables"])
    signature = lambda t, k: (int(t["count"][k]), t["isum"][k].tolist(), t["ibox"][k].tolist(), t["faces"][k, 0].tolist(), t["faces"][0, k].tolist())
    before = [signature(plain, k) for k in range(1, plain["count"].shape[0])]
    print(f"nodes {plain_stage['relations']['nodes']} -> {nodes}; at the destination: keys {moved.tolist()}")
    for k in moved:
        assert signature(ref, int(k)) not in before, f"node {nodes[int(k) - 1]} stands as a node of the unedited scene does"
