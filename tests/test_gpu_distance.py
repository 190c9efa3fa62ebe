"""The lattice distance transform on the GPU: clift_lattice_distance / backend="device" against backend="host", word for word,
on every case of tests/distance_cases.py -- the chunks of a row, searches of unbounded length, one site in a corner, all sites, no site, 1024
keys --, the buffers filled by the call itself, determinism, every refusal of the entry point, ``separation`` and the two identities against
the DEVICE relations and clearance, ``placement`` on the scene130 field of the shaped-edit suite, and the two command lines."""
import importlib
import json
import pickle
import types

import numpy as np
import pytest
import torch

import clearance_cases as cc
import distance_cases as dc
import edit_cases as ec
import relations_cases as rc
from test_gpu_clearance import _table, hover_translation
from test_gpu_edit_mesh import LEVEL, THINGS, UP, cli, scene, stages  # noqa: F401  (cli and scene are that module's fixtures, used here as they are)
from test_gpu_edit_program import box_C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = dc.device_cases()
NAMES = ("packed", "rejected", "key_min")


def names_of(want_min):
    return NAMES if want_min else NAMES[:2]


@pytest.fixture(scope="module")
def host_tables():
    """case name -> the tables of backend="host": computed once, left unchanged."""
    from contrastive_lift_amd import distance
    return {name: dc.to_numpy(distance.distance_tables(key, n_keys, sites, want_min, backend="host")) for name, (key, n_keys, sites, want_min) in CASES.items()}


def device(key, n_keys, sites=None, want_min=True):
    from contrastive_lift_amd import distance
    out = distance.distance_tables(torch.from_numpy(key).to(DEV), n_keys, sites, want_min)
    assert all(v.is_cuda for v in out.values()) and out["packed"].dtype == torch.int64 and out["rejected"].dtype == torch.int32
    assert ("key_min" in out) == bool(want_min) and tuple(out["packed"].shape) == key.shape
    return dc.to_numpy(out)


# ============================================================================ 1. parity, seams, determinism
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host(host_tables, name):
    key, n_keys, sites, want_min = CASES[name]
    got = device(key, n_keys, sites, want_min)
    assert dc.same(got, host_tables[name], names_of(want_min)) == "", (name, dc.same(got, host_tables[name], names_of(want_min)))


def test_hand_checked_cases_on_the_device():
    from contrastive_lift_amd import distance
    key = np.zeros((1, 1, 5), np.int32)
    key[0, 0, [0, 4]] = 1                                                   # two sites symmetric about a point: the lower index wins
    dist2, nearest = distance.split(device(key, 2)["packed"])
    assert dist2.reshape(-1).tolist() == [0, 1, 4, 1, 0] and nearest.reshape(-1).tolist() == [0, 0, 0, 4, 4]
    key = np.zeros((3, 3, 3), np.int32)
    key[::2, ::2, ::2] = 1
    dist2, nearest = distance.split(device(key, 2)["packed"])
    assert dist2[1, 1, 1] == 3 and nearest[1, 1, 1] == 0 and dist2[1, 1, 2] == 2 and nearest[1, 1, 2] == 2
    corner = device(*CASES["one site in the far corner of (40, 40, 70)"][:2])
    assert int(corner["packed"][0, 0, 0]) == ((39 * 39 * 2 + 69 * 69) << 31) | (40 * 40 * 70 - 1) and int(corner["key_min"][1]) == 40 * 40 * 70 - 1
    for name in ("all background", "(5, 6, 7) density 0.0"):
        got = device(*CASES[name][:2])
        assert (got["packed"] == dc.NONE_WORD).all() and (got["key_min"] == dc.NONE_WORD).all() and int(got["rejected"][0]) == 0, name
    got = device(*CASES["all sites"][:2])
    assert np.array_equal(got["packed"].reshape(-1), np.arange(7 * 6 * 70)) and got["key_min"].tolist() == [dc.NONE_WORD, 0]
    key, n_keys, sites, _ = CASES["rejected keys"]
    got = device(key, n_keys, sites)
    assert int(got["rejected"][0]) == int(((key < 0) | (key >= n_keys)).sum()) > 100 and dc.check_nearest(key, n_keys, dc.table_of(sites, n_keys), got["packed"]) == ""
    with pytest.raises(distance._lib.CliftError, match="outside"):
        distance.lattice_distance(torch.from_numpy(key).to(DEV), n_keys)
    free = device(*CASES["background as the site"][:3])                     # the complement: scipy's distances to the nearest empty point
    assert np.array_equal(free["packed"] >> 31, dc.scipy_dist2(CASES["background as the site"][0] == 0))


@pytest.mark.parametrize("name", ["1024 keys, many in a wave", "(33, 31, 95) density 0.1", "33 keys, sites 1 .. 4", "rejected keys", "(200, 33, 70) one key of 8"])
def test_two_runs_give_the_same_bits(name):
    key, n_keys, sites, want_min = CASES[name]
    a, b = device(key, n_keys, sites, want_min), device(key, n_keys, sites, want_min)
    assert dc.same(a, b, names_of(want_min)) == ""


@pytest.mark.parametrize("name", ["(17, 9, 70) density 0.002", "1024 keys at random", "all background", "rejected keys"])
def test_the_call_fills_its_buffers(host_tables, name):
    """The raw entry on buffers full of other numbers: the call itself fills out, key_min and rejected, on its stream."""
    from contrastive_lift_amd import _lib
    key, n_keys, sites, _ = CASES[name]
    k = torch.from_numpy(key).to(DEV)
    site = torch.from_numpy(dc.table_of(sites, n_keys).astype(np.uint8)).to(DEV)
    junk = lambda shape, dtype: torch.full(shape, 12345, dtype=dtype, device=DEV)
    out = dict(packed=junk(key.shape, torch.int64), key_min=junk((n_keys,), torch.int64), rejected=junk((1,), torch.int32))
    work = junk((key.size,), torch.int64)
    for _ in range(2):                                         # the second call starts from the first one's results
        _lib.call("clift_lattice_distance", _lib.ptr(k), *key.shape, n_keys, _lib.ptr(site), _lib.ptr(out["packed"]), _lib.ptr(work),
                  _lib.ptr(out["key_min"]), _lib.ptr(out["rejected"]), _lib.stream())
        assert dc.same(dc.to_numpy(out), host_tables[name], NAMES) == ""


# ============================================================================ 2. the errors of the entry point
def test_every_error_of_the_entry_point():
    from contrastive_lift_amd import _lib
    key = torch.from_numpy(cc.cup_room()).to(DEV)
    n = tuple(key.shape)
    both = torch.full((2 * key.numel(),), 0x55, dtype=torch.int64, device=DEV)
    out, work = both[:key.numel()], both[key.numel():]
    key_min, rejected = torch.full((4,), 0x55, dtype=torch.int64, device=DEV), torch.full((1,), 0x55, dtype=torch.int32, device=DEV)
    site = torch.tensor([0, 1, 1, 1], dtype=torch.uint8, device=DEV)
    good = dict(key=key, n=n, n_keys=4, site=site, out=out, work=work, key_min=key_min, rejected=rejected)

    def call(**kw):
        a = {**good, **kw}
        _lib.call("clift_lattice_distance", _lib.ptr(a["key"]), *a["n"], a["n_keys"], _lib.ptr(a["site"]), _lib.ptr(a["out"]), _lib.ptr(a["work"]),
                  _lib.ptr(a["key_min"]) if a["key_min"] is not None else None, _lib.ptr(a["rejected"]), _lib.stream())
    bad = [(dict(n=(0, 12, 12)), r"clift_lattice_distance: lattice dimensions must be 1 .. 16384 \(got 0 x 12 x 12\)"),
           (dict(n=(12, -3, 12)), r"lattice dimensions must be 1 .. 16384 \(got 12 x -3 x 12\)"),
           (dict(n=(12, 12, 0)), r"lattice dimensions must be 1 .. 16384 \(got 12 x 12 x 0\)"),
           (dict(n=(16385, 1, 1)), r"lattice dimensions must be 1 .. 16384 \(got 16385 x 1 x 1\)"),
           (dict(n=(2048, 1024, 1024)), r"clift_lattice_distance: 2147483648 lattice points \(2048 x 1024 x 1024\), must be < 2\^31"),
           (dict(n_keys=0), r"clift_lattice_distance: n_keys must be 1 .. 1024 \(got 0\)"), (dict(n_keys=1025), r"n_keys must be 1 .. 1024 \(got 1025\)"),
           (dict(work=out), "clift_lattice_distance: out and work overlap"), (dict(work=both[1:]), "out and work overlap"),
           (dict(out=both[key.numel() - 1:]), "out and work overlap")]
    bad += [({name: None}, "clift_lattice_distance: NULL device buffer") for name in ("key", "site", "out", "work", "rejected")]
    for kw, msg in bad:
        with pytest.raises(_lib.CliftError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((both == 0x55).all()) and bool((key_min == 0x55).all()) and bool((rejected == 0x55).all())      # nothing was launched
    call(key_min=None)                                                                            # key_min is optional
    assert bool((key_min == 0x55).all()) and int(rejected[0]) == 0
    call()
    want = dc.brute_packed(cc.cup_room(), 4, dc.table_of(None, 4))
    assert np.array_equal(out.cpu().numpy().reshape(n), want) and np.array_equal(key_min.cpu().numpy(), dc.loop_key_min(cc.cup_room(), 4, want))


# ============================================================================ 3. separation and the identities
@pytest.fixture(scope="module")
def device_separation():
    """name -> the device separation tables of the identity lattices: computed once."""
    from contrastive_lift_amd import distance
    return {name: dc.to_numpy(distance.separation(torch.from_numpy(key).to(DEV), n_keys)) for name, (key, n_keys) in dc.identity_lattices().items()}


@pytest.mark.parametrize("name", sorted(dc.identity_lattices()))
def test_separation_device_equals_host(device_separation, name):
    from contrastive_lift_amd import distance
    key, n_keys = dc.identity_lattices()[name]
    want = dc.to_numpy(distance.separation(key, n_keys, backend="host"))
    got = device_separation[name]
    assert all(v.dtype == np.int32 for v in got.values())
    assert dc.same(got, want, ("gap2", "at", "to", "rejected")) == "", dc.same(got, want, ("gap2", "at", "to", "rejected"))
    assert np.array_equal(got["gap2"], got["gap2"].T)


def test_separation_refusals_on_the_device():
    from contrastive_lift_amd import _lib, distance
    key, n_keys, _ = rc.cases()["rejected keys"]
    with pytest.raises(_lib.CliftError, match="outside"):
        distance.separation(torch.from_numpy(key).to(DEV), n_keys)
    with pytest.raises(ValueError, match="--min_component"):
        distance.separation(torch.from_numpy(key).to(DEV), 257)
    with pytest.raises(_lib.CliftError, match="on the GPU"):
        distance.lattice_distance(torch.from_numpy(cc.cup_room()), backend="device")              # a host tensor: no quiet fall-back


def test_the_identities_against_the_device_relations_and_clearance(device_separation):
    from contrastive_lift_amd import clearance, relations
    ones = bounded = 0
    for name, (key, n_keys) in dc.identity_lattices().items():
        k = torch.from_numpy(key).to(DEV)
        rel = rc.to_numpy(relations.lattice_relations(k, n_keys, 0))
        clr = cc.to_numpy(clearance.lattice_clearance(k, n_keys, 0))
        sep = device_separation[name]
        assert dc.identities(sep, clr, rel) == "", name
        ones += int((sep["gap2"] == 1).sum())
        bounded += int((clr["pair"][1:, 1:] != cc.NONE).sum())
    assert ones > 100 and bounded > 100


def test_voronoi_keys_on_the_device():
    from contrastive_lift_amd import distance
    key, n_keys = CASES["33 keys, sites 1 .. 4"][:2]
    k = torch.from_numpy(key).to(DEV)
    packed = distance.lattice_distance(k, n_keys)["packed"]
    owner = distance.voronoi_keys(k, packed, max_dist2=4)
    host = distance.distance_tables(key, n_keys, backend="host")["packed"]
    assert owner.is_cuda and torch.equal(owner.cpu(), distance.voronoi_keys(key, host, max_dist2=4)) and bool((owner.cpu()[torch.from_numpy(key) > 0] > 0).all())


# ============================================================================ 4. placement on scene130's field
def recomposed(scene, e, level):
    """``placement`` again from get_dense_sigma, apply_to_points and the HOST backend."""
    from contrastive_lift_amd import clearance, distance, edit
    _, m, r = scene
    program = edit.as_program(e)
    last = program[len(program) - 1]
    sigma = r.get_dense_sigma(m, UP, edit=program)
    ticks = r.lattice_ticks(sigma.shape)
    state = edit.EditProgram([last]).apply_to_points(clearance.lattice_points(ticks), backend="device")[2]
    moved = (((state & edit.STATE_REMAPS) >= 1).view(sigma.shape) & (sigma >= level)).cpu().numpy()
    head = list(program)[:-1] + ([edit.Edit(edit.DELETE, last.src, shape=last.shape)] if last.mode == edit.MANIPULATE else [])
    before = r.get_dense_sigma(m, UP, edit=edit.EditProgram(head)) if head else r.get_dense_sigma(m, UP)
    key = (before >= level).cpu().numpy().astype(np.int32) + 2 * moved.astype(np.int32)
    return key, distance.placement_from_keys(key, [t.cpu() for t in ticks], backend="host")


@pytest.fixture(scope="module")
def blob_moves(scene):
    """Two moves of the blob by its shape (read from the field in box C at LEVEL): ``free`` sets it 3 empty lattice points above everything
    else, as a copy that stays; ``occupied`` is the same copy followed by a MOVE of the original to the very same place."""
    from contrastive_lift_amd import edit
    _, m, r = scene
    sh = edit.EditShape.from_field(m, r, box_C(), _table(m), dims=(12, 12, 12), grow=0, sigma_min=LEVEL)
    tz, _, _ = hover_translation(scene, edit.copy(box_C(), shape=sh), LEVEL)
    up = edit.copy(box_C(), [0.0, 0.0, tz], shape=sh)
    return dict(free=edit.move(box_C(), [0.0, 0.0, tz], shape=sh), occupied=edit.EditProgram([up, edit.move(box_C(), [0.0, 0.0, tz], shape=sh)]))


@pytest.mark.parametrize("which", ["free", "occupied"])
def test_placement_equals_its_recomposition(scene, blob_moves, which):
    from contrastive_lift_amd import distance
    _, m, r = scene
    e = blob_moves[which]
    got = distance.placement(m, r, e, upsample=UP, level=LEVEL)
    key, want = recomposed(scene, e, LEVEL)
    dkey, _ = distance.placement_key(m, r, e, UP, LEVEL)
    print(f"placement ({which}): {got}")
    assert np.array_equal(dkey.cpu().numpy(), key) and got == want
    assert got["n_moved"] == int((key >= 2).sum()) > 20 and got["overlap"] == int((key == 3).sum())
    if which == "occupied":
        assert got["verdict"] == "collides" and got["overlap"] > 0 and got["gap2"] == 0 and got["depth2"] >= 1 and got["moved_point"] == got["rest_point"]
    else:
        assert got["verdict"] == "clear" and got["overlap"] == 0 and got["gap2"] > 3 and got["depth2"] == 0


def test_placement_refusals(scene):
    from contrastive_lift_amd import _lib, distance, edit
    _, m, r = scene
    with pytest.raises(ValueError, match="copy or a move"):
        distance.placement(m, r, edit.delete(box_C()), upsample=UP, level=LEVEL)
    with pytest.raises(ValueError, match="copy or a move"):
        distance.placement(m, r, edit.EditProgram([edit.move(box_C(), [0.1, 0, 0]), edit.extract(box_C())]), upsample=UP, level=LEVEL)
    with pytest.raises(_lib.CliftError, match="moved set is empty"):
        distance.placement(m, r, edit.copy(box_C(), [0.0, 0.0, 5.0]), upsample=UP, level=LEVEL)


# ============================================================================ 5. the two command lines
def tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_edit_scene_check_placement(cli, scene, tmp_path, monkeypatch, capsys):
    """inference/edit_scene.py --op copy --follow_shape --check_placement on scene130's field (the loader, the frames and the output folder
    are stubbed, the rest is the tool's own): one line, placement.json = ``distance.placement``, and every other file of the output tree
    byte-equal to the run without the flag."""
    from contrastive_lift_amd import distance
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
    from contrastive_lift_amd import edit
    box = edit.EditBox(np.eye(3), [-0.05, 0.0, 0.05], [-0.15, -0.15, -0.15], [0.15, 0.15, 0.15])  # the blob's core
    boxes = {1: {"bbox": (box.lo, box.hi), "orientation": box.axes, "position": box.centre}}
    path = tmp_path / "bboxes.pkl"
    with open(path, "wb") as f:
        pickle.dump(boxes, f)
    lines = {}
    shape_of = es.field_shapes(m, r, es.shape_table(cfg, data, None), 12, 0, 0.5)
    tz, _, _ = hover_translation(scene, es.resolve_edit(boxes, 1, "copy", shape=shape_of), cli.default_level(r, 0.5))    # 3 empty points over everything
    for name, t in (("collides", ["0.05", "0", "0.05"]), ("apart", ["0", "0", repr(tz)])):
        monkeypatch.setattr(es.rp, "output_dirname", lambda *a, root=tmp_path / name: root / "runs" / "scene130_test")      # a folder per edit
        out = tmp_path / name / "runs" / "scene130_test_edit_copy_1_shape"
        argv = ["--ckpt_path", "runs/x/checkpoints/y.ckpt", "--bboxes", str(path), "--instance", "1", "--op", "copy", "--translate", *t,
                "--follow_shape", "--shape_grid", "12", "--shape_grow", "0"]
        es.main(argv)
        plain = tree(out)
        capsys.readouterr()
        es.main(argv + ["--check_placement", "--placement_upsample", str(UP)])
        text = capsys.readouterr().out
        line = [ln for ln in text.splitlines() if ln.startswith("placement: ")]
        assert len(line) == 1, text
        lines[name] = line[0]
        print(line[0])
        after = tree(out)
        assert "placement.json" not in plain and sorted(set(after) - set(plain)) == ["placement.json"]
        assert all(after[k] == v for k, v in plain.items()) and "rgb/around.png" in plain                 # the render does not change
        e = es.resolve_edit(boxes, 1, "copy", [float(x) for x in t], shape=shape_of)
        want = distance.placement(m, r, e, upsample=UP)
        assert json.loads(after["placement.json"]) == json.loads(json.dumps(want)) and line[0] == es.placement_line(want)
    assert lines["collides"].startswith("placement: collides on ") and ", depth " in lines["collides"]
    assert lines["apart"].startswith("placement: clear, gap ") and " cells = " in lines["apart"]  # (at least 4 steps: dz alone is 4)


def test_separation_stage_writes_both_files(cli, scene, tmp_path):
    from contrastive_lift_amd import distance
    _, m, r = scene
    rel_options = dict(gap=1, up="+z", min_faces=4)
    every = stages(cli, scene, None, relations=rel_options, clearance=dict(slack=1), separation=dict(max_cells=None))[0]
    only = stages(cli, scene, None, separation=dict(max_cells=3.0))[0]
    base = stages(cli, scene, None, relations=rel_options, clearance=dict(slack=1))[0]
    assert "separation" not in base and "relations" not in only and "clearance" not in only
    found = every["separation"]
    assert found["key"] is every["relations"]["key"] and found["nodes"] == every["relations"]["nodes"] == only["separation"]["nodes"]    # one labelling
    assert torch.equal(only["separation"]["key"], found["key"]) and only["separation"]["summary"].nodes == found["summary"].nodes
    for name in ("relations", "clearance"):                                                       # relations and clearance do not change
        for k, v in base[name]["tables"].items():
            assert v is None or torch.equal(v, every[name]["tables"][k]), (name, k)
    assert all(torch.equal(every[k], base[k]) for k in ("verts", "faces", "normals", "sem", "inst", "rgb"))
    nodes = found["nodes"]
    ref = dc.to_numpy(distance.separation(found["key"].cpu(), len(nodes) + 1, backend="host"))
    assert dc.same(dc.to_numpy(found["tables"]), ref, ("gap2", "at", "to")) == "" and len(nodes) >= 1
    cli.write_separation(tmp_path, cli.separation_stem(None), found)
    cli.write_separation(tmp_path, cli.separation_stem("move_1"), only["separation"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["separation.json", "separation.npz", "separation_edit_move_1.json", "separation_edit_move_1.npz"]
    z = np.load(tmp_path / "separation.npz")
    assert dc.same({k: z[k] for k in ("gap2", "at", "to")}, ref, ("gap2", "at", "to")) == "" and z["nodes"].tolist() == [list(n) for n in nodes]
    ticks = r.lattice_ticks(found["key"].shape)
    js = json.load(open(tmp_path / "separation.json"))
    assert js == json.loads(distance.Separation.from_tables(ref, nodes, ticks).to_json()) and len(js["nodes"]) == len(nodes) and js["max_cells"] is None
    js3 = json.load(open(tmp_path / "separation_edit_move_1.json"))
    assert js3 == json.loads(distance.Separation.from_tables(ref, nodes, ticks, max_cells=3.0).to_json()) and js3["max_cells"] == 3.0
    assert all(p["cells"] <= 3.0 for p in js3["pairs"]) and len(js3["pairs"]) <= len(js["pairs"])
