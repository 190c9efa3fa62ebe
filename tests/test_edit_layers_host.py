"""CPU checks for the layers of an edited scene: the fp64 origin walk (``EditProgram.origins``), the copy columns of
``SlotTable.for_program``, ``layers.retarget``, ``layers.compare``, the ``--save_layers`` flags of inference/edit_scene.py, and what
tests/test_gpu_edit_layers.py takes for granted about its scene -- asserted here from the oracle and the fp64 walk alone."""
import os
import sys

import numpy as np
import pytest
import torch

import edit_layers_cases as elc
import edit_program_cases as epc
import edit_surface_cases as esc
from conftest import REPO, load_golden
from contrastive_lift_amd import edit as ed
from contrastive_lift_amd import layers as ly
from contrastive_lift_amd.layers import SlotTable


@pytest.fixture(scope="module")
def scene():
    g = load_golden("g27_dense_volume")
    P, cfg, res, C_, E, shift, aabb = elc.oracle_scene(g)
    assert res == (9, 13, 17) and cfg.n_samples == 75 and shift == -3.0
    rays = elc.scene_rays()
    lo, hi = aabb[0].double().numpy(), aabb[1].double().numpy()
    return dict(P=P, cfg=cfg, rays=rays, lo=lo, hi=hi, walks={k: elc.host_walk(rays, cfg, p) for k, p in elc.programs().items()})


# ----------------------------------------------------------------------------- EditProgram.origins
def test_origins_on_points_inside_the_boxes():
    b, progs = elc.boxes(), elc.programs()
    rng = np.random.default_rng(0)
    inside = lambda box: rng.uniform(-0.15, 0.15, (50, 3)) @ box.axes + box.centre
    far = np.array([[0.6, -0.5, -0.3]]) + rng.uniform(-0.02, 0.02, (50, 3))
    # [cp]: the copy has origin 1 and one hop, the original and everything else origin 0
    src, o, s = progs["cp"].origins(np.concatenate([inside(b["cp"].dst), inside(b["core"]), far]))
    assert o.dtype == np.uint8 and s.dtype == np.uint8
    assert (o[:50] == 1).all() and (s[:50] == 1).all() and (o[50:] == 0).all() and (s[50:] == 0).all()
    assert b["core"].contains(src[:50]).all()
    # [cp, mv]: the moved copy keeps origin 1, with two hops; where the copy stood is empty now
    src, o, s = progs["cp_mv"].origins(np.concatenate([inside(b["mv"].dst), inside(b["cp"].dst), inside(b["core"])]))
    assert (o[:50] == 1).all() and (s[:50] == 2).all() and b["core"].contains(src[:50]).all()
    assert ((s[50:100] & ed.STATE_KILLED) != 0).all() and (o[50:100] == 0).all()
    assert (o[100:] == 0).all() and (s[100:] == 0).all()
    # [cp, cp2]: the copy of the copy has origin 2 (the outer one wins) and two hops, the first copy origin 1
    src, o, s = progs["cp_cp2"].origins(np.concatenate([inside(b["cp2"].dst), inside(b["cp"].dst)]))
    assert (o[:50] == 2).all() and (s[:50] == 2).all() and (o[50:] == 1).all() and (s[50:] == 1).all()
    assert b["core"].contains(src).all()
    # a move alone: remapped, but no copy
    src, o, s = progs["mv_only"].origins(np.concatenate([inside(b["mv_only"].dst), inside(b["core"])]))
    assert (o == 0).all() and (s[:50] == 1).all() and ((s[50:] & ed.STATE_KILLED) != 0).all()


def test_origins_leave_jacobians_alone_and_agree_with_them():
    lo, hi = np.array([-0.9, -0.7, -0.5]), np.array([0.8, 0.7, 0.6])
    pts = esc.world_points(2000, lo, hi, 11).astype(np.float64)
    for name, prog in esc.programs(lo, hi).items():
        src, J, state = prog.jacobians(pts)
        src2, origin, state2 = prog.origins(pts)
        assert np.array_equal(src, src2) and np.array_equal(state, state2), name
        copies = {i + 1 for i in prog.copies()}
        assert set(np.unique(origin).tolist()) <= copies | {0}, name
        assert (origin[(state & ed.STATE_REMAPS) == 0] == 0).all(), name
    prog = esc.programs(lo, hi)["full8"]
    assert prog.copies() == [1, 4] and set(np.unique(prog.origins(pts)[1]).tolist()) == {0, 2, 5}
    p, d, dead, hops = prog._walk(pts, None)                                    # the walk's other callers see what they saw
    assert np.array_equal(p, prog.source_points(pts))


def test_origin_restatement_in_fp32_agrees_off_the_faces():
    lo, hi = np.array([-0.9, -0.7, -0.5]), np.array([0.8, 0.7, 0.6])
    pts = esc.world_points(3000, lo, hi, 12)
    for name, prog in esc.programs(lo, hi).items():
        _, o64, s64 = prog.origins(pts.astype(np.float64))
        _, o32, s32 = elc.origin_restatement(prog, pts)
        keep = esc.face_distance(prog, pts.astype(np.float64)) >= 1e-5
        assert keep.sum() > 2900 and np.array_equal(o32[keep], o64[keep]) and np.array_equal(s32[keep], s64[keep]), name


# ----------------------------------------------------------------------------- the table, the retargeting, compare
def _table(K_per=(2, 3)):
    cents = {c + 1: np.zeros((k, 3), np.float32) + c for c, k in enumerate(K_per)}
    return SlotTable.from_centroids(cents, list(cents), 4)


def test_for_program_numbers_the_copies_behind_the_slots():
    t = _table()
    b = elc.boxes()
    prog = ed.EditProgram([b["mv_only"], b["cp"], ed.delete(esc.empty_box()), b["cp2"]])
    x = t.for_program(prog)
    assert t.K == 5 and x.K == 7 and x.K_base == 5 and x.base is t
    assert x.copy_edit.tolist() == [1, 3] and x.slot_class.tolist() == t.slot_class.tolist() + [-1, -1]
    assert x.slot_index.tolist() == t.slot_index.tolist() + [1, 3]
    assert np.array_equal(x.cls_slots, t.cls_slots) and x.centroids.shape == (5, 3) and x.num_classes == 4 and x.mode == 0
    assert x.origin_columns().tolist() == [-1, -1, 5, -1, 6]
    same = t.for_program(b["mv_only"])                                          # an Edit, no copy: the same K slots
    assert same.K == 5 and same.copy_edit.shape == (0,)
    assert t.for_program([b["cp"]]).K == 6                                      # a sequence
    with pytest.raises(ValueError, match="copy slots"):
        x.for_program(prog)
    big = SlotTable.from_scores([1], 2, 250)
    six = ed.EditProgram([b["cp"]] * 6)
    assert big.for_program(ed.EditProgram([b["cp"]] * 5)).K == 255
    with pytest.raises(ValueError, match=r"250 slots and 6 copies"):
        big.for_program(six)
    L = torch.zeros((4, x.K + 1, 4))
    s = ly.summarise(L, x)                                                      # summarise and front_order take it unchanged
    assert s["amodal_pixels"].shape == (7,) and s["slot_class"].tolist()[-2:] == [-1, -1]
    assert ly.front_order(L)[0].shape == (4, 7)


def test_retarget_on_made_up_rows():
    t = _table()
    b = elc.boxes()
    x = t.for_program([b["cp"], b["mv"], b["cp2"]])                             # copies at program positions 0 and 2
    base = torch.tensor([0, 4, -1, -1, 3, 2, 1, 0], dtype=torch.int32)
    origin = torch.tensor([0, 1, 1, 0, 3, 3, 1, 0], dtype=torch.uint8)
    got = ly.retarget(base, origin, x)
    assert got.dtype == torch.int32 and got.tolist() == [0, 5, -1, -1, 6, 6, 5, 0]
    assert np.array_equal(elc.retarget_restatement(base.numpy(), origin.numpy(), 5, x.copy_edit), got.numpy())
    none = t.for_program(b["mv_only"])
    assert ly.retarget(base, torch.zeros(8, dtype=torch.uint8), none).tolist() == base.tolist()
    assert ly.retarget(base[:0], origin[:0], x).shape == (0,)


def test_compare_on_a_hand_made_pair():
    t = SlotTable.from_centroids({1: np.zeros((2, 3), np.float32)}, [1], 2)
    x = t.for_program(elc.boxes()["cp"])
    before = torch.zeros((5, 3, 4))
    after = torch.zeros((5, 4, 4))
    # slot 0: rays 0-2 amodal and visible before; after: ray 0 unchanged, ray 1 hidden (A stays), ray 2 gone
    before[0:3, 0, 0], before[0:3, 0, 1] = 0.9, 0.8
    after[0, 0, 0], after[0, 0, 1] = 0.9, 0.8
    after[1, 0, 0], after[1, 0, 1] = 0.9, 0.1
    # slot 1: rays 3-4 amodal and hidden before; after: ray 3 revealed, ray 4 as it was
    before[3:5, 1, 0], before[3:5, 1, 1] = 0.95, 0.2
    after[3, 1, 0], after[3, 1, 1] = 0.95, 0.7
    after[4, 1, 0], after[4, 1, 1] = 0.95, 0.2
    # the copy: rays 1 and 2, visible
    after[1:3, 2, 0], after[1:3, 2, 1] = 0.99, 0.9
    c = ly.compare(before, after, t, x, 0.5)
    assert c["amodal_pixels_before"].tolist() == [3, 2, 0] and c["amodal_pixels_after"].tolist() == [2, 2, 2]
    assert c["visible_pixels_before"].tolist() == [3, 0, 0] and c["visible_pixels_after"].tolist() == [1, 1, 2]
    assert c["newly_hidden"].tolist() == [1, 0, 0] and c["revealed"].tolist() == [0, 1, 0] and c["gone"].tolist() == [1, 0, 0]
    assert c["slot_class"].tolist() == [1, 1, -1] and c["slot_index"].tolist() == [0, 1, 0]
    same = ly.compare(before, before, t, t)
    assert all(int(same[k].sum()) == 0 for k in ("newly_hidden", "revealed", "gone"))
    with pytest.raises(ValueError, match="rays"):
        ly.compare(before[:4], after, t, x)
    with pytest.raises(ValueError, match="begin with"):
        ly.compare(after, before, x, t)


# ----------------------------------------------------------------------------- the command line
def test_edit_scene_parses_the_layer_flags(monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene
    finally:
        sys.path.pop(0)
    seen = {}
    monkeypatch.setattr(edit_scene, "load_run_config", lambda p: type("Cfg", (), {})())
    monkeypatch.setattr(edit_scene.pickle, "load", lambda f: {3: {"bbox": (-np.ones(3), np.ones(3)), "orientation": np.eye(3), "position": np.zeros(3)}})
    monkeypatch.setattr(edit_scene, "edit_scene_checkpoint", lambda cfg, e, tag, **kw: seen.update(kw, tag=tag) or "out")
    base = ["--ckpt_path", "runs/x/checkpoints/a.ckpt", "--bboxes", os.path.join(REPO, "pytest.ini"), "--instance", "3", "--op", "copy",
            "--translate", "0.1", "0", "0"]
    edit_scene.main(base)
    assert seen["save_layers"] is False and seen["cached_centroids_path"] is None and seen["layers_level"] == 0.5
    edit_scene.main(base + ["--save_layers", "--cached_centroids_path", "c.pkl", "--layers_level", "0.25"])
    assert seen["save_layers"] is True and seen["cached_centroids_path"] == "c.pkl" and seen["layers_level"] == 0.25 and seen["tag"] == "copy_3"


def test_change_summary_lists_the_slots_with_pixels():
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene
    finally:
        sys.path.pop(0)
    t = SlotTable.from_centroids({1: np.zeros((2, 3), np.float32)}, [1], 2)
    x = t.for_program(elc.boxes()["cp"])
    before, after = torch.zeros((4, 3, 4)), torch.zeros((4, 4, 4))
    before[:2, 1, :2] = 0.9
    after[:2, 2, :2] = 0.9
    js = edit_scene.change_summary("f0", before, after, t, x, 0.5)
    assert js["n_slots"] == 3 and js["n_base_slots"] == 2 and js["copy_edit"] == [0] and [s["slot"] for s in js["slots"]] == [1, 2]
    assert js["slots"][0]["gone"] == 2 and js["slots"][1]["amodal_pixels_after"] == 2 and js["slots"][1]["amodal_pixels_before"] == 0


# ----------------------------------------------------------------------------- the scene of the GPU tests
def test_the_scene_of_the_gpu_tests_holds_what_they_rely_on(scene):
    """From the fp32 oracle and the fp64 walk alone: the destination boxes lie inside the aabb; 2 of the 194 rays are left out per program;
    113, 110 and 105 rays are touched by no edit; hop counts reach 2 in the two longer programs and [cp, mv] kills 744 samples; the
    origins are {0, 1}, {0, 1} with 2 hops on the moved copy, {0, 1, 2}, and all 0 for the move alone."""
    b, progs, walks, rays, cfg = elc.boxes(), elc.programs(), scene["walks"], scene["rays"], scene["cfg"]
    assert rays.shape == (194, 8)
    for e in (b["cp"], b["mv"], b["cp2"]):
        assert (e.dst.centre - elc.CORE_HALF >= scene["lo"]).all() and (e.dst.centre + elc.CORE_HALF <= scene["hi"]).all()
    for name, untouched, hops_max in (("cp", 113, 1), ("cp_mv", 110, 2), ("cp_cp2", 105, 2)):
        keep = epc.rays_off_all_faces(rays, cfg, progs[name])
        assert int((~keep).sum()) == 2, name
        w = walks[name]
        assert int(elc.untouched_rays(w).sum()) == untouched, name
        assert int((w["state"] & ed.STATE_REMAPS).max()) == hops_max, name
    assert int(((walks["cp_mv"]["state"] & ed.STATE_KILLED) != 0).sum()) == 744
    assert set(np.unique(walks["cp"]["origin"]).tolist()) == {0, 1}
    w = walks["cp_mv"]
    in_mv = b["mv"].dst.contains(w["points"])
    assert in_mv.sum() > 100 and (w["origin"][in_mv] == 1).all() and (w["state"][in_mv] == 2).all()
    assert (w["origin"][~in_mv] == 0).all()                                     # where the copy stood nothing is left of it
    w = walks["cp_cp2"]
    in_cp2 = b["cp2"].dst.contains(w["points"])
    assert in_cp2.sum() > 30 and (w["origin"][in_cp2] == 2).all() and (w["origin"][b["cp"].dst.contains(w["points"])] == 1).all()
    assert (walks["mv_only"]["origin"] == 0).all() and (walks["mv_only"]["state"] != 0).any()


def test_the_copy_brings_the_hidden_core_into_view_in_the_oracle(scene):
    """On the 64 front rays, by the oracle: the samples inside ``core`` are jointly opaque (A = 1.000) and all but invisible (V < 1e-3),
    before and after the copy -- the blob's own tail hides them; the copy's samples are visible, V >= 0.88 on every ray."""
    P, cfg, lo, hi = scene["P"], scene["cfg"], scene["lo"], scene["hi"]
    front = elc.front_rays()
    core = elc.boxes()["core"]
    plain = elc.host_walk(front, cfg, ed.EditProgram([ed.delete(esc.empty_box())]))
    assert (plain["state"] == 0).all()
    copied = elc.host_walk(front, cfg, elc.programs()["cp"])
    thres = 1e-4
    in_core = core.contains(copied["points"]).reshape(64, -1)
    for walk in (plain, copied):
        a, w = elc.oracle_weights(P, cfg, walk, lo, hi)
        origin = walk["origin"].reshape(64, -1)
        sel = in_core & (origin == 0) & (a > thres)
        A = 1.0 - np.prod(np.where(sel, 1.0 - a, 1.0), 1)
        V = (w * sel).sum(1)
        assert A.min() > 0.9995 and V.max() < 1e-3
    v_copy = (w * ((origin == 1) & (a > thres))).sum(1)
    print(f"oracle: V_copy min {v_copy.min():.4f}")
    assert 0.88 < v_copy.min() < 0.89


def test_on_the_side_rays_only_the_moved_copy_is_opaque(scene):
    """The 16 side rays of the GPU test under [cp, mv], by the oracle: the samples the moved copy brought are jointly opaque (A > 0.99) and
    everything else listed along the ray -- the floor and the blob's tail, whatever slots they get -- gathers less than the level 0.9 of that test (0.857 at
    most), so no column but the copy's can be on."""
    P, cfg, lo, hi = scene["P"], scene["cfg"], scene["lo"], scene["hi"]
    walk = elc.host_walk(elc.side_rays(), cfg, elc.programs()["cp_mv"])
    a, _ = elc.oracle_weights(P, cfg, walk, lo, hi)
    origin, listed = walk["origin"].reshape(16, -1), a > 1e-4
    a_copy = 1.0 - np.prod(np.where((origin == 1) & listed, 1.0 - a, 1.0), 1)
    a_rest = 1.0 - np.prod(np.where((origin == 0) & listed, 1.0 - a, 1.0), 1)
    print(f"oracle: copy A min {a_copy.min():.4f}, everything else A max {a_rest.max():.4f}")
    assert a_copy.min() > 0.99 and a_rest.max() < 0.9


def test_every_rank_enters_the_same_collectives_under_save_layers(monkeypatch, tmp_path):
    """``render_rays_sharded`` ends in a collective, so under torch.distributed.run every rank has to call it the same number of times per
    frame, in the same order, with the same pass: with --save_layers the edit render, the edited layer pass and the plain layer pass on
    every rank, the files from rank 0 alone.  The renders are stubbed; the frame loop is the tool's own."""
    sys.path.insert(0, os.path.join(REPO, "inference"))
    try:
        import edit_scene as es
    finally:
        sys.path.pop(0)
    table = SlotTable.from_centroids({1: np.zeros((2, 3), np.float32)}, [1], 2)
    the_edit = elc.boxes()["cp"]
    H, W = 2, 3
    scene = type("Scene", (), {"image_dim": (H, W), "white_bg": False})()
    config = type("Cfg", (), {"chunk": 4, "use_delta": False})()
    frames = [("f0", torch.zeros(H * W, 8), None), ("f1", torch.zeros(H * W, 8), None)]

    def run(rank, **kw):
        calls, written = [], []
        out_root = tmp_path / f"rank{rank}_{len(kw)}"

        def sharded(model, renderer, rays, chunk, white_bg=False, render_fn=None):
            name = render_fn.func.__name__
            calls.append(name)
            n = rays.shape[0]
            if name == "render_rays_edit":
                return torch.zeros(n, 3), torch.zeros(n, 2), None, torch.ones(n)
            K = table.K + (1 if name == "render_rays_edit_layers" else 0)
            return torch.zeros(n, K + 1, 4), torch.zeros(n), torch.zeros(n)

        def write_frame(out, name, layers, tab, h, w, rgb, level):
            (out / "layers").mkdir(exist_ok=True, parents=True)
            written.append((name, tuple(layers.shape), tab.K))
        monkeypatch.setattr(es.rp, "distributed_device", lambda device: ("cpu", rank))
        monkeypatch.setattr(es.rp, "load_for_inference", lambda cfg, device: (scene, None, None))
        monkeypatch.setattr(es.rp, "scene_frames", lambda sc_, traj, test_only: iter(frames))
        monkeypatch.setattr(es.rp, "layers_table", lambda cfg, sc_, path: table)
        monkeypatch.setattr(es.rp, "output_dirname", lambda *a: out_root)
        monkeypatch.setattr(es.rp, "write_layers_frame", write_frame)
        monkeypatch.setattr(es.inf, "render_rays_sharded", sharded)
        monkeypatch.setattr(es.inf, "distance_to_depth", lambda K, d: d)
        out = es.edit_scene_checkpoint(config, the_edit, "copy_1", **kw)
        files = sorted(str(p.relative_to(out)) for p in out.rglob("*") if p.is_file()) if out.exists() else []
        return calls, written, files

    per_frame = ["render_rays_edit", "render_rays_edit_layers", "render_rays_layers"]
    calls0, written0, files0 = run(0, save_layers=True, cached_centroids_path="c.pkl")
    calls1, written1, files1 = run(1, save_layers=True, cached_centroids_path="c.pkl")
    assert calls0 == per_frame * 2 and calls1 == calls0
    assert written0 == [("f0", (H * W, table.K + 2, 4), table.K + 1), ("f1", (H * W, table.K + 2, 4), table.K + 1)]
    assert "layers/f0_change.json" in files0 and "layers/f1_change.json" in files0 and "rgb/f0.png" in files0
    assert written1 == [] and files1 == []
    plain0, _, plain_files = run(0)
    plain1, _, _ = run(1)
    assert plain0 == ["render_rays_edit"] * 2 and plain1 == plain0 and not any(f.startswith("layers") for f in plain_files)
