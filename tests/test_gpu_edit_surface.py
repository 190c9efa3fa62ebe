"""Surface outputs of an edited scene on the GPU (csrc/edit.hip): the gradient of the edited density against the fp64 reference
of tests/edit_surface_cases.py and its bit promises, then the route from the march to the command line on the G27 blob scene of
tests/test_gpu_surface.py.

What the scene allows (figures from the CPU oracle, see edit_surface_cases): the field has a floor softplus(-3) everywhere and the blob fills
the middle of a box only 1.1 to 1.7 wide, so a moved copy of the blob that stays inside the box stands less than a blob's width from where
it stood.  Rays aimed at the old position therefore still cross the moved blob (498 of the 512 gather an opacity above 0.97): "they all miss"
cannot be asked of this scene.  What is asked in its place is exact: no hit point lies in the region the move emptied, where every sample
has the weight 0.  Deleting the blob out to 0.8 normalised units leaves no ray with half its transmittance lost: nothing hits."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import edit_surface_cases as esc
import surface_cases as sc
from conftest import REPO, T, load_golden, rel_close
from oracle import params as op
from test_gpu_surface import blob_rays, build_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
RES = (9, 13, 17)
N_POINTS = 4097


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def g27():
    """The G27 scene as tests/test_gpu_surface.py builds it: the blob field as a model, the renderer at step ratio 0.25 (S = 75)."""
    import contrastive_lift_amd as cl
    g = load_golden("g27_dense_volume")
    res = tuple(int(x) for x in g["res"])
    assert res == RES
    aabb, shift, C_, E = T(g["aabb"]).float(), float(g["shift"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.25).to(DEV)
    assert r.n_samples == 75
    lo, hi = (np.asarray(x, np.float64) for x in r.bbox_aabb_host)
    return dict(aabb=aabb, shift=shift, C=C_, E=E, P=P, model=build_model(P, res, C_, E, shift), renderer=r, lo=lo, hi=hi)


def normalised_on_device(renderer, model, world):
    """xn = (p - lo) * inv2 - 1 in fp32 on the device, each op rounded on its own, with the very floats the kernels are given."""
    from contrastive_lift_amd import engine
    ms = engine.march_struct(renderer, model)
    lo = torch.tensor(list(ms.lo), dtype=torch.float32, device=DEV)
    inv2 = torch.tensor(list(ms.inv_ext2), dtype=torch.float32, device=DEV)
    return ((world - lo) * inv2) - 1.0


# ============================================================================ 1. the gradient of the edited density at points
@pytest.fixture(scope="module")
def kernel_cases(g27):
    """comps -> (model, points (4097, 3) fp32, {program name: (program, fp64 reference, rows left out)}): computed once, left unchanged.  The
    random field of make_params (every channel carries weight); a smaller n takes the first points."""
    progs = esc.programs(g27["lo"], g27["hi"])
    pts = esc.world_points(N_POINTS, g27["lo"], g27["hi"], esc.POINT_SEED)
    out = {}
    for comps in (16, 48):
        P = op.make_params(200 + comps, RES, g27["C"], g27["E"], n_dens=(comps,) * 3)
        refs = {}
        for name, prog in progs.items():
            ref = esc.reference(P, prog, pts, g27["lo"], g27["hi"], g27["shift"])
            refs[name] = (prog, ref, esc.left_out(ref, prog, pts, RES))
        out[comps] = (build_model(P, RES, g27["C"], g27["E"], g27["shift"], comps), pts, refs)
    return out


@pytest.mark.parametrize("ldp", [3, 4])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, N_POINTS])
@pytest.mark.parametrize("comps", [16, 48])
def test_edited_gradient_against_the_fp64_reference(g27, kernel_cases, comps, n, ldp):
    """Every program of edit_surface_cases.programs.  Per component |error| <= 1e-3 (|J|^T |g'_ref|) + the floor of conftest.rel_close
    (1e-5 of the largest reference entry); the rows left out (texel lines, box faces) are at most 1 % of each case; the bit promises (a)
    and (b), the state byte, the zeros of the killed rows and a second run are exact."""
    from contrastive_lift_amd import edit, engine
    m, pts, refs = kernel_cases[comps]
    r = g27["renderer"]
    x = torch.zeros((n, ldp), dtype=torch.float32)
    x[:, :3] = T(pts[:n])
    if ldp == 4:
        x[:, 3] = 7.5                                      # the pitch is honoured: column 3 is never read
    x = x.to(DEV)
    world = x[:, :3].contiguous()
    for name, (prog, ref, out_rows) in refs.items():
        what = f"{name} comps {comps} n {n} ldp {ldp}"
        keep = ~out_rows[:n]
        left = int((~keep).sum())
        assert left <= 0.01 * n, what
        got, state = engine.edit_density_grad_points(m, r, x, prog, want_state=True)
        assert got.shape == (n, 4) and got.dtype == torch.float32 and state.shape == (n,) and state.dtype == torch.uint8
        src, _, state_pts = prog.apply_to_points(world)
        assert torch.equal(state.to(torch.int32), state_pts.to(torch.int32)), what             # the byte of clift_edit_list_points
        st = state.cpu().numpy()
        assert np.array_equal(st[keep], ref["state"][:n][keep]), what                          # ... and, off the faces, of the fp64 walk
        killed = torch.from_numpy((st & edit.STATE_KILLED) != 0).to(DEV)
        hops = torch.from_numpy((st & edit.STATE_REMAPS).astype(np.int64)).to(DEV)
        live = ~killed
        assert bool((got[killed] == 0).all()), what                                            # killed rows: exact zeros
        # the tolerance
        g, bound, raw = ref["g"][:n], ref["bound"][:n], ref["raw"][:n]
        err = np.abs(got.cpu().numpy().astype(np.float64)[:, :3] - g)
        allowed = 1e-3 * bound + 1e-3 * 1e-2 * (np.abs(g).max() if n else 0.0)
        worst = float((err - allowed)[keep].max()) if keep.any() else 0.0
        if n == N_POINTS and ldp == 3:
            print(f"{what}: {left} rows left out, {int(killed.sum())} killed, hops {np.bincount(hops[live].cpu().numpy(), minlength=1).tolist()}; "
                  f"largest error {err[keep].max():.3g} of gradients up to {np.abs(g).max():.3g}")
        assert worst <= 0.0, f"{what}: a component {worst:.3g} outside its bound"
        kp = torch.from_numpy(keep)
        rel_close(got.cpu()[kp][:, 3], raw[keep], what=f"{what}: sigma_raw")
        # (a) column 3 of a live row: the bits of clift_density_points(activation = 0) where it is looked up
        xn = normalised_on_device(r, m, src)
        value = engine.density_points(m, xn, activation=False)
        assert torch.equal(got[live][:, 3], value[live]), what
        # (b) a live row that no edit remapped: all four columns of clift_density_grad_points
        plain = engine.density_grad_points(m, xn, world=True, renderer=r)
        still = live & (hops == 0)
        assert torch.equal(got[still], plain[still]), what
        assert torch.equal(engine.edit_density_grad_points(m, r, x, prog), got), what          # two runs: the same bits
        if n == N_POINTS:                                  # what the case is there for really occurs in the sample
            counts = np.bincount(hops[live].cpu().numpy(), minlength=4)
            if name == "full8":
                assert counts[:4].min() >= 8 and int(killed.sum()) > 100
            elif name == "kill_all":
                assert bool(killed.all()) and bool((hops > 0).any())
            elif name in ("delete", "extract"):
                assert int(killed.sum()) > 100 and counts[0] > 100
            else:
                assert counts[0] > 100 and counts[1] > 30
            if name == "copy":
                assert int(((xn.abs() > 1.0).any(1) & (hops > 0)).sum()) > 0                   # a remapped point that reads padding


def test_edited_gradient_errors_and_empty_input(g27):
    from contrastive_lift_amd import _lib, engine
    m, r = g27["model"], g27["renderer"]
    prog = esc.programs(g27["lo"], g27["hi"])["mixed3"]
    assert engine.edit_density_grad_points(m, r, torch.empty((0, 3), device=DEV), prog).shape == (0, 4)
    views = m.named_views()
    vd = engine.vm_struct(views, "density", engine.grid_res(views))
    ms = engine.march_struct(r, m)
    x, out = torch.zeros((4, 3), device=DEV), torch.full((4, 4), -7.5, device=DEV)
    nine = (_lib.EditRec * 9)(*(prog[i % 3].record() for i in range(9)))
    name = "clift_edit_list_density_grad_points"
    call = lambda recs, n, vd=vd, ldp=3, out=out: _lib.call(name, recs, n, C.byref(vd), _lib.ptr(x), ldp, 4, ms.lo, ms.inv_ext2, 0.0,
                                                            _lib.ptr(out) if out is not None else None, None, _lib.stream())
    for n in (0, 9):
        with pytest.raises(_lib.CliftError, match=f"{name}: .*n_edits = {n}"):
            call(nine, n)
    with pytest.raises(_lib.CliftError, match=f"{name}: ldp"):
        call(prog.records(), 3, ldp=2)
    bad = engine.vm_struct(views, "density", engine.grid_res(views))
    bad.comps = 6
    with pytest.raises(_lib.CliftError, match=f"{name}: comps"):
        call(prog.records(), 3, vd=bad)
    with pytest.raises(_lib.CliftError, match=f"{name}: NULL"):
        call(prog.records(), 3, out=None)
    act = torch.zeros((4,), dtype=torch.int32, device=DEV)
    rays = blob_rays()[:4].to(DEV)
    name_a = "clift_edit_list_density_grad_active"
    for n in (0, 9):
        with pytest.raises(_lib.CliftError, match=f"{name_a}: .*n_edits = {n}"):
            _lib.call(name_a, C.byref(ms), nine, n, C.byref(vd), _lib.ptr(rays), _lib.ptr(act), 4, _lib.ptr(out), _lib.stream())
    with pytest.raises(_lib.CliftError, match=f"{name_a}: comps"):
        _lib.call(name_a, C.byref(ms), prog.records(), 3, C.byref(bad), _lib.ptr(rays), _lib.ptr(act), 4, _lib.ptr(out), _lib.stream())
    with pytest.raises(_lib.CliftError, match=f"{name_a}: NULL"):
        _lib.call(name_a, C.byref(ms), prog.records(), 3, C.byref(vd), _lib.ptr(rays), _lib.ptr(act), 4, None, _lib.stream())
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())                       # nothing was launched


# ============================================================================ 2. end to end on the G27 blob scene
def world_samples(renderer, rays, act_idx, S):
    """The fp32 world points of the listed samples, o + d z with the march's own z (surface_cases.sample_z) and separately rounded ops:
    the bits the kernels form."""
    lo, hi = renderer.bbox_aabb_host
    rays = rays.cpu().numpy()
    z = sc.sample_z(rays, lo, hi, renderer.step_size_host, S, None)
    sid = act_idx.cpu().numpy().astype(np.int64)
    r, k = sid // S, sid % S
    zz = z[r, k]
    return torch.from_numpy((rays[r, 0:3] + (rays[r, 3:6] * zz[:, None]).astype(np.float32)).astype(np.float32)).to(DEV)


@pytest.fixture(scope="module")
def scene(g27):
    """The 512 + 64 rays of blob_rays(), the 512 turned and shifted by the move, and the passes the tests share (run once)."""
    from contrastive_lift_amd import edit, engine
    m, r = g27["model"], g27["renderer"]
    old = blob_rays()
    new = torch.from_numpy(esc.moved_rays(old[:512].numpy()))
    both = torch.cat([old, new], 0).to(DEV)
    box = esc.blob_box()
    move = edit.move(box, esc.MOVE_T, esc.MOVE_R)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * esc.BLOB_HALF
    corners = corners @ move.dst.axes + move.dst.centre
    assert (corners >= g27["lo"]).all() and (corners <= g27["hi"]).all()                  # the destination lies inside the aabb
    o, ctx = engine.edit_forward(m, r, both, move, False)
    before = {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}
    s = engine.edit_surface_from_ctx(m, r, ctx)
    torch.cuda.synchronize()
    return dict(old=old, new=new, both=both, dr=old.to(DEV), box=box, move=move, o=o, before=before, ctx=ctx, s=s)


KEYS = ("depth_median", "hit", "k_median", "normals", "points")


def test_deleting_an_empty_box_gives_the_bits_of_the_unedited_pass(g27, scene):
    from contrastive_lift_amd import edit, engine
    m, r = g27["model"], g27["renderer"]
    box = esc.empty_box()
    assert (box.centre - esc.EMPTY_HALF >= g27["lo"]).all() and (box.centre + esc.EMPTY_HALF <= g27["hi"]).all()
    p, _ = esc.sample_points(scene["old"].numpy(), *r.bbox_aabb_host, r.step_size_host, int(r.n_samples))
    grown = edit.EditBox(np.eye(3), box.centre, -esc.EMPTY_HALF - 1e-3, esc.EMPTY_HALF + 1e-3)
    assert not grown.contains(p.reshape(-1, 3)).any()                                    # no sample lies in the box
    plain, pctx = engine.surface_forward(m, r, scene["dr"], None)
    for e in (edit.delete(box), edit.EditProgram([edit.delete(box)])):
        got, ctx = engine.edit_surface_forward(m, r, scene["dr"], e, weight_thres=r.raymarch_weight_thres)
        assert ctx.M == pctx.M and ctx.xa is None and ctx.rgb_s is None                  # no head ran, no xa was made
        for k in KEYS + ("depth", "opacity"):
            assert torch.equal(got[k], plain[k]), k
    assert bool(plain["hit"][:512].all())


def test_moved_blob_equals_the_restatement_on_its_own_arrays(g27, scene):
    from contrastive_lift_amd import _lib, engine
    m, r, ctx, s = g27["model"], g27["renderer"], scene["ctx"], scene["s"]
    assert ctx.N == 1088 and ctx.S == 75 and ctx.M > 4000 and ctx.edited and len(ctx.edit_program) == 1
    s2, ctx2 = engine.edit_surface_forward(m, r, scene["both"], scene["move"])
    assert ctx2.rgb_s is None and ctx2.sem_s is None and ctx2.xa is None                 # geometry only
    for k in KEYS:
        assert torch.equal(s2[k], s[k]), k
    assert torch.equal(s2["depth"], scene["o"]["depth"]) and torch.equal(s2["opacity"], scene["o"]["opacity"])
    s3 = r.forward_edit_surface(m, scene["both"], scene["move"])
    assert all(torch.equal(s3[k], s2[k]) for k in s2)
    for k, v in scene["before"].items():                                                 # edit_forward's outputs are untouched
        assert torch.equal(scene["o"][k], v), k
    # the restatement, with G from the device's own point kernel at the samples' world points
    lo, hi = r.bbox_aabb_host
    rays = scene["both"].cpu().numpy()
    z, delta = sc.deltas(sc.sample_z(rays, lo, hi, r.step_size_host, ctx.S, None))
    world = world_samples(r, scene["both"], ctx.act_idx[:ctx.M], ctx.S)
    G = engine.edit_density_grad_points(m, r, world, scene["move"])
    ref = sc.ray_surface_reference(ctx.T.cpu().numpy(), ctx.w.cpu().numpy(), z, delta, ctx.ray_start.cpu().numpy(),
                                   ctx.act_idx.cpu().numpy()[:ctx.M], G.cpu().numpy(), 0.5)
    sc.check_ray_surface(ref, z, delta, s["depth_median"].cpu().numpy(), s["k_median"].cpu().numpy(), what="moved blob")
    rel_close(s["normals"].cpu(), ref["normal"], what="moved blob: normal sums")
    hit = s["hit"].cpu().numpy()
    assert s["hit"].dtype == torch.bool and np.array_equal(hit, ref["k_med"] >= 0)
    # (c) the active form and the points form: equal bits for the same world point
    views = m.named_views()
    vd = engine.vm_struct(views, "density", ctx.res)
    Ga = torch.empty((ctx.M, 4), dtype=torch.float32, device=DEV)
    prog = ctx.edit_program
    _lib.call("clift_edit_list_density_grad_active", C.byref(ctx.ms), prog.records(), len(prog), C.byref(vd), _lib.ptr(ctx.rays),
              _lib.ptr(ctx.act_idx), ctx.M, _lib.ptr(Ga), _lib.stream())
    assert torch.equal(Ga, G)
    remapped = scene["move"].dst.contains(world.cpu().numpy().astype(np.float64))
    assert remapped.sum() > 1000 and (~remapped).sum() > 1000                            # both kinds of rows among the active samples


def test_moved_blob_is_seen_where_it_stands_now(g27, scene):
    """Rays 576 .. 1087 are the 512 blob rays turned and shifted by the move: they all hit, their normals face them and are no longer than
    the opacity.  Of the rays aimed at the old position no hit point lies in the region the move emptied (in the source box, outside the
    destination box): every sample there has the weight 0, so the transmittance cannot cross 1 - q inside it.  The 64 rays that leave the
    box see nothing, before and after."""
    s, rays = scene["s"], scene["both"].cpu()
    hit = s["hit"].cpu().numpy()
    assert hit[576:].all()
    n, d = s["normals"].cpu().double()[576:], rays[576:, 3:6].double()
    assert bool(((n * d).sum(1) < 0).all())
    assert bool((n.norm(dim=1) <= scene["o"]["opacity"].cpu().double()[576:] * (1 + 1e-5)).all())
    miss = ~s["hit"]
    assert bool((s["depth_median"][miss] == 0).all()) and bool((s["k_median"][miss] == -1).all())
    assert not hit[512:576].any() and bool((s["normals"][512:576] == 0).all())
    pts = s["points"].cpu().double().numpy()[:512][hit[:512]]
    move = scene["move"]
    shrunk = lambda b, by: ((b.lo + by <= b.local(pts)) & (b.local(pts) <= b.hi - by)).all(1)
    step = float(g27["renderer"].step_size_host)
    emptied = shrunk(move.src, step) & ~shrunk(move.dst, -step)                           # surely killed, a sample's length from every face
    print(f"rays at the old position: {int(hit[:512].sum())} of 512 hit; {int(shrunk(move.dst, 0.0).sum())} of the hit points lie in the moved box")
    assert not emptied.any()


def test_copy_shows_both_and_delete_shows_neither(g27, scene):
    from contrastive_lift_amd import edit, engine
    m, r = g27["model"], g27["renderer"]
    s, _ = engine.edit_surface_forward(m, r, scene["both"], edit.copy(scene["box"], esc.MOVE_T, esc.MOVE_R))
    hit = s["hit"].cpu().numpy()
    assert hit[:512].all() and hit[576:].all() and not hit[512:576].any()
    s, ctx = engine.edit_surface_forward(m, r, scene["dr"], edit.delete(esc.blob_box(esc.DELETE_HALF)))
    assert ctx.M > 1000                                                                  # the floor and the tail are still marched
    assert not bool(s["hit"].any()) and bool((s["depth_median"] == 0).all()) and bool((s["k_median"] == -1).all())
    print(f"after the delete: opacity up to {float(s['opacity'].max()):.3f}")
    assert float(s["opacity"].max()) < 0.5


def test_wrappers_and_refusals(g27, scene):
    import functools
    from contrastive_lift_amd import _lib, engine
    from contrastive_lift_amd import inference as inf
    m, r, dr, move = g27["model"], g27["renderer"], scene["dr"], scene["move"]
    whole = inf.render_rays_edit_surface(m, r, dr, 0, edit=move)
    parts = inf.render_rays_edit_surface(m, r, dr, 100, edit=move)
    plain = inf.render_rays_edit(m, r, dr, 100, edit=move)
    assert len(whole) == 7 and [tuple(x.shape) for x in whole] == [(576, 3), (576, g27["C"]), (576, 2 * g27["E"]), (576,), (576,), (576,), (576, 3)]
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    for a, b in zip(parts[:4], plain):                                                   # the first four are render_rays_edit's own
        assert torch.equal(a, b)
    assert whole[5].dtype == torch.float32 and torch.equal(whole[5] > 0.5, scene["s"]["hit"][:576])
    assert torch.equal(whole[4], scene["s"]["depth_median"][:576]) and torch.equal(whole[6], scene["s"]["normals"][:576])
    fn = functools.partial(inf.render_rays_edit_surface, edit=move, weight_thres=0.0, q=0.5)
    sharded = inf.render_rays_sharded(m, r, dr, 100, render_fn=fn)                       # no process group: the function itself
    assert all(torch.equal(a, b) for a, b in zip(sharded, whole))
    with pytest.raises(ValueError, match="edit is required"):
        inf.render_rays_edit_surface(m, r, dr, 0)
    _, pctx = engine.render_forward(m, r, dr, None, False, grad_heads=())
    with pytest.raises(_lib.CliftError, match="surface_from_ctx"):
        engine.edit_surface_from_ctx(m, r, pctx)
    with pytest.raises(_lib.CliftError, match="edit_forward"):
        engine.edit_surface_from_ctx(m, r, None)
    with pytest.raises(_lib.CliftError, match="edit_forward"):                            # surface_from_ctx still refuses the edited context
        engine.surface_from_ctx(m, r, scene["ctx"])
    with pytest.raises(_lib.CliftError, match=r"\(0, 1\)"):
        engine.edit_surface_from_ctx(m, r, scene["ctx"], q=1.0)
    again = engine.edit_surface_from_ctx(m, r, scene["ctx"])                             # the context was only read
    assert all(torch.equal(again[k], scene["s"][k]) for k in KEYS)
    s9 = engine.edit_surface_from_ctx(m, r, scene["ctx"], q=0.9)                         # a later quantile lies deeper
    both_hit = scene["s"]["hit"] & s9["hit"]
    assert bool((s9["depth_median"][both_hit] >= scene["s"]["depth_median"][both_hit]).all())


def test_edit_scene_save_surface(tmp_path, monkeypatch):
    """The few-step synthetic PanopLi checkpoint of tests/test_gpu_surface.py's command-line test (a blob written into its density tables so
    that rays hit something), with a box around the blob moved: --save_surface writes surface/<frame>.npz and vis_normals/<frame>.png per
    frame with render_panopli.py's keys and encodings; a run without the flag writes neither, and its other files are the same bytes."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd.config import load_run_config
    from PIL import Image
    size = 24
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_panopli"), n_frames=12, size=size)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "edit_surface_flags")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_edit_surface")
    run_dir = train.main(["+experiment=contrastive_lift", f"dataset_root={scene_dir}", f"image_dim={size}", "min_grid_dim=16", "max_grid_dim=16",
                          "max_epoch=1", "steps_per_epoch=4", "batch_size=256", "chunk=0", "max_depth=3", "seed=3", "max_rays_instances=64",
                          "late_semantic_optimization=0", "instance_optimization_epoch=1", "segment_optimization_epoch=3"])
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = ck["state_dict"]
    res = [int(x) for x in sd["renderer.grid_dim"].tolist()]
    op.add_blob({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.density_")}, res, amplitude=3.0, sigma_g=0.5)
    torch.save(ck, ckpt)
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.image_dim, cfg.chunk = ckpt, [size, size], 300
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_scene_surface_gpu")
    scene, model, renderer = es.rp.load_for_inference(cfg, torch.device("cuda:0"))
    lo, hi = (np.asarray(x, np.float64) for x in renderer.bbox_aabb_host)
    boxes = {5: {"bbox": (-0.3 * (hi - lo), 0.3 * (hi - lo)), "orientation": np.eye(3), "position": (lo + hi) / 2}}
    the_edit = es.resolve_edit(boxes, 5, "move", translate=[0.15 * (hi - lo)[0], 0.0, 0.0], rotate_deg=[0.0, 0.0, 30.0])
    off = es.edit_scene_checkpoint(cfg, the_edit, "move_5_plain")
    on = es.edit_scene_checkpoint(cfg, the_edit, "move_5_surface", save_surface=True, surface_quantile=0.5)
    assert not (off / "surface").exists() and not (off / "vis_normals").exists()
    frames = list(es.rp.scene_frames(scene, "trajectory_blender", True))
    H, W = scene.image_dim
    assert len(frames) >= 1 and sorted(os.listdir(on / "surface")) == sorted(f"{name}.npz" for name, _, _ in frames)
    n_hit = 0
    for name, rays, K in frames:
        for sub, ext in (("rgb", "png"), ("pred_semantics", "png"), ("depth", "npy")):
            assert open(on / sub / f"{name}.{ext}", "rb").read() == open(off / sub / f"{name}.{ext}", "rb").read(), (sub, name)
        o = inf.render_rays_edit_surface(model, renderer, rays, 300, scene.white_bg, edit=the_edit)
        z = np.load(on / "surface" / f"{name}.npz")
        assert sorted(z.files) == ["depth_median", "hit", "normals"]
        hit = (o[5] > 0.5).reshape(H, W).cpu().numpy()
        assert z["hit"].dtype == np.bool_ and np.array_equal(z["hit"], hit)
        assert z["normals"].dtype == np.float32 and np.array_equal(z["normals"], o[6].reshape(H, W, 3).cpu().numpy())
        assert z["depth_median"].dtype == np.float32
        assert np.array_equal(z["depth_median"], inf.distance_to_depth(K, o[4].view(H, W)).reshape(H, W).cpu().numpy())
        vis = np.asarray(Image.open(on / "vis_normals" / f"{name}.png"))
        assert vis.shape == (H, W, 3) and (vis[~hit] == 0).all() and (vis[hit].max(-1) > 0).all()
        n_hit += int(hit.sum())
    print(f"{n_hit} of {len(frames) * H * W} pixels hit")
    assert 0 < n_hit < len(frames) * H * W
