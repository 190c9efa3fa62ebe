"""Surface outputs of the ray route on the GPU (csrc/surface.hip): the point gradient against the fp64 autograd reference, the
ray kernel on made-up marches against the literal numpy restatement (tests/surface_cases.py), both end to end on the G27 blob scene
against that restatement on the context's own arrays and against the CPU oracle's weights, the refusals, the chunked wrapper and
inference/render_panopli.py's two new flags."""
import ctypes as C
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import surface_cases as sc
from conftest import REPO, T, load_golden, rel_close
from oracle import params as op
from oracle import render as orender

pytestmark = pytest.mark.gpu

DEV = "cuda"
RES = (9, 13, 17)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(P, res, C_, E, shift, n_dens=16):
    import contrastive_lift_amd as cl
    m = cl.TensorVMSplit(list(res), num_density_comps=(n_dens,) * 3, num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32),
                         num_semantic_classes=C_, dim_feature_instance=2 * E, splus_density_shift=shift, use_semantic_mlp=True,
                         use_instance_mlp=True, slow_fast_mode=True, device=DEV)
    missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    assert not missing and not unexpected
    return m


@pytest.fixture(scope="module")
def g27():
    """The G27 scene (tests/test_gpu_mesh.py): its box and shift; the blob field as a model, the renderer at step ratio 0.25 (S = 75)."""
    import contrastive_lift_amd as cl
    g = load_golden("g27_dense_volume")
    res = tuple(int(x) for x in g["res"])
    assert res == RES
    aabb, shift, C_, E = T(g["aabb"]).float(), float(g["shift"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.25).to(DEV)
    assert r.n_samples == 75
    return dict(aabb=aabb, shift=shift, C=C_, E=E, P=P, model=build_model(P, res, C_, E, shift), renderer=r,
                cfg=orender.RenderCfg(aabb, res, step_ratio=0.25, density_shift=shift, semantic_weight_mode="softmax"))


# ============================================================================ 1. point gradient
N_POINTS = 4097


@pytest.fixture(scope="module")
def grad_cases(g27):
    """comps -> (model, points (4097, 3) fp32, fp64 reference gradient and value, keep): computed once, left unchanged.  The random field of
    make_params (no blob: every channel carries weight); n = 1 and 3 take the first points."""
    out = {}
    for comps in (16, 48):
        P = op.make_params(200 + comps, RES, g27["C"], g27["E"], n_dens=(comps,) * 3)
        pts = np.random.default_rng(comps).uniform(-1.2, 1.2, (N_POINTS, 3)).astype(np.float32)
        g, raw = sc.grad_reference(P, pts, g27["shift"])
        out[comps] = (build_model(P, RES, g27["C"], g27["E"], g27["shift"], comps), pts, g, raw, ~sc.near_texel_line(pts, RES))
    return out


@pytest.mark.parametrize("ldx", [3, 4])
@pytest.mark.parametrize("n", [1, 3, N_POINTS])
@pytest.mark.parametrize("comps", [16, 48])
def test_point_gradient_against_fp64_autograd(g27, grad_cases, comps, n, ldx):
    from contrastive_lift_amd import engine
    m, pts, g, raw, keep = grad_cases[comps]
    pts, g, raw, keep = pts[:n], g[:n], raw[:n], keep[:n]
    left = int((~keep).sum())
    print(f"comps {comps} n {n} ldx {ldx}: {left} of {n} points within 1e-4 of a texel line left out; gradients up to {np.abs(g).max():.3g}")
    assert left <= 0.005 * n
    x = torch.zeros((n, ldx), dtype=torch.float32)
    x[:, :3] = T(pts)
    if ldx == 4:
        x[:, 3] = 7.5                                      # the pitch is honoured: column 3 is never read
    x = x.to(DEV)
    out_n = engine.density_grad_points(m, x, world=False)
    out_w = engine.density_grad_points(m, x, world=True, renderer=g27["renderer"])
    assert out_n.shape == out_w.shape == (n, 4) and out_n.dtype == torch.float32
    kp = torch.from_numpy(keep)
    scale = (2.0 / (g27["aabb"][1] - g27["aabb"][0]).double()).numpy()
    rel_close(out_n.cpu()[kp][:, :3], g[keep], what="d sigma_raw / d xn")
    rel_close(out_w.cpu()[kp][:, :3], g[keep] * scale[None], what="world gradient")
    rel_close(out_n.cpu()[:, 3], raw, what="sigma_raw")
    value = engine.density_points(m, x, activation=False)
    assert torch.equal(out_n[:, 3], value) and torch.equal(out_w[:, 3], value)         # the bits of clift_density_points(activation = 0)
    f = sc.texel_coordinates(pts, RES)
    far = ((f < -1.0 - 1e-4) | (f > np.asarray(RES) + 1e-4)).any(1)                   # farther than one texel outside on some axis
    if n == N_POINTS:
        assert far.sum() > 100
    fr = torch.from_numpy(far)
    assert bool((out_n.cpu()[fr][:, :3] == 0).all()) and bool((out_w.cpu()[fr][:, :3] == 0).all())
    assert bool((out_n.cpu()[fr][:, 3] == g27["shift"]).all())
    assert torch.equal(engine.density_grad_points(m, x, world=False), out_n)          # two runs: the same bits


def test_point_gradient_errors_and_empty_input(g27):
    from contrastive_lift_amd import _lib, engine
    m = g27["model"]
    assert engine.density_grad_points(m, torch.empty((0, 3), device=DEV), world=False).shape == (0, 4)
    with pytest.raises(_lib.CliftError, match="renderer"):
        engine.density_grad_points(m, torch.zeros((2, 3), device=DEV))
    views = m.named_views()
    vd = engine.vm_struct(views, "density", engine.grid_res(views))
    x, out = torch.zeros((4, 3), device=DEV), torch.full((4, 4), -7.5, device=DEV)
    with pytest.raises(_lib.CliftError, match="ldx"):
        _lib.call("clift_density_grad_points", C.byref(vd), _lib.ptr(x), 2, 4, 0.0, None, _lib.ptr(out), _lib.stream())
    with pytest.raises(_lib.CliftError, match="NULL"):
        _lib.call("clift_density_grad_points", C.byref(vd), _lib.ptr(x), 3, 4, 0.0, None, None, _lib.stream())
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())


# ============================================================================ 2. the ray kernel on made-up marches
N_RAYS = 130


def made_up_rays(seed):
    """130 rays from a sphere of radius 0.95 towards the unit cube's middle, with jitter; the box is the unit cube, the step 0.03."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((N_RAYS, 3))
    o = 0.95 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.3, 0.3, (N_RAYS, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((N_RAYS, 1), 0.01), np.full((N_RAYS, 1), 4.0)], 1).astype(np.float32)
    return rays, rng.random(N_RAYS).astype(np.float32)


def march_record(S, step=0.03):
    from contrastive_lift_amd import _lib
    ms = _lib.March()
    for i in range(3):
        ms.lo[i], ms.hi[i], ms.inv_ext2[i] = -1.0, 1.0, 1.0
    ms.step_size, ms.n_samples, ms.distance_scale, ms.density_shift, ms.weight_thres = step, S, 25.0, -3.0, 1e-4
    return ms


def run_ray_surface(ms, rays, jitter, m, q):
    from contrastive_lift_amd import _lib
    N = rays.shape[0]
    d = {k: T(m[k]).to(DEV) for k in ("T", "w", "ray_start", "act_idx", "G")}
    M = int(m["act_idx"].shape[0])
    depth = torch.full((N,), -7.5, device=DEV)
    k_med = torch.full((N,), -77, dtype=torch.int32, device=DEV)
    nrm = torch.full((N, 4), -7.5, device=DEV)
    _lib.call("clift_ray_surface", C.byref(ms), _lib.ptr(rays), _lib.ptr(jitter), N, _lib.ptr(d["T"]), _lib.ptr(d["w"]), _lib.ptr(d["ray_start"]),
              _lib.ptr(d["act_idx"]) if M else None, M, _lib.ptr(d["G"]) if M else None, q, _lib.ptr(depth), _lib.ptr(k_med), _lib.ptr(nrm),
              _lib.stream())
    torch.cuda.synchronize()
    return depth, k_med, nrm


@pytest.mark.parametrize("q", [0.5, 0.9])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_ray_kernel_on_made_up_marches(S, q):
    ms = march_record(S)
    rays, jitter = made_up_rays(S)
    m = sc.made_up_march(N_RAYS, S, q, seed=S)
    z, delta = sc.deltas(sc.sample_z(rays, [-1.0] * 3, [1.0] * 3, 0.03, S, jitter))
    ref = sc.ray_surface_reference(m["T"], m["w"], z, delta, m["ray_start"], m["act_idx"], m["G"], q)
    depth, k_med, nrm = run_ray_surface(ms, T(rays).to(DEV), T(jitter).to(DEV), m, q)
    flat = sc.check_ray_surface(ref, z, delta, depth.cpu().numpy(), k_med.cpu().numpy(), what=f"S {S} q {q}")
    assert flat == 0                                                                  # the generator keeps den >= 2^-12
    for name, r in m["forced"].items():
        print(f"  {name}: ray {r} k_median {int(k_med[r])} depth {float(depth[r]):.6f}")
    rel_close(nrm.cpu()[:, :3], ref["normal"], what=f"S {S} q {q}: normal sums")
    assert bool((nrm[:, 3] == 0).all())
    n_act = np.diff(m["ray_start"])
    assert bool((nrm.cpu()[torch.from_numpy(n_act == 0)] == 0).all())                 # rays without active samples: exact zeros
    opac = m["w"].astype(np.float64).sum(1)
    assert (np.linalg.norm(nrm.cpu().numpy()[:, :3].astype(np.float64), axis=1) <= opac * (1 + 1e-5) + 1e-7).all()
    depth2, k2, nrm2 = run_ray_surface(ms, T(rays).to(DEV), T(jitter).to(DEV), m, q)
    assert torch.equal(depth2, depth) and torch.equal(k2, k_med) and torch.equal(nrm2, nrm)
    # without jitter (NULL), and with no active sample at all (M = 0, act_idx and G NULL)
    z0, delta0 = sc.deltas(sc.sample_z(rays, [-1.0] * 3, [1.0] * 3, 0.03, S, None))
    empty = dict(m, ray_start=np.zeros(N_RAYS + 1, np.int32), act_idx=np.zeros(0, np.int32), G=np.zeros((0, 4), np.float32))
    ref0 = sc.ray_surface_reference(m["T"], m["w"], z0, delta0, empty["ray_start"], empty["act_idx"], None, q)
    depth0, k0, nrm0 = run_ray_surface(ms, T(rays).to(DEV), None, empty, q)
    sc.check_ray_surface(ref0, z0, delta0, depth0.cpu().numpy(), k0.cpu().numpy(), what=f"S {S} q {q}, no jitter, M = 0")
    assert bool((nrm0 == 0).all())


def test_ray_kernel_errors():
    from contrastive_lift_amd import _lib
    ms = march_record(8)
    rays, _ = made_up_rays(0)
    m = sc.made_up_march(N_RAYS, 8, 0.5, seed=0)
    for q, msg in ((0.0, r"\(0, 1\)"), (1.0, r"\(0, 1\)"), (float("nan"), r"\(0, 1\)")):
        with pytest.raises(_lib.CliftError, match=msg):
            run_ray_surface(ms, T(rays).to(DEV), None, m, q)
    with pytest.raises(_lib.CliftError, match="no samples"):
        run_ray_surface(march_record(0), T(rays).to(DEV), None, m, 0.5)


# ============================================================================ 3. end to end on the G27 blob scene
def blob_rays():
    """512 rays from a sphere of radius 0.9 aimed near the blob (the middle of the box), then 64 rays that start below the box and point
    away from it."""
    rng = np.random.default_rng(27)
    eyes = rng.standard_normal((512, 3))
    eyes = 0.9 * eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
    target = np.array([[-0.05, 0.0, 0.05]]) + rng.uniform(-0.08, 0.08, (512, 3))
    d = target - eyes
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_miss = np.array([[0.0, 0.0, -0.95]]) + rng.uniform(-0.02, 0.02, (64, 3))
    d_miss = rng.standard_normal((64, 3)) * 0.1 + np.array([1.0, 0.0, -0.3])
    d_miss /= np.linalg.norm(d_miss, axis=1, keepdims=True)
    o, d = np.concatenate([eyes, o_miss]), np.concatenate([d, d_miss])
    return torch.from_numpy(np.concatenate([o, d, np.full((576, 1), 0.01), np.full((576, 1), 4.0)], 1).astype(np.float32))


@pytest.fixture(scope="module")
def blob(g27):
    """The rays, the CPU oracle's march over them (computed once), the device pass and its surface outputs."""
    from contrastive_lift_amd import engine
    rays = blob_rays()
    with torch.no_grad():
        _, z, inbox, dists, _, sigma, alpha, w, _ = orender._density_weights(g27["P"], rays, g27["cfg"], None)
    Tr = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    dr = rays.to(DEV)
    o, ctx = engine.render_forward(g27["model"], g27["renderer"], dr, None, False, grad_heads=())
    before = {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}
    s = engine.surface_from_ctx(g27["model"], g27["renderer"], ctx)
    torch.cuda.synchronize()
    return dict(rays=rays, dr=dr, o=o, before=before, ctx=ctx, s=s, oracle=dict(z=z.numpy(), delta=dists.numpy(), w=w.numpy(), T=Tr.numpy(),
                                                                               inbox=inbox.numpy()))


def test_blob_scene_equals_the_restatement_on_its_own_arrays(g27, blob):
    from contrastive_lift_amd import engine
    ctx, s, rays = blob["ctx"], blob["s"], blob["rays"]
    r = g27["renderer"]
    assert ctx.S == 75 and ctx.N == 576 and ctx.M > 2000
    lo, hi = r.bbox_aabb_host
    z, delta = sc.deltas(sc.sample_z(rays.numpy(), lo, hi, r.step_size_host, ctx.S, None))
    G = engine.density_grad_points(g27["model"], ctx.xa, world=True, renderer=r)                      # the device's own G
    ref = sc.ray_surface_reference(ctx.T.cpu().numpy(), ctx.w.cpu().numpy(), z, delta, ctx.ray_start.cpu().numpy(),
                                   ctx.act_idx.cpu().numpy()[:ctx.M], G.cpu().numpy(), 0.5)
    flat = sc.check_ray_surface(ref, z, delta, s["depth_median"].cpu().numpy(), s["k_median"].cpu().numpy(), what="blob scene")
    assert flat == 0
    rel_close(s["normals"].cpu(), ref["normal"], what="blob scene: normal sums")
    hit = s["hit"].cpu().numpy()
    assert s["hit"].dtype == torch.bool and np.array_equal(hit, ref["k_med"] >= 0)
    assert hit[:512].all() and not hit[512:].any()
    assert bool((s["depth_median"][512:] == 0).all()) and bool((s["k_median"][512:] == -1).all()) and bool((s["normals"][512:] == 0).all())
    pts = rays[:, 0:3].double() + s["depth_median"].cpu().double()[:, None] * rays[:, 3:6].double()
    # o + z d in fp32: a product of magnitude < 2 (error <= 2^-24 * 2) and a sum of magnitude < 4 (error <= 2^-23): 2.4e-7
    assert float((s["points"].cpu().double() - pts).abs().max()) <= 2.5e-7
    # the normals point back along the rays (a convex blob seen from outside), and their length is at most the opacity
    n, d = s["normals"].cpu().double()[:512], rays[:512, 3:6].double()
    assert bool(((n * d).sum(1) < 0).all())
    assert bool((n.norm(dim=1) <= blob["o"]["opacity"].cpu().double()[:512] * (1 + 1e-5)).all())
    # render_forward's outputs on that context are untouched
    for k, v in blob["before"].items():
        assert torch.equal(blob["o"][k], v), k


def test_blob_scene_geometry_only_pass_gives_the_same_bits(g27, blob):
    from contrastive_lift_amd import engine
    s = blob["s"]
    s2, ctx2 = engine.surface_forward(g27["model"], g27["renderer"], blob["dr"], None)
    assert ctx2.rgb_s is None and ctx2.sem_s is None and ctx2.inst_s is None                          # no head ran
    for k in ("depth_median", "hit", "k_median", "normals", "points"):
        assert torch.equal(s2[k], s[k]), k
    assert torch.equal(s2["depth"], blob["o"]["depth"]) and torch.equal(s2["opacity"], blob["o"]["opacity"])
    s3 = g27["renderer"].forward_surface(g27["model"], blob["dr"])
    assert all(torch.equal(s3[k], s2[k]) for k in s2)
    fctx = engine.feature_forward(g27["model"], g27["renderer"], blob["dr"], None, "semantic", grad_heads=())[1]
    s4 = engine.surface_from_ctx(g27["model"], g27["renderer"], fctx)
    assert all(torch.equal(s4[k], s[k]) for k in s)
    s9 = engine.surface_from_ctx(g27["model"], g27["renderer"], blob["ctx"], q=0.9)                   # a later quantile lies deeper
    assert bool((s9["depth_median"][:512] >= s["depth_median"][:512]).all()) and bool((s9["depth_median"][:512] > s["depth_median"][:512]).any())


def test_blob_scene_against_the_cpu_oracle(g27, blob):
    """The oracle's own weights through the same restatement: all 512 inside rays are opaque and cross the median inside a sample whose
    weight is at least 0.024 (asserted), so the device's depth can only leave the oracle's by the two marches' round-off: within one
    step for at least 99 % of the hit rays.  The 64 outside rays have no sample in the box."""
    oc, s = blob["oracle"], blob["s"]
    none = np.zeros(577, np.int32), np.zeros(0, np.int32)
    ref = sc.ray_surface_reference(oc["T"], oc["w"], oc["z"], oc["delta"], none[0], none[1], None, 0.5)
    assert not oc["inbox"][512:].any() and (ref["k_med"][512:] == -1).all() and (ref["k_med"][:512] >= 0).all()
    opac = oc["w"].astype(np.float64).sum(1)[:512]
    cross = oc["w"][np.arange(512), ref["k_med"][:512]]
    print(f"oracle: opacity {opac.min():.6f} .. {opac.max():.6f}, smallest crossing weight {cross.min():.4f}")
    assert opac.min() > 0.9999 and cross.min() >= 0.024
    err = np.abs(s["depth_median"].cpu().numpy().astype(np.float64)[:512] - ref["z_med"][:512])
    step = float(g27["cfg"].step_size)
    print(f"depth_median against the oracle's: max {err.max():.3g}, step {step:.4f}; k_median equal on {int((s['k_median'].cpu().numpy()[:512] == ref['k_med'][:512]).sum())} of 512")
    assert (err <= step).mean() >= 0.99


# ============================================================================ 4. refusals and the wrappers
def test_refusals(g27, blob):
    from contrastive_lift_amd import _lib, edit, engine
    m, r = g27["model"], g27["renderer"]
    try:
        _, capped = engine.render_forward(m, r, blob["dr"], None, False, grad_heads=(), cap=40000)
        with pytest.raises(_lib.CliftError, match="capped"):
            engine.surface_from_ctx(m, r, capped)
    finally:
        engine.reset_rows_limit()
    box = edit.EditBox(np.eye(3), [-0.05, 0.0, 0.05], [-0.2, -0.2, -0.2], [0.2, 0.2, 0.2])
    _, ectx = engine.edit_forward(m, r, blob["dr"], edit.delete(box), False)
    with pytest.raises(_lib.CliftError, match="edit_forward"):
        engine.surface_from_ctx(m, r, ectx)
    with pytest.raises(_lib.CliftError, match=r"\(0, 1\)"):
        engine.surface_from_ctx(m, r, blob["ctx"], q=1.5)
    with pytest.raises(_lib.CliftError, match="context"):
        engine.surface_from_ctx(m, r, None)
    s = engine.surface_from_ctx(m, r, blob["ctx"])                                      # and the good context still works afterwards
    assert torch.equal(s["depth_median"], blob["s"]["depth_median"])


def test_render_rays_surface_chunks(g27, blob):
    from contrastive_lift_amd import inference as inf
    m, r = g27["model"], g27["renderer"]
    whole = inf.render_rays_surface(m, r, blob["dr"], 0)
    parts = inf.render_rays_surface(m, r, blob["dr"], 200)
    plain = inf.render_rays(m, r, blob["dr"], 200)
    assert len(whole) == 7 and [tuple(x.shape) for x in whole] == [(576, 3), (576, g27["C"]), (576, 2 * g27["E"]), (576,), (576,), (576,), (576, 3)]
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    for a, b in zip(parts[:4], plain):                                                  # the first four are render_rays' own
        assert torch.equal(a, b)
    assert whole[5].dtype == torch.float32 and torch.equal(whole[5] > 0.5, blob["s"]["hit"])
    assert torch.equal(whole[4], blob["s"]["depth_median"]) and torch.equal(whole[6], blob["s"]["normals"])
    sharded = inf.render_rays_sharded(m, r, blob["dr"], 200, render_fn=inf.render_rays_surface)       # no process group: the function itself
    assert all(torch.equal(a, b) for a, b in zip(sharded, whole))


def test_render_panopli_surface_flags(tmp_path, monkeypatch):
    """A few training steps on the synthetic PanopLi scene give a checkpoint and its config; a blob is written into the checkpoint's density
    tables so that rays hit something.  --save_pointcloud --pointcloud_depth median --save_surface writes the surface files and the hit-point
    cloud; without the new flags pointcloud.pkl is what render_rays and backproject give."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd import points3d
    from contrastive_lift_amd.config import load_run_config
    from PIL import Image
    size = 24
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_panopli"), n_frames=12, size=size)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "surface_flags")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_surface")
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
    cents = {c: np.random.default_rng(c).standard_normal((2, 3)).astype(np.float32) for c in (2, 3, 4)}
    cpath = str(tmp_path / "cents.pkl")
    pickle.dump(cents, open(cpath, "wb"))
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_surface")
    out = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, save_pointcloud=True)
    plain = pickle.load(open(out / "pointcloud.pkl", "rb"))
    assert sorted(plain) == ["instances", "points", "rgb", "semantics"]
    assert not (out / "surface").exists() and not (out / "vis_normals").exists()
    scene, model, renderer = rp.load_for_inference(cfg, torch.device("cuda:0"))
    frames = list(rp.scene_frames(scene, "trajectory_blender", True))
    H, W = scene.image_dim
    rgb, pts, pts_med, keep, nrm, dmed = [], [], [], [], [], []
    for _, rays, K in frames:
        o = inf.render_rays_surface(model, renderer, rays, 300, scene.white_bg)
        pr = inf.render_rays(model, renderer, rays, 300, scene.white_bg)
        assert torch.equal(pr[3], o[3])
        pts.append(points3d.backproject(rays, pr[3]).float().cpu())
        rgb.append(pr[0].cpu())
        pts_med.append((rays[:, 0:3] + o[4][:, None] * rays[:, 3:6]).cpu())
        keep.append((o[5] > 0.5).cpu())
        nrm.append(o[6].cpu())
        dmed.append(inf.distance_to_depth(K, o[4].view(H, W)).cpu())
    P = len(frames) * H * W
    assert plain["points"].shape == (P, 3) and np.array_equal(plain["points"], torch.cat(pts, 0).numpy().astype(np.float32))
    assert np.array_equal(plain["rgb"], (torch.cat(rgb, 0).numpy().clip(0, 1) * 255).astype(np.uint8))
    out2 = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, save_pointcloud=True,
                                        pointcloud_depth="median", save_surface=True)
    assert out2 == out
    cloud = pickle.load(open(out / "pointcloud.pkl", "rb"))
    kp = torch.cat(keep, 0).numpy()
    n_keep = int(kp.sum())
    print(f"{n_keep} of {P} pixels hit")
    assert 0.02 * P < n_keep < P                                                      # the blob is seen, and so is the background
    assert sorted(cloud) == ["instances", "normals", "points", "rgb", "semantics"]
    for k in cloud:
        assert cloud[k].shape[0] == n_keep, k
    assert cloud["normals"].dtype == np.float32 and cloud["normals"].shape == (n_keep, 3) and cloud["points"].dtype == np.float32
    assert np.array_equal(cloud["points"], torch.cat(pts_med, 0).numpy().astype(np.float32)[kp])
    assert np.array_equal(cloud["normals"], torch.cat(nrm, 0).numpy().astype(np.float32)[kp])
    for k in ("instances", "semantics", "rgb"):
        assert np.array_equal(cloud[k], plain[k][kp]), k
    for j, (name, _, _) in enumerate(frames):
        z = np.load(out / "surface" / f"{name}.npz")
        assert sorted(z.files) == ["depth_median", "hit", "normals"]
        hit = keep[j].reshape(H, W).numpy()
        assert np.array_equal(z["hit"], hit) and np.array_equal(z["normals"], nrm[j].reshape(H, W, 3).numpy())
        assert np.array_equal(z["depth_median"], dmed[j].reshape(H, W).numpy())
        vis = np.asarray(Image.open(out / "vis_normals" / f"{name}.png"))
        assert vis.shape == (H, W, 3) and (vis[~hit] == 0).all() and (vis[hit].max(-1) > 0).all()
    # fit_bboxes.py reads the file as it is
    fb = _load(os.path.join(REPO, "inference", "fit_bboxes.py"), "clift_fit_bboxes_surface")
    boxes_path, _ = fb.fit_bboxes(str(out / "pointcloud.pkl"), "simple", "device")
    boxes = pickle.load(open(boxes_path, "rb"))
    assert isinstance(boxes, dict) and set(boxes) <= set(int(i) for i in np.unique(cloud["instances"]) if i != 0)
    with pytest.raises(ValueError, match="pointcloud_depth"):
        rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, pointcloud_depth="mean")
