"""Amodal instance layers on the GPU (csrc/layers.hip): clift_ray_layers on made-up marches and clift_sample_slots on made-up
rows against the fp32 numpy restatements and the fp64 object-alone reference (tests/layers_cases.py), the engine pass on the G27 blob scene
against those restatements on the context's own arrays, the refusals, the chunked wrapper and inference/render_panopli.py --save_layers."""
import ctypes as C
import importlib.util
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import layers_cases as lc
from conftest import REPO, T, load_golden
from oracle import params as op

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
BOX = ([-1.0] * 3, [1.0] * 3)
STEP = 0.03


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def made_up_rays(N, seed):
    """N rays from a sphere of radius 0.95 towards the unit cube's middle, with jitter; the box is the unit cube, the step 0.03."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((N, 3))
    o = 0.95 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.3, 0.3, (N, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((N, 1), 0.01), np.full((N, 1), 4.0)], 1).astype(F32)
    return rays, rng.random(N).astype(F32)


def march_record(S):
    from contrastive_lift_amd import _lib
    ms = _lib.March()
    for i in range(3):
        ms.lo[i], ms.hi[i], ms.inv_ext2[i] = -1.0, 1.0, 1.0
    ms.step_size, ms.n_samples, ms.distance_scale, ms.density_shift, ms.weight_thres = STEP, S, 25.0, -3.0, 1e-4
    return ms


def run_ray_layers(ms, rays, jitter, m, K, N=None, out=None):
    from contrastive_lift_amd import _lib
    N = rays.shape[0] if N is None else N
    d = {k: (None if m[k] is None else T(m[k]).to(DEV)) for k in ("alpha", "w", "ray_start", "act_idx", "slot")}
    M = 0 if m["act_idx"] is None else int(m["act_idx"].shape[0])
    if out is None:
        out = torch.full((max(N, 0), K + 1, 4), -7.5, device=DEV)
    _lib.call("clift_ray_layers", C.byref(ms) if ms is not None else None, _lib.ptr(rays), _lib.ptr(jitter), N, _lib.ptr(d["alpha"]), _lib.ptr(d["w"]),
              _lib.ptr(d["ray_start"]), _lib.ptr(d["act_idx"]) if M else None, M, _lib.ptr(d["slot"]) if M else None, K, _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out


# ============================================================================ 1. clift_ray_layers on made-up marches
@pytest.mark.parametrize("K", [0, 1, 63, 64, 200, 255])
@pytest.mark.parametrize("N", [1, 5, 9])
@pytest.mark.parametrize("S", [1, 64, 70, 130])
def test_ray_layers_on_made_up_marches(S, N, K):
    """Ray ranges of 0, 1, 63, 64, 65 and S entries (N = 9 has all of them; ray 0 lists all S), slots -1, K and K + 7 among random ones,
    alphas exactly 0 and exactly 1, an entry of another ray, one past N S and a negative one inside ray 2's range; with jitter and without."""
    ms = march_record(S)
    rays, jitter = made_up_rays(N, 1000 * S + N)
    m = lc.made_up_layers(N, S, K, seed=10000 * S + 100 * N + K)
    assert (m["alpha"] == 0).any() and ((m["alpha"] == 1).any() or S * N < 4)
    dr = T(rays).to(DEV)
    for jit in (jitter, None):
        z = lc.sample_z(rays, BOX[0], BOX[1], STEP, S, jit)
        z64 = lc.sample_z64(rays, BOX[0], BOX[1], STEP, S, jit)
        rest = lc.layers_restatement(m["alpha"], m["w"], z, m["ray_start"], m["act_idx"], m["slot"], K)
        ref, n_r = lc.object_alone_reference(m["alpha"], m["w"], z64, m["ray_start"], m["act_idx"], m["slot"], K)
        dj = None if jit is None else T(jit).to(DEV)
        out = run_ray_layers(ms, dr, dj, m, K)
        lc.check_layers(out.cpu().numpy(), rest, ref, n_r, what=f"S {S} N {N} K {K} jitter {'given' if jit is not None else 'NULL'}")
        assert torch.equal(run_ray_layers(ms, dr, dj, m, K), out)                          # two runs: the same bits
    empty = dict(m, ray_start=np.zeros(N + 1, np.int32), act_idx=None, slot=None)           # M = 0, act_idx and slot NULL: every row zeros
    assert bool((run_ray_layers(ms, dr, None, empty, K) == 0).all())


def test_ray_layers_two_surfaces_the_wall_is_whole_behind_the_shell():
    """two_surface_ray with shell = slot 0 and wall = slot 1.  Alone the wall is opaque, the scene shows it through the shell:
    A_1 > 0.9 and V_1 < A_1 (1 - alpha_shell)^shell + 1e-6, with the shell at sample 1 (shell = 1: the function's shell is ONE sample at that
    index, so the transmittance in front of the wall is (1 - alpha_shell)^1) and, at the default index 5, against that same single factor."""
    S = 64
    rays, _ = made_up_rays(1, 5)
    for shell, power in ((1, 1), (5, 1)):
        _, w, _, _ = lc.two_surface_ray(S=S, shell=shell, wall=40, alpha_shell=0.4)
        alpha = np.zeros((1, S), F32)
        alpha[0, shell], alpha[0, 40] = 0.4, 1.0
        m = dict(alpha=alpha, w=w, ray_start=np.asarray([0, 2], np.int32), act_idx=np.asarray([shell, 40], np.int32), slot=np.asarray([0, 1], np.int32))
        out = run_ray_layers(march_record(S), T(rays).to(DEV), None, m, 2).cpu().numpy()
        A1, V1 = float(out[0, 1, 0]), float(out[0, 1, 1])
        print(f"shell at {shell}: A_1 {A1:.6f} V_1 {V1:.6f} bound {A1 * (1 - 0.4) ** power + 1e-6:.6f}")
        assert A1 > 0.9 and V1 < A1 * (1 - 0.4) ** power + 1e-6
        assert abs(float(out[0, 0, 0]) - 0.4) < 1e-6 and (out[0, 2] == 0).all()


# ============================================================================ 2. clift_sample_slots
def run_sample_slots(c, K, mode, lds, ldf, use_add, n=None):
    from contrastive_lift_amd import _lib
    n_rows, Ccls = c["sem"].shape
    E = c["feat"].shape[1]
    sem = torch.full((n_rows, max(lds, Ccls)), 9.5e8)       # pad columns that would win every maximum if they were read
    sem[:, :Ccls] = T(c["sem"])
    feat = torch.full((n_rows, max(ldf, E)), 9.5e8)
    feat[:, :E] = T(c["feat"])
    add = T(c["add"]).to(DEV) if use_add else None
    slot = torch.full((n_rows,), -77, dtype=torch.int32, device=DEV)
    cent = T(c["cent"]).to(DEV) if c["cent"] is not None and K > 0 else None
    sem, feat, cs = sem.to(DEV), feat.to(DEV), T(c["cls_slots"]).to(DEV)
    _lib.call("clift_sample_slots", _lib.ptr(sem), lds, Ccls, _lib.ptr(feat), ldf, E, _lib.ptr(add), E, _lib.ptr(cs), _lib.ptr(cent), K, mode,
              n_rows if n is None else n, _lib.ptr(slot), _lib.stream())
    torch.cuda.synchronize()
    return slot.cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("E", [1, 3, 32])
@pytest.mark.parametrize("C_", [1, 5])
@pytest.mark.parametrize("n", [1, 257])
def test_sample_slots_equal_the_restatement(n, C_, E, mode):
    """Rows with NaN features, an exact tie, a NaN semantic output, a stuff class (C = 5: class 0) and a last class whose range runs past K;
    with row pitches above C and E and without, with the added term and without: every label equal, no row left out."""
    K = 13
    c = lc.made_up_slot_rows(n, C_, E, K, seed=1000 * n + 100 * C_ + 10 * E + mode, mode=mode)
    for lds, ldf, use_add in ((C_, E, False), (C_ + 3, E + 2, True), (C_, E + 1, True), (C_ + 1, E, False)):
        want = lc.slots_restatement(c["sem"], c["feat"], c["add"] if use_add else None, c["cls_slots"], c["cent"], K, mode)
        got = run_sample_slots(c, K, mode, lds, ldf, use_add)
        assert np.array_equal(got, want), f"n {n} C {C_} E {E} mode {mode} lds {lds} ldf {ldf} add {use_add}: {int((got != want).sum())} rows differ"
        assert ((want >= -1) & (want < K)).all()
    if n == 257:
        assert (want >= 0).any()
        if C_ == 5 or mode == 0:                                                            # rows of the stuff class, the NaN row
            assert (want == -1).any()
        if mode == 0:
            assert want[1] == -1                                                            # NaN features: no winner
            if C_ == 5 and K >= 2:
                assert want[2] == c["cls_slots"][1, 0]                                      # the tie: the lower index
        last = c["cls_slots"][-1] if C_ > 1 else c["cls_slots"][0]
        assert last[0] + last[1] > K                                                        # the clamped range is there
    k0 = lc.slots_restatement(c["sem"], c["feat"], None, c["cls_slots"], None, 0, mode)      # K = 0 (centroids NULL): every row -1
    assert (k0 == -1).all() and np.array_equal(run_sample_slots(dict(c, cent=None), 0, mode, C_, E, False), k0)


# ============================================================================ 3. the engine pass on the G27 blob scene
N_RAYS = 130


def build_model(P, res, C_, E, shift):
    import contrastive_lift_amd as cl
    m = cl.TensorVMSplit(list(res), num_density_comps=(16,) * 3, num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32),
                         num_semantic_classes=C_, dim_feature_instance=2 * E, splus_density_shift=shift, use_semantic_mlp=True,
                         use_instance_mlp=True, slow_fast_mode=True, device=DEV)
    missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    assert not missing and not unexpected
    return m


def blob_rays():
    """120 rays from a sphere of radius 0.9 aimed near the blob (the middle of the box), then 10 rays that start below the box and point
    away from it (the recipe of tests/test_gpu_surface.py)."""
    rng = np.random.default_rng(27)
    eyes = rng.standard_normal((120, 3))
    eyes = 0.9 * eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
    target = np.array([[-0.05, 0.0, 0.05]]) + rng.uniform(-0.08, 0.08, (120, 3))
    d = target - eyes
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_miss = np.array([[0.0, 0.0, -0.95]]) + rng.uniform(-0.02, 0.02, (10, 3))
    d_miss = rng.standard_normal((10, 3)) * 0.1 + np.array([1.0, 0.0, -0.3])
    d_miss /= np.linalg.norm(d_miss, axis=1, keepdims=True)
    o, d = np.concatenate([eyes, o_miss]), np.concatenate([d, d_miss])
    return torch.from_numpy(np.concatenate([o, d, np.full((N_RAYS, 1), 0.01), np.full((N_RAYS, 1), 4.0)], 1).astype(F32))


@pytest.fixture(scope="module")
def g27():
    """The G27 scene: the blob field as a model, the renderer at step ratio 0.25 (S = 75), 130 rays, a table of a few made-up centroids,
    a render before the layer pass, the layer pass, and the render again."""
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    g = load_golden("g27_dense_volume")
    res = tuple(int(x) for x in g["res"])
    aabb, shift, C_, E = T(g["aabb"]).float(), float(g["shift"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.25).to(DEV)
    assert r.n_samples == 75
    model = build_model(P, res, C_, E, shift)
    rng = np.random.default_rng(6)
    # every class counts as a thing and has centroids: whichever classes the made-up semantic head names, its samples get slots
    things = list(range(C_))
    cents = {c: (0.5 * rng.standard_normal((2 + c % 2, E))).astype(F32) for c in things}
    table = SlotTable.from_centroids(cents, things, C_)
    dr = blob_rays().to(DEV)
    before, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    before = {k: v.clone() for k, v in before.items() if torch.is_tensor(v)}
    out, ctx = engine.layers_forward(model, r, dr, table)
    after, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    torch.cuda.synchronize()
    return dict(model=model, renderer=r, C=C_, E=E, table=table, cents=cents, rays=dr, before=before, after=after, out=out, ctx=ctx)


def _host_lists(ctx):
    return (ctx.alpha.cpu().numpy(), ctx.w.cpu().numpy(), ctx.ray_start.cpu().numpy(), ctx.act_idx.cpu().numpy()[:ctx.M],
            ctx.slots.cpu().numpy())


def test_blob_scene_equals_the_restatements_on_its_own_arrays(g27):
    ctx, out, table, r = g27["ctx"], g27["out"], g27["table"], g27["renderer"]
    K = table.K
    assert ctx.S == 75 and ctx.N == N_RAYS and out["n_listed"] == ctx.M > ctx.M_render > 200 and K >= 4
    assert out["layers"].shape == (N_RAYS, K + 1, 4) and ctx.sem_s.shape == (ctx.M, g27["C"]) and ctx.inst_s.shape == (ctx.M, g27["E"])
    alpha, w, ray_start, act_idx, slots = _host_lists(ctx)
    # the alpha-list is what the definition says: alpha > threshold, by ray, then by sample
    want_list = np.nonzero(alpha.reshape(-1) > F32(r.raymarch_weight_thres))[0]
    assert np.array_equal(act_idx, want_list) and np.array_equal(ray_start[1:], np.cumsum((alpha > F32(r.raymarch_weight_thres)).sum(1)))
    want = lc.slots_restatement(ctx.sem_s.cpu().numpy(), ctx.inst_s.cpu().numpy(), None, table.cls_slots, table.centroids, K, 0)
    assert np.array_equal(slots, want), f"{int((slots != want).sum())} of {ctx.M} slots differ"
    print(f"M {ctx.M} (the render lists {ctx.M_render}); slots: {np.bincount(slots + 1, minlength=K + 1).tolist()} (first: unassigned)")
    assert (slots >= 0).all()
    lo, hi = r.bbox_aabb_host
    rays = g27["rays"].cpu().numpy()
    z = lc.sample_z(rays, lo, hi, r.step_size_host, ctx.S, None)
    z64 = lc.sample_z64(rays, lo, hi, r.step_size_host, ctx.S, None)
    rest = lc.layers_restatement(alpha, w, z, ray_start, act_idx, slots, K)
    ref, n_r = lc.object_alone_reference(alpha, w, z64, ray_start, act_idx, slots, K)
    L = out["layers"].cpu().numpy()
    lc.check_layers(L, rest, ref, n_r, what="blob scene")
    # what is visible of all columns together is what the scene's weights give the list
    v_sum = L[..., 1].astype(np.float64).sum(1)
    w_list = np.asarray([w.reshape(-1).astype(np.float64)[act_idx[ray_start[i]:ray_start[i + 1]]].sum() for i in range(N_RAYS)])
    print(f"sum V against sum w over the list: worst {np.abs(v_sum - w_list).max():.3g}")
    assert (np.abs(v_sum - w_list) <= n_r * lc.EPS * np.abs(w_list)).all()
    assert (L[..., 0] >= L[..., 1] - 1e-6).all()                                          # no column is more visible than it is there
    assert (L[120:] == 0).all() and (L[:120, :, 0].sum(1) > 0.9).all()                     # the rays that miss the box; the rays that hit the blob
    assert torch.equal(out["opacity"], g27["before"]["opacity"]) and torch.equal(out["depth"], g27["before"]["depth"])


def test_blob_scene_empty_table_rest_column_is_the_opacity(g27):
    """K = 0, alpha_thres = 0: every sample with any alpha is listed and falls into the rest column, whose A = 1 - prod (1 - alpha) is the
    opacity sum w of the march, to S 2^-23."""
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    empty = SlotTable.from_centroids({}, [1, 2], g27["C"])
    out, ctx = engine.layers_forward(g27["model"], g27["renderer"], g27["rays"], empty, alpha_thres=0.0)
    assert out["layers"].shape == (N_RAYS, 1, 4) and bool((ctx.slots == -1).all())
    err = (out["layers"][:, 0, 0].double() - ctx.ray_out[:, 0].double()).abs().max().item()
    print(f"A_rest against the march's opacity: worst {err:.3g}, bound {ctx.S * lc.EPS:.3g}")
    assert err <= ctx.S * lc.EPS


def test_blob_scene_chunks_and_no_state_left_behind(g27):
    from contrastive_lift_amd import inference as inf
    m, r, table = g27["model"], g27["renderer"], g27["table"]
    parts = inf.render_rays_layers(m, r, g27["rays"], 50, table=table)
    assert len(parts) == 3 and torch.equal(parts[0], g27["out"]["layers"])
    assert torch.equal(parts[1], g27["out"]["opacity"]) and torch.equal(parts[2], g27["out"]["depth"])
    whole = r.forward_layers(m, g27["rays"], table)
    assert torch.equal(whole["layers"], parts[0])
    import functools
    sharded = inf.render_rays_sharded(m, r, g27["rays"], 50, render_fn=functools.partial(inf.render_rays_layers, table=table))
    assert all(torch.equal(a, b) for a, b in zip(sharded, parts))                          # no process group: the function itself
    for k, v in g27["before"].items():                                                     # a render after the pass: the bits of the one before
        assert torch.equal(g27["after"][k], v), k


def test_use_delta_adds_world_positions(g27):
    """E = 3 here: with use_delta the feature is output + world position, de-normalised from xa; the restatement takes the context's sums."""
    from contrastive_lift_amd import engine
    if g27["E"] != 3:
        pytest.fail("the G27 scene is expected to have 3 instance features")
    out, ctx = engine.layers_forward(g27["model"], g27["renderer"], g27["rays"], g27["table"], use_delta=True)
    assert ctx.layer_add.shape == (ctx.M, 3)
    want = lc.slots_restatement(ctx.sem_s.cpu().numpy(), ctx.inst_s.cpu().numpy(), ctx.layer_add.cpu().numpy(), g27["table"].cls_slots,
                                g27["table"].centroids, g27["table"].K, 0)
    assert np.array_equal(ctx.slots.cpu().numpy(), want)
    lo, hi = g27["renderer"].bbox_aabb_host
    assert bool((ctx.layer_add.cpu() >= torch.tensor(lo) - 1e-4).all()) and bool((ctx.layer_add.cpu() <= torch.tensor(hi) + 1e-4).all())


def test_heads_on_their_own_grids_and_slot_scores():
    """A field whose semantic and instance heads sit on their own VM grids, its instance outputs read as slot scores (mode 1): the chains
    give the pass all it needs, and the slots equal the restatement on the context's own head outputs."""
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    torch.manual_seed(3)
    res, C_, E = (9, 13, 17), 4, 6
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    m = cl.TensorVMSplit(list(res), num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=C_,
                         dim_feature_instance=E, splus_density_shift=0.0, device=DEV)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.5).to(DEV)
    table = SlotTable.from_scores([1, 3], C_, E)
    out, ctx = engine.layers_forward(m, r, blob_rays().to(DEV), table)
    assert ctx.M > 500 and out["layers"].shape == (N_RAYS, E + 1, 4)
    want = lc.slots_restatement(ctx.sem_s.cpu().numpy(), ctx.inst_s.cpu().numpy(), None, table.cls_slots, None, E, 1)
    assert np.array_equal(ctx.slots.cpu().numpy(), want)
    assert torch.equal(engine.layers_forward(m, r, blob_rays().to(DEV), table)[0]["layers"], out["layers"])


# ============================================================================ 4. refusals
def test_refusals(g27):
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import _lib, engine
    from contrastive_lift_amd.layers import SlotTable
    S, N = 8, 5
    ms = march_record(S)
    rays, _ = made_up_rays(N, 0)
    dr = T(rays).to(DEV)
    m = lc.made_up_layers(N, S, 3, seed=0)
    out = torch.full((N, 300, 4), -7.5, device=DEV)
    with pytest.raises(_lib.CliftError, match="255"):
        run_ray_layers(ms, dr, None, m, 256, out=out)
    with pytest.raises(_lib.CliftError, match="255"):
        run_ray_layers(ms, dr, None, m, -1, out=out)
    with pytest.raises(_lib.CliftError, match="NULL"):
        run_ray_layers(ms, dr, None, dict(m, alpha=None), 3, out=out)
    with pytest.raises(_lib.CliftError, match="NULL"):
        run_ray_layers(ms, None, None, m, 3, N=N, out=out)
    with pytest.raises(_lib.CliftError, match="NULL"):
        run_ray_layers(None, dr, None, m, 3, out=out)
    with pytest.raises(_lib.CliftError, match="no samples"):
        run_ray_layers(march_record(0), dr, None, m, 3, out=out)
    run_ray_layers(ms, dr, None, m, 3, N=0, out=out)                                       # N = 0: nothing is launched
    assert bool((out == -7.5).all())
    c = lc.made_up_slot_rows(4, 3, 2, 5, seed=1, mode=0)
    with pytest.raises(_lib.CliftError, match="255"):
        run_sample_slots(c, 256, 0, 3, 2, False)
    with pytest.raises(_lib.CliftError, match="lds"):
        run_sample_slots(c, 5, 0, 2, 2, False)
    with pytest.raises(_lib.CliftError, match="ldf"):
        run_sample_slots(c, 5, 0, 3, 1, False)
    with pytest.raises(_lib.CliftError, match="centroids"):
        run_sample_slots(dict(c, cent=None), 5, 0, 3, 2, False)
    with pytest.raises(_lib.CliftError, match="mode"):
        run_sample_slots(c, 5, 2, 3, 2, False)
    assert (run_sample_slots(c, 5, 0, 3, 2, False, n=0) == -77).all()                      # n = 0: nothing is launched
    # the engine pass
    model, r, table = g27["model"], g27["renderer"], g27["table"]
    with pytest.raises(_lib.CliftError, match="capped"):
        engine.layers_forward(model, r, g27["rays"], table, cap=40000)
    headless = cl.TensorVMSplit([9, 13, 17], num_semantic_classes=g27["C"], use_semantic_mlp=True, device=DEV)
    with pytest.raises(ValueError, match="no instance head"):
        engine.layers_forward(headless, r, g27["rays"], table)
    with pytest.raises(ValueError, match="classes"):
        engine.layers_forward(model, r, g27["rays"], SlotTable.from_centroids(g27["cents"], [1], g27["C"] + 1))
    with pytest.raises(ValueError, match="feature columns"):
        engine.layers_forward(model, r, g27["rays"], SlotTable.from_centroids({1: np.zeros((2, g27["E"] + 1), F32)}, [1], g27["C"]))
    again, _ = engine.layers_forward(model, r, g27["rays"], table)                          # and the pass still works afterwards
    assert torch.equal(again["layers"], g27["out"]["layers"])


# ============================================================================ 5. inference/render_panopli.py --save_layers
def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_render_panopli_save_layers(tmp_path, monkeypatch):
    """The tiny checkpoint of the surface command-line test (a few training steps on the synthetic PanopLi scene, a blob written into its
    density tables).  Without the flag the script writes what it wrote before; with it the same files with the same bytes, and per frame
    layers/<frame>.npz, layers/<frame>.json and vis_amodal/<frame>.png."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd.config import load_run_config
    from contrastive_lift_amd.layers import SlotTable
    from PIL import Image
    size = 24
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_panopli"), n_frames=12, size=size)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "layers_flag")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_layers")
    run_dir = train.main(["+experiment=contrastive_lift", f"dataset_root={scene_dir}", f"image_dim={size}", "min_grid_dim=16", "max_grid_dim=16",
                          "max_epoch=1", "steps_per_epoch=4", "batch_size=256", "chunk=0", "max_depth=3", "seed=3", "max_rays_instances=64",
                          "late_semantic_optimization=0", "instance_optimization_epoch=1", "segment_optimization_epoch=3"])
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = ck["state_dict"]
    res = [int(x) for x in sd["renderer.grid_dim"].tolist()]
    op.add_blob({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.density_")}, res, amplitude=3.0, sigma_g=0.5)
    # four training steps leave the semantic head naming a stuff class everywhere: lift the output bias of thing class 2, so that the
    # blob's samples get slots and the files have something to hold
    last = max((k for k in sd if k.startswith("model.render_semantic_mlp.mlp.") and k.endswith(".bias")), key=lambda k: int(k.split(".")[-2]))
    sd[last][2] += 20.0
    torch.save(ck, ckpt)
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.image_dim, cfg.chunk = ckpt, [size, size], 300
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_layers")
    scene, model, renderer = rp.load_for_inference(cfg, torch.device("cuda:0"))
    fg = [int(c) for c in scene.segmentation_data.fg_classes]
    n_cls = len(scene.segmentation_data.bg_classes) + len(fg)
    E = int(model.render_instance_mlp.output_channels)
    cents = {c: np.random.default_rng(c).standard_normal((2, E)).astype(F32) for c in fg}
    cpath = str(tmp_path / "cents.pkl")
    pickle.dump(cents, open(cpath, "wb"))
    out = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath)
    plain = _tree(out)
    assert plain and not any(k.startswith(("layers", "vis_amodal")) for k in plain)
    out2 = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, save_layers=True, layers_level=0.5)
    assert out2 == out
    full = _tree(out)
    added = sorted(set(full) - set(plain))
    assert all(full[k] == v for k, v in plain.items())                                     # what was written before keeps its bytes
    frames = list(rp.scene_frames(scene, "trajectory_blender", True))
    H, W = scene.image_dim
    assert added == sorted([f"layers/{n}.npz" for n, _, _ in frames] + [f"layers/{n}.json" for n, _, _ in frames]
                           + [f"vis_amodal/{n}.png" for n, _, _ in frames])
    table = SlotTable.from_centroids(cents, fg, n_cls)
    seen = 0
    for name, rays, _ in frames:
        z = np.load(out / "layers" / f"{name}.npz")
        assert sorted(z.files) == ["amodal", "front", "slot_class", "slots", "visible"]
        n = z["slots"].shape[0]
        seen += n
        for k in ("amodal", "visible", "front"):
            assert z[k].shape == (n, H, W) and z[k].dtype == np.float16, k
        assert z["slot_class"].shape == (n,) and np.array_equal(z["slot_class"], table.slot_class[z["slots"]])
        L = inf.render_rays_layers(model, renderer, rays, 300, scene.white_bg, table=table)[0]
        A = L[:, :table.K, 0].T.reshape(table.K, H, W).cpu().numpy()
        assert np.array_equal(z["slots"], np.nonzero((A > 0.5).any((1, 2)))[0])
        assert np.array_equal(z["amodal"], A[z["slots"]].astype(np.float16))
        assert (z["amodal"].astype(np.float32) >= z["visible"].astype(np.float32) - 2e-3).all()
        js = json.load(open(out / "layers" / f"{name}.json"))
        assert js["level"] == 0.5 and js["n_slots"] == table.K and [s["slot"] for s in js["slots"]] == z["slots"].tolist()
        for s in js["slots"]:
            assert sorted(s) == ["amodal_pixels", "mean_distance", "occlusion", "slot", "slot_class", "slot_index", "visible_pixels"]
            assert s["amodal_pixels"] == int((A[s["slot"]] > 0.5).sum()) > 0 and 0 <= s["visible_pixels"] <= H * W
            assert s["occlusion"] <= 1.0 and s["mean_distance"] > 0
        vis = np.asarray(Image.open(out / "vis_amodal" / f"{name}.png"))
        assert vis.shape == (H, W, 3)
    print(f"{seen} slot layers over {len(frames)} frames")
    assert seen > 0                                                                        # the blob is seen as some instance
    with pytest.raises(ValueError, match="cached_centroids_path"):
        rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, save_layers=True)
