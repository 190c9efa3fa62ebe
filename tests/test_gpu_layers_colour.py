"""Amodal colour layers on the GPU (csrc/layers.hip): clift_ray_layer_colour on the made-up marches of 6i's grid against the
fp32 restatement, the fp64 column-alone reference (tests/layers_colour_cases.py) and clift_ray_layers' own A; two surfaces to the bit;
every refusal of the entry point; engine.layers_forward(colour=True) on the G27 blob scene and engine.edit_layers_forward(colour=True)
under a copy that is moved, against the restatement on the context's own arrays; and the two command lines with --layers_colour."""
import ctypes as C
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import edit_layers_cases as elc
import edit_shape_cases as shc
import layers_cases as lc
import layers_colour_cases as lcc
from conftest import REPO, T, load_golden, rel_close
from engine_recorder import Recorder
from oracle import params as op
from test_gpu_layers import N_RAYS, blob_rays, build_model, made_up_rays, march_record, run_ray_layers

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
NAME = "clift_ray_layer_colour"
SAYS = rf"\(rc=-?\d+\): {NAME}: "          # the library's message begins with the entry point's name, behind _lib.call's own prefix


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def run_colour(ms, m, K, rgb, rgb_row, ldc=3, N=None, n_rgb=None, out=None, M=None):
    """clift_ray_layer_colour on the host arrays of ``m`` (alpha, ray_start, act_idx, slot; None: NULL).  ``rgb`` (n, 3) is laid out with row
    pitch ``ldc``, the pad columns holding a value that would show in every sum if it were read."""
    from contrastive_lift_amd import _lib
    d = {k: (None if m[k] is None else T(m[k]).to(DEV)) for k in ("alpha", "ray_start", "act_idx", "slot")}
    N = m["alpha"].shape[0] if N is None else N
    M = (0 if m["act_idx"] is None else int(m["act_idx"].shape[0])) if M is None else M
    drgb = None
    if rgb is not None:
        wide = np.full((rgb.shape[0], max(ldc, 3)), 9.5e8, F32)
        wide[:, :3] = rgb
        drgb = T(wide).to(DEV)
    n_rgb = (0 if rgb is None else rgb.shape[0]) if n_rgb is None else n_rgb
    drow = None if rgb_row is None else T(np.asarray(rgb_row, np.int32)).to(DEV)
    if out is None:
        out = torch.full((max(N, 0), K + 1, 4), -7.5, device=DEV)
    _lib.call(NAME, C.byref(ms) if ms is not None else None, N, _lib.ptr(d["alpha"]), _lib.ptr(d["ray_start"]), _lib.ptr(d["act_idx"]), M,
              _lib.ptr(d["slot"]), K, _lib.ptr(drgb), ldc, n_rgb, _lib.ptr(drow), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out


# ============================================================================ 1. the kernel on made-up marches
@pytest.mark.parametrize("K", [0, 1, 63, 64, 200, 255])
@pytest.mark.parametrize("N", [1, 5, 9])
@pytest.mark.parametrize("S", [1, 64, 70, 130])
def test_ray_layer_colour_on_made_up_marches(S, N, K):
    """The grid of 6i's kernel test: ray ranges of 0, 1, 63, 64, 65 and S entries, slots -1, K and K + 7 among random ones, alphas exactly 0
    and exactly 1, an entry of another ray, one past N S and a negative one inside ray 2's range.  With one colour per list row (rgb_row
    NULL) at row pitch 3 and 4, and through an indirect rgb_row -- a permutation with entries -1 and n_rgb, which have no colour -- at both
    pitches: R, G, B, A bit-equal to the fp32 restatement, the colours within (n_r + 3) 2^-23 of the fp64 column-alone composite (relative
    where the alphas are 0, 1 or >= 1/16; with alphas down to 0.02 the same figure absolute), A bit-equal to clift_ray_layers' A, two runs
    equal."""
    ms = march_record(S)
    rays, _ = made_up_rays(N, 1000 * S + N)
    dr = T(rays).to(DEV)
    for floor, relative in ((1.0 / 16, True), (0.02, False)):
        m = lcc.made_up_colour_layers(N, S, K, seed=10000 * S + 100 * N + K, alpha_floor=floor)
        assert (m["alpha"] == 0).any() and ((m["alpha"] == 1).any() or S * N < 4)
        A_layers = run_ray_layers(ms, dr, None, m, K).cpu().numpy()[..., 0]
        for rgb, rgb_row, how in ((m["rgb"], None, "rgb_row NULL"), (m["rgb_perm"], m["rgb_row"], "indirect")):
            rest = lcc.colour_restatement(m["alpha"], m["ray_start"], m["act_idx"], m["slot"], K, rgb, rgb_row)
            ref, n_r = lcc.colour_alone_reference(m["alpha"], m["ray_start"], m["act_idx"], m["slot"], K, rgb, rgb_row)
            for ldc in (3, 4):
                what = f"S {S} N {N} K {K} alpha >= {floor:g} ldc {ldc} {how}"
                out = run_colour(ms, m, K, rgb, rgb_row, ldc)
                got = out.cpu().numpy()
                assert np.array_equal(_bits(got), _bits(rest)), f"{what}: {int((_bits(got) != _bits(rest)).sum())} elements differ from the fp32 restatement"
                lcc.check_colour(got, ref, n_r, what=what, relative=relative)
                assert np.array_equal(_bits(got[..., 3]), _bits(A_layers)), f"{what}: A differs from clift_ray_layers' A"
                assert torch.equal(run_colour(ms, m, K, rgb, rgb_row, ldc), out), what                # two runs: the same bits
        if m["act_idx"].size >= 3:
            assert (m["rgb_row"] == -1).any() and (m["rgb_row"] == m["rgb_perm"].shape[0]).any()
    empty = dict(m, ray_start=np.zeros(N + 1, np.int32), act_idx=None, slot=None)           # M = 0, every list pointer NULL: zeros, A = 0
    assert bool((run_colour(ms, empty, K, None, None) == 0).all())
    # no colours at all (n_rgb = 0, rgb NULL) with a list: the colours are zeros and A is still there
    bare = run_colour(ms, m, K, None, None).cpu().numpy()
    assert (bare[..., :3] == 0).all() and np.array_equal(_bits(bare[..., 3]), _bits(A_layers))


def test_two_surfaces_to_the_bit():
    """A shell sample in slot 0 (alpha 0.4, red) in front of a wall in slot 1 (alpha 1, green): alone the shell is (0.4f, 0, 0, A) -- and
    the wall, which the scene shows through the shell only, is whole: (0, 1, 0, 1), to the bit.

    The shell's A is 1 - (1 - 0.4f), the recurrence's own expression and the bits clift_ray_layers gives: 0.4f is an odd multiple of 2^-25,
    1 - 0.4f a tie that rounds to even, and the second subtraction gives 0x3ECCCCCC, one unit in the last place BELOW 0.4f = 0x3ECCCCCD.
    "A = 0.4f to the bit" cannot hold together with "A has the bits of clift_ray_layers' A"; the test holds A to the recurrence, to the
    layer kernel's A, and to within that one unit of 0.4f.  R = (1 * 0.4f) * 1 is 0.4f exactly."""
    S = 64
    alpha = np.zeros((1, S), F32)
    alpha[0, 5], alpha[0, 40] = 0.4, 1.0
    m = dict(alpha=alpha, w=np.zeros((1, S), F32), ray_start=np.asarray([0, 2], np.int32), act_idx=np.asarray([5, 40], np.int32),
             slot=np.asarray([0, 1], np.int32))
    rgb = np.asarray([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
    ms = march_record(S)
    out = run_colour(ms, m, 2, rgb, None).cpu().numpy()
    a0 = F32(F32(1) - F32(F32(1) - F32(0.4)))
    assert int(_bits(np.asarray([a0]))[0]) == 0x3ECCCCCC and int(_bits(np.asarray([F32(0.4)]))[0]) == 0x3ECCCCCD
    assert np.array_equal(_bits(out[0, 0]), _bits(np.asarray([F32(0.4), 0, 0, a0], F32)))
    assert np.array_equal(_bits(out[0, 1]), _bits(np.asarray([0, 1, 0, 1], F32))) and (out[0, 2] == 0).all()
    rays, _ = made_up_rays(1, 5)
    A = run_ray_layers(ms, T(rays).to(DEV), None, m, 2).cpu().numpy()[..., 0]
    assert np.array_equal(_bits(out[..., 3]), _bits(A))


# ============================================================================ 2. refusals, message by message
def test_every_refusal_names_the_entry_point():
    from contrastive_lift_amd import _lib
    S, N, K = 8, 5, 3
    ms = march_record(S)
    m = lcc.made_up_colour_layers(N, S, K, seed=0)
    out = torch.full((N, 300, 4), -7.5, device=DEV)
    go = lambda ms=ms, m=m, K=K, rgb=m["rgb"], **kw: run_colour(ms, m, K, rgb, None, out=out, **{"N": N, **kw})
    for bad_K in (256, -1):
        with pytest.raises(_lib.CliftError, match=rf"{SAYS}K must lie in \[0, 255\] \(got {bad_K}\)"):
            go(K=bad_K)
    with pytest.raises(_lib.CliftError, match=f"{SAYS}the march has no samples"):
        go(ms=march_record(0))
    with pytest.raises(_lib.CliftError, match=f"{SAYS}negative M"):
        go(M=-1)
    big = march_record(2 ** 29)
    with pytest.raises(_lib.CliftError, match=rf"{SAYS}N\*S overflows int32 sample ids"):
        go(ms=big, N=4)                                                                     # 4 * 2^29 = 2^31 >= 2^31 - 1
    with pytest.raises(_lib.CliftError, match=rf"{SAYS}ldc must be >= 3 \(got 2\)"):
        go(ldc=2)
    with pytest.raises(_lib.CliftError, match=f"{SAYS}negative n_rgb"):
        go(n_rgb=-1)
    with pytest.raises(_lib.CliftError, match=f"{SAYS}NULL march record"):
        go(ms=None)
    for gone in ("alpha", "ray_start"):
        with pytest.raises(_lib.CliftError, match=f"{SAYS}NULL buffer"):
            go(m=dict(m, **{gone: None}))
    with pytest.raises(_lib.CliftError, match=f"{SAYS}NULL buffer"):
        _lib.call(NAME, C.byref(ms), N, _lib.ptr(T(m["alpha"]).to(DEV)), _lib.ptr(T(m["ray_start"]).to(DEV)), None, 0, None, K, None, 3, 0, None, None,
                  _lib.stream())                                                            # NULL out
    M = int(m["act_idx"].shape[0])
    for gone in ("act_idx", "slot"):
        with pytest.raises(_lib.CliftError, match=rf"{SAYS}NULL act_idx / slot with M = {M}"):
            go(m=dict(m, **{gone: None}), M=M)
    with pytest.raises(_lib.CliftError, match=rf"{SAYS}NULL rgb with n_rgb = 7"):
        go(rgb=None, n_rgb=7)
    go(N=0)                                                                                 # N = 0: nothing is launched ...
    go(N=-3)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())                                                        # ... and no refusal launched anything either


# ============================================================================ 3. the pass on the G27 blob scene
@pytest.fixture(scope="module")
def g27():
    """The G27 scene of tests/test_gpu_layers.py (the blob field, step ratio 0.25, S = 75, 130 rays, that file's table): a render, the layer
    pass without colour, with colour, with colour_rest, and the render again -- run once, left unchanged."""
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    g = load_golden("g27_dense_volume")
    res = tuple(int(x) for x in g["res"])
    aabb, shift, C_, E = T(g["aabb"]).float(), float(g["shift"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.25).to(DEV)
    model = build_model(P, res, C_, E, shift)
    rng = np.random.default_rng(6)
    cents = {c: (0.5 * rng.standard_normal((2 + c % 2, E))).astype(F32) for c in range(C_)}
    table = SlotTable.from_centroids(cents, list(range(C_)), C_)
    dr = blob_rays().to(DEV)
    # a second table in which only the class the made-up semantic head names most often is a thing: the other listed rows then have no
    # slot, and only colour_rest colours them
    named = torch.bincount(engine.layers_forward(model, r, dr, table)[1].sem_s.argmax(1), minlength=C_).cpu().numpy()
    assert (named > 0).sum() >= 2, f"the made-up semantic head is expected to name two classes or more over the list, it names {named.tolist()}"
    some = SlotTable.from_centroids(cents, [int(named.argmax())], C_)
    before, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    before = {k: v.clone() for k, v in before.items() if torch.is_tensor(v)}
    passes = {}
    for tname, t in (("all", table), ("some", some)):
        passes[tname, "plain"] = engine.layers_forward(model, r, dr, t)
        passes[tname, "colour"] = engine.layers_forward(model, r, dr, t, colour=True)
        passes[tname, "rest"] = engine.layers_forward(model, r, dr, t, colour=True, colour_rest=True)
    after, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    torch.cuda.synchronize()
    return dict(model=model, renderer=r, C=C_, E=E, table=table, some=some, tables=dict(all=table, some=some), cents=cents, rays=dr, before=before,
                after=after, passes=passes)


def _restate(ctx, K):
    """The restatement and the fp64 reference fed with the context's own arrays."""
    alpha, ray_start, act = ctx.alpha.cpu().numpy(), ctx.ray_start.cpu().numpy(), ctx.act_idx.cpu().numpy()[:ctx.M]
    slots, row = ctx.slots.cpu().numpy(), ctx.layer_rgb_row.cpu().numpy()
    rgb = None if ctx.layer_rgb is None else ctx.layer_rgb.cpu().numpy()
    return (lcc.colour_restatement(alpha, ray_start, act, slots, K, rgb, row),) + lcc.colour_alone_reference(alpha, ray_start, act, slots, K, rgb, row)


@pytest.mark.parametrize("tname", ["all", "some"])
def test_blob_scene_colour_equals_the_restatement_on_its_own_arrays(g27, tname):
    table = g27["tables"][tname]
    K = table.K
    plain, pctx = g27["passes"][tname, "plain"]
    out, ctx = g27["passes"][tname, "colour"]
    rest_out, rctx = g27["passes"][tname, "rest"]
    assert "colour" not in plain and sorted(plain) == ["depth", "layers", "n_listed", "opacity"]
    assert pctx.layer_rgb is None and pctx.layer_rgb_row is None and pctx.layer_dirs is None
    for o in (out, rest_out):
        assert sorted(o) == ["colour", "depth", "layers", "n_listed", "opacity"] and o["colour"].shape == (N_RAYS, K + 1, 4)
        for k in ("layers", "opacity", "depth"):
            assert torch.equal(o[k], plain[k]), k                                          # the other outputs keep their bits
        assert o["n_listed"] == plain["n_listed"]
    # the coloured rows are exactly those with a slot; with colour_rest every row
    slots, row = ctx.slots.cpu().numpy(), ctx.layer_rgb_row.cpu().numpy()
    has = (slots >= 0) & (slots < K)
    Mc = int(has.sum())
    assert row.dtype == np.int32 and row.shape == (ctx.M,) and np.array_equal(row >= 0, has) and np.array_equal(row[has], np.arange(Mc))
    assert (row[~has] == -1).all() and ctx.layer_rgb.shape == (Mc, 3) and ctx.layer_dirs.shape == (Mc, 3) and Mc > 0 and ctx.M > 200
    assert np.array_equal(rctx.layer_rgb_row.cpu().numpy(), np.arange(rctx.M)) and rctx.layer_rgb.shape == (rctx.M, 3)
    if tname == "some":
        assert Mc < ctx.M                                                                    # (the fixture made sure of it)
    else:
        assert Mc == ctx.M
    print(f"{tname}: M {ctx.M}, coloured {Mc} ({Mc / ctx.M:.2f}); with colour_rest {rctx.M}")
    for o, c, what in ((out, ctx, "colour"), (rest_out, rctx, "colour_rest")):
        rest, ref, n_r = _restate(c, K)
        got = o["colour"].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(rest)), f"{tname} {what}: {int((_bits(got) != _bits(rest)).sum())} elements differ from the restatement"
        assert np.array_equal(_bits(got[..., 3]), _bits(o["layers"].cpu().numpy()[..., 0]))       # A: the bits of the layers' own A
        assert (got[120:] == 0).all()                                                       # the rays that miss the box
    got = out["colour"].cpu().numpy()
    assert (got[:, K, :3] == 0).all()                                                       # without colour_rest the rest column has no colour
    # the instance columns do not depend on whether the rest is coloured: the same rows, the same colours' bits?  The appearance chain runs
    # over another row count there, so only the product tolerance holds
    rel_close(rest_out["colour"][:, :K], out["colour"][:, :K], 1e-3, what="instance columns with and without colour_rest")
    # the directions are the rays', bit for bit
    act = ctx.act_idx[:ctx.M].long()
    assert torch.equal(ctx.layer_dirs, g27["rays"][act[torch.from_numpy(has).to(DEV)] // ctx.S, 3:6])
    for k, v in g27["before"].items():                                                     # a render after the passes: the bits of the one before
        assert torch.equal(g27["after"][k], v), k


def test_blob_scene_empty_table_rest_column_is_the_scene(g27):
    """K = 0 with colour_rest: the one column is the whole list, and its colour is the fp64 composite of the context's arrays within the
    bound (the scene's alphas go below 1/16, so the figure holds as an absolute error on colours in [0, 1])."""
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    empty = SlotTable.from_centroids({}, [1, 2], g27["C"])
    out, ctx = engine.layers_forward(g27["model"], g27["renderer"], g27["rays"], empty, colour=True, colour_rest=True)
    assert out["colour"].shape == (N_RAYS, 1, 4) and bool((ctx.slots == -1).all()) and ctx.layer_rgb.shape == (ctx.M, 3)
    rest, ref, n_r = _restate(ctx, 0)
    got = out["colour"].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(rest))
    lcc.check_colour(got, ref, n_r, what="empty table, rest column", relative=False)
    assert float(got[:120, 0, :3].max()) > 0.05
    none, nctx = engine.layers_forward(g27["model"], g27["renderer"], g27["rays"], empty, colour=True)        # Mc = 0: the kernel still runs
    assert nctx.layer_rgb is None and bool((nctx.layer_rgb_row == -1).all())
    assert bool((none["colour"][..., :3] == 0).all()) and torch.equal(none["colour"][..., 3], out["colour"][..., 3])
    with pytest.raises(ValueError, match="colour_rest needs colour=True"):
        engine.layers_forward(g27["model"], g27["renderer"], g27["rays"], empty, colour_rest=True)


def test_blob_scene_layer_rgb_is_the_fields_own_colour(g27):
    """ctx.layer_rgb against the field's point-wise methods on the same points and directions, at the product tolerance the edit renders
    are held to."""
    model = g27["model"]
    for tname, how in (("some", "colour"), ("all", "rest")):
        ctx = g27["passes"][tname, how][1]
        rows = torch.nonzero(ctx.layer_rgb_row >= 0).reshape(-1)
        xn = ctx.xa[rows, :3].contiguous()
        with torch.no_grad():
            want = model.render_appearance_mlp(ctx.layer_dirs, model.compute_appearance_feature(xn))
        rel_close(ctx.layer_rgb, want, 1e-3, what=f"layer_rgb ({tname}, {how})")
        assert float(ctx.layer_rgb.min()) >= 0 and float(ctx.layer_rgb.max()) <= 1


@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16", "fp32x6"])
def test_blob_scene_colour_in_every_mlp_mode(g27, mlp_dtype):
    """The colour step runs inside the appearance chain's own precision choice: in each of the three modes the composite equals the
    restatement on the context's own arrays bit for bit (the kernel does not care where the colours came from), and the colours are the
    field's own -- at 1e-3 in the two fp32-faithful modes, within 2e-2 of their scale (colours lie in [0, 1]; bf16 has 8 significant bits,
    the figure tests/test_gpu_round3.py holds rendered colours of that mode to) in bf16 mode."""
    from contrastive_lift_amd import engine
    model, table = g27["model"], g27["some"]
    engine.set_mlp_precision(mlp_dtype)                     # (conftest's autouse fixture puts the default back)
    out, ctx = engine.layers_forward(model, g27["renderer"], g27["rays"], table, colour=True)
    rest, _, _ = _restate(ctx, table.K)
    assert np.array_equal(_bits(out["colour"].cpu().numpy()), _bits(rest))
    assert torch.equal(out["colour"][..., 3], out["layers"][..., 0])
    rows = torch.nonzero(ctx.layer_rgb_row >= 0).reshape(-1)
    engine.set_mlp_precision("fp32")
    with torch.no_grad():
        want = model.render_appearance_mlp(ctx.layer_dirs, model.compute_appearance_feature(ctx.xa[rows, :3].contiguous()))
    if mlp_dtype == "bf16":
        err = float((ctx.layer_rgb - want).abs().max())
        print(f"bf16 mode: layer_rgb within {err:.2e} of the field's fp32 colours")
        assert err < 2e-2
    else:
        rel_close(ctx.layer_rgb, want, 1e-3, what=f"layer_rgb in {mlp_dtype} mode")


def test_blob_scene_chunks_and_wrappers(g27):
    from contrastive_lift_amd import inference as inf
    m, r, table = g27["model"], g27["renderer"], g27["table"]
    plain, colour = g27["passes"]["all", "plain"][0], g27["passes"]["all", "colour"][0]
    three = inf.render_rays_layers(m, r, g27["rays"], 50, table=table)
    assert len(three) == 3 and torch.equal(three[0], plain["layers"])                       # without colour: the three outputs of before
    parts = inf.render_rays_layers(m, r, g27["rays"], 50, table=table, colour=True)
    assert len(parts) == 4 and parts[3].shape == colour["colour"].shape
    assert torch.equal(parts[0], plain["layers"]) and torch.equal(parts[1], plain["opacity"]) and torch.equal(parts[2], plain["depth"])
    assert torch.equal(parts[3][..., 3], colour["colour"][..., 3])                          # A depends on the ray alone: the bits of the whole
    rel_close(parts[3][..., :3], colour["colour"][..., :3], 1e-3, what="colour in chunks of 50")
    whole = r.forward_layers(m, g27["rays"], table, colour=True)
    assert torch.equal(whole["colour"], colour["colour"]) and "colour" not in r.forward_layers(m, g27["rays"], table)
    rest = inf.render_rays_layers(m, r, g27["rays"], 0, table=g27["some"], colour=True, colour_rest=True)
    assert torch.equal(rest[3], g27["passes"]["some", "rest"][0]["colour"])
    import functools
    sharded = inf.render_rays_sharded(m, r, g27["rays"], 50, render_fn=functools.partial(inf.render_rays_layers, table=table, colour=True))
    assert len(sharded) == 4 and all(torch.equal(a, b) for a, b in zip(sharded, parts))       # no process group: the function itself


def _names(fn):
    from contrastive_lift_amd import engine
    with Recorder(launch=engine.call, pointers=False) as rec:
        fn()
    torch.cuda.synchronize()
    return [e[0] for e in rec.launches]


def _app_layer_names(model, Mc):
    """What the appearance layers launch over Mc fp32-stored encoded rows, as the colour step reaches them."""
    from contrastive_lift_amd import engine
    params = engine._head_params(model.named_views())
    X = torch.zeros((Mc, engine._pitch(params["app"][0][0])), dtype=torch.float32, device=DEV)

    def run():
        with engine._app_precision():
            engine._app_layers(Mc, X, params["app"], torch.float32, False, [])
    return _names(run)


def test_launch_sequences(g27):
    """Without colour the pass launches what it launched before this option existed (tests/test_engine_launches.py pins that sequence
    without a GPU; here: colour=False twice gives one sequence, and it is the head of the coloured one).  With colour the tail is
    clift_vm_products_points, the basis Linear, clift_app_encode_points, the appearance layers, clift_ray_layer_colour -- and in the edited
    pass one clift_edit_list_active before them."""
    from contrastive_lift_amd import engine
    m, r, dr, table = g27["model"], g27["renderer"], g27["rays"], g27["some"]
    plain = _names(lambda: engine.layers_forward(m, r, dr, table))
    assert plain[-1] == "clift_ray_layers" and NAME not in plain and "clift_vm_products_points" not in plain
    assert _names(lambda: engine.layers_forward(m, r, dr, table, colour=False, colour_rest=False)) == plain
    ctx = g27["passes"]["some", "colour"][1]
    Mc = int(ctx.layer_rgb.shape[0])
    tail = ["clift_vm_products_points", "clift_gemm", "clift_app_encode_points"] + _app_layer_names(m, Mc) + [NAME]
    assert _names(lambda: engine.layers_forward(m, r, dr, table, colour=True)) == plain + tail
    prog = elc.programs()["cp_mv"]
    eplain = _names(lambda: engine.edit_layers_forward(m, r, dr, prog, table))
    assert eplain[-1] == "clift_ray_layers" and NAME not in eplain and eplain.count("clift_edit_list_active") == 0
    ectx = engine.edit_layers_forward(m, r, dr, prog, table, colour=True)[1]
    etail = ["clift_edit_list_active", "clift_vm_products_points", "clift_gemm", "clift_app_encode_points"] \
        + _app_layer_names(m, int(ectx.layer_rgb.shape[0])) + [NAME]
    assert _names(lambda: engine.edit_layers_forward(m, r, dr, prog, table, colour=True)) == eplain + etail


# ============================================================================ 4. the edited pass
def test_edited_pass_under_a_copy_that_is_moved(g27):
    """[cp, mv] of tests/edit_layers_cases.py on its 130 + 64 rays: colour equals the restatement on the context's arrays with ext.K + 1
    columns; the xa beside the directions has the bits of the origin kernel's; a row no edit remapped keeps its ray's direction; every
    row of the copy's column came through that copy and is coloured; a shaped program stays refused."""
    from contrastive_lift_amd import edit as ed, engine
    m, r, table = g27["model"], g27["renderer"], g27["table"]
    rays = elc.scene_rays()
    dr = rays.to(DEV)
    prog = elc.programs()["cp_mv"]
    plain, _ = engine.edit_layers_forward(m, r, dr, prog, table)
    out, ctx = engine.edit_layers_forward(m, r, dr, prog, table, colour=True)
    ext = out["table"]
    K = table.K
    assert ext.K == K + 1 and out["colour"].shape == (rays.shape[0], K + 2, 4) and "colour" not in plain
    for k in ("layers", "opacity", "depth"):
        assert torch.equal(out[k], plain[k]), k
    rest, ref, n_r = _restate(ctx, ext.K)
    got = out["colour"].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(rest)), f"{int((_bits(got) != _bits(rest)).sum())} elements differ from the restatement"
    assert np.array_equal(_bits(got[..., 3]), _bits(out["layers"].cpu().numpy()[..., 0]))
    assert ctx.layer_xa.shape == (ctx.M, 4) and torch.equal(ctx.layer_xa, ctx.xa)            # clift_edit_list_active's xa: the origin kernel's bits
    slots, origin, state = ctx.slots.cpu().numpy(), ctx.origin.cpu().numpy(), ctx.state.cpu().numpy()
    row = ctx.layer_rgb_row.cpu().numpy()
    has = (slots >= 0) & (slots < ext.K)
    assert np.array_equal(row >= 0, has) and ctx.layer_dirs.shape == (int(has.sum()), 3)
    act = ctx.act_idx[:ctx.M].cpu().numpy().astype(np.int64)
    ray_dirs = rays.numpy()[act[has] // ctx.S, 3:6]
    dirs = ctx.layer_dirs.cpu().numpy()
    still = state[has] == 0
    assert still.sum() > 200 and np.array_equal(_bits(dirs[still]), _bits(ray_dirs[still]))
    # a move by a translation alone turns nothing: those directions are the rays' too; what matters is that they are unit vectors
    assert np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1).max() < 1e-5
    copy = slots == K
    assert copy.sum() >= 20 and (origin[copy] == ext.copy_edit[0] + 1).all() and (row[copy] >= 0).all() and (state[copy] & 0x0f).min() >= 1
    assert float(got[:, K, 3].max()) > 0.5 and float(got[:, K, :3].max()) > 0.05            # the copy is there, in colour
    # the copy shows the blob's own colours: its rows are looked up inside the core box
    xn = ctx.xa[torch.from_numpy(copy).to(DEV), :3]
    lo, hi = (torch.tensor(x, device=DEV) for x in r.bbox_aabb_host)
    world = (xn + 1) / 2 * (hi - lo) + lo
    core = elc.boxes()["core"]
    grown = ed.EditBox(core.axes, core.centre, core.lo - 1e-4, core.hi + 1e-4)              # (fp32 box tests against an fp64 one: off the faces)
    assert grown.contains(world.cpu().double().numpy()).all()
    rest_out, rctx = engine.edit_layers_forward(m, r, dr, prog, table, colour=True, colour_rest=True)
    assert np.array_equal(rctx.layer_rgb_row.cpu().numpy(), np.arange(rctx.M))
    assert np.array_equal(_bits(rest_out["colour"].cpu().numpy()), _bits(_restate(rctx, ext.K)[0]))
    shaped = shc.with_shapes(prog, shc.bernoulli_shapes(len(prog), (5, 6, 7)))
    with pytest.raises(NotImplementedError, match=r"edit_layers_forward: a shaped edit program \(an edit with an EditShape\) is not supported here"):
        engine.edit_layers_forward(m, r, dr, shaped, table, colour=True)
    with pytest.raises(ValueError, match="colour_rest needs colour=True"):
        engine.edit_layers_forward(m, r, dr, prog, table, colour_rest=True)
    from contrastive_lift_amd import inference as inf
    parts = inf.render_rays_edit_layers(m, r, dr, 50, table=table, edit=prog, colour=True)
    assert len(parts) == 4 and torch.equal(parts[0], out["layers"]) and torch.equal(parts[3][..., 3], out["colour"][..., 3])
    rel_close(parts[3][..., :3], out["colour"][..., :3], 1e-3, what="edited colour in chunks of 50")
    assert torch.equal(r.forward_edit_layers(m, dr, prog, table, colour=True)["colour"], out["colour"])
    assert len(inf.render_rays_edit_layers(m, r, dr, 50, table=table, edit=prog)) == 3


# ============================================================================ 5. the two command lines
def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_both_tools_write_colour_layers(tmp_path, monkeypatch):
    """The few-step synthetic PanopLi checkpoint of the other command-line tests (a blob in its density tables, the output bias of thing
    class 2 lifted so that the blob's samples get slots).  With --layers_colour both tools write, beside the files of --save_layers (same
    names; the npz gains one key), vis_amodal_rgb/<frame>/slot_<k>.png per slot the frame's summary reports; without it the file set of
    --save_layers that the existing tests list."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd import layers as ly
    from contrastive_lift_amd.config import load_run_config
    from contrastive_lift_amd.layers import SlotTable
    from PIL import Image
    size = 24
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_panopli"), n_frames=12, size=size)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "layers_colour_flag")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_layers_colour")
    run_dir = train.main(["+experiment=contrastive_lift", f"dataset_root={scene_dir}", f"image_dim={size}", "min_grid_dim=16", "max_grid_dim=16",
                          "max_epoch=1", "steps_per_epoch=4", "batch_size=256", "chunk=0", "max_depth=3", "seed=3", "max_rays_instances=64",
                          "late_semantic_optimization=0", "instance_optimization_epoch=1", "segment_optimization_epoch=3"])
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = ck["state_dict"]
    res = [int(x) for x in sd["renderer.grid_dim"].tolist()]
    op.add_blob({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.density_")}, res, amplitude=3.0, sigma_g=0.5)
    last = max((k for k in sd if k.startswith("model.render_semantic_mlp.mlp.") and k.endswith(".bias")), key=lambda k: int(k.split(".")[-2]))
    sd[last][2] += 20.0
    torch.save(ck, ckpt)
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.image_dim, cfg.chunk = ckpt, [size, size], 300
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_scene_layers_colour")
    rp = es.rp
    scene, model, renderer = rp.load_for_inference(cfg, torch.device("cuda:0"))
    fg = [int(c) for c in scene.segmentation_data.fg_classes]
    n_cls = len(scene.segmentation_data.bg_classes) + len(fg)
    E = int(model.render_instance_mlp.output_channels)
    cents = {c: np.random.default_rng(c).standard_normal((2, E)).astype(F32) for c in fg}
    cpath = str(tmp_path / "cents.pkl")
    pickle.dump(cents, open(cpath, "wb"))
    table = SlotTable.from_centroids(cents, fg, n_cls)
    frames = list(rp.scene_frames(scene, "trajectory_blender", True))
    H, W = scene.image_dim
    layer_files = [f"layers/{n}.npz" for n, _, _ in frames] + [f"layers/{n}.json" for n, _, _ in frames] + [f"vis_amodal/{n}.png" for n, _, _ in frames]

    def check(out, fn, tab, change):
        """The tree ``out`` of a run with the flags; ``fn``: the chunked pass that gives a frame's layers and colour."""
        full = _tree(out)
        seen = 0
        want_rgb = []
        for name, rays, _ in frames:
            z = np.load(out / "layers" / f"{name}.npz")
            assert sorted(z.files) == ["amodal", "colour", "front", "slot_class", "slots", "visible"]
            n = z["slots"].shape[0]
            seen += n
            assert z["colour"].shape == (n, H, W, 4) and z["colour"].dtype == np.uint8
            L, _, _, col = fn(rays)
            s = ly.summarise(L, tab, 0.5)
            present = torch.nonzero(s["amodal_pixels"] > 0).reshape(-1)
            assert np.array_equal(z["slots"], present.cpu().numpy())
            want = (ly.unpremultiply(col[:, present]).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 0, 2).reshape(n, H, W, 4).cpu().numpy()
            assert np.abs(z["colour"].astype(np.int32) - want.astype(np.int32)).max() <= 1       # (chunks of 300 both times; one grey level for the product tolerance)
            assert np.array_equal(z["colour"][..., 3], want[..., 3])                            # A: to the bit, so to the level
            for i, k in enumerate(z["slots"]):
                want_rgb.append(f"vis_amodal_rgb/{name}/slot_{int(k)}.png")
                img = Image.open(out / want_rgb[-1])
                assert img.mode == "RGBA" and img.size == (W, H) and np.array_equal(np.asarray(img), z["colour"][i])
                assert (z["colour"][i][..., 3] > 127).any()                                   # the slot has an amodal pixel at level 0.5
        assert sorted(k for k in full if k.startswith(("layers", "vis_amodal"))) == sorted(layer_files + change + want_rgb)
        return seen

    # render_panopli.py
    plain_dir = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, save_layers=True, layers_level=0.5)
    plain = _tree(plain_dir)
    assert sorted(k for k in plain if k.startswith(("layers", "vis_amodal"))) == sorted(layer_files)       # without the flag: the set of before
    assert all(sorted(np.load(plain_dir / "layers" / f"{n}.npz").files) == ["amodal", "front", "slot_class", "slots", "visible"] for n, _, _ in frames)
    out = rp.render_panopli_checkpoint(cfg, "trajectory_blender", test_only=True, cached_centroids_path=cpath, save_layers=True, layers_level=0.5,
                                       layers_colour=True)
    assert out == plain_dir
    full = _tree(out)
    assert all(full[k] == v for k, v in plain.items() if not k.endswith(".npz"))             # everything but the npz keeps its bytes
    seen = check(out, lambda rays: inf.render_rays_layers(model, renderer, rays, 300, scene.white_bg, table=table, colour=True), table, [])
    print(f"render_panopli: {seen} coloured slot layers over {len(frames)} frames")
    assert seen > 0
    # edit_scene.py: a box around the blob copied -- the copy has a slot and so an image of its own
    lo, hi = (np.asarray(x, np.float64) for x in renderer.bbox_aabb_host)
    boxes = {5: {"bbox": (-0.3 * (hi - lo), 0.3 * (hi - lo)), "orientation": np.eye(3), "position": (lo + hi) / 2}}
    the_edit = es.resolve_edit(boxes, 5, "copy", translate=[0.15 * (hi - lo)[0], 0.0, 0.0], rotate_deg=[0.0, 0.0, 30.0])
    ext = table.for_program(the_edit)
    change = [f"layers/{n}_change.json" for n, _, _ in frames]
    off = es.edit_scene_checkpoint(cfg, the_edit, "copy_5_layers", save_layers=True, cached_centroids_path=cpath, layers_level=0.5)
    assert sorted(k for k in _tree(off) if k.startswith(("layers", "vis_amodal"))) == sorted(layer_files + change)
    on = es.edit_scene_checkpoint(cfg, the_edit, "copy_5_colour", save_layers=True, cached_centroids_path=cpath, layers_level=0.5, layers_colour=True)
    a, b = _tree(off), _tree(on)
    assert all(b[k] == v for k, v in a.items() if not k.endswith(".npz"))
    seen = check(on, lambda rays: inf.render_rays_edit_layers(model, renderer, rays, 300, scene.white_bg, table=table, edit=the_edit, colour=True),
                 ext, change)
    copy_images = [k for k in b if k.startswith("vis_amodal_rgb/") and k.endswith(f"slot_{table.K}.png")]
    print(f"edit_scene: {seen} coloured slot layers, {len(copy_images)} of them the copy's")
    assert seen > 0 and copy_images
