"""Amodal instance layers of an edited scene on the GPU: clift_edit_list_active_origin against its restatements, then
engine.edit_layers_forward on the G27 blob scene of tests/test_gpu_layers.py (res 9 x 13 x 17, step ratio 0.25, S = 75, that file's table)
under a copy, a copy that is moved and a copy of the copy -- against the restatements on the context's own arrays, the plain layer pass
and the CPU oracle --, the wrappers, the refusals and inference/edit_scene.py --save_layers.  What the scene is relied on for is asserted
without a GPU in tests/test_edit_layers_host.py."""
import ctypes as C
import functools
import importlib.util
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import edit_layers_cases as elc
import edit_program_cases as epc
import edit_surface_cases as esc
import layers_cases as lc
from conftest import REPO, T, load_golden
from oracle import params as op

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
PROGRAMS = ("cp", "cp_mv", "cp_cp2")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(P, res, C_, E, shift):
    import contrastive_lift_amd as cl
    m = cl.TensorVMSplit(list(res), num_density_comps=(16,) * 3, num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32),
                         num_semantic_classes=C_, dim_feature_instance=2 * E, splus_density_shift=shift, use_semantic_mlp=True,
                         use_instance_mlp=True, slow_fast_mode=True, device=DEV)
    missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    assert not missing and not unexpected
    return m


@pytest.fixture(scope="module")
def g27():
    """The scene, its table (every class has centroids, as in tests/test_gpu_layers.py), the 130 + 64 rays, the fp64 walks, a render before
    every pass, the plain layer pass, the edited passes of the three programs and the render again: run once, left unchanged."""
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.layers import SlotTable
    g = load_golden("g27_dense_volume")
    P, cfg, res, C_, E, shift, aabb = elc.oracle_scene(g)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax", step_ratio=0.25).to(DEV)
    assert r.n_samples == 75
    model = build_model(P, res, C_, E, shift)
    rng = np.random.default_rng(6)
    things = list(range(C_))
    cents = {c: (0.5 * rng.standard_normal((2 + c % 2, E))).astype(F32) for c in things}
    table = SlotTable.from_centroids(cents, things, C_)
    rays = elc.scene_rays()
    dr = rays.to(DEV)
    progs = elc.programs()
    before, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    before = {k: v.clone() for k, v in before.items() if torch.is_tensor(v)}
    plain, pctx = engine.layers_forward(model, r, dr, table)
    passes = {name: engine.edit_layers_forward(model, r, dr, progs[name], table) for name in PROGRAMS}
    after, _ = engine.render_forward(model, r, dr, None, False, grad_heads=())
    torch.cuda.synchronize()
    lo, hi = (np.asarray(x, np.float64) for x in r.bbox_aabb_host)
    walks = {name: elc.host_walk(rays, cfg, progs[name]) for name in PROGRAMS}
    return dict(P=P, cfg=cfg, C=C_, E=E, model=model, renderer=r, table=table, cents=cents, rays=rays, dr=dr, progs=progs, before=before,
                after=after, plain=plain, pctx=pctx, passes=passes, walks=walks, lo=lo, hi=hi, boxes=elc.boxes())


def _world(g27, act_idx):
    r = g27["renderer"]
    lo, hi = r.bbox_aabb_host
    return elc.world_samples_np(lo, hi, r.step_size_host, g27["rays"].numpy(), act_idx, int(r.n_samples))


# ============================================================================ 1. the kernel against restatements
def run_origin(ms, prog, dr, act, M=None, want_state=True):
    from contrastive_lift_amd import _lib
    M = act.shape[0] if M is None else M
    xa = torch.full((act.shape[0], 4), -7.5, device=DEV)
    origin = torch.full((act.shape[0],), 99, dtype=torch.uint8, device=DEV)
    state = torch.full((act.shape[0],), 99, dtype=torch.uint8, device=DEV) if want_state else None
    _lib.call("clift_edit_list_active_origin", C.byref(ms), prog.records(), len(prog), _lib.ptr(dr), _lib.ptr(act), M, _lib.ptr(xa),
              _lib.ptr(origin), _lib.ptr(state), _lib.stream())
    torch.cuda.synchronize()
    return xa, origin, state


def run_active(ms, prog, dr, act):
    from contrastive_lift_amd import _lib
    xa = torch.full((act.shape[0], 4), -7.5, device=DEV)
    dirs = torch.empty((act.shape[0], 4), device=DEV)
    _lib.call("clift_edit_list_active", C.byref(ms), prog.records(), len(prog), _lib.ptr(dr), _lib.ptr(act), act.shape[0], _lib.ptr(xa),
              _lib.ptr(dirs), _lib.stream())
    torch.cuda.synchronize()
    return xa


def test_origin_kernel_equals_its_restatements(g27):
    """The programs [cp], [cp, mv], [cp, cp2], a move alone and the full eight of edit_surface_cases.programs, on the scene's alpha-lists
    and on made-up lists of 1, 255, 256 and 257 entries of several rays: xa has the bits of clift_edit_list_active, state is the byte of
    clift_edit_list_points for the same fp32 world points, origin equals the fp32 restatement on every row and the fp64 walk on the rows
    of the rays that lie off all faces; two runs give equal bytes."""
    from contrastive_lift_amd import edit, engine
    r, model, dr, cfg = g27["renderer"], g27["model"], g27["dr"], g27["cfg"]
    ms = engine.march_struct(r, model)
    S, N = int(r.n_samples), g27["rays"].shape[0]
    progs = dict(g27["progs"], full8=esc.programs(g27["lo"], g27["hi"])["full8"])
    lists = {f"made-up {M}": elc.made_up_list(M, N, S, 40 + M) for M in (1, 255, 256, 257)}
    for name in PROGRAMS:
        ctx = g27["passes"][name][1]
        lists[f"alpha-list of {name}"] = ctx.act_idx[:ctx.M].cpu().numpy()
    seen = {}
    for pname, prog in progs.items():
        keep_rays = epc.rays_off_all_faces(g27["rays"], cfg, prog).numpy()
        for lname, ids in lists.items():
            what = f"{pname} on {lname}"
            act = torch.from_numpy(ids).to(DEV)
            xa, origin, state = run_origin(ms, prog, dr, act)
            assert torch.equal(xa, run_active(ms, prog, dr, act)), what
            assert bool((xa[:, 3] == 0).all()), what
            world = _world(g27, ids)
            _, _, state_pts = prog.apply_to_points(torch.from_numpy(world).to(DEV))
            assert torch.equal(state, state_pts), what
            _, o32, s32 = elc.origin_restatement(prog, world)
            o, s = origin.cpu().numpy(), state.cpu().numpy()
            assert np.array_equal(o, o32) and np.array_equal(s, s32), what
            keep = keep_rays[ids.astype(np.int64) // S]
            _, o64, s64 = prog.origins(world.astype(np.float64))
            assert np.array_equal(o[keep], o64[keep]) and np.array_equal(s[keep], s64[keep]), what
            xa2, origin2, state2 = run_origin(ms, prog, dr, act)
            assert torch.equal(xa2, xa) and torch.equal(origin2, origin) and torch.equal(state2, state), what
            assert torch.equal(run_origin(ms, prog, dr, act, want_state=False)[1], origin), what      # state NULL
            seen.setdefault(pname, set()).update(np.unique(o).tolist())
            if lname == f"alpha-list of {pname}":
                assert not (s & edit.STATE_KILLED).any(), what                                  # a killed sample is in no alpha-list
                if pname == "cp_mv":
                    assert ((o == 1) == ((s & edit.STATE_REMAPS) == 2)).all() and (o == 1).sum() > 50, what
    assert seen["cp"] == {0, 1} and seen["cp_mv"] == {0, 1} and seen["cp_cp2"] == {0, 1, 2} and seen["mv_only"] == {0}
    assert seen["full8"] == {0, 2, 5}
    # M = 0: nothing is launched; M below the buffer: the rows past M are not written
    act = torch.from_numpy(lists["made-up 257"]).to(DEV)
    xa, origin, state = run_origin(ms, progs["cp"], dr, act, M=0)
    assert bool((xa == -7.5).all()) and bool((origin == 99).all()) and bool((state == 99).all())
    xa, origin, state = run_origin(ms, progs["cp"], dr, act, M=200)
    assert bool((xa[200:] == -7.5).all()) and bool((origin[200:] == 99).all()) and bool((origin[:200] <= 1).all())


def test_origin_kernel_errors_name_the_entry_point(g27):
    from contrastive_lift_amd import _lib, engine
    r, model, dr = g27["renderer"], g27["model"], g27["dr"]
    ms = engine.march_struct(r, model)
    name = "clift_edit_list_active_origin"
    prog = esc.programs(g27["lo"], g27["hi"])["full8"]
    nine = (_lib.EditRec * 9)(*(prog[i % 8].record() for i in range(9)))
    act = torch.zeros((4,), dtype=torch.int32, device=DEV)
    xa = torch.full((4, 4), -7.5, device=DEV)
    origin = torch.full((4,), 99, dtype=torch.uint8, device=DEV)
    call = lambda recs, n, ms=ms, xa=xa, origin=origin: _lib.call(name, C.byref(ms), recs, n, _lib.ptr(dr), _lib.ptr(act), 4, _lib.ptr(xa),
                                                                  _lib.ptr(origin) if origin is not None else None, None, _lib.stream())
    for n in (0, 9):
        with pytest.raises(_lib.CliftError, match=f"{name}: .*n_edits = {n}"):
            call(nine, n)
    bad = prog.records()
    bad[3].map_t[1] = float("nan")
    with pytest.raises(_lib.CliftError, match=f"{name}: edit 3: .*not finite"):
        call(bad, 8)
    with pytest.raises(_lib.CliftError, match=f"{name}: .*NULL"):
        call(prog.records(), 8, origin=None)
    empty = engine.march_struct(r, model)
    empty.n_samples = 0
    with pytest.raises(_lib.CliftError, match=f"{name}: n_samples"):
        call(prog.records(), 8, ms=empty)
    torch.cuda.synchronize()
    assert bool((xa == -7.5).all()) and bool((origin == 99).all())                          # nothing was launched


# ============================================================================ 2. nothing edited, nothing changed
def test_an_empty_delete_gives_the_bits_of_the_plain_pass(g27):
    from contrastive_lift_amd import edit, engine
    m, r, dr, table = g27["model"], g27["renderer"], g27["dr"], g27["table"]
    out, ctx = engine.edit_layers_forward(m, r, dr, edit.delete(esc.empty_box()), table)
    plain = g27["plain"]
    assert out["table"].K == table.K and out["table"].copy_edit.shape == (0,) and ctx.edited and out["n_listed"] == plain["n_listed"]
    for k in ("layers", "opacity", "depth"):
        assert torch.equal(out[k], plain[k]), k
    assert bool((ctx.origin == 0).all()) and bool((ctx.state == 0).all()) and torch.equal(ctx.slots, g27["pctx"].slots)


def test_rays_no_edit_touches_keep_their_bits_under_a_copy(g27):
    """[cp]: the rays none of whose in-aabb samples the fp64 walk remaps or kills, less those with a sample within 1e-3 of the copy's
    destination box: every base column has the bits of the plain pass, the copy column is zeros."""
    from contrastive_lift_amd import edit
    out, ctx = g27["passes"]["cp"]
    walk, cp = g27["walks"]["cp"], g27["boxes"]["cp"]
    K = g27["table"].K
    untouched = elc.untouched_rays(walk)
    grown = edit.EditBox(cp.dst.axes, cp.dst.centre, cp.dst.lo - 1e-3, cp.dst.hi + 1e-3)
    near = (grown.contains(walk["points"]).reshape(walk["N"], walk["S"]) & walk["inbox"]).any(1)
    still = torch.from_numpy(untouched & ~near).to(DEV)
    touched = torch.from_numpy(~untouched).to(DEV)
    print(f"{int(still.sum())} rays untouched and clear of the copy, {int(touched.sum())} touched")
    assert int(still.sum()) >= 90 and int(touched.sum()) >= 60
    assert out["layers"].shape == (194, K + 2, 4)
    L, Lp = out["layers"], g27["plain"]["layers"]
    assert torch.equal(L[still][:, :K], Lp[still][:, :K]) and torch.equal(L[still][:, K + 1], Lp[still][:, K])
    assert bool((L[still][:, K] == 0).all())
    assert torch.equal(out["opacity"][still], g27["plain"]["opacity"][still]) and torch.equal(out["depth"][still], g27["plain"]["depth"][still])
    assert float(L[touched][:, K, 0].max()) > 0.5                                        # ... and the copy is there on touched rays


# ============================================================================ 3. the pass equals the restatements on its own arrays
@pytest.mark.parametrize("name", PROGRAMS)
def test_the_pass_equals_the_restatements_on_its_own_arrays(g27, name):
    from contrastive_lift_amd import edit
    out, ctx = g27["passes"][name]
    table, r, prog = g27["table"], g27["renderer"], g27["progs"][name]
    ext = out["table"]
    K, c = table.K, len(prog.copies())
    N = g27["rays"].shape[0]
    assert ext.K == K + c and ext.copy_edit.tolist() == prog.copies() and out["layers"].shape == (N, K + c + 1, 4)
    assert ctx.edited and ctx.edit_program is prog and ctx.S == 75 and ctx.N == N and out["n_listed"] == ctx.M > 200
    assert ctx.sem_s.shape == (ctx.M, g27["C"]) and ctx.inst_s.shape == (ctx.M, g27["E"]) and ctx.xa.shape == (ctx.M, 4)
    alpha, w = ctx.alpha.cpu().numpy(), ctx.w.cpu().numpy()
    ray_start, act_idx = ctx.ray_start.cpu().numpy(), ctx.act_idx.cpu().numpy()[:ctx.M]
    thres = F32(r.raymarch_weight_thres)
    assert np.array_equal(act_idx, np.nonzero(alpha.reshape(-1) > thres)[0]) and np.array_equal(ray_start[1:], np.cumsum((alpha > thres).sum(1)))
    base = ctx.base_slots.cpu().numpy()
    want = lc.slots_restatement(ctx.sem_s.cpu().numpy(), ctx.inst_s.cpu().numpy(), None, table.cls_slots, table.centroids, K, 0)
    assert np.array_equal(base, want), f"{int((base != want).sum())} of {ctx.M} base slots differ"
    assert (base >= 0).all() and (base < K).all()
    origin, state, slots = ctx.origin.cpu().numpy(), ctx.state.cpu().numpy(), ctx.slots.cpu().numpy()
    assert np.array_equal(slots, elc.retarget_restatement(base, origin, K, ext.copy_edit))
    assert not (state & edit.STATE_KILLED).any()                                          # no listed sample is killed
    print(f"{name}: M {ctx.M}; columns {np.bincount(slots + 1, minlength=K + c + 1).tolist()} (first: unassigned); origins {np.bincount(origin).tolist()}")
    for j in range(c):
        assert (slots == K + j).sum() >= 20                                               # every copy has samples in its column
    lo, hi = r.bbox_aabb_host
    rays = g27["rays"].numpy()
    z = lc.sample_z(rays, lo, hi, r.step_size_host, ctx.S, None)
    z64 = lc.sample_z64(rays, lo, hi, r.step_size_host, ctx.S, None)
    rest = lc.layers_restatement(alpha, w, z, ray_start, act_idx, slots, K + c)
    ref, n_r = lc.object_alone_reference(alpha, w, z64, ray_start, act_idx, slots, K + c)
    L = out["layers"].cpu().numpy()
    lc.check_layers(L, rest, ref, n_r, what=f"blob scene under {name}")
    v_sum = L[..., 1].astype(np.float64).sum(1)
    w_list = np.asarray([w.reshape(-1).astype(np.float64)[act_idx[ray_start[i]:ray_start[i + 1]]].sum() for i in range(N)])
    print(f"sum V against sum w over the list: worst {np.abs(v_sum - w_list).max():.3g}")
    assert (np.abs(v_sum - w_list) <= n_r * lc.EPS * np.abs(w_list)).all()
    assert (L[..., 0] >= L[..., 1] - 1e-6).all()
    assert torch.equal(out["opacity"], ctx.ray_out[:, 0]) and torch.equal(out["depth"], ctx.ray_out[:, 1])


def test_chunks_and_no_state_left_behind(g27):
    from contrastive_lift_amd import inference as inf
    m, r, table, dr = g27["model"], g27["renderer"], g27["table"], g27["dr"]
    for name in PROGRAMS:
        out = g27["passes"][name][0]
        parts = inf.render_rays_edit_layers(m, r, dr, 50, table=table, edit=g27["progs"][name])
        assert len(parts) == 3 and torch.equal(parts[0], out["layers"]), name
        assert torch.equal(parts[1], out["opacity"]) and torch.equal(parts[2], out["depth"]), name
    for k, v in g27["before"].items():                                                     # a plain render afterwards: the bits of one before
        assert torch.equal(g27["after"][k], v), k


# ============================================================================ 4. the copy brings a hidden core into view
def test_the_copy_brings_the_hidden_core_into_view(g27):
    """[cp] on the 64 front rays.  The oracle (fp32, on the CPU): the untouched samples inside ``core`` are jointly opaque and have a visible
    weight below 1e-3 (the host test pins that); the copy's samples are visible.  The device: the base columns' V over the list entries
    inside ``core`` (restated from w and the list) within S 1e-4 of the oracle's, per ray V_copy within S 1e-4 of the oracle's -- 1e-4 is
    what the march tests hold w to against the oracle, a sum of at most S terms gets S times that -- and A_copy >= V_copy - 1e-6."""
    from contrastive_lift_amd import layers as ly
    out, ctx = g27["passes"]["cp"]
    K, S = g27["table"].K, ctx.S
    front = slice(elc.N_BLOB, elc.N_BLOB + elc.N_FRONT)
    walk = g27["walks"]["cp"]
    a, w = elc.oracle_weights(g27["P"], g27["cfg"], walk, g27["lo"], g27["hi"])
    origin = walk["origin"].reshape(walk["N"], S)
    in_core = g27["boxes"]["core"].contains(walk["points"]).reshape(walk["N"], S)
    listed = a > 1e-4
    core_sel = in_core & (origin == 0) & listed
    v_core = (w * core_sel).sum(1)[front]
    a_core = (1.0 - np.prod(np.where(core_sel, 1.0 - a, 1.0), 1))[front]
    v_copy = (w * ((origin == 1) & listed)).sum(1)[front]
    print(f"oracle: core A min {a_core.min():.4f}, core V max {v_core.max():.2e}, V_copy min {v_copy.min():.4f}")
    assert a_core.min() > 0.9995 and v_core.max() < 1e-3
    # the device: sum of w over the list entries inside core that no copy brought there
    act = ctx.act_idx[:ctx.M].cpu().numpy().astype(np.int64)
    world = _world(g27, act).astype(np.float64)
    dev_origin, slots = ctx.origin.cpu().numpy(), ctx.slots.cpu().numpy()
    sel = g27["boxes"]["core"].contains(world) & (dev_origin == 0) & (slots >= 0) & (slots < K)
    dev_w = ctx.w.cpu().numpy().astype(np.float64).reshape(-1)
    dev_v_core = np.bincount(act[sel] // S, weights=dev_w[act[sel]], minlength=walk["N"])[front]
    tol = S * 1e-4
    print(f"device: core V max {dev_v_core.max():.2e} (worst difference to the oracle {np.abs(dev_v_core - v_core).max():.2e}, bound {tol:.2e})")
    assert (np.abs(dev_v_core - v_core) <= tol).all()
    L = out["layers"][front].cpu().numpy().astype(np.float64)
    print(f"device: V_copy min {L[:, K, 1].min():.4f}, worst difference to the oracle {np.abs(L[:, K, 1] - v_copy).max():.2e}")
    assert (np.abs(L[:, K, 1] - v_copy) <= tol).all()
    assert (L[:, K, 0] >= L[:, K, 1] - 1e-6).all()
    cmp = ly.compare(g27["plain"]["layers"][front], out["layers"][front], g27["table"], out["table"])
    assert int(cmp["amodal_pixels_after"][K]) >= 62
    assert int(cmp["amodal_pixels_before"][K]) == 0 and int(cmp["visible_pixels_before"][K]) == 0
    assert int(cmp["newly_hidden"][K]) == 0 and int(cmp["revealed"][K]) == 0 and int(cmp["gone"][K]) == 0
    assert cmp["slot_class"][K] == -1 and cmp["slot_index"][K] == 0


# ============================================================================ 5. a move keeps the slot, a moved copy keeps its column
def test_a_move_keeps_the_slot_and_a_moved_copy_its_column(g27):
    from contrastive_lift_amd import layers as ly
    out, ctx = g27["passes"]["cp_mv"]
    K, S, N = g27["table"].K, ctx.S, g27["rays"].shape[0]
    assert out["table"].K == K + 1 and out["table"].copy_edit.tolist() == [0]              # no column for the move
    act = ctx.act_idx[:ctx.M].cpu().numpy().astype(np.int64)
    world = _world(g27, act).astype(np.float64)
    in_mv = g27["boxes"]["mv"].dst.contains(world)
    slots, origin = ctx.slots.cpu().numpy(), ctx.origin.cpu().numpy()
    keep_rays = epc.rays_off_all_faces(g27["rays"], g27["cfg"], g27["progs"]["cp_mv"]).numpy()     # (fp64 against fp32 box tests: off the faces)
    kr = keep_rays[act // S]
    assert (in_mv & kr).sum() > 50 and (slots[in_mv & kr] == K).all() and (origin[in_mv & kr] == 1).all() and not (slots[~in_mv & kr] == K).any()
    L = out["layers"]
    through = np.bincount(act[in_mv] // S, minlength=N) > 0
    thr, miss = torch.from_numpy(through & keep_rays).to(DEV), torch.from_numpy(~through & keep_rays).to(DEV)
    # a ray through the moved copy has that column: A > 0 and a first distance.  V_K is the sum of w over those rows and is held to the bit
    # by check_layers above; it is no assertion here, because behind the opaque blob the transmittance is exactly 0 in fp32, and so is w
    print(f"{int(thr.sum())} rays pass through the moved copy, {int((L[thr][:, K, 1] > 0).sum())} of them give it weight")
    assert int(thr.sum()) > 20 and bool((L[thr][:, K, 0] > 0).all()) and bool((L[thr][:, K, 3] > 0).all()) and bool((L[miss][:, K] == 0).all())
    # the same objects under a move alone keep their base slots: nothing is retargeted
    from contrastive_lift_amd import engine
    o2, c2 = engine.edit_layers_forward(g27["model"], g27["renderer"], g27["dr"], g27["progs"]["mv_only"], g27["table"])
    assert o2["table"].K == K and torch.equal(c2.slots, c2.base_slots) and bool((c2.origin == 0).all()) and bool(((c2.state & 0x0f) == 1).any())
    # front_order, restated from zf: the nearest column with A > level comes first, a tie goes to the lower column
    order, count = ly.front_order(L)
    A, zf = L[:, :K + 1, 0].cpu().numpy(), L[:, :K + 1, 3].cpu().numpy()
    on = A > 0.5
    key = np.where(on, zf, np.inf)
    first = np.where(on.any(1), key.argmin(1), -1)
    assert np.array_equal(order[:, 0].cpu().numpy(), first) and np.array_equal(count.cpu().numpy(), on.sum(1))
    # ... the moved copy stands in the order where its first listed sample stands among the first samples of the other columns that are
    # on.  On these rays that is never the front: the density floor in front of it is listed too and shares a slot with the blob
    lead = _copy_rank_in_front_order(ctx, L, K, 0.5)
    print(f"the moved copy is on for {int(on[:, K].sum())} rays of the scene and leads on {int(lead.sum())}")
    assert on[:, K].sum() > 20 and (first[lead] == K).all() and (first[on[:, K] & ~lead] != K).all()
    # ... and it IS the front on the 16 side rays, which pass through it and clear of the blob, at level 0.9: along them the floor and
    # the blob's tail together gather an opacity below 0.9 (tests/test_edit_layers_host.py), so the copy's is the only column that is on
    side = elc.side_rays().to(DEV)
    so, sctx = engine.edit_layers_forward(g27["model"], g27["renderer"], side, g27["progs"]["cp_mv"], g27["table"])
    SL = so["layers"]
    lead = _copy_rank_in_front_order(sctx, SL, K, 0.9)
    order9 = ly.front_order(SL, 0.9)[0].cpu().numpy()
    print(f"side rays: A_K min {float(SL[:, K, 0].min()):.4f}, largest other column {float(SL[:, :K, 0].max()):.4f}; the copy leads on {int(lead.sum())} of 16")
    assert lead.all() and (order9[:, 0] == K).all()


def _copy_rank_in_front_order(ctx, L, K, level):
    """front_order(L, level) restated per ray from the list: column K stands behind exactly the columns that are on and whose first listed
    sample precedes its own.  Asserts that, and returns (N,) bool: K is on and nothing stands in front of it."""
    from contrastive_lift_amd import layers as ly
    order = ly.front_order(L, level)[0].cpu().numpy()
    on = L[:, :K + 1, 0].cpu().numpy() > level
    slots, rs = ctx.slots.cpu().numpy(), ctx.ray_start.cpu().numpy()
    lead = np.zeros(L.shape[0], bool)
    for i in np.nonzero(on[:, K])[0]:
        cols = slots[rs[i]:rs[i + 1]]
        first_row = {int(c_): int(np.nonzero(cols == c_)[0][0]) for c_ in np.unique(cols) if 0 <= c_ <= K and on[i, c_]}
        ahead = sum(1 for c_, j in first_row.items() if c_ != K and j < first_row[K])
        assert order[i, ahead] == K, f"ray {i}: column K at {order[i].tolist()}, {ahead} columns start in front of it"
        lead[i] = ahead == 0
    return lead


# ============================================================================ 6. wrappers, refusals, the command line
def test_wrappers_and_refusals(g27):
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd.layers import SlotTable
    m, r, table, dr, prog = g27["model"], g27["renderer"], g27["table"], g27["dr"], g27["progs"]["cp_mv"]
    out = g27["passes"]["cp_mv"][0]
    whole = r.forward_edit_layers(m, dr, prog, table)
    assert torch.equal(whole["layers"], out["layers"]) and whole["table"].K == table.K + 1
    assert torch.equal(r.forward_edit_layers(m, dr, list(prog), table)["layers"], out["layers"])          # a sequence of edits
    fn = functools.partial(inf.render_rays_edit_layers, table=table, edit=prog)
    sharded = inf.render_rays_sharded(m, r, dr, 50, render_fn=fn)                           # no process group: the function itself
    assert torch.equal(sharded[0], out["layers"]) and torch.equal(sharded[1], out["opacity"]) and torch.equal(sharded[2], out["depth"])
    with pytest.raises(ValueError, match="slot table"):
        inf.render_rays_edit_layers(m, r, dr, 0, edit=prog)
    with pytest.raises(ValueError, match="edit is required"):
        inf.render_rays_edit_layers(m, r, dr, 0, table=table)
    with pytest.raises(ValueError, match="alpha_thres"):
        engine.edit_layers_forward(m, r, dr, prog, table, alpha_thres=-1e-3)
    headless = cl.TensorVMSplit([9, 13, 17], num_semantic_classes=g27["C"], use_semantic_mlp=True, device=DEV)
    with pytest.raises(ValueError, match="no instance head"):
        engine.edit_layers_forward(headless, r, dr, prog, table)
    with pytest.raises(ValueError, match="classes"):
        engine.edit_layers_forward(m, r, dr, prog, SlotTable.from_centroids(g27["cents"], [1], g27["C"] + 1))
    with pytest.raises(ValueError, match="feature columns"):
        engine.edit_layers_forward(m, r, dr, prog, SlotTable.from_centroids({1: np.zeros((2, g27["E"] + 1), F32)}, [1], g27["C"]))
    grid = cl.TensorVMSplit([9, 13, 17], num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=g27["C"],
                            dim_feature_instance=g27["E"], splus_density_shift=0.0, device=DEV)
    with pytest.raises(NotImplementedError, match="VM grid"):
        engine.edit_layers_forward(grid, r, dr, prog, SlotTable.from_scores([1], g27["C"], g27["E"]))
    with pytest.raises(TypeError):
        engine.layers_forward(m, r, dr, table, edit=prog)                                   # the plain pass takes no edit
    again, _ = engine.edit_layers_forward(m, r, dr, prog, table)                            # and the pass still works afterwards
    assert torch.equal(again["layers"], out["layers"])
    assert torch.equal(engine.layers_forward(m, r, dr, table)[0]["layers"], g27["plain"]["layers"])
    # alpha_thres = 0: every sample with any alpha is listed, and still none that an edit killed; use_delta: the looked-up world position
    zero, zctx = engine.edit_layers_forward(m, r, dr, prog, table, alpha_thres=0.0, use_delta=True)
    assert zctx.M >= out["n_listed"] and not bool((zctx.state & 0x80).any()) and zctx.layer_add.shape == (zctx.M, 3)
    want = lc.slots_restatement(zctx.sem_s.cpu().numpy(), zctx.inst_s.cpu().numpy(), zctx.layer_add.cpu().numpy(), table.cls_slots,
                                table.centroids, table.K, 0)
    assert np.array_equal(zctx.base_slots.cpu().numpy(), want)
    src = prog.origins(_world(g27, zctx.act_idx[:zctx.M].cpu().numpy()).astype(np.float64))[0]
    assert np.abs(zctx.layer_add.cpu().numpy() - src).max() < 1e-4                          # ... of the looked-up point, not of the sample


def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_edit_scene_save_layers(tmp_path, monkeypatch):
    """The few-step synthetic PanopLi checkpoint of the other command-line tests (a blob in its density tables, the output bias of thing
    class 2 lifted so that the blob's samples get slots), a box around the blob copied: --save_layers writes layers/<frame>.npz,
    layers/<frame>.json, vis_amodal/<frame>.png and layers/<frame>_change.json per frame; without the flag none of them, and the other
    files are the same bytes."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd.config import load_run_config
    from contrastive_lift_amd.layers import SlotTable
    size = 24
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_panopli"), n_frames=12, size=size)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "edit_layers_flag")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_edit_layers")
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
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_scene_layers_gpu")
    scene, model, renderer = es.rp.load_for_inference(cfg, torch.device("cuda:0"))
    lo, hi = (np.asarray(x, np.float64) for x in renderer.bbox_aabb_host)
    boxes = {5: {"bbox": (-0.3 * (hi - lo), 0.3 * (hi - lo)), "orientation": np.eye(3), "position": (lo + hi) / 2}}
    the_edit = es.resolve_edit(boxes, 5, "copy", translate=[0.15 * (hi - lo)[0], 0.0, 0.0], rotate_deg=[0.0, 0.0, 30.0])
    fg = [int(c) for c in scene.segmentation_data.fg_classes]
    n_cls = len(scene.segmentation_data.bg_classes) + len(fg)
    E = int(model.render_instance_mlp.output_channels)
    cents = {c: np.random.default_rng(c).standard_normal((2, E)).astype(F32) for c in fg}
    cpath = str(tmp_path / "cents.pkl")
    pickle.dump(cents, open(cpath, "wb"))
    off = es.edit_scene_checkpoint(cfg, the_edit, "copy_5_plain")
    on = es.edit_scene_checkpoint(cfg, the_edit, "copy_5_layers", save_layers=True, cached_centroids_path=cpath, layers_level=0.5)
    plain, full = _tree(off), _tree(on)
    assert plain and not any(k.startswith(("layers", "vis_amodal")) for k in plain)
    assert all(full[k] == v for k, v in plain.items())                                     # what was written before keeps its bytes
    frames = list(es.rp.scene_frames(scene, "trajectory_blender", True))
    H, W = scene.image_dim
    assert sorted(set(full) - set(plain)) == sorted([f"layers/{n}.npz" for n, _, _ in frames] + [f"layers/{n}.json" for n, _, _ in frames]
                                                     + [f"layers/{n}_change.json" for n, _, _ in frames]
                                                     + [f"vis_amodal/{n}.png" for n, _, _ in frames])
    table = SlotTable.from_centroids(cents, fg, n_cls)
    ext = table.for_program(the_edit)
    assert ext.K == table.K + 1
    copy_seen = 0
    for name, rays, _ in frames:
        z = np.load(on / "layers" / f"{name}.npz")
        L = inf.render_rays_edit_layers(model, renderer, rays, 300, scene.white_bg, table=table, edit=the_edit)[0]
        A = L[:, :ext.K, 0].T.reshape(ext.K, H, W).cpu().numpy()
        assert np.array_equal(z["slots"], np.nonzero((A > 0.5).any((1, 2)))[0])
        assert np.array_equal(z["amodal"], A[z["slots"]].astype(np.float16)) and np.array_equal(z["slot_class"], ext.slot_class[z["slots"]])
        js = json.load(open(on / "layers" / f"{name}.json"))
        assert js["n_slots"] == ext.K and [s["slot"] for s in js["slots"]] == z["slots"].tolist()
        ch = json.load(open(on / "layers" / f"{name}_change.json"))
        assert ch["n_slots"] == ext.K and ch["n_base_slots"] == table.K and ch["copy_edit"] == [0] and ch["level"] == 0.5
        Lb = inf.render_rays_layers(model, renderer, rays, 300, scene.white_bg, table=table)[0]
        for s in ch["slots"]:
            i = s["slot"]
            assert s["amodal_pixels_after"] == int((A[i] > 0.5).sum())
            assert s["amodal_pixels_before"] == (int((Lb[:, i, 0] > 0.5).sum()) if i < table.K else 0)
            if i == table.K:
                assert s["slot_class"] == -1 and s["slot_index"] == 0 and s["gone"] == 0
                copy_seen += s["amodal_pixels_after"]
    print(f"the copy covers {copy_seen} pixels over {len(frames)} frames")
    assert copy_seen > 0
    with pytest.raises(ValueError, match="cached_centroids_path"):
        es.edit_scene_checkpoint(cfg, the_edit, "copy_5_none", save_layers=True)
