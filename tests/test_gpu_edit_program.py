"""Edit programs on the GPU (csrc/edit.hip: k_edit_list_density_fwd / k_edit_list_active through engine.edit_forward): an ordered list of
edits applied in one render.  Anchors that hold bit for bit -- a list of one is the single edit; deletes compose to the minimum of the
single-edit sigma arrays in either order -- and chained remaps, order dependence and the chunked / sharded render against the CPU
restatement of the backward walk (tests/edit_program_cases.py).

Tolerance: ``rel_close(..., 1e-3)``, the product tolerance G6 and the single-edit tests are held to.  Rays with a sample within 1e-5 of a
box face at some stage of the walk are left out by the fp64 criterion ``rays_off_all_faces`` (at most 4 per case; the boxes below leave
out none or one)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import edit_cases as ec
import edit_program_cases as epc
from conftest import T, load_golden, rel_close
from oracle import render as orender
from test_gpu_scene_edit import DEV, NAMES, build_model, build_renderer, outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_scene_edit")


@pytest.fixture(scope="module")
def scene130():
    P, rays = ec.scene130()
    return P, rays, rays.to(DEV)


def scene(which, g25, scene130):
    """(P, rays): the golden's 96 rays or scene130's 130 rays (8 of them past the aabb)."""
    if which == "golden":
        return ec.golden_params(g25), T(g25["rays"])
    return scene130[0], scene130[1]


def cfg_of(mode):
    return orender.RenderCfg(ec.AABB, ec.RES, density_shift=ec.SHIFT, semantic_weight_mode=mode)


def samples(rays, cfg):
    """fp64 sample positions (N * S, 3) and the in-aabb mask (N * S,)."""
    pts, _, inbox = orender.sample_along_rays(rays, cfg, None)
    return pts.reshape(-1, 3).double().numpy(), inbox.reshape(-1).numpy()


def ebox(rot, centre, lo, hi):
    from contrastive_lift_amd import edit
    return edit.EditBox(ec.rot_xyz(*rot).double().numpy(), centre, lo, hi)


# the boxes of the cases (world units; the aabb is [-0.9, 0.8] x [-0.7, 0.7] x [-0.5, 0.6], the blob sits at its centre)
def box_A():        # test_gpu_scene_edit's rays130 box: it sticks out of the aabb's +x face
    return ebox((0.1, -0.15, 0.4), [0.6, 0.25, 0.15], [-0.37, -0.31, -0.28], [0.33, 0.3, 0.26])


MOVE_A = (torch.tensor([-0.55, -0.2, -0.1]), ec.rot_xyz(0.3, -0.2, 0.5))          # sets A down over the blob
COPY_A_DST = (torch.tensor([-0.42, 0.12, 0.08]), ec.rot_xyz(-0.25, 0.15, -0.4))   # and a turned copy of THAT beside it


def box_B():        # overlaps neither A nor where A is set down
    return ebox((0.05, 0.1, -0.2), [0.05, -0.53, -0.2], [-0.3, -0.13, -0.22], [0.28, 0.12, 0.25])


def box_C():        # around the blob's centre
    return ebox((0.2, 0.1, -0.3), [-0.05, 0.0, 0.05], [-0.3, -0.26, -0.24], [0.27, 0.3, 0.22])


def box_D():        # overlaps C in part
    return ebox((-0.1, 0.25, 0.2), [0.2, 0.15, -0.05], [-0.28, -0.25, -0.3], [0.3, 0.27, 0.21])


def spec_of_box(op, b):
    return epc.box_spec(op, b.axes, b.centre, b.lo, b.hi)


def rigid_spec(op, b, t, R):
    return ec.rigid_edit(op, T(b.axes), T(b.centre), T(b.lo), T(b.hi), t, R)


def chain_case():
    """[move(A, t, R), delete(B), copy(A_dst, t2, R2)] as an EditProgram and, independently, as a list of Spec."""
    from contrastive_lift_amd import edit
    A, B = box_A(), box_B()
    (t, R), (t2, R2) = MOVE_A, COPY_A_DST
    mv = edit.move(A, t, R)
    prog = edit.EditProgram([mv, edit.delete(B), edit.copy(mv.dst, t2, R2)])
    axes_d, centre_d = epc.moved_box(A.axes, A.centre, t.double().numpy(), R.double().numpy())     # A_dst from the motion, not from edit.py
    A_dst = edit.EditBox(axes_d, centre_d, A.lo, A.hi)
    specs = [rigid_spec("move", A, t, R), spec_of_box("delete", B), rigid_spec("copy", A_dst, t2, R2)]
    return prog, specs, (A, A_dst, B)


def order_case(first):
    """[copy(C, t), delete(C)] (``first`` = "copy") or [delete(C), copy(C, t)] (``first`` = "delete")."""
    from contrastive_lift_amd import edit
    Cb, t, R = box_C(), torch.tensor([0.45, -0.3, 0.1]), torch.eye(3)
    pair = [(edit.copy(Cb, t, R), rigid_spec("copy", Cb, t, R)), (edit.delete(Cb), spec_of_box("delete", Cb))]
    if first == "delete":
        pair.reverse()
    return edit.EditProgram([e for e, _ in pair]), [s for _, s in pair]


def small_boxes():
    """Eight small boxes inside the blob, turned differently."""
    out = []
    for i in range(8):
        c = [0.3 * np.cos(0.8 * i) - 0.05, 0.28 * np.sin(0.8 * i), 0.25 * np.cos(1.7 * i + 0.4)]
        out.append(ebox((0.1 * i, -0.07 * i, 0.23 * i), c, [-0.13, -0.12, -0.14], [0.12, 0.14, 0.13]))
    return out


def check_against_restatement(P, rays, mode, white, prog, specs, what, min_m=1000):
    """edit_forward under ``prog`` against render_program over ``specs`` at 1e-3 on sigma and the four outputs, over the kept rays."""
    from contrastive_lift_amd import engine
    cfg = cfg_of(mode)
    keep = epc.rays_off_all_faces(rays, cfg, prog)
    print(f"{what}: {int((~keep).sum())} of {rays.shape[0]} rays left out (a sample within 1e-5 of a box face)")
    ref, ref_sigma, hops = epc.render_program(P, rays, cfg, specs, white)
    o, ctx = engine.edit_forward(build_model(P, mode), build_renderer(mode), rays.to(DEV), prog, white)
    assert ctx.M > min_m
    rel_close(ctx.sigma.cpu()[keep], ref_sigma[keep], 1e-3, what=f"{what} sigma")
    for name, x, y in zip(NAMES, outputs(o), ref):
        rel_close(x.cpu()[keep], y[keep], 1e-3, what=f"{what} {name}")
    return o, ctx, hops


# ---------------------------------------------------------------------------- 1. a list of one is the single edit
@pytest.mark.parametrize("mlp_dtype", [None, "fp32"])
@pytest.mark.parametrize("op", ["delete", "extract", "duplicate", "manipulate", "copy", "move"])
def test_a_list_of_one_is_the_single_edit_bit_for_bit(scene130, g25, op, mlp_dtype):
    from contrastive_lift_amd import edit, engine
    if mlp_dtype is not None:
        engine.set_mlp_precision(mlp_dtype)
    P, _, rays = scene130
    bbox, t, R = ec.golden_bbox(g25), T(g25["translation"]), T(g25["rotation"])
    e = {"delete": lambda: edit.reference_delete(bbox), "extract": lambda: edit.reference_extract(bbox),
         "duplicate": lambda: edit.reference_duplicate(bbox, t, R), "manipulate": lambda: edit.reference_manipulate(bbox, t, R),
         "copy": lambda: edit.copy(box_A(), *MOVE_A), "move": lambda: edit.move(box_A(), *MOVE_A)}[op]()
    m, r = build_model(P, "softmax"), build_renderer("softmax")
    o1, c1 = engine.edit_forward(m, r, rays, e, True)
    o2, c2 = engine.edit_forward(m, r, rays, edit.EditProgram([e]), True)
    assert c1.M == c2.M > 300
    assert torch.equal(c1.sigma, c2.sigma) and torch.equal(c1.act_idx, c2.act_idx) and torch.equal(c1.xa, c2.xa)
    for name, a, b in zip(NAMES, outputs(o1), outputs(o2)):
        assert torch.equal(a, b), name
    if op in ("copy", "move"):                               # the remap is in play: the edit's sigma is not the plain one
        _, pctx = engine.render_forward(m, r, rays, None, True, grad_heads=())
        assert int((c2.sigma != pctx.sigma).sum()) > 100


# ---------------------------------------------------------------------------- 2. deletes compose exactly
def test_deletes_compose_to_the_minimum(scene130):
    from contrastive_lift_amd import edit, engine
    P, rays_cpu, rays = scene130
    m, r = build_model(P, "none"), build_renderer("none")
    sig = lambda e: engine.edit_forward(m, r, rays, e, False)[1].sigma
    Cb, Db = box_C(), box_D()
    pts, inbox = samples(rays_cpu, cfg_of("none"))
    in_c, in_d = Cb.contains(pts) & inbox, Db.contains(pts) & inbox
    assert in_c.sum() > 200 and in_d.sum() > 200                             # each box holds samples ...
    assert (in_c & in_d).sum() > 20 and (in_c & ~in_d).sum() > 50 and (in_d & ~in_c).sum() > 50       # ... and they overlap in part
    dC, dD = edit.delete(Cb), edit.delete(Db)
    sC, sD = sig(dC), sig(dD)
    want = torch.minimum(sC, sD)
    assert int((want != sC).sum()) > 20 and int((want != sD).sum()) > 20
    assert torch.equal(sig(edit.EditProgram([dC, dD])), want)
    assert torch.equal(sig(edit.EditProgram([dD, dC])), want)
    nowhere = edit.delete(ebox((0.1, 0.2, 0.3), [3.0, 3.0, 3.0], [-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]))      # disjoint from the aabb
    assert torch.equal(sig(edit.EditProgram([dC, nowhere, dD])), want)
    # at the maximum: eight deletes of small boxes
    eight = [edit.delete(b) for b in small_boxes()]
    assert len(eight) == edit.MAX_EDITS
    singles = [sig(e) for e in eight]
    plain = engine.render_forward(m, r, rays, None, False, grad_heads=())[1].sigma
    for s in singles:
        assert int((s != plain).sum()) > 5                                   # every one of the eight removes something
    want8 = functools.reduce(torch.minimum, singles)
    assert torch.equal(sig(edit.EditProgram(eight)), want8)


# ---------------------------------------------------------------------------- 3. chained remaps against the restatement
@pytest.mark.parametrize("mode,white", [("softmax", False), ("none", True)])
@pytest.mark.parametrize("which", ["golden", "rays130"])
def test_chained_remaps_match_the_restatement(g25, scene130, which, mode, white):
    P, rays = scene(which, g25, scene130)
    prog, specs, (A, A_dst, B) = chain_case()
    # fp64, on the host: B overlaps neither A nor A_dst; more than 100 in-aabb samples are remapped twice; remapped samples leave the aabb
    cloud = np.random.default_rng(5).uniform(-1.0, 1.0, (200000, 3))
    assert not (B.contains(cloud) & (A.contains(cloud) | A_dst.contains(cloud))).any()
    assert np.abs(prog[0].dst.axes - A_dst.axes).max() < 1e-12 and np.abs(prog[0].dst.centre - A_dst.centre).max() < 1e-12
    cfg = cfg_of(mode)
    pts, inbox = samples(rays, cfg)
    first = prog[2].dst.contains(pts)                                        # the walk starts at the last edit: the copy's destination box ...
    twice = first & prog[0].dst.contains(prog[2].source_points(pts))         # ... sends a sample into A_dst, which the move sends on into A
    assert (twice & inbox).sum() > 100
    looked_up, _ = prog.source_points(pts, np.zeros_like(pts))
    remapped = (np.abs(looked_up - pts).max(1) > 0) & inbox & ~prog.killed(pts)
    xn = orender.normalize(torch.from_numpy(looked_up[remapped]).float(), cfg)
    assert int((xn.abs() > 1).any(1).sum()) > 20
    o, ctx, hops = check_against_restatement(P, rays, mode, white, prog, specs, f"chain {which} {mode}")
    assert int((hops.reshape(-1).numpy() == 2)[inbox].sum()) > 100           # (the restatement walked them twice as well)
    if which == "rays130":
        miss = ~torch.from_numpy(inbox.reshape(rays.shape[0], -1)).any(1)
        assert int(miss.sum()) >= 8
        assert bool((o["rgb"].cpu()[miss] == (1.0 if white else 0.0)).all()) and bool((o["depth"].cpu()[miss] == 0).all())


# ---------------------------------------------------------------------------- 4. order matters
@pytest.mark.parametrize("which", ["golden", "rays130"])
def test_order_matters(g25, scene130, which):
    """[copy(C, t), delete(C)] keeps the copy (it was made before the original went); [delete(C), copy(C, t)] copies emptiness."""
    P, rays = scene(which, g25, scene130)
    depth = {}
    for first in ("copy", "delete"):
        prog, specs = order_case(first)
        o, ctx, _ = check_against_restatement(P, rays, "softmax", False, prog, specs, f"{first} first, {which}", min_m=300)
        depth[first] = o["depth"].cpu()
    assert float((depth["copy"] - depth["delete"]).abs().max()) > 0.05


# ---------------------------------------------------------------------------- 5. error paths through the raw ABI
def test_errors_through_the_raw_abi(scene130):
    from contrastive_lift_amd import _lib, edit, engine
    P, _, rays = scene130
    m, r = build_model(P, "none"), build_renderer("none")
    views = m.named_views()
    ms = engine.march_struct(r, m)
    vd = engine.vm_struct(views, "density", engine.grid_res(views))
    N = rays.shape[0]
    sigma = torch.full((N, int(r.n_samples)), -7.0, device=DEV)
    boxes = small_boxes()

    def run(recs, n):
        _lib.call("clift_edit_list_density_fwd", C.byref(ms), recs, n, C.byref(vd), _lib.ptr(rays), N, _lib.ptr(sigma), _lib.stream())

    nine = (_lib.EditRec * 9)(*([edit.delete(b).record() for b in boxes] + [edit.delete(boxes[0]).record()]))
    with pytest.raises(_lib.CliftError, match="n_edits = 0"):
        run(nine, 0)
    with pytest.raises(_lib.CliftError, match="n_edits = 9"):
        run(nine, 9)
    three = edit.EditProgram([edit.delete(b) for b in boxes[:3]]).records()
    three[2].map_t[1] = float("nan")
    with pytest.raises(_lib.CliftError, match=r"edit 2\b.*not finite"):
        run(three, 3)
    three[2].map_t[1] = 0.0
    three[1].mode = 7
    with pytest.raises(_lib.CliftError, match=r"edit 1\b.*unknown edit mode 7"):
        run(three, 3)
    torch.cuda.synchronize()
    assert bool((sigma == -7.0).all())                                       # nothing was launched
    three[1].mode = edit.DELETE
    run(three, 3)                                                            # ... and the mended program runs
    assert bool((sigma >= 0).all())


# ---------------------------------------------------------------------------- 6. chunked / sharded
def test_program_through_the_sharded_render(scene130):
    from contrastive_lift_amd import inference as inf
    P, _, rays = scene130
    m, r = build_model(P, "softmax"), build_renderer("softmax")
    prog, _, _ = chain_case()
    fn = functools.partial(inf.render_rays_edit, edit=prog)
    sharded = inf.render_rays_sharded(m, r, rays, 50, True, render_fn=fn)
    direct = inf.render_rays_edit(m, r, rays, 50, True, edit=prog)
    whole = inf.render_rays_edit(m, r, rays, 0, True, edit=prog)
    assert [tuple(x.shape) for x in sharded] == [(130, 3), (130, ec.C_CLS), (130, 2 * ec.E_INST), (130,)]
    for name, a, b, c in zip(NAMES, sharded, direct, whole):
        assert torch.equal(a, b), name
        rel_close(a.cpu(), c.cpu(), 1e-3, what=f"chunked against whole {name}")
    plain = inf.render_rays(m, r, rays, 50, True)
    assert float((plain[3] - sharded[3]).abs().max()) > 0.05                   # (the program shows in this frame)
