"""Meshes of an edited scene on the GPU: the edit-program walk over arbitrary points (clift_edit_list_points) and over the density lattice
(clift_edit_list_dense_sigma) against the fp64 walk of tests/edit_mesh_cases.py, their errors through the raw ABI,
``mesh.label_vertices(edit=)`` against the CPU oracle at the source points, and the invariants of the meshes inference/extract_mesh.py makes
of edited lattices.

Rows within 1e-5 of a box face at some stage of the walk are left out by the fp64 face rule (edit_mesh_cases); every test asserts its cap on
their number from the fp64 walk alone."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import edit_cases as ec
import edit_mesh_cases as emc
import mesh_cases as mc
from conftest import REPO, T, rel_close
from oracle import field as fld
from test_gpu_edit_program import box_C, ebox
from test_gpu_scene_edit import DEV, build_model, build_renderer

pytestmark = pytest.mark.gpu

KILLED, REMAPS = 0x80, 0x0f


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def scene():
    """scene130's field as a model with its renderer (no ray is used here)."""
    P, _ = ec.scene130()
    return P, build_model(P, "softmax"), build_renderer("softmax")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_edit_gpu", os.path.join(REPO, "inference", "extract_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ============================================================================ 1. the walker against the fp64 walk
@pytest.mark.parametrize("name", ["chain", "eight"])
def test_walker_against_the_fp64_walk(name):
    """Tolerances, from the arithmetic: a remap is 6 separately rounded fp32 ops per coordinate (3 products, 2 sums, the offset) on
    magnitudes <= 2.5 (positions within +-1.5, translations <= 1.5: asserted below), so <= 6 * 2^-24 * 2.5 = 9e-7 per coordinate and
    <= 1.6e-6 in 2-norm; the near-orthonormal M carries the error of earlier remaps at norm 1: 2e-6 per remap.  Directions: 5 ops on
    magnitudes <= 1: 3e-7 per coordinate, 6e-7 in 2-norm per remap."""
    prog = emc.program(name)
    pts, dirs = emc.cloud_points(4096)
    w = emc.ref_walk(prog, pts, dirs)
    keep = w["keep"]
    print(f"{name}: {int((~keep).sum())} of {pts.shape[0]} rows left out; remaps {np.bincount(w['hops']).tolist()}, killed {int(w['killed'].sum())}")
    assert int((~keep).sum()) <= 8
    assert np.abs(pts).max() <= 1.5 and np.abs(w["p"]).max() <= 1.5 and max(np.abs(e.t).max() for e in prog) <= 1.5
    assert (w["hops"] >= 2).sum() >= 5 and w["killed"].sum() >= 50
    dp, dd = T(pts).to(DEV), T(dirs).to(DEV)
    op_, od_, st_ = prog.apply_to_points(dp, dd)
    assert op_.shape == dp.shape and od_.shape == dd.shape and st_.shape == (pts.shape[0],) and st_.dtype == torch.uint8
    op, od, st = op_.cpu().numpy(), od_.cpu().numpy(), st_.cpu().numpy()
    assert np.array_equal(st[keep], w["state"][keep])
    still = (st & REMAPS) == 0                                             # killed rows that stopped unmoved included
    assert (still & ((st & KILLED) != 0)).sum() > 20
    assert np.array_equal(bits(op[still]), bits(pts[still])) and np.array_equal(bits(od[still]), bits(dirs[still]))
    moved = ~still & keep
    hops = (st & REMAPS).astype(np.float64)
    e_p, e_d = np.linalg.norm(op - w["p"], axis=1), np.linalg.norm(od - w["d"], axis=1)
    print(f"{name}: worst point error / remap {float((e_p[moved] / hops[moved]).max()):.3g}, direction {float((e_d[moved] / hops[moved]).max()):.3g}")
    assert (e_p[moved] <= 2e-6 * hops[moved]).all() and (e_d[moved] <= 6e-7 * hops[moved]).all()
    op2, od2, st2 = prog.apply_to_points(dp)                               # dirs = NULL: the same points
    assert od2 is None and torch.equal(op2, op_) and torch.equal(st2, st_)
    e0 = prog.apply_to_points(torch.empty((0, 3), device=DEV), torch.empty((0, 3), device=DEV))       # n = 0 returns cleanly
    assert e0[0].shape == (0, 3) and e0[1].shape == (0, 3) and e0[2].shape == (0,)
    torch.cuda.synchronize()


# ============================================================================ 2. the edited lattice
@pytest.mark.parametrize("name,upsample", [("chain", 1), ("chain", 2), ("eight", 3)])
def test_edited_lattice(scene, name, upsample):
    P, m, r = scene
    prog = emc.program(name)
    lp, n = emc.lattice_points(upsample)
    g = lp.reshape(n + (3,))
    for t, mine in zip(r.lattice_ticks(n), (g[:, 0, 0, 0], g[0, :, 0, 1], g[0, 0, :, 2])):       # the helper's points are the kernel's lattice
        assert np.array_equal(bits(t.cpu().numpy()), bits(mine))
    w = emc.ref_walk(prog, lp)
    keep = w["keep"]
    left = int((~keep).sum())
    print(f"{name} x{upsample}: {left} of {lp.shape[0]} lattice points left out")
    assert left <= (8 if name == "chain" else 0.002 * lp.shape[0])
    sigma, state = r.get_dense_sigma(m, upsample, edit=prog, return_state=True)
    plain = r.get_dense_sigma(m, upsample)
    assert tuple(sigma.shape) == tuple(state.shape) == n and state.dtype == torch.uint8
    st = state.reshape(-1).cpu().numpy()
    assert np.array_equal(st[keep], w["state"][keep])
    untouched = state.reshape(-1) == 0
    assert int(untouched.sum()) > lp.shape[0] // 2
    assert torch.equal(sigma.reshape(-1)[untouched], plain.reshape(-1)[untouched])
    killed = (st & KILLED) != 0
    sg = sigma.reshape(-1).cpu().numpy()
    assert (bits(sg[killed]) == 0).all()                                   # exactly +0.0
    remapped = ((st & REMAPS) > 0) & ~killed & keep
    print(f"{name} x{upsample}: {int(remapped.sum())} remapped and alive, {int((killed & keep).sum())} killed")
    assert remapped.sum() >= 100 and (killed & keep).sum() >= 100
    with torch.no_grad():
        ref = fld.density(P, T(emc.normalise64(w["p"][remapped])).float(), ec.SHIFT)
    rel_close(sg[remapped], ref, 1e-3, atol=1e-6, what=f"{name} x{upsample}: sigma at the remapped points")
    assert int((sigma != plain).sum()) >= 100
    again, state2 = r.get_dense_sigma(m, upsample, edit=prog, return_state=True)                       # two runs: the same bits
    assert torch.equal(again, sigma) and torch.equal(state2, state)
    assert torch.equal(r.get_dense_sigma(m, upsample, edit=prog), sigma)                               # state = NULL: the same sigma
    if name == "chain":                                                    # an Edit and a sequence are taken as edit_forward takes them
        assert torch.equal(r.get_dense_sigma(m, upsample, edit=list(prog)), sigma)
    s0, z0 = r.get_dense_sigma(m, upsample, return_state=True)
    assert torch.equal(s0, plain) and int(z0.count_nonzero()) == 0 and z0.shape == plain.shape


# ============================================================================ 3. errors through the raw ABI
def _bad_programs():
    from contrastive_lift_amd import _lib
    good = emc.program("chain").records()
    mode7 = emc.program("chain").records()
    mode7[1].mode = 7
    nan2 = emc.program("chain").records()
    nan2[2].dst.centre[1] = float("nan")
    nine = (_lib.EditRec * 9)(*([good[0]] * 9))
    return [("n_edits = 0", good, 0, "1 to 8"), ("n_edits = 9", nine, 9, "1 to 8"), ("mode 7", mode7, 3, "edit 1: unknown edit mode 7"),
            ("NaN in record 2", nan2, 3, "edit 2"), ("NULL output", good, 3, "NULL")]


def test_errors_of_the_point_walk():
    from contrastive_lift_amd import _lib
    pts = T(emc.cloud_points(256)[0]).to(DEV)
    out = torch.full_like(pts, -7.5)
    state = torch.full((256,), 0x55, dtype=torch.uint8, device=DEV)
    for what, recs, n_edits, msg in _bad_programs():
        with pytest.raises(_lib.CliftError, match=msg):
            _lib.call("clift_edit_list_points", recs, n_edits, _lib.ptr(pts), 3, None, 3, 256, None if what == "NULL output" else _lib.ptr(out), None,
                      _lib.ptr(state), _lib.stream())
        torch.cuda.synchronize()
        assert bool((out == -7.5).all()) and bool((state == 0x55).all()), what
    good = _bad_programs()[0][1]
    with pytest.raises(_lib.CliftError, match="ldp"):
        _lib.call("clift_edit_list_points", good, 3, _lib.ptr(pts), 2, None, 3, 256, _lib.ptr(out), None, None, _lib.stream())
    with pytest.raises(_lib.CliftError, match="out_dirs"):
        _lib.call("clift_edit_list_points", good, 3, _lib.ptr(pts), 3, _lib.ptr(pts), 3, 256, _lib.ptr(out), None, None, _lib.stream())
    assert bool((out == -7.5).all())


def test_errors_of_the_edited_lattice(scene):
    from contrastive_lift_amd import _lib, engine
    _, m, r = scene
    n = [int(x) for x in r.grid_dim.tolist()]
    ticks = [torch.linspace(0, 1, k).to(DEV) for k in n]
    views = m.named_views()
    vd = engine.vm_struct(views, "density", engine.grid_res(views))
    lo, hi = r.bbox_aabb_host
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    out = torch.full(tuple(n), -7.5, device=DEV)
    state = torch.full(tuple(n), 0x55, dtype=torch.uint8, device=DEV)

    def run(recs, n_edits, o, n0=n[0]):
        _lib.call("clift_edit_list_dense_sigma", C.byref(vd), recs, n_edits, f3(lo), f3(hi), f3(r.inv_box_extent_host), _lib.ptr(ticks[0]),
                  _lib.ptr(ticks[1]), _lib.ptr(ticks[2]), n0, n[1], n[2], float(m.splus_density_shift), o, _lib.ptr(state), _lib.stream())
    for what, recs, n_edits, msg in _bad_programs():
        with pytest.raises(_lib.CliftError, match=msg):
            run(recs, n_edits, None if what == "NULL output" else _lib.ptr(out))
        torch.cuda.synchronize()
        assert bool((out == -7.5).all()) and bool((state == 0x55).all()), what
    with pytest.raises(_lib.CliftError, match="positive"):                   # clift_dense_sigma's own errors are kept
        run(_bad_programs()[0][1], 3, _lib.ptr(out), n0=0)
    assert bool((out == -7.5).all())
    run(_bad_programs()[0][1], 3, _lib.ptr(out))                            # and the good call does write
    assert torch.equal(out, r.get_dense_sigma(m, 1, edit=emc.program("chain")))


# ============================================================================ 4. label_vertices under an edit
def sphere_program():
    """Four edits whose boxes cut the sphere of radius 0.45: a cap moved to the other side, a turned copy of a second cap, a third cap
    deleted, and a copy of the moved cap (two remaps)."""
    from contrastive_lift_amd import edit
    bx = ebox((0.1, -0.1, 0.2), [0.35, 0.0, 0.0], [-0.2, -0.3, -0.3], [0.2, 0.3, 0.3])
    by = ebox((0.0, 0.2, -0.1), [0.0, 0.35, 0.05], [-0.25, -0.15, -0.25], [0.25, 0.2, 0.25])
    bz = ebox((0.1, 0.0, 0.0), [0.0, 0.0, 0.42], [-0.2, -0.2, -0.12], [0.2, 0.2, 0.15])
    mv = edit.move(bx, [-0.7, 0.02, 0.03], ec.rot_xyz(0.2, -0.1, 0.3))
    return edit.EditProgram([mv, edit.copy(by, [0.03, -0.72, -0.1], ec.rot_xyz(-0.2, 0.1, 0.25)), edit.delete(bz),
                             edit.copy(mv.dst, [0.3, 0.45, -0.25], ec.rot_xyz(0.1, 0.3, -0.2))])


def test_label_vertices_under_an_edit():
    """The model and the vertices of test_gpu_mesh.test_label_vertices_against_oracle; every vertex is held to the oracle AT ITS fp64 SOURCE
    POINT (its own position where no edit remaps it) under that test's near-tie rule, the colour along the turned normal."""
    import contrastive_lift_amd as cl
    import test_gpu_mesh as tgm
    from contrastive_lift_amd import mesh
    from oracle import params as op
    verts, _, normals, _ = tgm.gpu_mesh(mc.sphere_case())
    res, C_, E = (9, 13, 17), 4, 3
    aabb = torch.tensor([[-1.0, -0.8, -0.6], [1.0, 0.8, 0.6]])
    P = op.make_params(tgm.MODEL_SEED, res, C_, E)
    m = tgm.build_model(P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    prog = sphere_program()
    w = emc.ref_walk(prog, verts, -normals)
    V, keep = verts.shape[0], w["keep"]
    assert int((~keep).sum()) <= 8
    dv, dn = T(verts).to(DEV), T(normals).to(DEV)
    st = prog.apply_to_points(dv, -dn)[2].cpu().numpy()
    assert np.array_equal(st[keep], w["state"][keep])
    remapped = ((st & REMAPS) > 0) & keep
    print(f"{V} vertices: remaps {np.bincount(w['hops']).tolist()}, {int(w['killed'].sum())} killed, {int((~keep).sum())} left out")
    assert remapped.sum() >= 50 and ((st & REMAPS) == 2).sum() >= 10
    sem0, inst0, rgb0 = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3))
    sem, inst, rgb = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3), edit=prog)
    same = torch.from_numpy(st == 0).to(DEV)                               # rows the program does not touch: today's bits
    assert int(same.sum()) > 100
    assert torch.equal(sem[same], sem0[same]) and torch.equal(inst[same], inst0[same]) and torch.equal(rgb[same], rgb0[same])
    assert not torch.equal(rgb, rgb0)
    o_sem, o_inst, o_rgb = tgm.oracle_labels(P, aabb, w["p"].astype(np.float32), (-w["d"]).astype(np.float32), E)      # view = the turned -normal
    sem_ok, inst_ok = tgm.top_two_gap(o_sem) >= tgm.TIE_GAP, tgm.top_two_gap(o_inst) >= tgm.TIE_GAP
    print(f"left out as near ties: {int((~sem_ok).sum())} classes, {int((~inst_ok).sum())} ids of {V}")
    assert (~sem_ok).sum() <= tgm.TIE_SHARE * V and (~inst_ok).sum() <= tgm.TIE_SHARE * V
    exp_sem, exp_inst = o_sem.argmax(1).numpy(), o_inst.argmax(1).numpy()
    u_sem, u_inst, _ = tgm.oracle_labels(P, aabb, verts, normals, E)      # the same vertices without the edit: the edit must change labels
    assert (exp_sem != u_sem.argmax(1).numpy()).sum() >= 10 and (exp_inst != u_inst.argmax(1).numpy()).sum() >= 10
    assert len(np.unique(exp_inst[remapped])) > 1
    assert np.array_equal(sem.cpu().numpy()[sem_ok & keep], exp_sem[sem_ok & keep])
    assert np.array_equal(inst.cpu().numpy()[inst_ok & keep], exp_inst[inst_ok & keep])
    rel_close(rgb.cpu()[torch.from_numpy(keep)], o_rgb[torch.from_numpy(keep)], 1e-3, what="vertex rgb under the edit")
    s2, i2, c2 = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3), chunk=100, edit=prog)         # chunking changes nothing
    assert torch.equal(s2, sem) and torch.equal(i2, inst) and torch.equal(c2, rgb)
    # cached centroids: a remapped vertex gets the id the oracle assigns at its source (the numbering of test_label_vertices_against_oracle)
    rng = np.random.default_rng(30)
    scale = float(u_inst.abs().max())
    cents = {c: (rng.standard_normal((k, E)) * scale).astype(np.float32) for c, k in ((2, 3), (3, 2))}
    exp, ok, nxt = np.zeros(V, np.int64), sem_ok & keep, 0
    for c in sorted(set(exp_sem[np.isin(exp_sem, (2, 3))].tolist())):
        sel = exp_sem == c
        d = torch.cdist(o_inst[sel].double(), T(cents[c]).double())
        exp[sel] = d.argmin(1).numpy() + nxt + 1
        ok[sel] &= tgm.top_two_gap(-d) >= tgm.TIE_GAP
        nxt = int(exp[sel].max())
    assert (~ok).sum() <= tgm.TIE_SHARE * V + int((~keep).sum()), int((~ok).sum())
    s3, i3, _ = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3), centroids=cents, edit=prog)
    assert torch.equal(s3, sem)
    assert np.array_equal(i3.cpu().numpy()[ok], exp[ok]) and (ok & remapped).sum() >= 50
    assert len(np.unique(exp[ok & remapped])) > 1


# ============================================================================ 5. invariants of the edited meshes
# scene130's lattice at upsample 2 is (18, 26, 34); sigma runs from 0.05 to 13.7 and the level 3 surface of the blob has about 1900 vertices, 700
# of them inside box C.  The heads of make_params are nearly flat: every point of this field has class 0, which is therefore the thing class
# here, so that the ids are not all "stuff".  The chain program sets box A down over the blob: its test takes the level 0.5 surface (about 3500
# vertices), most of which lies away from every box.
LEVEL, LEVEL_WIDE, UP, THINGS = 3.0, 0.5, 2, (0,)


def stages(cli, scene, edit, level=LEVEL, **kw):
    """(the dict of surface_stages, lattice state, keys of the vertices) of the scene130 model under ``edit`` (None: unedited)."""
    from contrastive_lift_amd import mesh
    _, m, r = scene
    sigma, state = r.get_dense_sigma(m, UP, edit=edit, return_state=True)
    out = cli.surface_stages(m, r, sigma, level, THINGS, None, False, cli.StageTimer(), edit=edit, **kw)
    v, f, nrm, keys = mesh.extract_isosurface(out["sigma"], level, r.lattice_ticks(sigma.shape), return_keys=True)
    assert torch.equal(v, out["verts"]) and torch.equal(f, out["faces"])
    assert out["verts"].shape[0] > 500
    return out, state, keys


@pytest.fixture(scope="module")
def unedited(cli, scene):
    return {level: stages(cli, scene, None, level) for level in (LEVEL, LEVEL_WIDE)}


def test_mesh_of_the_chain_program(cli, scene, unedited):
    """Consistently wound; and every active edge the edited and the unedited mesh share whose two endpoints no edit touches carries a
    vertex with the same position bits.  Class and id of such a vertex are equal where the vertex itself is untouched.  The colour is seen
    along minus the NORMAL, a central difference of the lattice over the endpoints' neighbours: it is equal wherever the normal is, and the
    normal is equal wherever those neighbours are untouched too (both asserted)."""
    prog = emc.program("chain")
    me, state, ke = stages(cli, scene, prog, LEVEL_WIDE)
    mu, _, ku = unedited[LEVEL_WIDE]
    assert mc.closed_oriented(me["faces"].cpu().numpy())[0]
    n0, n1, n2 = (int(x) for x in state.shape)
    st = state.reshape(-1).cpu().numpy()
    ke_, ku_ = ke.cpu().numpy(), ku.cpu().numpy()
    common, ie, iu = np.intersect1d(ke_, ku_, return_indices=True)
    owner, cls = common // 7, common % 7
    off = np.asarray(mc.CLASS_OFFSETS, np.int64)[cls]
    other = owner + (off[:, 0] * n1 + off[:, 1]) * n2 + off[:, 2]
    free = (st[owner] == 0) & (st[other] == 0)
    assert free.sum() > 300 and (~free).sum() >= 20 and ke_.shape[0] != ku_.shape[0]
    ve, vu = me["verts"].cpu().numpy()[ie[free]], mu["verts"].cpu().numpy()[iu[free]]
    assert np.array_equal(bits(ve), bits(vu))
    vstate = prog.apply_to_points(me["verts"], -me["normals"])[2].cpu().numpy()[ie[free]]
    own = vstate == 0
    assert own.sum() > 300
    for k in ("sem", "inst"):
        assert np.array_equal(me[k].cpu().numpy()[ie[free]][own], mu[k].cpu().numpy()[iu[free]][own]), k
    ne, nu = bits(me["normals"].cpu().numpy()[ie[free]]), bits(mu["normals"].cpu().numpy()[iu[free]])
    same_normal = (ne == nu).all(1)
    ce, cu = bits(me["rgb"].cpu().numpy()[ie[free]]), bits(mu["rgb"].cpu().numpy()[iu[free]])
    assert np.array_equal(ce[own & same_normal], cu[own & same_normal])
    idx = np.stack(np.unravel_index(np.concatenate([owner[free], other[free]]), (n0, n1, n2)), 1)      # the normals' stencil: +-1 per axis, clamped
    quiet = np.ones(idx.shape[0], bool)
    st3 = st.reshape(n0, n1, n2)
    for ax, size in enumerate((n0, n1, n2)):
        for step in (-1, 1):
            j = idx.copy()
            j[:, ax] = np.clip(j[:, ax] + step, 0, size - 1)
            quiet &= st3[j[:, 0], j[:, 1], j[:, 2]] == 0
    quiet = quiet[:free.sum()] & quiet[free.sum():]
    assert (quiet & own).sum() > 200 and same_normal[quiet].all()


def test_mesh_under_delete_and_extract(cli, scene):
    """A vertex sits on a lattice edge between an inside and an outside endpoint.  Under delete(C) the inside endpoint is alive, hence
    outside C: no vertex lies deeper inside C than one cell diagonal.  Under extract(C) it is inside C: every vertex lies within C grown
    by one cell diagonal."""
    from contrastive_lift_amd import edit
    Cb = box_C()
    diag = emc.cell_diagonal([r_ * UP for r_ in ec.RES])
    md, _, _ = stages(cli, scene, edit.delete(Cb))
    depth = emc.box_depth(Cb, md["verts"].cpu().numpy())
    print(f"delete: deepest vertex {depth.max():.4f} inside C, cell diagonal {diag:.4f}")
    assert depth.max() <= diag + 1e-5 and (depth > 0).sum() > 20            # the cap of the hole is there
    assert mc.closed_oriented(md["faces"].cpu().numpy())[0]
    mx, _, _ = stages(cli, scene, edit.extract(Cb))
    depth = emc.box_depth(Cb, mx["verts"].cpu().numpy())
    print(f"extract: farthest vertex {-depth.min():.4f} outside C")
    assert depth.min() >= -(diag + 1e-5)
    assert mc.closed_oriented(mx["faces"].cpu().numpy())[0]
    mf, _, _ = stages(cli, scene, edit.extract(Cb), min_component=8)
    assert mf["info"] is not None and mc.closed_oriented(mf["faces"].cpu().numpy())[0]
    assert emc.box_depth(Cb, mf["verts"].cpu().numpy()).min() >= -(diag + 1e-5)


def test_mesh_under_move_keeps_the_ids(cli, scene, unedited):
    """move(C, t) with --split_disconnected: the ids of the vertices inside the destination box are ids the unedited mesh carries inside C
    (a piece that the split renumbers is taken back to the id it was split from: ``table`` maps fresh ids to their parents)."""
    from contrastive_lift_amd import edit
    Cb = box_C()
    mv = edit.move(Cb, [0.45, -0.3, 0.1], ec.rot_xyz(0.0, 0.0, 0.3))
    mm, _, _ = stages(cli, scene, mv, split_disconnected=1)
    mu, _, _ = unedited[LEVEL]
    assert mm["table"] is not None and mc.closed_oriented(mm["faces"].cpu().numpy())[0]
    inside_dst = emc.box_depth(mv.dst, mm["verts"].cpu().numpy()) > 1e-5
    inside_src = emc.box_depth(Cb, mu["verts"].cpu().numpy()) > 1e-5
    assert inside_dst.sum() > 100 and inside_src.sum() > 100
    table = {int(k): int(v) for k, v in mm["table"].items()}
    got_raw = set(mm["inst"].cpu().numpy()[inside_dst].tolist())
    got = set()
    for i in got_raw:
        while i in table:
            i = table[i]
        got.add(i)
    have = set(mu["inst"].cpu().numpy()[inside_src].tolist())
    print(f"ids inside the destination box {sorted(got_raw)} (parents {sorted(got)}), inside C before the move {sorted(have)}")
    assert got <= have and len(got - {0}) >= 1 and (mu["inst"] > 0).any()
