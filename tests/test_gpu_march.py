"""Every entry point of csrc/march.hip against the references of tests/march_cases.py, called through _lib.call with raw pointers and the
ctypes March / VM / VMGrad structs as engine.py builds them; the engine's own struct builders and density_points get a case each.

A device result is held to |device - fp64| <= 8 * yardstick + 4 * 2^-24 * scale (loss_cases.bound; march_cases.WIDENED would list what needs
more).  Integers (n_active, ray_start, act_idx, the alpha box), tmin, zeros outside the box and untouched gradient texels are compared
exactly.  Each test prints the worst ``yardstick | device error | bound`` row per quantity."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import march_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _L():
    from contrastive_lift_amd import _lib
    _lib.load()
    return _lib


def _d(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


class Table:
    """Rows of ``yardstick | device error | bound``; ``hold`` records a row and remembers a break; ``close`` prints the worst row of each
    (kernel, quantity, call) and every break.  ``cases``: the case module whose references and bounds apply."""

    def __init__(self, cases=mc):
        self.rows, self.broken, self.cases = {}, [], cases

    def hold(self, case, q, dev, how="raw"):
        mc = self.cases
        yard, err, bnd = mc.yardstick(case, q), mc.max_error(dev, mc.reference(case)[q]), mc.bound_for(case, q)
        row = f"{case.kernel:7s} {case.name:34s} {q:8s} {how:12s} | {yard:9.3e} | {err:9.3e} | {bnd:9.3e}"
        key, ratio = (case.kernel, q, how), (err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf")))
        if key not in self.rows or not ratio <= self.rows[key][0]:
            self.rows[key] = (ratio, row)
        if mc.exceeds(err, bnd):
            self.broken.append(row)

    def fail(self, case, what):
        self.broken.append(f"{case}: {what}")

    def close(self, capsys):
        with capsys.disabled():
            print("\nkernel  worst case                         what     call         | yardstick | dev error | bound\n" + "\n".join(r for _, r in self.rows.values()))
        assert not self.broken, "outside the bound, or not exact:\n" + "\n".join(self.broken)


def _march_struct(L, c):
    m = L.March()
    for i in range(3):
        m.lo[i], m.hi[i], m.inv_ext2[i] = float(c.lo[i]), float(c.hi[i]), float(c.inv2[i])
    m.step_size, m.n_samples, m.distance_scale = c.step, c.S, getattr(c, "dist_scale", 1.0)
    m.density_shift, m.weight_thres = c.shift, getattr(c, "thres", 0.0)
    return m


def _vm(L, c):
    """(VM struct, the device tables it points to): channels-last planes [res[b]][res[a]][C] and lines [res[v]][C]."""
    tabs = [_d(p) for p in c.plane] + [_d(p) for p in c.line]
    v = L.VM()
    for i in range(3):
        v.plane[i], v.line[i], v.res[i] = tabs[i].data_ptr(), tabs[3 + i].data_ptr(), c.res[i]
    v.comps = c.comps
    return v, tabs


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ---------------------------------------------------------------------------------------------------------------- density forward
def _density_fwd(L, c, thread_form):
    from contrastive_lift_amd import engine
    m, (v, tabs) = _march_struct(L, c), _vm(L, c)
    rays, jit = _d(c.rays), _d(c.jitter)
    sigma = torch.full((c.N, c.S), float(SENTINEL), device=DEV)
    with engine.kernel_switches(dens_fwd_thread=thread_form):
        L.call("clift_density_fwd", C.byref(m), C.byref(v), L.ptr(rays), L.ptr(jit), c.N, L.ptr(sigma), L.stream())
    return sigma.cpu()


def test_density_fwd_both_forms(capsys):
    L, t = _L(), Table()
    for c in mc.march_cases():
        mask = torch.from_numpy(mc.geometry(c).mask)
        got = {form: _density_fwd(L, c, form) for form in (False, True)}
        if not torch.equal(got[False].view(torch.int32), got[True].view(torch.int32)):
            t.fail(c, "the per-ray and the per-thread form differ in some bit")
        for form, s in got.items():
            t.hold(c, "sigma", s, "thread" if form else "ray")
            if float(s[~mask].abs().max() if (~mask).any() else 0.0) != 0.0:
                t.fail(c, f"form {form}: sigma outside the box is not exactly 0")
    t.close(capsys)


def test_density_sweep_is_one_body_for_the_march_and_the_edits():
    """k_density_fwd_ray and the edit density kernel run ONE sweep body (csrc/density_sweep_dev.h), and a single edit is a program of one.  At
    every march case (S < 64, S no multiple of 64, N * ceil(S / 64) no multiple of a block's four waves, rays that miss the box), without
    jitter and under a DELETE whose box no sample of the scene can reach: the plain pass in both forms, the single-edit entry point and the
    program entry point with the edit once and eight times give the same bits, and none writes past row N.  Then, over the in-box samples:
    clift_active_xyz, clift_edit_active and clift_edit_list_active give the same positions, and the view directions come back untouched."""
    from contrastive_lift_amd import edit, engine
    L, broken = _L(), []
    for c in mc.march_cases():
        ext = np.asarray(c.hi, np.float64) - np.asarray(c.lo, np.float64)
        far = edit.Edit(edit.DELETE, edit.EditBox(np.eye(3), np.asarray(c.hi, np.float64) + 64.0 * ext, -0.5 * np.ones(3), 0.5 * np.ones(3)))
        one, eight = far.record(), (L.EditRec * 8)(*(far.record() for _ in range(8)))
        m, (v, tabs), rays = _march_struct(L, c), _vm(L, c), _d(c.rays)
        sig = {k: torch.full((c.N + 1, c.S), float(SENTINEL), device=DEV) for k in ("ray", "thread", "edit", "list1", "list8")}
        for form in (False, True):
            with engine.kernel_switches(dens_fwd_thread=form):
                L.call("clift_density_fwd", C.byref(m), C.byref(v), L.ptr(rays), None, c.N, L.ptr(sig["thread" if form else "ray"]), L.stream())
        L.call("clift_edit_density_fwd", C.byref(m), C.byref(one), C.byref(v), L.ptr(rays), c.N, L.ptr(sig["edit"]), L.stream())
        L.call("clift_edit_list_density_fwd", C.byref(m), C.byref(one), 1, C.byref(v), L.ptr(rays), c.N, L.ptr(sig["list1"]), L.stream())
        L.call("clift_edit_list_density_fwd", C.byref(m), eight, 8, C.byref(v), L.ptr(rays), c.N, L.ptr(sig["list8"]), L.stream())
        sig = {k: s.cpu() for k, s in sig.items()}
        for k, s in sig.items():
            if not torch.equal(s[:c.N].view(torch.int32), sig["ray"][:c.N].view(torch.int32)):
                broken.append(f"{c.name}: sigma of '{k}' differs from the ray form in some bit")
            if not bool((s[c.N] == SENTINEL).all()):
                broken.append(f"{c.name}: '{k}' wrote past row N")

        act_np = np.flatnonzero(mc.geometry(c).mask.reshape(-1)).astype(np.int32)          # row-major: sid = r * S + k
        if act_np.size == 0:
            continue
        M, act = int(act_np.size), _d(act_np, torch.int32)
        xa = {k: torch.full((M, 4), float(SENTINEL), device=DEV) for k in ("plain", "edit", "list1")}
        dirs = {k: torch.full((M, 4), float(SENTINEL), device=DEV) for k in ("edit", "list1")}
        L.call("clift_active_xyz", C.byref(m), L.ptr(rays), None, L.ptr(act), M, L.ptr(xa["plain"]), L.stream())
        L.call("clift_edit_active", C.byref(m), C.byref(one), L.ptr(rays), L.ptr(act), M, L.ptr(xa["edit"]), L.ptr(dirs["edit"]), L.stream())
        L.call("clift_edit_list_active", C.byref(m), C.byref(one), 1, L.ptr(rays), L.ptr(act), M, L.ptr(xa["list1"]), L.ptr(dirs["list1"]), L.stream())
        want_d = torch.from_numpy(np.ascontiguousarray(c.rays[act_np // c.S, 3:6])).view(torch.int32)
        for k in ("edit", "list1"):
            if not torch.equal(xa[k].cpu().view(torch.int32), xa["plain"].cpu().view(torch.int32)):
                broken.append(f"{c.name}: xa of '{k}' differs from clift_active_xyz in some bit")
            d = dirs[k].cpu()
            if not torch.equal(d[:, :3].contiguous().view(torch.int32), want_d):
                broken.append(f"{c.name}: dirs[:, :3] of '{k}' are not the ray directions")
            if not bool((d[:, 3] == 0).all()):
                broken.append(f"{c.name}: dirs[:, 3] of '{k}' is not 0")
    assert not broken, "not bit for bit:\n" + "\n".join(broken)


def test_density_points(capsys):
    L, t = _L(), Table()
    for c in mc.points_cases():
        v, tabs = _vm(L, c)
        x = torch.full((c.n, c.ldx), float(SENTINEL), device=DEV)
        x[:, :3] = _d(c.xn)
        for act, q in ((1, "sigma"), (0, "raw")):
            out = torch.full((c.n + 8,), float(SENTINEL), device=DEV)
            L.call("clift_density_points", C.byref(v), L.ptr(x), c.ldx, c.n, c.shift, act, L.ptr(out), L.stream())
            t.hold(c, q, out[:c.n].cpu())
            if not bool((out[c.n:] == SENTINEL).all()):
                t.fail(c, "wrote past n")
    t.close(capsys)


def test_alpha_bbox(capsys):
    L, t = _L(), Table()
    for c in mc.bbox_cases():
        v, tabs = _vm(L, c)
        ticks = [_d(s) for s in c.ticks]
        n = int(np.prod(c.dims))
        alpha = torch.full((n + 8,), float(SENTINEL), device=DEV)
        box = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
        L.call("clift_alpha_bbox", C.byref(v), _f3(c.lo), _f3(c.hi), _f3(c.inv2), L.ptr(ticks[0]), L.ptr(ticks[1]), L.ptr(ticks[2]), c.dims[0], c.dims[1],
               c.dims[2], c.shift, c.step, c.thr, L.ptr(alpha), L.ptr(box), L.stream())
        a = alpha.cpu()
        t.hold(c, "alpha", a[:n])
        want = mc.pool_box(mc.reference(c)["alpha"].numpy(), c.dims, c.thr)[1]
        own = mc.pool_box(a[:n].numpy(), c.dims, np.float32(c.thr))[1]           # the pool and the reduction alone, on the device's own alpha
        if box.cpu().tolist() != want + [SENTINEL] or own != want:
            t.fail(c, f"box {box.cpu().tolist()} / pooled from the device's alpha {own} / reference {want}")
        if not bool((a[n:] == SENTINEL).all()):
            t.fail(c, "wrote past the lattice")
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- transmittance
RAY_OUT = ("opacity", "depth", "Tlast", "Wsum", "WMsum", "dist")


def _march_fwd(L, c, sigma):
    m, rays, jit = _march_struct(L, c), _d(c.rays), _d(c.jitter)
    outs = [torch.full((c.N, c.S), float(SENTINEL), device=DEV) for _ in range(3)]
    ray_out = torch.full((c.N, 8), float(SENTINEL), device=DEV)
    n_act = torch.full((c.N,), SENTINEL, dtype=torch.int32, device=DEV)
    L.call("clift_march_fwd", C.byref(m), L.ptr(rays), L.ptr(jit), c.N, L.ptr(sigma), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(ray_out),
           L.ptr(n_act), L.stream())
    return outs[0], outs[1], outs[2], ray_out, n_act


def test_march_fwd(capsys):
    L, t = _L(), Table()
    for c in mc.march_cases():
        ref, g = mc.reference(c), mc.geometry(c)
        alpha, T, w, ray_out, n_act = _march_fwd(L, c, _d(ref["sigma"].float().numpy()))
        got = {"alpha": alpha.cpu(), "T": T.cpu(), "w": w.cpu()}
        got.update({q: ray_out[:, j].cpu() for j, q in enumerate(RAY_OUT)})
        for q in mc.checked(c):
            if q in got:
                t.hold(c, q, got[q])
        if c.only is None:
            if not np.array_equal(ray_out[:, 6].cpu().numpy(), g.tmin) or float(ray_out[:, 7].abs().max()) != 0.0:
                t.fail(c, "ray_out[6] is not the fp32 tmin, or ray_out[7] not 0")
            if not torch.equal(n_act.cpu(), mc.extras(c)["n_active"]):
                t.fail(c, "n_active")
    t.close(capsys)


def test_march_bwd(capsys):
    L, t = _L(), Table()
    for c in mc.march_cases():
        if "dsigma" not in mc.checked(c):
            continue
        ref = mc.reference(c)
        m, rays, jit = _march_struct(L, c), _d(c.rays), _d(c.jitter)
        g_w = _d(c.g_w) if "w" in c.cots else None
        g_op = _d(c.g_op) if "op" in c.cots else None
        g_d = torch.full((1,), c.g_dist, device=DEV) if "dist" in c.cots else None
        own = _march_fwd(L, c, _d(ref["sigma"].float().numpy()))[:4]
        ro = torch.zeros((c.N, 8))
        ro[:, 3], ro[:, 4] = ref["Wsum"].float(), ref["WMsum"].float()
        rounded = tuple(_d(ref[q].float().numpy()) for q in ("alpha", "T", "w")) + (ro.to(DEV),)
        for how, (alpha, T, w, ray_out) in (("own_forward", own), ("ref_forward", rounded)):
            ds = torch.full((c.N, c.S), float(SENTINEL), device=DEV)
            L.call("clift_march_bwd", C.byref(m), L.ptr(rays), L.ptr(jit), c.N, L.ptr(alpha), L.ptr(T), L.ptr(w), L.ptr(ray_out), L.ptr(g_w), L.ptr(g_op),
                   L.ptr(g_d), L.ptr(ds), L.stream())
            t.hold(c, "dsigma", ds.cpu(), how)
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- scan and compaction
def test_scan_counts():
    L = _L()
    for c in mc.scan_cases():
        cnt = _d(c.cnt, torch.int32)
        start = torch.full((c.N + 9,), SENTINEL, dtype=torch.int32, device=DEV)
        L.call("clift_scan_counts", L.ptr(cnt), c.N, L.ptr(start), L.stream())
        want = mc.scan_reference(c.cnt)[0]
        assert np.array_equal(start[:c.N + 1].cpu().numpy(), want) and bool((start[c.N + 1:] == SENTINEL).all()), c
        for cap in c.caps:
            for over in c.overflows:
                start.fill_(SENTINEL)
                limit = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
                overflow = torch.full((1,), over, dtype=torch.int32, device=DEV)
                L.call("clift_scan_counts_capped", L.ptr(cnt), c.N, L.ptr(start), cap, L.ptr(limit), L.ptr(overflow), L.stream())
                ws, wl, wo = mc.scan_reference(c.cnt, cap, over)
                assert np.array_equal(start[:c.N + 1].cpu().numpy(), ws) and bool((start[c.N + 1:] == SENTINEL).all()), (c, cap)
                assert int(limit) == wl and int(overflow) == wo, (c, cap, over, int(limit), int(overflow))
    with pytest.raises(L.CliftError):
        L.call("clift_scan_counts", None, -1, None, L.stream())


def test_compact_fill():
    L = _L()
    for c in mc.compact_cases():
        w = _d(c.w)
        n_act, ids = mc.compact_reference(c)
        assert c.S == 1 or bool((c.w == np.float32(c.thres)).any()), "a weight equal to the threshold (not active)"
        start = _d(mc.scan_reference(n_act)[0], torch.int32)
        act = torch.full((c.total + 64,), SENTINEL, dtype=torch.int32, device=DEV)
        L.call("clift_compact_fill", L.ptr(w), L.ptr(start), c.N, c.S, c.thres, L.ptr(act), L.stream())
        assert np.array_equal(act[:c.total].cpu().numpy(), ids) and bool((act[c.total:] == SENTINEL).all()), c
        for cap in c.caps:
            start = _d(mc.scan_reference(n_act, cap)[0], torch.int32)
            act = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device=DEV)
            L.call("clift_compact_fill_capped", L.ptr(w), L.ptr(start), c.N, c.S, c.thres, L.ptr(act), cap, L.stream())
            k = min(c.total, cap)
            assert np.array_equal(act[:k].cpu().numpy(), ids[:k]) and bool((act[k:] == SENTINEL).all()), (c, cap)


def test_compaction_of_the_march_cases():
    """n_active of the device's own march, scanned and compacted: ray_start and act_idx are the reference's, exactly."""
    L = _L()
    for c in mc.march_cases():
        if c.only is not None:
            continue
        ref = mc.reference(c)
        _, _, w, _, n_act = _march_fwd(L, c, _d(ref["sigma"].float().numpy()))
        start = torch.full((c.N + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        L.call("clift_scan_counts", L.ptr(n_act), c.N, L.ptr(start), L.stream())
        on = ref["w"].numpy() > float(np.float32(c.thres))
        ids = np.nonzero(on.reshape(-1))[0].astype(np.int32)
        assert np.array_equal(start.cpu().numpy(), mc.scan_reference(on.sum(1))[0]), c
        act = torch.full((ids.size + 64,), SENTINEL, dtype=torch.int32, device=DEV)
        L.call("clift_compact_fill", L.ptr(w), L.ptr(start), c.N, c.S, c.thres, L.ptr(act), L.stream())
        assert np.array_equal(act[:ids.size].cpu().numpy(), ids) and bool((act[ids.size:] == SENTINEL).all()), c


# ---------------------------------------------------------------------------------------------------------------- density backward
GRADS = ("gp0", "gp1", "gp2", "gl0", "gl1", "gl2")


def _density_bwd(L, c, walk_switch, xcd, with_sigma):
    """The six gradient tensors after clift_density_bwd on top of the pre-fill: straight into them (xcd_stride = 0), or into eight zeroed
    accumulation copies that clift_xcd_reduce folds onto the pre-fill."""
    from contrastive_lift_amd import engine
    ref = mc.reference(c)
    m, (v, tabs) = _march_struct(L, c), _vm(L, c)
    rays, jit, ds = _d(c.rays), _d(c.jitter), _d(c.ds_in)
    sigma = _d(ref["sigma"].float().numpy()) if with_sigma else None
    pre = list(c.prefill_plane) + list(c.prefill_line)
    sizes = [p.size for p in pre]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1])
    dst = _d(np.concatenate([p.reshape(-1) for p in pre]))
    work = torch.zeros((8 * n,), device=DEV) if xcd else None
    g = L.VMGrad()
    base = (work if xcd else dst).data_ptr()
    for i in range(3):
        g.plane[i], g.line[i] = base + 4 * int(offs[i]), base + 4 * int(offs[3 + i])
    g.xcd_stride = n if xcd else 0
    with engine.kernel_switches(dens_scatter_walk=walk_switch):
        L.call("clift_density_bwd", C.byref(m), C.byref(v), C.byref(g), L.ptr(rays), L.ptr(jit), c.N, L.ptr(ds), L.ptr(sigma), L.stream())
    if xcd:
        L.call("clift_xcd_reduce", L.ptr(work), n, n, L.ptr(dst), L.stream())
        assert float(work.abs().max()) == 0.0, (c, "the accumulation copies are not left zero")
    out = dst.cpu()
    return {q: out[int(offs[j]):int(offs[j + 1])].reshape(pre[j].shape) for j, q in enumerate(GRADS)}


def test_density_bwd_every_branch(capsys):
    L, t = _L(), Table()
    reached = set()
    for c in mc.march_cases():
        if "gp0" not in mc.checked(c):
            continue
        ex = mc.extras(c)
        pre = dict(zip(GRADS, list(c.prefill_plane) + list(c.prefill_line)))
        touched = dict(zip(GRADS, [ex[f"touched_p{i}"] for i in range(3)] + [ex[f"touched_l{i}"] for i in range(3)]))
        for walk_switch in (False, True):
            branch = mc.density_bwd_branch(c, walk_switch)
            for xcd in (False, True):
                for with_sigma in ((True, False) if branch[0] == "wave" else (False,)):      # (the group walk takes no sigma)
                    reached.add(branch + (xcd,) + ((with_sigma,) if branch[0] == "wave" else ()))
                    how = f"{branch[0]}{int(branch[1])}" + ("_xcd" if xcd else "") + ("_sig" if with_sigma else "")
                    got = _density_bwd(L, c, walk_switch, xcd, with_sigma)
                    for q in GRADS:
                        t.hold(c, q, got[q], how)
                        same = got[q].view(torch.int32) == torch.from_numpy(pre[q]).view(torch.int32)
                        if not bool(same[~touched[q]].all()):
                            t.fail(c, f"{how} {q}: a texel without a contribution lost its pre-fill")
    want = {b + (x,) + ((s,) if b[0] == "wave" else ()) for b in mc.ALL_BRANCHES for x in (False, True) for s in ((True, False) if b[0] == "wave" else (None,))}
    assert reached == want, want ^ reached
    t.close(capsys)


def test_density_bwd_refuses_other_widths():
    L = _L()
    c = mc.march_cases()[0]
    m, (v, tabs), g = _march_struct(L, c), _vm(L, c), L.VMGrad()
    for comps in (2, 12, 128):
        v.comps = comps
        with pytest.raises(L.CliftError):
            L.call("clift_density_bwd", C.byref(m), C.byref(v), C.byref(g), None, None, 1, None, None, L.stream())


# ---------------------------------------------------------------------------------------------------------------- the fold
def test_xcd_reduce(capsys):
    L, t = _L(), Table()
    for c in mc.fold_cases():
        work, dst = _d(c.work), _d(np.concatenate([c.dst, np.full(8, SENTINEL, np.float32)]))
        L.call("clift_xcd_reduce", L.ptr(work), c.stride, c.n, L.ptr(dst), L.stream())
        t.hold(c, "dst", dst[:c.n].cpu())
        w = work.cpu().reshape(8, c.stride)
        if float(w[:, :c.n].abs().max()) != 0.0:
            t.fail(c, "a copy is not left exactly zero")
        if not torch.equal(w[:, c.n:], torch.from_numpy(c.work).reshape(8, c.stride)[:, c.n:]) or not bool((dst[c.n:] == SENTINEL).all()):
            t.fail(c, "touched the gap between the copies, or wrote past n")
    with pytest.raises(L.CliftError):
        L.call("clift_xcd_reduce", None, 8, 6, None, L.stream())
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- the engine's plumbing
def _model_of(c):
    import contrastive_lift_amd as cl
    model = cl.TensorVMSplit(list(c.res), num_density_comps=(c.comps,) * 3, num_semantic_classes=4, use_semantic_mlp=True, splus_density_shift=c.shift,
                             device=DEV)
    views = model.named_views()
    with torch.no_grad():
        for i in range(3):
            views[f"density_plane.{i}"].copy_(_d(c.plane[i]).permute(2, 0, 1)[None])
            views[f"density_line.{i}"].copy_(_d(c.line[i]).permute(1, 0)[None, :, :, None])
    return model


def test_engine_wrappers(capsys):
    """density_points, and march_struct / vm_struct / vm_grad_struct + vm_grad_finish around the raw calls, on a model's own arena."""
    from contrastive_lift_amd import engine
    L, t = _L(), Table()
    c = next(c for c in mc.points_cases() if c.comps == 16 and c.n == 1000)
    model = _model_of(c)
    x = torch.zeros((c.n, c.ldx), device=DEV)
    x[:, :3] = _d(c.xn)
    t.hold(c, "sigma", engine.density_points(model, x, activation=True).cpu(), "wrapper")
    t.hold(c, "raw", engine.density_points(model, x, activation=False).cpu(), "wrapper")
    for name in ("N257_S33_C16_5x7x9", "N5_S5_C16_5x7x9_nojit"):
        c = next(k for k in mc.march_cases() if k.name == name)
        ref, model = mc.reference(c), _model_of(c)
        renderer = types.SimpleNamespace(bbox_aabb_host=([float(x) for x in c.lo], [float(x) for x in c.hi]), inv_box_extent_host=[float(x) for x in c.inv2],
                                         step_size_host=c.step, n_samples=c.S, distance_scale=c.dist_scale, raymarch_weight_thres=c.thres)
        m = engine.march_struct(renderer, model)
        views, gviews = model.named_views(), model.named_grad_views()
        vd = engine.vm_struct(views, "density", c.res)
        rays, jit = _d(c.rays), _d(c.jitter)
        sigma = torch.empty((c.N, c.S), device=DEV)
        L.call("clift_density_fwd", C.byref(m), C.byref(vd), L.ptr(rays), L.ptr(jit), c.N, L.ptr(sigma), L.stream())
        t.hold(c, "sigma", sigma.cpu(), "wrapper")
        alpha, T, w, ray_out, n_act = _march_fwd(L, c, sigma)
        assert torch.equal(n_act.cpu(), mc.extras(c)["n_active"]), c
        with torch.no_grad():
            for i in range(3):
                gviews[f"density_plane.{i}"].copy_(_d(c.prefill_plane[i]).permute(2, 0, 1)[None])
                gviews[f"density_line.{i}"].copy_(_d(c.prefill_line[i]).permute(1, 0)[None, :, :, None])
        gd = engine.vm_grad_struct(model, gviews, "density")
        assert gd.xcd_stride > 0
        L.call("clift_density_bwd", C.byref(m), C.byref(vd), C.byref(gd), L.ptr(rays), L.ptr(jit), c.N, L.ptr(_d(c.ds_in)), L.ptr(sigma), L.stream())
        engine.vm_grad_finish(model, gviews, "density", gd)
        for i in range(3):
            t.hold(c, f"gp{i}", gviews[f"density_plane.{i}"][0].permute(1, 2, 0).cpu(), "wrapper")
            t.hold(c, f"gl{i}", gviews[f"density_line.{i}"][0, :, :, 0].permute(1, 0).cpu(), "wrapper")
    t.close(capsys)
