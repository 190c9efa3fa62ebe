"""Surface export on the GPU: clift_dense_sigma against the reference (G27), the device marching tetrahedra against the numpy restatement of
its rules (tests/mesh_cases.py) and against the mesh invariants, determinism, get_instance_clusters against G27, label_vertices against
the CPU oracle, and inference/extract_mesh.py end to end."""
import importlib.util
import os
import pickle
import random
import sys
import time

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, T, rel_close

import mesh_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TIE_GAP, TIE_SHARE = 1e-4, 0.01


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(P, res, C_, E, shift, slow_fast=True):
    import contrastive_lift_amd as cl
    m = cl.TensorVMSplit(list(res), num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=C_,
                         dim_feature_instance=(2 * E if slow_fast else E), splus_density_shift=shift, use_semantic_mlp=True,
                         use_instance_mlp=True, slow_fast_mode=slow_fast, device=DEV)
    missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    assert not missing and not unexpected
    return m


def g27_scene():
    import contrastive_lift_amd as cl
    from oracle import params as op
    g = load_golden("g27_dense_volume")
    res = tuple(int(x) for x in g["res"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, int(g["C"]), int(g["E"])), res, amplitude=2.5, sigma_g=0.3)
    m = build_model(P, res, int(g["C"]), int(g["E"]), float(g["shift"]))
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode="softmax").to(DEV)
    return g, m, r


def gpu_mesh(case, **kw):
    from contrastive_lift_amd import mesh
    out = mesh.extract_isosurface(torch.from_numpy(case["vol"]).to(DEV), case["level"], [torch.from_numpy(t).to(DEV) for t in case["ticks"]],
                                  return_keys=True, **kw)
    torch.cuda.synchronize()
    verts, faces, normals, keys = (x.cpu().numpy() for x in out)
    return verts, faces, normals, keys


@pytest.fixture(scope="module")
def restated():
    """name -> (case, keys, verts, faces) of the CPU restatement, computed once and left unchanged."""
    return {c["name"]: (c,) + mc.marching_tetrahedra(c["vol"], c["level"], c["ticks"]) for c in mc.closed_cases() + [mc.open_case()]}


# ============================================================================ 1. dense sigma
@pytest.mark.parametrize("upsample", [1, 2])
def test_dense_sigma_golden_g27(upsample):
    g, m, r = g27_scene()
    sigma = r.get_dense_sigma(m, upsample)
    assert tuple(sigma.shape) == tuple(int(x) * upsample for x in g["res"]) and sigma.is_cuda
    rel_close(sigma, g[f"sigma_u{upsample}"], 1e-3, atol=1e-6, what=f"dense sigma, upsample {upsample}")
    ticks = r.lattice_ticks(sigma.shape)                       # where the lattice sits: the box corners at both ends of every axis
    for a in range(3):
        assert ticks[a].shape[0] == sigma.shape[a]
        assert float(ticks[a][0]) == float(r.bbox_aabb[0][a]) and float(ticks[a][-1]) == float(r.bbox_aabb[1][a])


# ============================================================================ 2. iso-surface against the restatement
def check_against_restatement(case, ref, got):
    keys_r, verts_r, faces_r = ref
    verts, faces, normals, keys = got
    name = case["name"]
    assert np.array_equal(keys, keys_r), f"{name}: active-edge keys / vertex order differ"
    ulp = mc.ulp_distance(verts, verts_r)
    print(f"{name}: V {verts.shape[0]} F {faces.shape[0]}, positions {'bit-equal' if ulp == 0 else f'within {ulp} ulp'}")
    assert ulp <= 1, f"{name}: a coordinate {ulp} ulp from the restatement"
    assert np.array_equal(mc.canonical_faces(faces), mc.canonical_faces(faces_r)), f"{name}: face sets differ"
    assert np.array_equal(faces, faces_r), f"{name}: face order differs from the documented scan order"
    if keys.shape[0]:
        n_ref = mc.vertex_normals(case["vol"], case["level"], case["ticks"], keys_r)
        # the same fp32 operations on both sides, a handful per component of a unit vector: 16 ulp of 1.0
        assert np.abs(normals - n_ref).max() <= 2e-6, f"{name}: normals differ by {np.abs(normals - n_ref).max():.3g}"


@pytest.mark.parametrize("name", ["sphere", "torus", "random0", "random1", "random2", "tie", "open"])
def test_isosurface_matches_restatement(restated, name):
    case, *ref = restated[name]
    got = gpu_mesh(case)
    check_against_restatement(case, ref, got)
    verts, faces, normals, _ = got
    directed_once, two_per_edge = mc.closed_oriented(faces)                 # on the GPU output itself
    assert directed_once, f"{name}: a directed edge appears twice"
    assert two_per_edge == case["closed"]
    if case["closed"]:
        chi = mc.euler_characteristic(verts.shape[0], faces)
        assert chi % 2 == 0 and (case["chi"] is None or chi == case["chi"]), (name, chi)
        assert mc.signed_volume(verts, faces) > 0
    if case.get("analytic_volume"):
        v = mc.signed_volume(verts, faces)
        assert 0 < v < case["analytic_volume"] and 1 - v / case["analytic_volume"] < 0.10
    if name == "sphere":
        assert (np.einsum("ij,ij->i", normals, verts) > 0).all() and np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)


def test_single_cell_exhaustive():
    """All 256 corner sign patterns of one (2, 2, 2) cell: a wrong table entry or a geometric winding cannot hide."""
    for pattern in range(256):
        case = mc.single_cell_case(pattern)
        ref = mc.marching_tetrahedra(case["vol"], case["level"], case["ticks"])
        got = gpu_mesh(case)
        if pattern in (0, 255):
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[3].shape == (0,)
        else:
            assert got[1].shape[0] > 0
        check_against_restatement(case, ref, got)


def test_empty_cases():
    from contrastive_lift_amd import mesh
    ticks = lambda shape: [torch.linspace(-1, 1, n, device=DEV) for n in shape]
    for shape in ((1, 5, 6), (5, 1, 6), (5, 6, 1)):                        # a lattice without a cell
        vol = torch.randn(shape, device=DEV)
        v, f, n = mesh.extract_isosurface(vol, 0.0, ticks(shape))
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and f.dtype == torch.int32
    for value in (1.0, -1.0):                                                # all inside, all outside
        v, f, n, k = mesh.extract_isosurface(torch.full((4, 5, 6), value, device=DEV), 0.0, ticks((4, 5, 6)), return_keys=True)
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and k.shape == (0,)
    v, f, n = mesh.extract_isosurface(torch.full((4, 5, 6), float("nan"), device=DEV), 0.0, ticks((4, 5, 6)))      # NaN is outside
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.extract_isosurface(torch.zeros((4, 5, 6), device=DEV), 0.0, ticks((4, 5, 7)))


def test_nan_and_inf_values_follow_the_rules(restated):
    """NaN counts as outside and a non-finite t becomes 0: the kernels and the restatement agree on a field with both."""
    case = mc.random_case(5)
    case["vol"][3, 4, 5], case["vol"][2, 2, 2], case["name"] = np.nan, np.inf, "nonfinite"
    got = gpu_mesh(case)
    ref = mc.marching_tetrahedra(case["vol"], case["level"], case["ticks"])
    assert np.isfinite(got[0]).all()
    check_against_restatement(case, ref, got)


# ============================================================================ 3. determinism
def test_two_runs_are_bit_identical():
    case = mc.torus_case()
    a, b = gpu_mesh(case), gpu_mesh(case)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_without_normals_the_mesh_is_the_same():
    from contrastive_lift_amd import mesh
    case = mc.torus_case()
    vol, ticks = torch.from_numpy(case["vol"]).to(DEV), [torch.from_numpy(t).to(DEV) for t in case["ticks"]]
    v, f, n = mesh.extract_isosurface(vol, case["level"], ticks)
    v2, f2, n2 = mesh.extract_isosurface(vol, case["level"], ticks, want_normals=False)
    assert n2 is None and n.shape == v.shape and torch.equal(v, v2) and torch.equal(f, f2)


# ============================================================================ 4. get_instance_clusters
@pytest.mark.parametrize("mode", ["alpha", "full"])
def test_instance_clusters_golden_g27(mode):
    g, m, r = g27_scene()
    res = np.array([int(x) for x in g["res"]])
    gap = g["inst_gap"].reshape(-1)
    assert int(g["n_near_tie"]) == int((gap < TIE_GAP).sum()) <= TIE_SHARE * gap.size
    random.seed(0)
    xyz, labels = r.get_instance_clusters(m, mode)
    assert xyz.is_cuda and labels.dtype == torch.int32 and xyz.shape == (labels.shape[0], 3)
    lo, hi = g["aabb"][0].astype(np.float64), g["aabb"][1].astype(np.float64)

    def rows(points, lab):                       # voxel (x-major linear index) -> (label, point)
        idx = np.rint((points.astype(np.float64) - lo) / (hi - lo) * (res - 1)).astype(np.int64)
        lin = (idx[:, 0] * res[1] + idx[:, 1]) * res[2] + idx[:, 2]
        assert np.unique(lin).shape[0] == lin.shape[0]
        return {int(v): (int(c), p) for v, c, p in zip(lin, lab, points)}
    ref, got = rows(g[f"{mode}.xyz"], g[f"{mode}.labels"]), rows(xyz.cpu().numpy(), labels.cpu().numpy())
    assert sorted(ref) == sorted(got), f"{mode}: the kept voxels differ"
    assert len(ref) == (gap.size if mode == "full" else int(g[f"{mode}.xyz"].shape[0]))
    for v in ref:
        assert np.abs(ref[v][1] - got[v][1]).max() <= 1e-6, (mode, v)
        if gap[v] >= TIE_GAP:
            assert ref[v][0] == got[v][0], (mode, v, ref[v][0], got[v][0], float(gap[v]))
    with pytest.raises(ValueError):
        r.get_instance_clusters(m, "sigma")


# ============================================================================ 5. label_vertices
MODEL_SEED = 598        # make_params heads are nearly flat: of seeds 300..699 this one has both classes and ids mixed over the sphere with the near ties within the cap


def oracle_labels(P, aabb, verts, normals, E):
    """(semantic probabilities, fast instance outputs, rgb) of the CPU oracle at world points."""
    from oracle import field as ofld
    xn = (T(verts) - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1
    with torch.no_grad():
        sem = ofld.semantic_head(P, xn)
        inst = ofld.instance_head(P, xn)[:, :E]
        rgb = ofld.appearance_mlp(P, -T(normals), ofld.appearance_feature(P, xn))
    return sem, inst, rgb


def top_two_gap(scores):
    top = torch.topk(scores, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).numpy()


def test_label_vertices_against_oracle(restated):
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import mesh
    from oracle import params as op
    case = restated["sphere"][0]
    verts, _, normals, _ = gpu_mesh(case)
    res, C_, E = (9, 13, 17), 4, 3
    aabb = torch.tensor([[-1.0, -0.8, -0.6], [1.0, 0.8, 0.6]])
    P = op.make_params(MODEL_SEED, res, C_, E)
    m = build_model(P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    o_sem, o_inst, o_rgb = oracle_labels(P, aabb, verts, normals, E)
    V = verts.shape[0]
    sem_ok, inst_ok = top_two_gap(o_sem) >= TIE_GAP, top_two_gap(o_inst) >= TIE_GAP
    print(f"left out as near ties: {int((~sem_ok).sum())} classes, {int((~inst_ok).sum())} ids of {V}")
    assert (~sem_ok).sum() <= TIE_SHARE * V and (~inst_ok).sum() <= TIE_SHARE * V
    exp_sem, exp_inst = o_sem.argmax(1).numpy(), o_inst.argmax(1).numpy()
    assert len(np.unique(exp_sem)) > 1 and len(np.unique(exp_inst)) > 1
    dv, dn = T(verts).to(DEV), T(normals).to(DEV)
    sem, inst, rgb = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3))
    assert sem.shape == inst.shape == (V,) and rgb.shape == (V, 3)
    assert np.array_equal(sem.cpu().numpy()[sem_ok], exp_sem[sem_ok])
    assert np.array_equal(inst.cpu().numpy()[inst_ok], exp_inst[inst_ok])
    rel_close(rgb, o_rgb, 1e-3, what="vertex rgb")
    s2, i2, c2 = mesh.label_vertices(m, r, dv, dn, thing_classes=(2, 3), chunk=100)          # chunking changes nothing
    assert torch.equal(s2, sem) and torch.equal(i2, inst) and torch.equal(c2, rgb)
    # cached centroids: nearest centroid of the vertex's class, numbered like inference.assign_clusters numbers pred_surrogateid
    rng = np.random.default_rng(30)                  # of seeds 11..39 the one whose centroids are all three used with no distance near-tie beyond the class ones
    scale = float(o_inst.abs().max())
    cents = {c: (rng.standard_normal((k, E)) * scale).astype(np.float32) for c, k in ((2, 3), (3, 2))}
    for things in ((2, 3), (3,)):
        exp, ok, nxt = np.zeros(V, np.int64), sem_ok.copy(), 0
        for c in sorted(set(exp_sem[np.isin(exp_sem, things)].tolist())):
            sel = exp_sem == c
            d = torch.cdist(o_inst[sel].double(), T(cents[c]).double())
            exp[sel] = d.argmin(1).numpy() + nxt + 1
            ok[sel] &= top_two_gap(-d) >= TIE_GAP
            nxt = int(exp[sel].max())
        assert (~ok).sum() <= TIE_SHARE * V, int((~ok).sum())
        s3, i3, _ = mesh.label_vertices(m, r, dv, dn, thing_classes=things, centroids=cents)
        assert torch.equal(s3, sem)
        assert np.array_equal(i3.cpu().numpy()[ok], exp[ok]), things
        assert (i3.cpu().numpy()[~np.isin(sem.cpu().numpy(), things)] == 0).all()              # stuff is 0


# ============================================================================ 6. command line, end to end
def test_extract_mesh_cli_end_to_end(tmp_path, monkeypatch):
    """The synthetic checkpoint of test_gpu_end_to_end.py -- the same scene and the same train-CLI arguments, built here again because
    tests share no state; a run of 300 steps was tried first and leaves the semantic head without the thing class and the density a
    froth of 185 000 faces, so there is nothing to label (the seconds of the run and of the export are printed) -- then
    inference/extract_mesh.py on it: mesh.ply parses and has faces, ids are in range, voxelcloud.pkl loads in fit_bboxes.py."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_mos as gen
    from contrastive_lift_amd import mesh
    from contrastive_lift_amd.config import load_run_config
    scene_dir = gen.make_scene(str(tmp_path / "data" / "synth_scene"), n_frames=40, size=64, trajectory_frames=3)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("experiment", "e2e_mesh")
    train = _load(os.path.join(REPO, "trainer", "train_panopli_tensorf.py"), "clift_train_cli_mesh")
    t0 = time.perf_counter()
    run_dir = train.main(["+experiment=contrastive_lift_MOS", f"dataset_root={scene_dir}", "image_dim=64", "min_grid_dim=32",
                          "max_grid_dim=64", "max_epoch=6", "steps_per_epoch=400", "batch_size=2048", "chunk=0", "max_depth=3",
                          "seed=3", "max_rays_instances=512", "decay_step=[4,5]"])
    t_train = time.perf_counter() - t0
    ckpt = os.path.join(run_dir, "checkpoints", sorted(os.listdir(os.path.join(run_dir, "checkpoints")))[-1])
    cfg = load_run_config(os.path.join(run_dir, "config.yaml"))
    cfg.resume, cfg.subsample_frames, cfg.image_dim = ckpt, 2, [64, 64]
    cents = {1: np.array([[0.5, 0.0, 0.0], [-0.5, 0.3, 0.1], [0.0, -0.4, 0.2]], np.float32)}
    cpath = str(tmp_path / "all_centroids.pkl")
    pickle.dump(cents, open(cpath, "wb"))
    cli = _load(os.path.join(REPO, "inference", "extract_mesh.py"), "clift_extract_mesh_cli_gpu")
    t0 = time.perf_counter()
    state = random.getstate()
    out, times = cli.extract_mesh(cfg, upsample=2, alpha_level=0.5, cached_centroids_path=cpath, split_instances=True, save_voxel_cloud=True)
    assert random.getstate() == state                                                        # the tool leaves the caller's generator alone
    print(f"scene + training run {t_train:.1f} s, extract_mesh (mesh, split, voxel cloud) {time.perf_counter() - t0:.1f} s")
    assert set(times) == {"dense_sigma", "isosurface", "label_vertices"} and all(t >= 0 for t in times.values())
    ply = mesh.read_ply(out / "mesh.ply")
    V, F = ply["verts"].shape[0], ply["faces"].shape[0]
    print(f"mesh.ply: {V} vertices, {F} faces, classes {np.unique(ply['semantics']).tolist()}, ids {np.unique(ply['instances']).tolist()}")
    assert F > 0 and V > 0 and ply["faces"].min() >= 0 and ply["faces"].max() < V
    assert mc.closed_oriented(ply["faces"])[0]                                               # consistently wound
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    box = ck["state_dict"]["renderer.bbox_aabb"].numpy()
    assert (ply["verts"] >= box[0] - 1e-5).all() and (ply["verts"] <= box[1] + 1e-5).all()
    assert ply["semantics"].max() < 2                                                        # the MOS layout has two classes: 0 stuff, 1 thing
    assert ply["instances"].max() <= 3 and ((ply["instances"] == 0) == (ply["semantics"] != 1)).all()      # 3 centroids of thing class 1; stuff is 0
    f_inst = ply["instances"][ply["faces"]]                                                  # (F, 3)
    with_faces = [int(i) for i in np.unique(ply["instances"]) if (f_inst == i).all(1).any()]
    assert with_faces and sorted(p.name for p in out.glob("mesh_instance_*.ply")) == sorted(f"mesh_instance_{i}.ply" for i in with_faces)
    for i in with_faces:                          # one file per id that owns a face: exactly the faces whose three vertices carry it
        sub = mesh.read_ply(out / f"mesh_instance_{i}.ply")
        assert (sub["instances"] == i).all() and sub["faces"].shape[0] == int((f_inst == i).all(1).sum())
        assert sub["faces"].min() >= 0 and sub["faces"].max() < sub["verts"].shape[0]
    cloud = pickle.load(open(out / "voxelcloud.pkl", "rb"))
    P_ = cloud["points"].shape[0]
    assert cloud["points"].dtype == np.float32 and cloud["points"].shape == (P_, 3) and P_ > 0
    assert cloud["instances"].shape == (P_,) and cloud["instances"].dtype == np.uint16 and cloud["semantics"].dtype == np.uint8
    assert cloud["rgb"].shape == (P_, 3) and cloud["rgb"].dtype == np.uint8 and cloud["instances"].max() <= 3
    fb = _load(os.path.join(REPO, "inference", "fit_bboxes.py"), "clift_fit_bboxes_cli_mesh")
    points, instances = fb.load_pointcloud(str(out / "voxelcloud.pkl"))
    assert points.shape == (P_, 3) and instances.shape == (P_,) and np.array_equal(instances, cloud["instances"].astype(np.int64))
    assert (instances > 0).any()                                                             # the trained scene has occupied thing voxels
    pkl, _ = fb.fit_bboxes(str(out / "voxelcloud.pkl"), method="simple")
    boxes = pickle.load(open(pkl, "rb"))
    assert isinstance(boxes, dict) and set(boxes) <= set(np.unique(instances[instances > 0]).tolist())
    # without centroids: 1 + the head's argmax on thing classes, 0 on stuff
    out2, _ = cli.extract_mesh(cfg, upsample=1)
    ply2 = mesh.read_ply(out2 / "mesh.ply")
    E = int(cfg.max_instances)
    assert ply2["faces"].shape[0] > 0 and ply2["instances"].max() <= E and ((ply2["instances"] == 0) == (ply2["semantics"] != 1)).all()
