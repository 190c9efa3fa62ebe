"""Connected components on the GPU: clift_cc_label / backend="device" against backend="host" on every case of tests/components_cases.py under
all three connectivities (exact integers: no tolerances), determinism, filter_components + extract_isosurface = an exact sub-mesh, and the
stages of inference/extract_mesh.py with --min_component and --split_disconnected on the G27 scene."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, T

import components_cases as cc
import mesh_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def host_results():
    """(case name, connectivity) -> (labels, sizes, roots) of backend="host": computed once, left unchanged."""
    from contrastive_lift_amd import components
    out = {}
    for name, key in cc.key_cases().items():
        for conn in cc.CONNECTIVITIES:
            labels, sizes = components.label_components(key, connectivity=conn, backend="host")
            out[(name, conn)] = (labels.numpy(), sizes.numpy(), components.component_roots(key, connectivity=conn, backend="host").numpy())
    return out


# ============================================================================ 1. parity and determinism
@pytest.mark.parametrize("name", sorted(cc.key_cases()))
def test_device_equals_host(host_results, name):
    from contrastive_lift_amd import components
    key = torch.from_numpy(cc.key_cases()[name]).to(DEV)
    for conn in cc.CONNECTIVITIES:
        ref_labels, ref_sizes, ref_roots = host_results[(name, conn)]
        roots = components.component_roots(key, connectivity=conn)
        assert roots.is_cuda and roots.dtype == torch.int32 and roots.shape == key.shape
        assert np.array_equal(roots.cpu().numpy(), ref_roots), f"{name}, {conn}: roots differ"
        labels, sizes = components.label_components(key, connectivity=conn)
        assert labels.is_cuda and labels.dtype == torch.int32 and sizes.dtype == torch.int64
        assert np.array_equal(labels.cpu().numpy(), ref_labels), f"{name}, {conn}: labels differ"
        assert np.array_equal(sizes.cpu().numpy(), ref_sizes), f"{name}, {conn}: sizes differ"
    if name == "random":
        assert {c: int(host_results[(name, c)][1].shape[0] - 1) for c in cc.CONNECTIVITIES} == cc.RANDOM_MASK_COUNTS
    assert np.array_equal(components.component_roots(key, connectivity=14).cpu().numpy(), host_results[(name, "kuhn")][2])      # 14 = "kuhn"


@pytest.mark.parametrize("name", ["snake", "checkerboard"])
def test_two_runs_give_the_same_bits(name):
    from contrastive_lift_amd import components
    key = torch.from_numpy(cc.key_cases()[name]).to(DEV)
    for conn in cc.CONNECTIVITIES:
        a, b = components.component_roots(key, connectivity=conn), components.component_roots(key, connectivity=conn)
        assert torch.equal(a, b)
        (la, sa), (lb, sb) = components.label_components(key, connectivity=conn), components.label_components(key, connectivity=conn)
        assert torch.equal(la, lb) and torch.equal(sa, sb)


def test_device_refuses_what_it_cannot_label():
    from contrastive_lift_amd import _lib, components
    with pytest.raises(_lib.CliftError):
        components.label_components(torch.from_numpy(cc.keyed()), backend="device")          # a host tensor: no quiet fall-back
    with pytest.raises(ValueError):
        components.label_components(torch.from_numpy(cc.keyed()).to(DEV), connectivity=18)
    labels, sizes = components.label_components(torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV))
    assert labels.shape == (0, 4, 4) and sizes.tolist() == [0]


# ============================================================================ 2. filtering gives an exact sub-mesh
def device_mesh(vol, case):
    from contrastive_lift_amd import mesh
    out = mesh.extract_isosurface(vol, case["level"], [torch.from_numpy(t).to(DEV) for t in case["ticks"]], return_keys=True)
    return [x.cpu().numpy() for x in out]                      # verts, faces, normals, keys


@pytest.fixture(scope="module")
def floater():
    from contrastive_lift_amd import components
    case = cc.floater_volume()
    vol = torch.from_numpy(case["vol"]).to(DEV)
    verts, faces, _, keys = device_mesh(vol, case)
    labels, sizes = components.label_components(vol >= case["level"])
    inside = components.vertex_owner_inside(torch.from_numpy(keys).to(DEV), vol, case["level"])
    comp_of_vertex = labels.reshape(-1)[inside].cpu().numpy()
    return dict(case=case, vol=vol, verts=verts, faces=faces, keys=keys, sizes=sizes.cpu().numpy(), comp_of_vertex=comp_of_vertex)


@pytest.mark.parametrize("options", [dict(min_voxels=2), dict(keep_largest=1), dict(keep_largest=3), dict(min_voxels=30, keep_largest=5)])
def test_filtered_mesh_is_a_sub_mesh(floater, options):
    from contrastive_lift_amd import components
    case, vol, sizes = floater["case"], floater["vol"], floater["sizes"]
    before = vol.clone()
    out, info = components.filter_components(vol, case["level"], **options)
    assert torch.equal(vol, before) and out is not vol
    ref, ref_info = components.filter_components(vol.cpu(), case["level"], backend="host", **options)
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32)) and info["kept"].tolist() == ref_info["kept"].tolist()
    assert info["K"] == 7 and info["dropped"] == ref_info["dropped"] == int(sizes.sum() - sizes[info["kept"].cpu().numpy()].sum())
    kept = info["kept"].cpu().numpy()
    order = sorted(range(1, 8), key=lambda c: (-sizes[c], c))
    expect = [c for c in range(1, 8) if sizes[c] >= options.get("min_voxels", 0) and c in order[:options.get("keep_largest", 7)]]
    assert kept.tolist() == expect and 0 < len(expect) < 7
    verts, faces, _, keys = device_mesh(out, case)
    # its keys are a subset of the unfiltered keys, positions at equal keys are bit-identical
    vert_stays = np.isin(floater["comp_of_vertex"], kept)
    assert np.array_equal(keys, floater["keys"][vert_stays])
    assert np.array_equal(verts.view(np.int32), floater["verts"][vert_stays].view(np.int32))
    # its faces are the unfiltered faces minus the dropped components' faces, renumbered, in the same order
    comp_of_face = floater["comp_of_vertex"][floater["faces"]]
    assert (comp_of_face == comp_of_face[:, :1]).all()                                       # a face belongs to one component (Kuhn)
    renumber = np.cumsum(vert_stays) - 1
    assert np.array_equal(faces, renumber[floater["faces"][np.isin(comp_of_face[:, 0], kept)]].astype(np.int32))
    # one closed sphere per component left
    assert mc.closed_oriented(faces) == (True, True)
    assert mc.euler_characteristic(verts.shape[0], faces) == 2 * len(expect)
    assert mc.signed_volume(verts, faces) > 0


def test_filter_with_both_options_off_returns_the_input(floater):
    from contrastive_lift_amd import components
    out, info = components.filter_components(floater["vol"], 0.0)
    assert out is floater["vol"] and info["dropped"] == 0


# ============================================================================ 3. the stages of inference/extract_mesh.py
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def g27():
    """The scene of the G27 golden (as tests/test_gpu_mesh.py builds it): model, renderer, its sigma lattice at upsample 2 and the tool."""
    import contrastive_lift_amd as cl
    from oracle import params as op
    g = load_golden("g27_dense_volume")
    res, C_, E = tuple(int(x) for x in g["res"]), int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, amplitude=2.5, sigma_g=0.3)
    m = cl.TensorVMSplit(list(res), num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=C_,
                         dim_feature_instance=2 * E, splus_density_shift=float(g["shift"]), use_semantic_mlp=True, use_instance_mlp=True,
                         slow_fast_mode=True, device=DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode="softmax").to(DEV)
    cli = _load(os.path.join(REPO, "inference", "extract_mesh.py"), "clift_extract_mesh_cli_components")
    return dict(model=m, renderer=r, sigma=r.get_dense_sigma(m, 2), cli=cli, C=C_, E=E)


def stages(g27, sigma, level, centroids=None, **kw):
    timer = g27["cli"].StageTimer()
    out = g27["cli"].surface_stages(g27["model"], g27["renderer"], sigma, level, list(range(g27["C"])), centroids, False, timer, **kw)
    return out, timer.report()


def same_mesh(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("verts", "faces", "normals", "sem", "inst", "rgb"))


def test_min_component_removes_exactly_the_specks(g27):
    """The G27 blob is one component of about a hundred lattice points at half its peak.  Specks written into the density by hand, three
    lattice steps or more from the blob, from the border and from each other (so that no gradient stencil of a blob vertex sees one):
    without the flag the stages give what the tool gave before it had the flag, specks included; with --min_component the mesh of the
    clean scene comes back bit for bit -- vertices, faces, normals and labels."""
    from contrastive_lift_amd import mesh
    from scipy import ndimage
    cli, sigma = g27["cli"], g27["sigma"]
    level = 0.5 * float(sigma.max())
    inside = (sigma >= level).cpu().numpy()
    assert ndimage.label(inside, structure=cc.structure("kuhn"))[1] == 1 and inside.sum() > 50
    free = ~ndimage.binary_dilation(inside, structure=np.ones((3, 3, 3), bool), iterations=4)
    free[:3], free[-3:], free[:, :3], free[:, -3:], free[:, :, :3], free[:, :, -3:] = (False,) * 6
    specks = []
    for p in np.argwhere(free):                                # greedy, in scan order: at least 4 steps apart
        if all(np.abs(p - q).max() >= 4 for q in specks):
            specks.append(p)
        if len(specks) == 5:
            break
    assert len(specks) == 5
    dirty = sigma.clone()
    for n, p in enumerate(specks):
        dirty[tuple(p)] = 2.0 * level
        if n % 2:                                              # two-point specks too
            dirty[p[0], p[1], p[2] + 1] = 1.5 * level
    n_speck_points = 5 + 2
    clean, times = stages(g27, sigma, level)
    assert set(times) == {"isosurface", "label_vertices"}
    # without the flag: the parent's sequence, specks and all
    raw, _ = stages(g27, dirty, level)
    v, f, n = mesh.extract_isosurface(dirty, level, g27["renderer"].lattice_ticks(dirty.shape))
    s, i, c = cli.surrogate_ids(g27["model"], g27["renderer"], v, n, list(range(g27["C"])), None, False)
    assert same_mesh(raw, dict(verts=v, faces=f, normals=n, sem=s, inst=i, rgb=c)) and raw["info"] is None and raw["sigma"] is dirty
    assert raw["faces"].shape[0] > clean["faces"].shape[0]
    got, times = stages(g27, dirty, level, min_component=3)
    assert set(times) == {"components", "isosurface", "label_vertices"} and all(t >= 0 for t in times.values())
    assert got["info"]["K"] == 6 and got["info"]["dropped"] == n_speck_points and len(got["info"]["kept"]) == 1
    assert same_mesh(got, clean), "the filtered mesh is not the clean scene's mesh"
    assert mc.closed_oriented(got["faces"].cpu().numpy()) == (True, True)
    got, _ = stages(g27, dirty, level, keep_largest=1, connectivity="26")
    assert same_mesh(got, clean)
    got, _ = stages(g27, dirty, level, min_component=2)       # the two-point specks stay
    assert got["info"]["dropped"] == 3 and clean["faces"].shape[0] < got["faces"].shape[0] < raw["faces"].shape[0]


def test_split_disconnected_gives_separated_blobs_two_ids(g27):
    """Two separated balls of density on the G27 lattice and ONE centroid per class: every vertex of a class carries the same id on both
    balls.  --split_disconnected leaves the id to its largest piece and gives every other piece a fresh one, so no id is left on both
    balls; the vertex ids are exactly the rule of the tool restated with backend="host", and vertices of largest pieces keep their ids."""
    from contrastive_lift_amd import components
    cli = g27["cli"]
    shape = tuple(g27["sigma"].shape)                          # (18, 26, 34)
    idx = np.indices(shape).astype(np.float64)
    ball = lambda c, r: r - np.sqrt(sum((idx[a] - c[a]) ** 2 for a in range(3)))
    sigma = torch.from_numpy((10.0 + 4.0 * np.maximum(ball((8, 7, 9), 4.5), ball((9, 18, 24), 3.5))).astype(np.float32)).to(DEV)
    level = 10.0
    cents = {c: np.zeros((1, g27["E"]), np.float32) for c in range(g27["C"])}
    base, times = stages(g27, sigma, level, centroids=cents)
    assert "split" not in times
    got, times = stages(g27, sigma, level, centroids=cents, split_disconnected=1)
    assert set(times) == {"isosurface", "label_vertices", "split"}
    for k in ("verts", "faces", "normals", "sem", "rgb"):      # only the ids change
        assert torch.equal(got[k], base[k])
    verts, old, new = base["verts"].cpu().numpy(), base["inst"].cpu().numpy(), got["inst"].cpu().numpy()
    ticks1 = g27["renderer"].lattice_ticks(shape)[1].cpu().numpy()
    on_a = verts[:, 1] < 0.5 * (ticks1[12] + ticks1[13])       # the balls are separated along axis 1
    assert on_a.any() and (~on_a).any() and old.min() >= 1
    shared = set(old[on_a]) & set(old[~on_a])
    assert shared, "the scene was meant to have an id on both balls"
    # the tool's rule restated: host components of the id lattice, the inside endpoint's new id where the vertex's id is its old one
    ids = cli.lattice_ids(g27["model"], g27["renderer"], sigma, level, list(range(g27["C"])), cents, False)
    assert ((ids > 0) == (sigma >= level)).all()
    new_ids, table = components.split_disconnected(ids.cpu(), backend="host", first_fresh=int(old.max()) + 1)       # fresh ids above the vertices' too
    assert got["table"] == table and len(table) >= len(shared) and set(table.values()) <= set(np.unique(old).tolist())
    keys = device_keys(sigma, level, g27)
    at = components.vertex_owner_inside(keys, sigma, level).cpu().numpy()
    p_old, p_new = ids.cpu().numpy().reshape(-1)[at], new_ids.numpy().reshape(-1)[at]
    expect = np.where(old == p_old, p_new, old)
    assert np.array_equal(new, expect)
    agree = old == p_old                                       # (a vertex on a class boundary may carry another id than its lattice point: it keeps it)
    print(f"{verts.shape[0]} vertices, ids {np.unique(old).tolist()} -> {np.unique(new).tolist()}, {int((~agree).sum())} differ from their lattice point")
    assert agree.mean() > 0.9
    assert not (set(new[on_a & agree]) & set(new[~on_a & agree])), "an id is still on both balls"
    assert (new[p_new == p_old] == old[p_new == p_old]).all() and (new == old).any() and (new != old).any()
    assert set(np.unique(new).tolist()) <= set(np.unique(old).tolist()) | set(table)
    # pieces below MIN_VOXELS keep the parent's id: with a bound above the smaller ball nothing is split
    small = int((sigma >= level).sum()) // 2
    got, _ = stages(g27, sigma, level, centroids=cents, split_disconnected=small)
    assert got["table"] == {} and torch.equal(got["inst"], base["inst"])


def test_id_lattice_numbering_does_not_depend_on_the_chunk(g27):
    """With cached centroids the numbering of the ids offsets every class by the labels seen before it IN ONE CALL, so the id lattice has
    to come from one call over all inside points: ``chunk`` (the field-evaluation chunk) must not change it.  Two classes with three
    centroids each, taken from the instance features of inside points themselves so that several ids of each class are in use."""
    cli, model, renderer, E = g27["cli"], g27["model"], g27["renderer"], g27["E"]
    sigma = g27["sigma"]
    level = 0.0                                                # every lattice point is inside: both classes of the field occur
    things = list(range(g27["C"]))
    inside = (sigma >= level).reshape(-1).nonzero().reshape(-1)
    ticks = renderer.lattice_ticks(sigma.shape)
    n1, n2 = int(sigma.shape[1]), int(sigma.shape[2])
    xyz = torch.stack([ticks[0][inside // (n1 * n2)], ticks[1][(inside // n2) % n1], ticks[2][inside % n2]], 1).contiguous()
    xn = renderer.normalize_coordinates(xyz).contiguous()
    feats = model.render_instance_mlp(None, model.compute_instance_feature(xn))[:, :E]
    sem = model.render_semantic_mlp(None, model.compute_semantic_feature(xn)).argmax(-1)
    cents = {}
    for c in things:
        of_c = (sem == c).nonzero().reshape(-1)
        assert of_c.shape[0] >= 3, f"class {c} has {of_c.shape[0]} inside points"
        cents[c] = feats[of_c[[0, of_c.shape[0] // 2, of_c.shape[0] - 1]]].cpu().numpy()
    whole = cli.lattice_ids(model, renderer, sigma, level, things, cents, False)
    once = cli.surrogate_ids(model, renderer, xyz, torch.zeros_like(xyz), things, cents, False)[1]
    assert torch.equal(whole.reshape(-1)[inside].long(), once) and int((whole != 0).sum()) == inside.shape[0] > 200
    used = torch.unique(once).tolist()
    print(f"{inside.shape[0]} inside points, ids in use {used}")
    assert len(used) >= 4 and min(used) >= 1
    for chunk in (37, 100, inside.shape[0] - 1):
        assert torch.equal(cli.lattice_ids(model, renderer, sigma, level, things, cents, False, chunk=chunk), whole), chunk


def device_keys(sigma, level, g27):
    from contrastive_lift_amd import mesh
    return mesh.extract_isosurface(sigma, level, g27["renderer"].lattice_ticks(sigma.shape), return_keys=True)[3]
