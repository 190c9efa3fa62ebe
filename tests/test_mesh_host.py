"""Surface export without a GPU: the numpy restatement of the iso-surface rules (tests/mesh_cases.py) validates itself by mesh invariants,
the new library entries are declared / exported / bound at ABI 27 and refuse bad sizes before they touch the device, the PLY writer
round-trips, and the command line exposes its flags."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import REPO

import mesh_cases as mc

NEW_SYMBOLS = ("clift_dense_sigma", "clift_iso_classify", "clift_iso_vertices", "clift_iso_faces")


@pytest.fixture(scope="module")
def restated():
    """name -> (case, keys, verts, faces): every closed case and the open one, computed once."""
    return {c["name"]: (c,) + mc.marching_tetrahedra(c["vol"], c["level"], c["ticks"]) for c in mc.closed_cases() + [mc.open_case()]}


@pytest.mark.parametrize("name", ["sphere", "torus", "random0", "random1", "random2", "tie"])
def test_restatement_gives_closed_oriented_manifolds(restated, name):
    """Every undirected edge in exactly two triangles, every directed edge once, chi = 2 (sphere) / 0 (torus), positive signed volume."""
    case, keys, verts, faces = restated[name]
    assert keys.shape[0] == verts.shape[0] > 0 and faces.shape[0] > 0 and np.all(np.diff(keys) > 0)
    assert faces.min() >= 0 and faces.max() < verts.shape[0] and np.isfinite(verts).all()
    directed_once, two_per_edge = mc.closed_oriented(faces)
    assert directed_once, f"{name}: a directed edge appears twice (inconsistent winding)"
    assert two_per_edge, f"{name}: an edge that is not in exactly two triangles (not closed)"
    chi = mc.euler_characteristic(verts.shape[0], faces)
    print(f"{name}: V {verts.shape[0]} F {faces.shape[0]} chi {chi} signed volume {mc.signed_volume(verts, faces):.6f}")
    if case["chi"] is not None:
        assert chi == case["chi"]
    assert chi % 2 == 0                                       # closed orientable surfaces: chi = sum of 2 - 2 g
    assert mc.signed_volume(verts, faces) > 0, f"{name}: normals point inwards"


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_restatement_volume_against_analytic(restated, name):
    """The mesh of a convex-section body interpolated linearly lies inside it: 0 < V_mesh < V_analytic, deficit under 10 % on these coarse
    lattices (restatement: sphere 7.0 %, torus 3.1 %)."""
    case, _, verts, faces = restated[name]
    v, va = mc.signed_volume(verts, faces), case["analytic_volume"]
    print(f"{name}: mesh volume {v:.6f} analytic {va:.6f} deficit {100 * (1 - v / va):.2f} %")
    assert 0 < v < va and 1 - v / va < 0.10


def test_sphere_has_lattice_points_on_the_level_and_ties_make_zero_area_faces(restated):
    """The cases that defeat a geometric winding test are really in the inputs: lattice points exactly on the level (t = 0 or 1), hence
    coincident vertices and zero-area triangles -- and the combinatorial invariants above hold all the same."""
    assert int((mc.sphere_case()["vol"] == 0).sum()) >= 2
    case, _, verts, faces = restated["tie"]
    assert int((case["vol"] == 0).sum()) > 50
    v = verts.astype(np.float64)
    area2 = np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)
    assert int((area2 == 0).sum()) > 0


def test_open_and_single_cell_cases_are_consistent(restated):
    """An open surface: no directed edge twice, but boundary edges.  Every one of the 256 single cells: faces name distinct existing
    vertices, every vertex is used, no directed edge twice, and pattern p and its complement give the same vertices with mirrored faces."""
    _, _, verts, faces = restated["open"]
    directed_once, two_per_edge = mc.closed_oriented(faces)
    assert directed_once and not two_per_edge and faces.shape[0] > 0
    got = {}
    for p in range(256):
        c = mc.single_cell_case(p)
        keys, verts, faces = mc.marching_tetrahedra(c["vol"], c["level"], c["ticks"])
        got[p] = (keys, faces)
        if p in (0, 255):
            assert keys.shape[0] == 0 and faces.shape[0] == 0
            continue
        assert faces.shape[0] > 0 and set(np.unique(faces)) == set(range(keys.shape[0]))
        assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
        assert mc.closed_oriented(faces)[0]
    for p in range(1, 128):
        (ka, fa), (kb, fb) = got[p], got[255 - p]
        assert np.array_equal(ka, kb)
        assert np.array_equal(mc.canonical_faces(fa), mc.canonical_faces(fb[:, ::-1]))


def test_normals_of_the_restatement_point_outwards(restated):
    case, keys, verts, _ = restated["sphere"]
    n = mc.vertex_normals(case["vol"], case["level"], case["ticks"], keys)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    assert (np.einsum("ij,ij->i", n, verts) > 0).all()       # the sphere sits at the origin: outwards = along the position


def test_abi_27_declares_exports_and_binds_the_surface_entries():
    from contrastive_lift_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "clift.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(clift_[a-z0-9_]+)\s*\(", src))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/clift.h"
        assert hasattr(lib, s), f"{s} is not exported by libclift.so"
        assert s in _lib.exported_symbols(), f"{s} has no row in the ctypes table"
    assert sorted(_lib.exported_symbols()) == sorted(declared)
    assert _lib.ABI_VERSION == 27 and _lib.load().clift_version() == 27
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ABI 27 addition" in open(os.path.join(REPO, doc)).read(), doc


def test_size_checks_need_no_gpu():
    """The iso-surface entries refuse a lattice, a vertex count or a face count of 2^31 or more before any device call, and say which limit;
    lattices without a cell and empty meshes return at once."""
    from contrastive_lift_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                    # never followed: every call below returns before it touches a buffer
    big = (2048, 1024, 1024)                                   # 2^31 lattice points
    calls = (("clift_iso_classify", (p, *big, 0.0, p, p, p, None), "lattice points"),
             ("clift_iso_vertices", (p, *big, 0.0, p, p, p, p, p, 10, p, p, None), "lattice points"),
             ("clift_iso_faces", (p, *big, 0.0, p, p, p, 10, 10, p, None), "lattice points"),
             ("clift_iso_vertices", (p, 4, 4, 4, 0.0, p, p, p, p, p, 2 ** 31, p, p, None), "vertices"),
             ("clift_iso_faces", (p, 4, 4, 4, 0.0, p, p, p, 2 ** 31, 10, p, None), "vertices"),
             ("clift_iso_faces", (p, 4, 4, 4, 0.0, p, p, p, 10, 2 ** 31, p, None), "faces"),
             ("clift_iso_faces", (p, 4, 4, 4, 0.0, p, p, p, 10, -1, p, None), "faces"))
    for name, args, word in calls:
        assert getattr(lib, name)(*args) != 0, name
        msg = lib.clift_last_error().decode()
        assert word in msg and "2^31" in msg, (name, msg)
    assert lib.clift_iso_classify(p, 4, 4, 4, float("nan"), p, p, p, None) != 0 and "NaN" in lib.clift_last_error().decode()
    for n in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (0, 4, 4), (-3, 4, 4)):                      # no cell: nothing to do, nothing launched
        assert lib.clift_iso_classify(None, *n, 0.0, None, None, None, None) == 0
        assert lib.clift_iso_vertices(None, *n, 0.0, None, None, None, None, None, 0, None, None, None) == 0
        assert lib.clift_iso_faces(None, *n, 0.0, None, None, None, 0, 0, None, None) == 0
    assert lib.clift_iso_vertices(None, 4, 4, 4, 0.0, None, None, None, None, None, 0, None, None, None) == 0      # all inside / all outside
    assert lib.clift_iso_faces(None, 4, 4, 4, 0.0, None, None, None, 0, 0, None, None) == 0
    assert lib.clift_dense_sigma(None, None, None, None, None, None, None, 4, 4, 4, 0.0, None, None) != 0 and "NULL" in lib.clift_last_error().decode()
    vm, f3 = _lib.VM(), (ctypes.c_float * 3)()
    vm.comps = 16
    assert lib.clift_dense_sigma(ctypes.byref(vm), f3, f3, f3, p, p, p, 8192, 8192, 1024, 0.0, p, None) != 0
    assert "2^36" in lib.clift_last_error().decode()
    assert lib.clift_dense_sigma(ctypes.byref(vm), f3, f3, f3, p, p, p, 4, 0, 4, 0.0, p, None) != 0 and "positive" in lib.clift_last_error().decode()


def test_ply_round_trip(tmp_path):
    from contrastive_lift_amd import mesh
    rng = np.random.default_rng(3)
    V, F = 37, 52
    verts, normals = rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    rgb8 = rng.integers(0, 256, (V, 3)).astype(np.uint8)
    sem, inst = rng.integers(0, 256, V), rng.integers(0, 65536, V)
    path = tmp_path / "m.ply"
    mesh.write_ply(path, verts, faces, normals, rgb8.astype(np.float32) / 255.0, sem, inst)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and f"element vertex {V}" in head and f"element face {F}" in head
    assert [ln for ln in head if ln.startswith("property")] == [
        "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
        "property uchar red", "property uchar green", "property uchar blue", "property uchar semantic", "property ushort instance",
        "property list uchar int vertex_indices"]
    back = mesh.read_ply(path)
    assert np.array_equal(back["verts"], verts) and np.array_equal(back["normals"], normals) and np.array_equal(back["faces"], faces)
    assert np.array_equal(back["rgb"], rgb8) and np.array_equal(back["semantics"], sem) and np.array_equal(back["instances"], inst)
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + V * 30 + F * 13
    mesh.write_ply(path, verts[:0], faces[:0], normals[:0], rgb8[:0], sem[:0], inst[:0])                   # an empty mesh is a valid file
    assert mesh.read_ply(path)["faces"].shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.write_ply(path, verts, faces + V, normals, rgb8, sem, inst)
    with pytest.raises(ValueError):
        mesh.write_ply(path, verts, faces, normals, rgb8, sem + 256, inst)


def test_extract_mesh_cli_flags():
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    a = ap.parse_args(["--ckpt_path", "x.ckpt"])
    assert a.upsample == 2 and a.alpha_level == 0.5 and a.level is None and a.cached_centroids_path is None
    assert not a.split_instances and not a.save_voxel_cloud
    a = ap.parse_args(["--ckpt_path", "x.ckpt", "--upsample", "3", "--level", "12.5", "--cached_centroids_path", "c.pkl", "--split_instances",
                       "--save_voxel_cloud"])
    assert a.upsample == 3 and a.level == 12.5 and a.cached_centroids_path == "c.pkl" and a.split_instances and a.save_voxel_cloud
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt_path", "x.ckpt", "--alpha_level", "0.3", "--level", "2"])                 # one way to name the level
    assert "judgement" in ap.format_help() and "measured" in ap.format_help()

    class R:
        step_size_host, distance_scale = 0.01, 25
    assert abs(cli.default_level(R, 0.5) - np.log(2.0) / (0.02 * 25)) < 1e-12
    assert cli.rp.load_for_inference is not None and not hasattr(cli, "build_from_checkpoint")          # the loader is shared, not copied
