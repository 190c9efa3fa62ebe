"""Connected components without a GPU: backend="host" against the restatements of tests/components_cases.py and the stated counts, the
rules of filter_components / split_disconnected / vertex_owner_inside, the reason the mesh's connectivity is the Kuhn one, the new library
entry declared / exported / bound at ABI 27 and refusing bad arguments before it touches the device, and the command line's new flags."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import components_cases as cc
import mesh_cases as mc


@pytest.fixture(scope="module")
def filled():
    """(case name, connectivity) -> flood_fill's (labels, sizes, roots): computed once, left unchanged."""
    return {(name, conn): cc.flood_fill(key, conn) for name, key in cc.key_cases().items() for conn in cc.CONNECTIVITIES}


def host(key, conn):
    from contrastive_lift_amd import components
    labels, sizes = components.label_components(key, connectivity=conn, backend="host")
    return labels.numpy(), sizes.numpy()


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
def test_random_mask_counts_and_numbering(filled, conn):
    """3248 / 828 / 74 components; numbering by ascending first point, which for a mask is scipy's own order."""
    from scipy import ndimage
    mask = cc.random_mask()
    labels, sizes = host(mask, conn)
    assert labels.dtype == np.int32 and labels.shape == mask.shape and sizes.dtype == np.int64
    assert sizes.shape[0] - 1 == cc.RANDOM_MASK_COUNTS[conn] == int(labels.max()) and sizes[0] == 0
    assert np.array_equal(labels, ndimage.label(mask, structure=cc.structure(conn))[0])
    assert np.array_equal(labels, filled[("random", conn)][0]) and np.array_equal(sizes, filled[("random", conn)][1])
    first = [int(np.flatnonzero(labels.reshape(-1) == c)[0]) for c in range(1, 40)]
    assert first == sorted(first)
    assert np.array_equal(sizes[1:], np.bincount(labels.reshape(-1))[1:]) and sizes.sum() == mask.sum()


@pytest.mark.parametrize("name", sorted(cc.key_cases()))
def test_host_backend_matches_both_restatements(filled, name):
    from contrastive_lift_amd import components
    key = cc.key_cases()[name]
    for conn in cc.CONNECTIVITIES:
        labels, sizes = host(key, conn)
        ref_labels, ref_sizes, ref_roots = filled[(name, conn)]
        assert np.array_equal(labels, ref_labels) and np.array_equal(sizes, ref_sizes), (name, conn)
        sl, ss = cc.scipy_labels(key, conn)
        assert np.array_equal(sl, ref_labels) and np.array_equal(ss, ref_sizes), (name, conn)
        roots = components.component_roots(key, connectivity=conn, backend="host").numpy()
        assert roots.dtype == np.int32 and np.array_equal(roots, ref_roots), (name, conn)


def test_named_cases_have_the_stated_structure(filled):
    """A sanity check of the FIXTURES (tests/components_cases.py and its flood fill), not of the product: the inputs the other tests and
    the device are compared on really are what their names say."""
    n = cc.checkerboard().size
    assert filled[("checkerboard", 6)][1].shape[0] - 1 == n // 2 and (filled[("checkerboard", 6)][1][1:] == 1).all()
    assert filled[("checkerboard", 26)][1].shape[0] - 1 == 1
    assert int(cc.snake().sum()) == 1457 and filled[("snake", 6)][1].tolist() == [0, 1457]
    assert filled[("empty", 26)][1].tolist() == [0] and filled[("full", 6)][1].tolist() == [0, 6 * 11 * 21]
    key = cc.keyed()
    for conn in cc.CONNECTIVITIES:                             # equal keys join, different keys never do
        labels = filled[("keyed", conn)][0]
        for c in range(1, int(labels.max()) + 1):
            assert len(np.unique(key[labels == c])) == 1
        assert ((labels > 0) == (key != 0)).all()
    f = cc.floater_volume()
    for conn in cc.CONNECTIVITIES:                             # nothing touches, whatever the connectivity
        assert filled[("floater", conn)][1].shape[0] - 1 == f["n_components"] == 7
    assert sorted(filled[("split", "kuhn")][1].tolist()) == [0, 3, 120, 120, 210, 336]


def test_connectivity_names_and_refusals():
    from contrastive_lift_amd import components
    assert [components.connectivity_code(c) for c in (6, 26, 14, "kuhn", "6", "26")] == [6, 26, 14, 14, 6, 26]
    for conn in cc.CONNECTIVITIES:
        assert np.array_equal(components.structure(conn), cc.structure(conn))
    for bad in (18, "faces", None, 6.5):
        with pytest.raises(ValueError):
            components.label_components(cc.keyed(), connectivity=bad, backend="host")
    with pytest.raises(ValueError):
        components.label_components(cc.keyed(), backend="scipy")
    with pytest.raises(ValueError):
        components.label_components(cc.keyed()[0], backend="host")
    with pytest.raises(ValueError):
        components.label_components(cc.keyed().astype(np.float32), backend="host")
    from contrastive_lift_amd import _lib
    with pytest.raises(_lib.CliftError, match="wants the key on the GPU"):       # the device backend never falls back to the host
        components.label_components(torch.from_numpy(cc.keyed()), backend="device")
    src = open(os.path.join(REPO, "contrastive_lift_amd", "components.py")).read()
    assert "oracle" not in src


# ============================================================================ filter_components
def filtered(vol, level, **kw):
    from contrastive_lift_amd import components
    out, info = components.filter_components(torch.from_numpy(vol), level, backend="host", **kw)
    return out.numpy(), info


def test_filter_components_rules(filled):
    f = cc.floater_volume()
    vol, level = f["vol"], f["level"]
    labels, sizes, _ = filled[("floater", "kuhn")]
    assert sizes[1:].max() > 3000 and sorted(sizes[1:].tolist())[:3] == [1, 1, 1]
    before = vol.copy()
    out, info = filtered(vol, level, min_voxels=2)
    assert np.array_equal(vol.view(np.int32), before.view(np.int32))                         # the input is not modified
    assert info["K"] == 7 and np.array_equal(info["sizes"].numpy(), sizes) and info["dropped"] == 3
    assert info["kept"].tolist() == [c for c in range(1, 8) if sizes[c] >= 2]
    specks = np.zeros(vol.shape, bool)
    for s in cc.FLOATER_SPECKS:
        specks[s] = True
    assert np.array_equal(out.view(np.int32)[~specks], vol.view(np.int32)[~specks])          # everything else bit for bit
    assert np.isfinite(out[specks]).all() and (out[specks] < level).all() and (out[specks] == -np.finfo(np.float32).tiny).all()
    # min_voxels is "fewer than": a component of exactly that size stays
    small = int(np.sort(sizes[1:])[3])                                                       # the two tied small balls
    assert int((sizes == small).sum()) == 2
    assert filtered(vol, level, min_voxels=small)[1]["kept"].shape[0] == 4 and filtered(vol, level, min_voxels=small + 1)[1]["kept"].shape[0] == 2
    # keep_largest: by size, ties to the smaller first point (= the smaller id)
    order = sorted(range(1, 8), key=lambda c: (-sizes[c], c))
    for k in range(0, 9):
        out, info = filtered(vol, level, keep_largest=k)
        assert info["kept"].tolist() == sorted(order[:k]), k
        assert info["dropped"] == int(sizes[[c for c in range(1, 8) if c not in order[:k]]].sum())
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out >= level, np.isin(labels, order[:k]))
    tied = [c for c in range(1, 8) if sizes[c] == small]
    assert filtered(vol, level, keep_largest=3)[1]["kept"].tolist() == sorted([order[0], order[1], min(tied)])
    # both together; NaN is outside
    out, info = filtered(vol, level, min_voxels=small + 1, keep_largest=5)
    assert info["kept"].shape[0] == 2
    nan = vol.copy()
    nan[14, 15, 16] = np.nan                                                                 # the centre of the large ball: a hole of one point
    out, info = filtered(nan, level, min_voxels=2)
    assert np.isnan(out[14, 15, 16]) and info["K"] == 7 and info["sizes"].max() == sizes.max() - 1
    # both options off: the input object itself
    t = torch.from_numpy(vol)
    from contrastive_lift_amd import components
    same, info = components.filter_components(t, level, backend="host")
    assert same is t and info["dropped"] == 0
    with pytest.raises(ValueError):
        filtered(vol, float("inf"), min_voxels=2)


# ============================================================================ split_disconnected
def test_split_disconnected_rules():
    from contrastive_lift_amd import components
    key = cc.split_lattice()
    new, table = components.split_disconnected(torch.from_numpy(key), backend="host")
    new = new.numpy()
    assert new.dtype == key.dtype and table == {4: 2, 5: 2}                                  # 120 points -> 4, the crumb (3 points) -> 5
    assert (new[2:6, 12:17, 14:20] == 4).all() and (new[9, 16, 3:6] == 5).all() and (new[6:11, 2:8, 2:9] == 2).all()
    rest = np.ones(key.shape, bool)
    rest[2:6, 12:17, 14:20] = False
    rest[9, 16, 3:6] = False
    assert np.array_equal(new[rest], key[rest])
    new, table = components.split_disconnected(torch.from_numpy(key), min_voxels=4, backend="host")          # crumbs keep the parent's id
    assert table == {4: 2} and (new.numpy()[9, 16, 3:6] == 2).all() and (new.numpy()[2:6, 12:17, 14:20] == 4).all()
    # fresh ids: ascending original id, then descending size, then ascending first point
    row = cc.split_order_lattice()
    new, table = components.split_disconnected(row, backend="host")
    runs = lambda a: [int(a[0, 0, s]) for s in (1, 8, 14, 19, 27, 32)]
    assert runs(new.numpy()) == [1, 5, 3, 2, 4, 6] and table == {3: 1, 4: 1, 5: 2, 6: 2}
    new, table = components.split_disconnected(row, min_voxels=3, backend="host")
    assert runs(new.numpy()) == [1, 5, 3, 2, 4, 2] and table == {3: 1, 4: 1, 5: 2}
    assert np.array_equal(new.numpy() == 0, row == 0)
    new, table = components.split_disconnected(np.zeros((3, 3, 3), np.int32), backend="host")
    assert table == {} and not new.any() and new.dtype == torch.int32
    # a caller that holds ids the lattice does not: the fresh ids start above them, never below max(key) + 1
    new, table = components.split_disconnected(row, backend="host", first_fresh=10)
    assert runs(new.numpy()) == [1, 12, 10, 2, 11, 13] and table == {10: 1, 11: 1, 12: 2, 13: 2}
    assert components.split_disconnected(row, backend="host", first_fresh=2)[1] == {3: 1, 4: 1, 5: 2, 6: 2}
    # a bool key comes back int32, with or without components; negative ids are refused (max + 1 could be the background)
    mask = row > 0
    new, table = components.split_disconnected(mask, backend="host")
    assert new.dtype == torch.int32 and sorted(table) == [2, 3, 4, 5, 6] and set(table.values()) == {1}
    new, table = components.split_disconnected(np.zeros((3, 3, 3), bool), backend="host")
    assert new.dtype == torch.int32 and table == {}
    with pytest.raises(ValueError, match="positive"):
        components.split_disconnected(-row, backend="host")
    # connectivity decides what is one piece
    diag = np.zeros((1, 4, 4), np.int32)
    diag[0, 0, 0] = diag[0, 1, 1] = diag[0, 2, 1] = 7                                        # (0,0)-(1,1) is a Kuhn edge, not a face
    assert components.split_disconnected(diag, connectivity=6, backend="host")[1] == {8: 7}
    assert components.split_disconnected(diag, connectivity="kuhn", backend="host")[1] == {}


# ============================================================================ the mesh and its components
def test_vertex_owner_inside_against_the_restated_keys():
    from contrastive_lift_amd import components
    for case in (mc.random_case(0), mc.tie_case(), mc.open_case()):
        vol, level = case["vol"], case["level"]
        keys, _, _ = mc.marching_tetrahedra(vol, level, case["ticks"])
        got = components.vertex_owner_inside(keys, vol, level).numpy()
        owner = np.stack(np.unravel_index(keys // 7, vol.shape), 1)
        other = owner + np.asarray(mc.CLASS_OFFSETS)[keys % 7]
        own_in = vol[tuple(owner.T)] >= np.float32(level)
        exp = np.where(own_in, np.ravel_multi_index(tuple(owner.T), vol.shape), np.ravel_multi_index(tuple(other.T), vol.shape))
        assert np.array_equal(got, exp)
        assert (vol.reshape(-1)[got] >= np.float32(level)).all()                             # every active edge has exactly one inside end


def test_kuhn_connectivity_puts_every_face_in_one_component():
    """All vertex pairs of a Kuhn tetrahedron are Kuhn edges: the inside endpoints of a face's three vertices lie in one component under
    'kuhn' -- and not always under 6, which is why 6 is not the mesh's connectivity."""
    from contrastive_lift_amd import components
    split6 = 0
    for seed in (0, 1, 2):
        case = mc.random_case(seed)
        vol, level = case["vol"], case["level"]
        keys, _, faces = mc.marching_tetrahedra(vol, level, case["ticks"])
        inside = components.vertex_owner_inside(keys, vol, level).numpy()
        for conn in ("kuhn", 6):
            labels, _ = host(vol >= np.float32(level), conn)
            of_face = labels.reshape(-1)[inside][faces]                                      # (F, 3)
            assert (of_face > 0).all()
            one = (of_face == of_face[:, :1]).all(1)
            if conn == "kuhn":
                assert one.all(), f"random{seed}: a face between two components"
            else:
                split6 += int((~one).sum())
    assert split6 > 0


# ============================================================================ the library entry
def test_abi_27_declares_exports_and_binds_the_component_entry():
    from contrastive_lift_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "clift.h")).read(), flags=re.S)
    assert re.search(r"\bclift_cc_label\s*\(", src), "clift_cc_label is not declared in include/clift.h"
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clift_cc_label"), "clift_cc_label is not exported by libclift.so"
    assert "clift_cc_label" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 27 and _lib.load().clift_version() == 27
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "ABI 27 addition" in text and "clift_cc_label" in text, doc


def test_bad_arguments_are_refused_without_a_gpu():
    from contrastive_lift_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                    # never followed: every call below returns before it touches a buffer
    for n in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.clift_cc_label(p, *n, 14, p, None) != 0 and "positive" in lib.clift_last_error().decode(), n
    assert lib.clift_cc_label(p, 2048, 1024, 1024, 14, p, None) != 0
    assert "2^31" in lib.clift_last_error().decode() and "lattice points" in lib.clift_last_error().decode()
    for conn in (0, 7, 18, 27, -6):
        assert lib.clift_cc_label(p, 4, 4, 4, conn, p, None) != 0 and "connectivity" in lib.clift_last_error().decode(), conn
    for key, root in ((None, p), (p, None)):
        assert lib.clift_cc_label(key, 4, 4, 4, 6, root, None) != 0 and "NULL" in lib.clift_last_error().decode()


def test_extract_mesh_cli_component_flags():
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_cc", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    a = ap.parse_args(["--ckpt_path", "x.ckpt"])
    assert a.min_component == 0 and a.keep_largest is None and a.connectivity == "kuhn" and a.split_disconnected is None
    a = ap.parse_args(["--ckpt_path", "x.ckpt", "--min_component", "64", "--keep_largest", "3", "--connectivity", "26", "--split_disconnected"])
    assert a.min_component == 64 and a.keep_largest == 3 and a.connectivity == "26" and a.split_disconnected == 1
    assert ap.parse_args(["--ckpt_path", "x.ckpt", "--split_disconnected", "50", "--connectivity", "6"]).split_disconnected == 50
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt_path", "x.ckpt", "--connectivity", "18"])
