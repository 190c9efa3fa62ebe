"""Amodal colour layers on the host: the fp32 restatement of clift_ray_layer_colour against the fp64 column-alone reference
and against the restatement of clift_ray_layers, what an entry without a colour does, the two pure helpers of contrastive_lift_amd.layers
on a hand-made array, and the new flags of both command lines."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import layers_cases as lc
import layers_colour_cases as lcc
from conftest import REPO

F32 = np.float32


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("K", [0, 1, 5, 64])
@pytest.mark.parametrize("S", [1, 64, 70, 130])
def test_restatement_against_the_column_alone_reference(S, K):
    """R, G and B of the fp32 recurrence within (n_r + 3) 2^-23 RELATIVE of the fp64 composite of the column alone for alphas of 0, 1 or at
    least 1/16, and the same figure as an ABSOLUTE error for alphas down to 1e-4 -- with one colour per list row (rgb_row None) and through
    an indirect rgb_row with rows that have no colour.  A has the bits of the layer restatement's A on the same list."""
    N = 9
    for floor, relative in ((1.0 / 16, True), (1e-4, False)):
        m = lcc.made_up_colour_layers(N, S, K, seed=100 * S + K, alpha_floor=floor)
        z = np.zeros((N, S), F32)
        layers = lc.layers_restatement(m["alpha"], m["w"], z, m["ray_start"], m["act_idx"], m["slot"], K)
        for rgb, rgb_row, how in ((m["rgb"], None, "direct"), (m["rgb_perm"], m["rgb_row"], "indirect")):
            rest = lcc.colour_restatement(m["alpha"], m["ray_start"], m["act_idx"], m["slot"], K, rgb, rgb_row)
            ref, n_r = lcc.colour_alone_reference(m["alpha"], m["ray_start"], m["act_idx"], m["slot"], K, rgb, rgb_row)
            assert rest.shape == ref.shape == (N, K + 1, 4) and rest.dtype == F32
            lcc.check_colour(rest, ref, n_r, what=f"S {S} K {K} alpha >= {floor:g} {how}", relative=relative)
            assert np.array_equal(rest[..., 3].view(np.uint32), layers[..., 0].view(np.uint32))         # A: the bits of clift_ray_layers' A
            assert (rest[..., :3] >= 0).all()
            listed = np.diff(m["ray_start"])
            assert (rest[listed == 0] == 0).all()
        if m["act_idx"].size >= 3:
            assert (m["rgb_row"] == -1).any() and (m["rgb_row"] == m["rgb_perm"].shape[0]).any()


def test_an_entry_without_a_colour_changes_the_opacity_and_no_colour():
    """One ray, one column: a coloured entry, an uncoloured one (rgb_row -1), a coloured one.  Against the same list without the middle
    entry: A differs (the middle entry is opaque matter), the colour of the first entry is untouched, and what lies behind is attenuated
    by it.  Against the same list with the middle entry's alpha but a colour of zeros: every bit equal."""
    alpha = np.asarray([[0.25, 0.5, 0.75]], F32)
    rgb = np.asarray([[1.0, 0.5, 0.25], [9.0, 9.0, 9.0], [0.5, 1.0, 0.0]], F32)
    start, act, slot = np.asarray([0, 3], np.int32), np.asarray([0, 1, 2], np.int32), np.zeros(3, np.int32)
    without = lcc.colour_restatement(alpha, start, act, slot, 1, rgb, np.asarray([0, -1, 2], np.int32))
    black = lcc.colour_restatement(alpha, start, act, slot, 1, np.where(np.arange(3)[:, None] == 1, F32(0), rgb), None)
    assert np.array_equal(without.view(np.uint32), black.view(np.uint32))
    past = lcc.colour_restatement(alpha, start, act, slot, 1, rgb, np.asarray([0, 3, 2], np.int32))             # n_rgb itself: no colour either
    assert np.array_equal(past.view(np.uint32), without.view(np.uint32))
    shorter = lcc.colour_restatement(alpha, np.asarray([0, 2], np.int32), np.asarray([0, 2], np.int32), np.zeros(2, np.int32), 1, rgb,
                                     np.asarray([0, 2], np.int32))
    assert without[0, 0, 3] == F32(1 - 0.75 * 0.5 * 0.25) and shorter[0, 0, 3] == F32(1 - 0.75 * 0.25) and without[0, 0, 3] != shorter[0, 0, 3]
    # exact in fp32: R = 0.25 * 1 + (0.75 * 0.5 * 0.75) * 0.5; without the middle entry the third term is twice as large
    assert without[0, 0, 0] == F32(0.25 + 0.28125 * 0.5) and shorter[0, 0, 0] == F32(0.25 + 0.5625 * 0.5)
    assert (without[0, 1] == 0).all()


def test_unpremultiply_and_over_on_a_hand_made_array():
    from contrastive_lift_amd import layers as ly
    c = torch.tensor([[[0.2, 0.1, 0.0, 0.4], [0.0, 0.0, 0.0, 0.0]],
                      [[0.5, 0.25, 1.0, 1.0], [1e-8, 1e-8, 1e-8, 5e-7]]])
    u = ly.unpremultiply(c)
    assert u.shape == c.shape
    np.testing.assert_allclose(u[0, 0].numpy(), [0.5, 0.25, 0.0, 0.4], rtol=1e-6)
    assert u[0, 1].tolist() == [0, 0, 0, 0] and u[1, 0].tolist() == [0.5, 0.25, 1.0, 1.0]
    assert u[1, 1, :3].tolist() == [0, 0, 0] and float(u[1, 1, 3]) == float(c[1, 1, 3])     # A <= eps: colour 0, A kept
    np.testing.assert_allclose(ly.unpremultiply(c, eps=1e-7)[1, 1, :3].numpy(), [0.02] * 3, rtol=1e-5)
    o = ly.over(c, torch.tensor([1.0, 0.5, 0.0]))
    assert o.shape == (2, 2, 3)
    np.testing.assert_allclose(o[0, 0].numpy(), [0.2 + 0.6, 0.1 + 0.3, 0.0], rtol=1e-6)
    np.testing.assert_allclose(o[0, 1].numpy(), [1.0, 0.5, 0.0], rtol=1e-6)               # nothing there: the background
    np.testing.assert_allclose(o[1, 0].numpy(), [0.5, 0.25, 1.0], rtol=1e-6)              # opaque: the colour
    np.testing.assert_allclose(ly.over(c, 1.0)[0, 0].numpy(), [0.8, 0.7, 0.6], rtol=1e-6)  # a scalar background
    assert ly.unpremultiply(np.zeros((3, 4), F32)).shape == (3, 4)
    with pytest.raises(ValueError, match="R, G, B, A"):
        ly.unpremultiply(torch.zeros((3, 3)))
    with pytest.raises(ValueError, match="R, G, B, A"):
        ly.over(torch.zeros((3, 5)), 0.0)


def test_both_parsers_know_the_colour_flags(capsys):
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_colour_host")
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_cli_colour_host")
    cases = ((rp, ["--ckpt_path", "x.ckpt"]), (es, ["--ckpt_path", "x.ckpt", "--bboxes", "b.pkl", "--instance", "3", "--op", "copy"]))
    for mod, base in cases:
        a = mod.parse_args(base)
        assert a.layers_colour is False and a.layers_colour_rest is False and a.save_layers is False and a.layers_level == 0.5
        a = mod.parse_args(base + ["--save_layers", "--layers_colour"])
        assert a.save_layers is True and a.layers_colour is True and a.layers_colour_rest is False
        a = mod.parse_args(base + ["--save_layers", "--layers_colour", "--layers_colour_rest", "--layers_level", "0.25"])
        assert a.layers_colour is True and a.layers_colour_rest is True and a.layers_level == 0.25
        for bad, word in ((["--layers_colour"], "--layers_colour needs --save_layers"),
                          (["--layers_colour", "--layers_colour_rest"], "--layers_colour needs --save_layers"),
                          (["--save_layers", "--layers_colour_rest"], "--layers_colour_rest needs --layers_colour")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(base + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err               # a parser error, not a traceback
    a = rp.build_parser().parse_args(["--ckpt_path", "x.ckpt", "--save_surface"])           # the flags from before are still there
    assert a.save_surface is True and a.pointcloud_depth == "expected"


def test_the_checkpoint_functions_refuse_colour_without_layers():
    """The keyword route of both tools says the same before anything is loaded."""
    rp = _load(os.path.join(REPO, "inference", "render_panopli.py"), "clift_render_cli_colour_host2")
    es = _load(os.path.join(REPO, "inference", "edit_scene.py"), "clift_edit_cli_colour_host2")
    with pytest.raises(ValueError, match="layers_colour needs save_layers"):
        rp.render_panopli_checkpoint(None, "trajectory_blender", layers_colour=True)
    with pytest.raises(ValueError, match="layers_colour needs save_layers"):
        es.edit_scene_checkpoint(None, None, "x", layers_colour=True)
