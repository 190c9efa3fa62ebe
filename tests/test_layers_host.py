"""Amodal instance layers on the host: the fp32 restatement of the per-ray recurrence against the fp64 object-alone reference,
the slot table's fixed numbering, the per-slot summary and the front order on a hand-made array, and the new command-line flags."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import layers_cases as lc
from conftest import REPO

F32 = np.float32


def _rays(N, seed):
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((N, 3))
    o = 0.95 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.3, 0.3, (N, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((N, 1), 0.01), np.full((N, 1), 4.0)], 1).astype(F32)
    return rays, rng.random(N).astype(F32)


@pytest.mark.parametrize("K", [0, 1, 5, 64])
@pytest.mark.parametrize("S", [1, 64, 70, 130])
def test_restatement_against_the_object_alone_reference(S, K):
    """A, V and Z of the fp32 recurrence within (n_r + 3) 2^-23 RELATIVE of the fp64 composite of the column alone, n_r the entries of the
    ray.  Both sides take the same fp32 distances here (the distances' own rounding is the GPU test's zf check).  The alphas are 0, 1 or
    at least 1/16: A = 1 - Tc cancels, one entry of alpha a leaves |A32 - A64| up to 2^-25 (the rounding of 1 - a), which is within
    4 * 2^-23 of A = a only from a = 1/16 on.  Below that no bound relative to A itself can hold; the second half of the test holds such
    alphas (down to 1e-4) to the same figure as an ABSOLUTE error, which is what the cancellation leaves."""
    N = 9
    rays, jitter = _rays(N, S)
    z = lc.sample_z(rays, [-1.0] * 3, [1.0] * 3, 0.03, S, jitter)
    for floor, relative in ((1.0 / 16, True), (1e-4, False)):
        m = lc.made_up_layers(N, S, K, seed=100 * S + K, alpha_floor=floor)
        rest = lc.layers_restatement(m["alpha"], m["w"], z, m["ray_start"], m["act_idx"], m["slot"], K)
        ref, n_r = lc.object_alone_reference(m["alpha"], m["w"], z.astype(np.float64), m["ray_start"], m["act_idx"], m["slot"], K)
        assert rest.shape == ref.shape == (N, K + 1, 4) and rest.dtype == F32
        bound = ((n_r + 3) * lc.EPS)[:, None]
        for i, name in enumerate("AVZ"):
            err = np.abs(rest[..., i].astype(np.float64) - ref[..., i])
            scale = np.abs(ref[..., i]) if (relative or name != "A") else np.ones_like(err)
            worst = (err / np.where(scale > 0, scale, 1.0) / bound).max()
            print(f"S {S} K {K} alpha >= {floor:g}: {name} worst error {worst:.3f} of (n_r + 3) 2^-23 {'relative' if relative or name != 'A' else 'absolute'}")
            assert (err <= bound * scale).all(), name
        assert np.array_equal(rest[..., 3].astype(np.float64), ref[..., 3])               # zf: the same fp32 number
        empty = ref[..., 0] == 0
        assert (rest[empty][:, [0, 2]] == 0).all()                                        # a column of alpha 0 entries only: A and Z exactly 0
        # the rest column collects -1, K and everything past K; the stray entries of ray 2 took no part
        listed = np.diff(m["ray_start"])
        assert n_r[2] == listed[2] - 3 and (np.delete(n_r, 2) == np.delete(listed, 2)).all()
        assert (rest[listed == 0] == 0).all()


def test_two_surface_ray_the_wall_is_whole_behind_the_shell():
    """shell = slot 0, wall = slot 1: alone the wall is opaque (A_1 = 1) while the scene shows it through the shell only:
    V_1 = A_1 (1 - alpha_shell)."""
    Tr, w, z, _ = lc.two_surface_ray(S=64, shell=5, wall=40, alpha_shell=0.4)
    alpha = np.zeros((1, 64), F32)
    alpha[0, 5], alpha[0, 40] = 0.4, 1.0
    out = lc.layers_restatement(alpha, w, z, [0, 2], [5, 40], [0, 1], 2)
    assert out[0, 1, 0] == 1.0 and abs(out[0, 1, 1] - 0.6) < 1e-6 and abs(out[0, 0, 0] - 0.4) < 1e-6 and out[0, 0, 1] == w[0, 5]
    assert out[0, 0, 3] == z[0, 5] and out[0, 1, 3] == z[0, 40] and (out[0, 2] == 0).all()


def test_slot_table_numbering():
    from contrastive_lift_amd.layers import SlotTable
    cents = {2: np.zeros((3, 4), F32), 5: np.ones((2, 4), F32), 4: np.zeros((0, 4), F32), 9: np.ones((1, 4), F32)}
    # thing classes 1 (no centroids at all), 2, 4 (an empty array), 5, 7 (absent from the dict); 9 is past num_classes
    t = SlotTable.from_centroids(cents, [5, 1, 2, 4, 7, 9], 8)
    assert t.K == 5 and t.mode == 0 and t.E == 4 and t.num_classes == 8
    assert t.slot_class.tolist() == [2, 2, 2, 5, 5] and t.slot_index.tolist() == [0, 1, 2, 0, 1]
    want = np.zeros((8, 2), np.int32)
    want[2], want[5] = (0, 3), (3, 2)
    assert np.array_equal(t.cls_slots, want) and t.cls_slots.dtype == np.int32
    assert np.array_equal(t.centroids, np.concatenate([cents[2], cents[5]]))
    # the numbering does not depend on what else is there: dropping class 5's frames' worth of nothing changes nothing, and an order of
    # thing_classes does not matter
    t2 = SlotTable.from_centroids(cents, [2, 5], 8)
    assert np.array_equal(t2.cls_slots, t.cls_slots) and t2.slot_class.tolist() == t.slot_class.tolist()
    empty = SlotTable.from_centroids({}, [1, 2], 4)
    assert empty.K == 0 and empty.centroids.shape[0] == 0 and not empty.cls_slots.any()
    s = SlotTable.from_scores([1, 3], 4, 6)
    assert s.K == 6 and s.mode == 1 and s.centroids is None and s.cls_slots.tolist() == [[0, 0], [0, 6], [0, 0], [0, 6]]
    assert s.slot_class.tolist() == [-1] * 6 and s.slot_index.tolist() == list(range(6))
    SlotTable.from_centroids({1: np.zeros((255, 2), F32)}, [1], 2)
    with pytest.raises(ValueError, match="255"):
        SlotTable.from_centroids({1: np.zeros((200, 2), F32), 2: np.zeros((56, 2), F32)}, [1, 2], 3)
    with pytest.raises(ValueError, match="255"):
        SlotTable.from_scores([1], 2, 256)
    with pytest.raises(ValueError, match="width"):
        SlotTable.from_centroids({1: np.zeros((2, 2), F32), 2: np.zeros((2, 3), F32)}, [1, 2], 3)


def test_summarise_and_front_order_on_a_hand_made_array():
    from contrastive_lift_amd import layers as ly
    t = ly.SlotTable.from_centroids({1: np.zeros((2, 3), F32)}, [1], 2)
    #                  slot 0                  slot 1                  rest
    L = torch.tensor([[[0.8, 0.2, 1.6, 2.5], [0.9, 0.9, 0.9, 1.0], [1.0, 0.1, 3.0, 3.0]],
                      [[0.6, 0.6, 1.5, 2.0], [0.0, 0.0, 0.0, 0.0], [0.3, 0.3, 0.9, 3.0]]])
    s = ly.summarise(L, t, level=0.5)
    assert s["amodal_pixels"].tolist() == [2, 1] and s["visible_pixels"].tolist() == [1, 1]
    assert s["slot_class"].tolist() == [1, 1] and s["slot_index"].tolist() == [0, 1]
    np.testing.assert_allclose(s["occlusion"].numpy(), [1 - 0.8 / 1.4, 0.0], atol=1e-6)
    np.testing.assert_allclose(s["mean_distance"].numpy(), [(1.6 / 0.8 + 1.5 / 0.6) / 2, 1.0], atol=1e-6)
    order, count = ly.front_order(L, 0.5)
    assert order.tolist() == [[1, 0], [0, -1]] and count.tolist() == [2, 1]
    order, count = ly.front_order(L, 0.85)
    assert order.tolist() == [[1, -1], [-1, -1]] and count.tolist() == [1, 0]
    none = ly.summarise(torch.zeros((3, 3, 4)), t)
    assert none["occlusion"].tolist() == [0, 0] and none["mean_distance"].tolist() == [0, 0] and none["amodal_pixels"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="columns"):
        ly.summarise(torch.zeros((3, 5, 4)), t)
    with pytest.raises(ValueError, match="K \\+ 1"):
        ly.front_order(torch.zeros((3, 4)))


def test_the_parser_knows_the_new_flags():
    spec = importlib.util.spec_from_file_location("clift_render_cli_layers_host", os.path.join(REPO, "inference", "render_panopli.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    ap = rp.build_parser()
    a = ap.parse_args(["--ckpt_path", "x.ckpt"])
    assert a.save_layers is False and a.layers_level == 0.5
    a = ap.parse_args(["--ckpt_path", "x.ckpt", "--save_layers", "--layers_level", "0.25", "--cached_centroids_path", "c.pkl"])
    assert a.save_layers is True and a.layers_level == 0.25
    a = ap.parse_args(["--ckpt_path", "x.ckpt", "--save_surface"])                         # the flags from before are still there
    assert a.save_surface is True and a.pointcloud_depth == "expected"
