"""The count backends of the scoring code on the host: ``backend="counts"`` (overlap.label_overlap_numpy, the numpy restatement of
clift_label_overlap's contract) against ``backend="host"`` -- identical bits, not a tolerance: the counting is integer work and the matching
loop is one shared function.  Goldens G11, G16, G23, the random maps of test_pq_per_frame.py, the confusion matrix, the table cap and the
reject rules of the contract."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_close
import overlap_cases as oc

sys.path.insert(0, os.path.join(REPO, "tools"))

def _same_match(a, b):
    assert a[0] == b[0] and a[1] == b[1] and list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
    for x, y in zip(a[2:], b[2:]):
        assert x.dtype == y.dtype and x.shape == y.shape and bool((x == y).all())


def _same_pq(a, b):
    assert all(float(x) == float(y) or (np.isnan(float(x)) and np.isnan(float(y))) for x, y in zip(a, b)), (a, b)


def g23_cases():
    g = load_golden("g23_pq_per_frame")
    is_thing = [bool(x) for x in g["is_thing"]]
    for key, thing_list, faulty in (("mos0", [False, True], ()), ("mos1", [False, True], ()), ("pan0", is_thing, (0,)), ("pan1", is_thing, (0,))):
        names = [str(n) for n in g[f"{key}.names"]]
        d = {nm: {n: g[f"{key}.{nm}"][j] for j, n in enumerate(names)} for nm in ("sem_pred", "inst_pred", "sem_target", "inst_target")}
        yield key, d, thing_list, faulty, g[f"{key}.metrics"]


def test_g23_per_frame_counts_equals_host():
    from contrastive_lift_amd.metrics import panoptic_quality_per_frame
    for key, d, thing_list, faulty, want in g23_cases():
        host = panoptic_quality_per_frame(d["sem_pred"], d["inst_pred"], d["sem_target"], d["inst_target"], thing_list, faulty)
        got = panoptic_quality_per_frame(d["sem_pred"], d["inst_pred"], d["sem_target"], d["inst_target"], thing_list, faulty, backend="counts")
        assert got == host, key
        np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9, err_msg=key)
        # the stacked form: flat arrays + frame_off, frames in numeric order
        names = sorted(d["sem_pred"], key=lambda x: int(str(x).split(".")[0]))
        flat = [np.concatenate([np.asarray(d[nm][n]).reshape(-1) for n in names]) for nm in ("sem_pred", "inst_pred", "sem_target", "inst_target")]
        off = np.concatenate([[0], np.cumsum([np.asarray(d["sem_pred"][n]).size for n in names])])
        assert panoptic_quality_per_frame(*flat, thing_list, faulty, backend="counts", frame_off=off) == host, key


def test_g11_counts_equals_host():
    from contrastive_lift_amd.inference import ConfusionMatrix
    from contrastive_lift_amd.metrics import panoptic_quality, panoptic_quality_match
    g = load_golden("g11_metrics")
    T = lambda a: torch.from_numpy(np.asarray(a))
    for k in range(6):
        args = (T(g[f"pq{k}.preds"]), T(g[f"pq{k}.target"]), {1, 2}, {0, 3})
        _same_match(panoptic_quality_match(*args, allow_unknown_preds_category=True), panoptic_quality_match(*args, allow_unknown_preds_category=True, backend="counts"))
        got = panoptic_quality(*args, allow_unknown_preds_category=True, backend="counts")
        _same_pq(got, panoptic_quality(*args, allow_unknown_preds_category=True))
        rel_close(torch.stack(got), g[f"pq{k}.out"], 1e-6, atol=1e-9, what=f"pq case {k}")
    with pytest.raises(ValueError, match="Unknown categories"):
        panoptic_quality(T(g["pq0.preds"]), T(g["pq0.target"]), {1, 2}, {0, 3}, allow_unknown_preds_category=False, backend="counts")
    host, cnt = ConfusionMatrix(6, ignore_class=[0]), ConfusionMatrix(6, ignore_class=[0], backend="counts")
    a, b = host.add_batch(g["cm_pred"], g["cm_gt"], return_miou=True), cnt.add_batch(g["cm_pred"], g["cm_gt"], return_miou=True)
    assert a == b and bool((host.cm == cnt.cm).all()) and host.cm.dtype == cnt.cm.dtype and host.get_miou() == cnt.get_miou()
    rel_close(b, g["cm_batch_miou"], 1e-9, what="batch miou")
    rel_close(cnt.get_miou(), g["cm_miou"], 1e-9, what="miou")
    # ground truth outside [0, n) is left out, as the host mask does; the keyword of add_batch overrides the constructor's
    gt = np.concatenate([g["cm_pred"].reshape(-1), [-1, 6, 99]])
    pr = np.concatenate([g["cm_gt"].reshape(-1), [0, 1, 2]])
    assert bool((ConfusionMatrix(6)._matrix(gt, pr) == ConfusionMatrix(6)._matrix_counted(gt, pr, "counts")).all())
    c2 = ConfusionMatrix(6, ignore_class=[0])
    assert c2.add_batch(g["cm_pred"], g["cm_gt"], return_miou=True, backend="counts") == a
    with pytest.raises(ValueError):
        ConfusionMatrix(6, backend="gpu")


def test_g16_scene_evaluators_counts_equals_host(tmp_path):
    """The label sets of G16 (the scene generators + fake predictions of test_data_config.py, read as inference/evaluate.py reads them) through
    the confusion matrix and the scene-level match with both backends."""
    import make_synthetic_mos as gen_m
    import make_synthetic_panopli as gen_p
    from PIL import Image
    from make_fake_predictions import write_fake_predictions
    spec = importlib.util.spec_from_file_location("clift_eval_counts", os.path.join(REPO, "inference", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    g = load_golden("g16_scene_evaluators")
    root = gen_m.make_scene(str(tmp_path / "mos"), n_frames=10, size=24, seed=7)
    names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(root, "semantic")))
    val = names[int(len(names) * 0.8):]
    rng = np.random.default_rng(161)
    write_fake_predictions(str(tmp_path / "mos_exp"), val, [np.load(os.path.join(root, "semantic", n + ".npy")) for n in val],
                           [np.load(os.path.join(root, "instance", n + ".npy")) for n in val], rng)
    rootp = gen_p.make_scene(str(tmp_path / "pan"), n_frames=10, size=24, seed=5)
    test = [str(x) for x in json.load(open(os.path.join(rootp, "splits.json")))["test"]]
    rd = lambda d, n: np.array(Image.open(os.path.join(rootp, d, n + ".png")))
    write_fake_predictions(str(tmp_path / "pan_exp"), test, [rd("rs_semantics", n) for n in test], [rd("rs_instance", n) for n in test], rng)
    is_thing = [bool(x) for x in g["is_thing"]]
    from contrastive_lift_amd.inference import ConfusionMatrix
    from contrastive_lift_amd.metrics import panoptic_quality

    def both(pairs, n, things, stuff):
        """(mIoU, pq, sq, rq) of the scene evaluators -- every frame into the confusion matrix, all frames concatenated into one match --
        with the host and the counts backend."""
        out = []
        for backend in ("host", "counts"):
            cm = ConfusionMatrix(num_classes=n, ignore_class=[], backend=backend)
            for ps, pi, ts, ti in pairs:
                cm.add_batch(ps, ts)
            pred = np.concatenate([np.stack([ps, pi], -1) for ps, pi, ts, ti in pairs]).astype(np.int64)
            tgt = np.concatenate([np.stack([ts, ti], -1) for ps, pi, ts, ti in pairs]).astype(np.int64)
            pq = panoptic_quality(torch.from_numpy(pred), torch.from_numpy(tgt), things, stuff, allow_unknown_preds_category=True, backend=backend)
            out.append((cm.get_miou(),) + tuple(float(x) for x in pq))
        return out
    things_p, stuff_p = {i for i, t in enumerate(is_thing) if t}, {i for i, t in enumerate(is_thing) if not t}
    for tag in ("sq", "ns"):
        dim = tuple(int(x) for x in g[f"mos.{tag}.dim"])
        pairs = [(ev.read_png(tmp_path / "mos_exp" / "pred_semantics" / f"{n}.png", dim).reshape(-1), ev.read_png(tmp_path / "mos_exp" / "pred_surrogateid" / f"{n}.png", dim).reshape(-1),
                  ev.read_npy(os.path.join(root, "semantic", f"{n}.npy"), dim).reshape(-1), ev.read_npy(os.path.join(root, "instance", f"{n}.npy"), dim).reshape(-1)) for n in val]
        host, got = both(pairs, 2, {1}, {0})
        assert got == host and host == ev.evaluate_mos(str(tmp_path / "mos_exp"), root, dim)
        np.testing.assert_allclose(np.array(got), g[f"mos.{tag}.metrics"], rtol=1e-6, atol=1e-9)
        dim = tuple(int(x) for x in g[f"pan.{tag}.dim"])
        pairs = []
        for n in test:
            ts = ev.read_png(os.path.join(rootp, "rs_semantics", f"{n}.png"), dim)
            valid = ~np.isin(ts, [0])
            pairs.append((ev.read_png(tmp_path / "pan_exp" / "pred_semantics" / f"{n}.png", dim)[valid], ev.read_png(tmp_path / "pan_exp" / "pred_surrogateid" / f"{n}.png", dim)[valid],
                          ts[valid], ev.read_png(os.path.join(rootp, "rs_instance", f"{n}.png"), dim)[valid]))
        host, got = both(pairs, len(is_thing), things_p, stuff_p)
        assert got == host and host == ev.evaluate_panopli(str(tmp_path / "pan_exp"), rootp, dim, is_thing)
        np.testing.assert_allclose(np.array(got), g[f"pan.{tag}.metrics"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("seed", list(oc.SEEDS))
def test_random_maps_counts_equals_host(seed):
    from contrastive_lift_amd.metrics import panoptic_quality, panoptic_quality_match, panoptic_quality_per_frame
    p, t = oc.random_map(seed)
    _same_match(panoptic_quality_match(p, t, oc.THINGS, oc.STUFF, True), panoptic_quality_match(p, t, oc.THINGS, oc.STUFF, True, backend="counts"))
    _same_match(panoptic_quality_match(p.tolist(), t.tolist(), oc.THINGS, oc.STUFF, True), panoptic_quality_match(p.tolist(), t.tolist(), oc.THINGS, oc.STUFF, True, backend="counts"))
    _same_pq(panoptic_quality(torch.from_numpy(p), torch.from_numpy(t), oc.THINGS, oc.STUFF, True),
             panoptic_quality(torch.from_numpy(p), torch.from_numpy(t), oc.THINGS, oc.STUFF, True, backend="counts"))
    frames = oc.special_frames(seed)
    for name, (fp, ft) in frames.items():                          # every special frame on its own, with the robust filter at work
        host = panoptic_quality_match(fp, ft, oc.THINGS, oc.STUFF, True)
        _same_match(host, panoptic_quality_match(fp, ft, oc.THINGS, oc.STUFF, True, backend="counts"))
        if name in ("1", "2"):
            assert 2 not in host[0]                                # the rare class did fall under the robust share
        if name in ("3", "4", "5"):
            assert len(host[0]) == 0 and (name == "3") == (len(host[1]) > 0)
    d = [{n: f[side][:, col] for n, f in frames.items()} for side, col in ((0, 0), (0, 1), (1, 0), (1, 1))]
    for faulty in ((), (0,)):
        assert panoptic_quality_per_frame(*d, oc.IS_THING, faulty) == panoptic_quality_per_frame(*d, oc.IS_THING, faulty, backend="counts")


def test_table_cap():
    from contrastive_lift_amd import _lib, overlap
    from contrastive_lift_amd.metrics import panoptic_quality_match
    assert overlap.TABLE_CAP_BYTES == 1 << 30
    overlap.check_table(1, 1 << 14, 1 << 14)                       # exactly 1 GiB is allowed
    with pytest.raises(_lib.CliftError, match="1 GiB"):
        overlap.check_table(1, (1 << 14) + 1, 1 << 14)
    z = np.zeros(4, np.int32)
    one = np.zeros((1, 1), np.int32)
    with pytest.raises(_lib.CliftError, match="1 GiB"):
        overlap.label_overlap_numpy(z, None, z, None, [0, 4], one, one, one, one, 1 << 15, 1 << 15)
    # through the metric: two thing classes with instance ids up to 20 000 on both sides ask for a (1, 40 004, 40 004) table ...
    p = np.array([[1, 20000], [2, 3], [0, 0]] * 100)
    with pytest.raises(_lib.CliftError, match="1 GiB"):
        panoptic_quality_match(p, p.copy(), {1, 2}, {0}, True, robust=0.0, backend="counts")
    # ... while ids that are not read do not size the table: a huge id on a stuff pixel, and thing classes that the per-frame merge empties
    q = np.array([[1, 5], [2, 3], [0, 10 ** 6]] * 100)
    _same_match(panoptic_quality_match(q, q.copy(), {1, 2}, {0}, True, robust=0.0), panoptic_quality_match(q, q.copy(), {1, 2}, {0}, True, robust=0.0, backend="counts"))
    from contrastive_lift_amd.metrics import panoptic_quality_per_frame
    big = [{"0": np.array([1, 2, 3, 0] * 50)}, {"0": np.array([3000, 5, 7, 0] * 50)}, {"0": np.array([1, 2, 3, 0] * 50)}, {"0": np.array([3000, 4000, 5000, 0] * 50)}]
    assert panoptic_quality_per_frame(*big, [False, True, True, True], ()) == panoptic_quality_per_frame(*big, [False, True, True, True], (), backend="counts")


def test_reject_rules_of_the_contract():
    from contrastive_lift_amd import _lib, overlap
    from contrastive_lift_amd.metrics import panoptic_quality_match
    i32 = lambda *v: np.array(v, np.int32)
    tab = lambda *v: np.array([v], np.int32)
    kw = dict(frame_off=[0, 4], a_base=tab(0, 1), a_stride=tab(0, 1), b_base=tab(0, -1), b_stride=tab(0, 0), NA=3, NB=1)
    count = lambda a_cls, a_inst, b_cls: overlap.label_overlap_numpy(a_cls, a_inst, b_cls, None, **kw)
    c, r = count(i32(0, 1, 1, 0), i32(9, 0, 1, -4), i32(0, 0, 0, 0))            # nothing wrong: stride 0 ignores the instance
    assert r.tolist() == [0] and c[0, :, 0].tolist() == [2, 1, 1]
    assert count(i32(0, 2, -1, 0), i32(0, 0, 0, 0), i32(0, 0, 0, 0))[1].tolist() == [2]      # classes outside [0, Ca)
    assert count(i32(0, 0, 0, 0), i32(0, 0, 0, 0), i32(0, 2, 0, 0))[1].tolist() == [1]       # ... outside [0, Cb)
    assert count(i32(1, 1, 0, 0), i32(2, 1, 0, 0), i32(0, 0, 0, 0))[1].tolist() == [1]       # slot 1 + 2 outside [0, NA)
    assert count(i32(1, 1, 0, 0), i32(-1, 1, 0, 0), i32(0, 0, 0, 0))[1].tolist() == [1]      # negative instance under stride 1
    c, r = count(i32(1, 1, 0, 0), None, i32(0, 0, 0, 0))                                     # no instance array under stride 1
    assert r.tolist() == [2] and int(c.sum()) == 2
    c, r = count(i32(1, 1, 0, 2), i32(-1, 5, 0, 0), i32(1, 1, 1, 1))                         # a dropped row is not rejected ... but a class outside is
    assert r.tolist() == [1] and int(c.sum()) == 0
    for bad in (dict(frame_off=[0, 5, 4]), dict(frame_off=[1, 4]), dict(NA=0)):
        with pytest.raises(_lib.CliftError):
            overlap.label_overlap_numpy(i32(0, 0, 0, 0), None, i32(0, 0, 0, 0), None, **{**kw, **bad})
    # the wrapper raises on rejected rows: a negative instance id of a thing class cannot be scored by a count backend
    p = np.array([[1, 2], [1, -3], [0, 0], [0, 0]])
    with pytest.raises(_lib.CliftError, match="rejected"):
        panoptic_quality_match(p, p.copy(), {1}, {0}, True, backend="counts")
    with pytest.raises(ValueError, match="backend"):
        panoptic_quality_match(p, p.copy(), {1}, {0}, True, backend="numpy")
    # a label that would wrap to a valid id in the int32 cast is refused, not counted; a stuff pixel's instance id is never read
    for bad in ([[1, 2 ** 32 + 1], [0, 0]], [[-2 ** 32 + 1, 0], [0, 0]]):
        with pytest.raises(_lib.CliftError, match="int32"):
            panoptic_quality_match(np.array(bad), np.array([[1, 1], [0, 0]]), {1}, {0}, True, backend="counts")
    p = np.array([[1, 2], [1, 3], [0, -7], [0, 2 ** 40]])
    a, b = panoptic_quality_match(p, p.copy(), {1}, {0}, True, robust=0.0), panoptic_quality_match(p, p.copy(), {1}, {0}, True, robust=0.0, backend="counts")
    assert all(bool((x == y).all()) for x, y in zip(a[2:], b[2:]))


def test_abi_table_has_the_overlap_entry():
    from contrastive_lift_amd import _lib
    args, res = _lib._SIGNATURES["clift_label_overlap"]
    assert len(args) == 17 and res is not None
    src = open(os.path.join(REPO, "include", "clift.h")).read()
    assert "int clift_label_overlap(" in src
    assert "overlap.hip" in open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "Makefile")).read()
