#!/usr/bin/env python3
"""Golden G23: the per-frame PQ by which the reference's bandwidth search scores a clustering (inference/find_bandwidth.py:314-376,
MY_calculate_panoptic_quality_per_frame_folders and its _MOS twin), computed by the REFERENCE on small fake label images.

    python tests/golden/make_pq_golden.py            # needs the reference checkout (CL_REFERENCE, read-only, never copied)

The reference module is imported with the stand-in modules of make_golden.py (its third-party imports contribute no arithmetic to
the scoring).  Stored: the images (inputs), the is_thing list the ScanNet variant reads from resources/scannet_reduced_things.csv,
and the (pq, sq, rq) the reference returns.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402  (puts the reference and the repository on sys.path)


def fake_frames(rng, n, H, W, classes, things, n_inst=6, flip=0.1):
    """Target / prediction pairs: blocky class and instance maps, the prediction = target with a fraction of pixels relabelled and the
    instance ids permuted (what a clustering that found the objects writes)."""
    sem_t, inst_t, sem_p, inst_p = {}, {}, {}, {}
    for f in range(n):
        name = f"{3 * f + 1}.png"
        s = rng.choice(classes, size=(H // 4, W // 4)).repeat(4, 0).repeat(4, 1)
        i = rng.integers(1, n_inst + 1, size=(H // 8, W // 8)).repeat(8, 0).repeat(8, 1)
        i = np.where(np.isin(s, things), i, 0)
        perm = np.concatenate([[0], 1 + rng.permutation(n_inst + 2)])
        ps = np.where(rng.uniform(0, 1, s.shape) < flip, rng.choice(classes, size=s.shape), s)
        ps = np.where(np.isin(ps, things), things[0], ps)                     # the sweep's single-class predictions
        pi = np.where(rng.uniform(0, 1, s.shape) < flip, rng.integers(0, n_inst + 3, size=s.shape), perm[i])
        sem_t[name], inst_t[name] = s.astype(np.uint8), i.astype(np.uint8)
        sem_p[name], inst_p[name] = ps.astype(np.uint8), pi.astype(np.int32)
    return sem_p, inst_p, sem_t, inst_t


def main():
    mg.install_stand_ins()
    mg.install_quaternion()
    sys.modules["hdbscan"].HDBSCAN = mg._Inert
    cwd = os.getcwd()
    os.chdir(mg.REF)                                 # get_thing_semantics reads resources/ relative to the working directory
    try:
        with mg.quiet():
            FB = importlib.import_module("inference.find_bandwidth")
        from dataset.preprocessing.preprocess_scannet import get_thing_semantics
        is_thing = get_thing_semantics()
        rng = np.random.default_rng(23)
        out = {"is_thing": np.array(is_thing)}
        things = [i for i, t in enumerate(is_thing) if t]
        stuff = [i for i, t in enumerate(is_thing) if not t]
        for tag, fn, classes, th in (("mos", FB.MY_calculate_panoptic_quality_per_frame_folders_MOS, [0, 1], [1]),
                                     ("pan", FB.MY_calculate_panoptic_quality_per_frame_folders, [0] + stuff[1:4] + things[:3], things[:3])):
            for k, flip in enumerate((0.05, 0.3)):
                sp, ip, st, it = fake_frames(rng, 4, 32, 48, np.array(classes), np.array(th), flip=flip)
                with mg.quiet():
                    pq, sq, rq = fn(sp, ip, st, it)
                key = f"{tag}{k}"
                out[f"{key}.names"] = np.array(list(sp))
                for nm, d in (("sem_pred", sp), ("inst_pred", ip), ("sem_target", st), ("inst_target", it)):
                    out[f"{key}.{nm}"] = np.stack([d[n] for n in sp])
                out[f"{key}.metrics"] = np.array([pq, sq, rq])
                print(key, pq, sq, rq)
    finally:
        os.chdir(cwd)
    mg.npz("g23_pq_per_frame", **out)


if __name__ == "__main__":
    main()
