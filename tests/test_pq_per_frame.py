"""metrics.panoptic_quality_per_frame against the reference's per-frame PQ of the bandwidth search (golden G23, tests/golden/make_pq_golden.py),
and the match / compute split of panoptic_quality."""
import numpy as np

from conftest import load_golden


def test_per_frame_pq_vs_reference():
    from contrastive_lift_amd.metrics import panoptic_quality_per_frame
    g = load_golden("g23_pq_per_frame")
    is_thing = [bool(x) for x in g["is_thing"]]
    for key, thing_list, faulty in (("mos0", [False, True], ()), ("mos1", [False, True], ()), ("pan0", is_thing, (0,)), ("pan1", is_thing, (0,))):
        names = [str(n) for n in g[f"{key}.names"]]
        d = {nm: {n: g[f"{key}.{nm}"][j] for j, n in enumerate(names)} for nm in ("sem_pred", "inst_pred", "sem_target", "inst_target")}
        got = panoptic_quality_per_frame(d["sem_pred"], d["inst_pred"], d["sem_target"], d["inst_target"], thing_list, faulty)
        np.testing.assert_allclose(got, g[f"{key}.metrics"], rtol=1e-7, atol=1e-9, err_msg=key)      # (the reference divides areas in fp32)


def test_match_compute_split_is_panoptic_quality():
    import torch
    from contrastive_lift_amd.metrics import panoptic_quality, panoptic_quality_compute, panoptic_quality_match
    rng = np.random.default_rng(4)
    t = np.stack([rng.integers(0, 4, 4000), rng.integers(0, 5, 4000)], -1)
    p = t.copy()
    p[rng.uniform(0, 1, 4000) < 0.2] = [1, 7]
    whole = panoptic_quality(torch.from_numpy(p), torch.from_numpy(t), {1, 2}, {0, 3}, True)
    split = panoptic_quality_compute(*panoptic_quality_match(p, t, {1, 2}, {0, 3}, True))
    assert all(float(a) == float(b) for a, b in zip(whole, split))
