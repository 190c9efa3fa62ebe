"""clift_label_overlap (csrc/overlap.hip) on the GPU: the kernel against the numpy restatement of its contract (``==``, it is integer
counting), its error returns, and ``backend="device"`` of the scoring code against ``backend="host"`` -- identical bits -- on goldens G23
and G11, the random maps and the confusion matrix."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import overlap_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """(inputs, numpy counts, numpy rejected) of every kernel case: the reference is computed once."""
    from contrastive_lift_amd import overlap
    out = {}
    for c in oc.kernel_cases():
        kw = {k: v for k, v in c.items() if k != "name"}
        out[c["name"]] = (kw,) + overlap.label_overlap_numpy(**kw)
    return out


@pytest.mark.parametrize("name", [c["name"] for c in oc.kernel_cases()])
def test_kernel_equals_numpy_restatement(cases, name):
    from contrastive_lift_amd import overlap
    kw, want_counts, want_rej = cases[name]
    args = {k: (_dev(v) if k != "frame_off" and isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    counts, rej = overlap.label_overlap(**args)
    again, rej2 = overlap.label_overlap(**args)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int32 and tuple(counts.shape) == want_counts.shape
    assert bool((counts.cpu().numpy() == want_counts).all()) and bool((rej.cpu().numpy() == want_rej).all())
    assert torch.equal(counts, again) and torch.equal(rej, rej2)                       # two runs: identical tensors
    if name == "drop_and_reject":
        assert int(want_rej.sum()) > 0 and int(want_counts.sum()) + int(want_rej.sum()) < int(kw["frame_off"][-1])      # rejected AND dropped rows exist


def test_error_returns_and_empty_input():
    from contrastive_lift_amd import _lib, overlap
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    tab = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 8], dtype=torch.int64, device=DEV)
    counts, rej = torch.full((1, 1, 1), -7, dtype=torch.int32, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV)
    P = _lib.ptr

    def call(a_cls=z, frame_off=off, F=1, NA=1, NB=1, out=counts):
        _lib.call("clift_label_overlap", P(a_cls), None, P(z), None, P(frame_off), F, P(tab), P(tab), 1, P(tab), P(tab), 1, NA, NB, P(out), P(rej), _lib.stream())
    with pytest.raises(_lib.CliftError, match="NULL"):
        call(out=None)
    with pytest.raises(_lib.CliftError, match="NULL"):
        call(a_cls=None)
    with pytest.raises(_lib.CliftError, match="NA >= 1"):
        call(NA=0)
    with pytest.raises(_lib.CliftError, match="F >= 0"):
        call(F=-1)
    call(F=0)                                                                          # the no-op: nothing is touched
    torch.cuda.synchronize()
    assert int(counts[0, 0, 0]) == -7 and int(rej[0]) == -7
    call()                                                                             # and the call clears and fills the tables itself
    assert int(counts[0, 0, 0]) == 8 and int(rej[0]) == 0
    call(frame_off=torch.zeros(2, dtype=torch.int64, device=DEV))                      # no rows: the cleared tables
    assert int(counts[0, 0, 0]) == 0 and int(rej[0]) == 0
    c, r = overlap.label_overlap(z[:0], None, z[:0], None, [0, 0, 0], tab.expand(2, 1).contiguous(), tab.expand(2, 1).contiguous(),
                                 tab.expand(2, 1).contiguous(), tab.expand(2, 1).contiguous(), 2, 3)
    assert tuple(c.shape) == (2, 2, 3) and int(c.abs().sum()) == 0 and int(r.abs().sum()) == 0
    with pytest.raises(_lib.CliftError, match="1 GiB"):
        overlap.label_overlap(z, None, z, None, [0, 8], tab, tab, tab, tab, 1 << 15, 1 << 15)
    with pytest.raises(_lib.CliftError, match="CUDA"):
        overlap.label_overlap(z.cpu(), None, z.cpu(), None, [0, 8], tab, tab, tab, tab, 1, 1)


def _same_match(a, b):
    assert a[0] == b[0] and a[1] == b[1] and list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
    for x, y in zip(a[2:], b[2:]):
        assert x.dtype == y.dtype and x.shape == y.shape and bool((x == y).all())


def test_device_backend_equals_host_on_goldens():
    from contrastive_lift_amd.inference import ConfusionMatrix
    from contrastive_lift_amd.metrics import panoptic_quality, panoptic_quality_match, panoptic_quality_per_frame
    g = load_golden("g23_pq_per_frame")
    is_thing = [bool(x) for x in g["is_thing"]]
    for key, thing_list, faulty in (("mos0", [False, True], ()), ("mos1", [False, True], ()), ("pan0", is_thing, (0,)), ("pan1", is_thing, (0,))):
        names = [str(n) for n in g[f"{key}.names"]]
        d = [{n: g[f"{key}.{nm}"][j] for j, n in enumerate(names)} for nm in ("sem_pred", "inst_pred", "sem_target", "inst_target")]
        host = panoptic_quality_per_frame(*d, thing_list, faulty)
        assert panoptic_quality_per_frame(*d, thing_list, faulty, backend="device") == host, key
        order = sorted(names, key=lambda x: int(str(x).split(".")[0]))
        stacked = [torch.from_numpy(np.stack([np.asarray(x[n]) for n in order]).astype(np.int32)).to(DEV) for x in d]      # (F, H, W) device tensors
        assert panoptic_quality_per_frame(*stacked, thing_list, faulty, backend="device") == host, key
        np.testing.assert_allclose(host, g[f"{key}.metrics"], rtol=1e-7, atol=1e-9, err_msg=key)
    g = load_golden("g11_metrics")
    T = lambda a: torch.from_numpy(np.asarray(a))
    for k in range(6):
        p, t = T(g[f"pq{k}.preds"]), T(g[f"pq{k}.target"])
        _same_match(panoptic_quality_match(p, t, {1, 2}, {0, 3}, True), panoptic_quality_match(p.to(DEV), t.to(DEV), {1, 2}, {0, 3}, True, backend="device"))
        a, b = panoptic_quality(p, t, {1, 2}, {0, 3}, True), panoptic_quality(p.to(DEV), t.to(DEV), {1, 2}, {0, 3}, True, backend="device")
        assert all(float(x) == float(y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="Unknown categories"):
        panoptic_quality(T(g["pq0.preds"]).to(DEV), T(g["pq0.target"]).to(DEV), {1, 2}, {0, 3}, allow_unknown_preds_category=False, backend="device")
    host, dev = ConfusionMatrix(6, ignore_class=[0]), ConfusionMatrix(6, ignore_class=[0], backend="device")
    a = host.add_batch(g["cm_pred"], g["cm_gt"], return_miou=True)
    b = dev.add_batch(T(g["cm_pred"]).to(DEV), T(g["cm_gt"]).to(DEV), return_miou=True)
    assert a == b and bool((host.cm == dev.cm).all()) and host.get_miou() == dev.get_miou()


def test_device_backend_equals_host_on_random_maps():
    from contrastive_lift_amd.metrics import panoptic_quality_match, panoptic_quality_per_frame
    for seed in oc.SEEDS:
        p, t = oc.random_map(seed)
        _same_match(panoptic_quality_match(p, t, oc.THINGS, oc.STUFF, True),
                    panoptic_quality_match(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), oc.THINGS, oc.STUFF, True, backend="device"))
    for seed in (0, 1, 2):
        frames = oc.special_frames(seed)
        d = [{n: f[side][:, col] for n, f in frames.items()} for side, col in ((0, 0), (0, 1), (1, 0), (1, 1))]
        dd = [{n: torch.from_numpy(v).to(DEV) for n, v in x.items()} for x in d]
        for faulty in ((), (0,)):
            assert panoptic_quality_per_frame(*d, oc.IS_THING, faulty) == panoptic_quality_per_frame(*dd, oc.IS_THING, faulty, backend="device")
