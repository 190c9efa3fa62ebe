"""Inputs shared by tests/test_label_overlap_host.py and tests/test_gpu_label_overlap.py: the random label maps of the PQ tests and the
shapes at which the label-overlap kernel's design can go wrong (csrc/overlap.hip).  Not a test module."""
import numpy as np

from contrastive_lift_amd import overlap

THINGS, STUFF = {1, 2}, {0, 3}
IS_THING = [False, True, True, False]
SEEDS = range(20)


def random_map(seed, n=4000):
    """The generator of test_pq_per_frame.py::test_match_compute_split_is_panoptic_quality, by seed: (preds, target) (n, 2) int64."""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.integers(0, 4, n), rng.integers(0, 5, n)], -1)
    p = t.copy()
    p[rng.uniform(0, 1, n) < 0.2] = [1, 7]
    return p, t


def special_frames(seed):
    """{name: (preds, target)}: a random frame, one where class 2 falls under the robust share (3 of 4000 pixels) on one side and one where it
    does on both, one with stuff only, one that is all void (classes outside things and stuff) and an empty one."""
    rng = np.random.default_rng(1000 + seed)
    frames = {"0": random_map(seed)}
    p, t = random_map(seed + 100)
    t[t[:, 0] == 2, 0] = 1
    t[:3, 0] = 2
    frames["1"] = (p, t)
    p, t = p.copy(), t.copy()
    p[p[:, 0] == 2, 0] = 3
    p[5:7, 0] = 2
    frames["2"] = (p, t)
    t = np.stack([rng.choice([0, 3], 1500), rng.integers(0, 3, 1500)], -1)
    p = t.copy()
    p[rng.uniform(0, 1, 1500) < 0.3, 0] = 0
    frames["3"] = (p, t)
    frames["4"] = (np.stack([rng.integers(4, 6, 700), rng.integers(0, 3, 700)], -1), np.stack([rng.integers(4, 7, 700), rng.integers(0, 3, 700)], -1))
    frames["5"] = (np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64))
    return frames


def _case(name, sizes, a_cls, a_inst, b_cls, b_inst, a_base, a_stride, b_base, b_stride, NA, NB):
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x), dtype=np.int32)
    F = len(sizes)
    tab = lambda t: np.array(np.broadcast_to(np.asarray(t, dtype=np.int32), (F, np.asarray(t).shape[-1])) if np.asarray(t).ndim == 1 else np.asarray(t, dtype=np.int32), order="C")
    return dict(name=name, frame_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), a_cls=i32(a_cls), a_inst=i32(a_inst), b_cls=i32(b_cls),
                b_inst=i32(b_inst), a_base=tab(a_base), a_stride=tab(a_stride), b_base=tab(b_base), b_stride=tab(b_stride), NA=int(NA), NB=int(NB))


def kernel_cases():
    """The smallest shapes at which the kernel can go wrong, as keyword dicts of ``overlap.label_overlap_numpy`` (plus ``name``)."""
    B, T = overlap.BLOCK_ROWS, overlap.LDS_TABLE_INTS
    rng = np.random.default_rng(77)
    out = []
    # five frames: empty, shorter than a wave, exactly a wave, across block pieces; piecewise-constant labels; classes 0 .. 3, class 1 and 2 with instances
    sizes = [0, 37, 64, 257, 4 * B + 1]
    P = sum(sizes)
    runs = lambda hi, n: np.repeat(rng.integers(0, hi, n // 16 + 1), 16)[:n]
    base, stride = [0, 1, 6, 11], [0, 1, 1, 0]
    out.append(_case("five_frames", sizes, runs(4, P), runs(5, P), runs(4, P), runs(5, P), base, stride, base, stride, 12, 12))
    # all rows of a frame one key (full aggregation); 64 consecutive rows with 64 distinct keys (none); half / half inside one wave
    n = 2 * B + 17
    out.append(_case("one_key", [n, 130], np.full(n + 130, 2), np.full(n + 130, 3), np.full(n + 130, 1), np.full(n + 130, 4), base, stride, base, stride, 12, 12))
    out.append(_case("distinct_keys", [64, 192], np.zeros(256), np.tile(np.arange(64), 4), np.zeros(256), np.tile(np.arange(64)[::-1], 4), [0], [1], [0], [1], 64, 64))
    out.append(_case("half_half", [64], np.zeros(64), np.repeat([3, 9], 32), np.zeros(64), np.repeat([1, 0], 32), [0], [1], [0], [1], 10, 2))
    # NA * NB at the LDS threshold (the table path) and just above and below it (3 * 2731 = T + 1: the global path; T - 1 = 8191 is prime)
    n = B + 300
    for name, NA, NB in (("lds_at_threshold", 64, T // 64), ("lds_one_below", 1, T - 1), ("global_one_above", 3, (T + 1) // 3)):
        assert (NA * NB <= T) == name.startswith("lds") and abs(NA * NB - T) <= 1
        out.append(_case(name, [n, 77], np.zeros(n + 77), runs(NA, n + 77), np.zeros(n + 77), runs(NB, n + 77), [0], [1], [0], [1], NA, NB))
    out.append(_case("one_slot", [300, 0, 5], rng.integers(0, 3, 305), None, rng.integers(0, 2, 305), None, [0, 0, 0], [0, 0, 0], [0, 0], [0, 0], 1, 1))
    # dropped rows (a negative base on either side, also where the other side would be rejected) and rows that must be rejected: a class outside
    # the table, a slot outside [0, N), a negative instance under a non-zero stride
    n = 1000
    a_cls, b_cls = rng.integers(0, 4, n), rng.integers(0, 3, n)
    a_inst, b_inst = rng.integers(0, 4, n), rng.integers(0, 4, n)
    a_cls[10], b_cls[20], a_cls[30] = 4, -1, -5                        # classes outside the tables
    a_inst[rng.integers(0, n, 25)] = 7                                 # slot 1 + 7 outside NA = 6 where the class is 1
    b_inst[rng.integers(0, n, 25)] = -2                                # negative instance where the class is 2 (stride 1)
    out.append(_case("drop_and_reject", [400, 600], a_cls, a_inst, b_cls, b_inst, [0, 1, -1, 5], [0, 1, 1, 0], [-1, 0, 1], [0, 0, 1], 6, 5))
    # per-frame tables that differ between frames
    sizes = [500, 3, 900]
    P = sum(sizes)
    out.append(_case("tables_per_frame", sizes, runs(3, P), runs(4, P), runs(3, P), runs(2, P), [[0, 1, 5], [5, -1, 0], [2, 2, 2]], [[0, 1, 0], [0, 0, 1], [1, 1, 0]],
                     [[0, 1, 2], [2, 1, 0], [-1, 0, 0]], [[0, 0, 1], [1, 0, 0], [0, 0, 2]], 6, 4))
    # no instance array with all strides 0; and one with a non-zero stride, which rejects those rows
    n = 700
    out.append(_case("null_inst", [n], runs(3, n), None, runs(3, n), None, [2, 0, 1], [0, 0, 0], [0, 1, 1], [0, 0, 0], 3, 2))
    out.append(_case("null_inst_with_stride", [n], runs(3, n), None, runs(3, n), runs(2, n), [2, 0, 1], [0, 1, 0], [0, 1, 1], [0, 0, 1], 3, 3))
    return out
