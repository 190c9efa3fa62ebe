"""Label-overlap counting: the joint histogram of two label maps, per frame, after a per-frame class remapping -- the one table under
panoptic quality, the confusion matrix and the robust-class shares (metrics.py, inference.ConfusionMatrix).

Two counters with one contract (include/clift.h, ``clift_label_overlap``):

* ``label_overlap``        -- the kernel (csrc/overlap.hip) on CUDA int32 tensors;
* ``label_overlap_numpy``  -- its numpy restatement (``np.bincount`` per frame, the same drop and reject rules), for machines without a GPU
  and as the reference of the kernel's tests.

``Counter("device")`` / ``Counter("counts")`` wrap the two behind the few operations the scoring code needs (flatten to int32, maxima in one
reduction, count, non-zero triplets), so that everything above the counting is one code path.
"""
import numpy as np
import torch

from . import _lib

LDS_TABLE_INTS = 8192        # csrc/overlap.hip OV_LDS_INTS: NA * NB up to this many ints is counted in a block-private LDS table
BLOCK_ROWS = 4096            # csrc/overlap.hip OV_BLOCK_ROWS: the row axis is cut into pieces of this many rows
TABLE_CAP_BYTES = 1 << 30    # the wrappers refuse count tables above 1 GiB (F * NA * NB * 4 bytes)
BACKENDS = ("host", "device", "counts")


def check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    return backend


def check_table(F, NA, NB):
    """The 1 GiB cap on a (F, NA, NB) int32 table; callers that hit it score with backend="host"."""
    need = int(F) * int(NA) * int(NB) * 4
    if need > TABLE_CAP_BYTES:
        raise _lib.CliftError(f"label overlap: a count table of {F} x {NA} x {NB} int32 = {need} bytes is above the cap of {TABLE_CAP_BYTES} "
                              f"bytes (1 GiB); score this input with backend=\"host\"")


def check_frame_off(frame_off):
    """Host-side list of F + 1 row offsets: starts at 0, non-decreasing.  Returns it as an int64 numpy array."""
    off = np.asarray(frame_off, dtype=np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise _lib.CliftError("label overlap: frame_off must hold F + 1 non-decreasing row offsets starting at 0")
    return off


def _tables_numpy(t, F, what):
    t = np.asarray(t)
    if t.ndim != 2 or t.shape[0] != F or t.shape[1] < 1:
        raise _lib.CliftError(f"label overlap: {what} must be (F, C) with C >= 1, got {t.shape}")
    return t.astype(np.int64)


def label_overlap_numpy(a_cls, a_inst, b_cls, b_inst, frame_off, a_base, a_stride, b_base, b_stride, NA, NB):
    """The contract of ``clift_label_overlap`` in numpy: (counts (F, NA, NB) int32, rejected (F,) int32).  In this order, per row: a class
    outside its table on either side -> rejected; a negative base on either side -> dropped; a non-zero stride with no instance array or a
    negative instance id, or a slot outside [0, N), on either side -> rejected; every other row adds 1 to counts[f][sa][sb]."""
    off = check_frame_off(frame_off)
    F = off.size - 1
    if NA < 1 or NB < 1:
        raise _lib.CliftError(f"label overlap: need NA >= 1 and NB >= 1 (got {NA}, {NB})")
    check_table(F, NA, NB)
    a_base, a_stride = _tables_numpy(a_base, F, "a_base"), _tables_numpy(a_stride, F, "a_stride")
    b_base, b_stride = _tables_numpy(b_base, F, "b_base"), _tables_numpy(b_stride, F, "b_stride")
    counts, rejected = np.zeros((F, NA, NB), np.int32), np.zeros(F, np.int32)

    def side(cls, inst, base, stride, N, lo, hi):
        """(ok-so-far, dropped, rejected-late, slot) of rows lo .. hi whose class is inside the table."""
        b, st = base[cls], stride[cls]
        dropped = b < 0
        if inst is None:
            bad = st != 0
            slot = b.copy()
        else:
            v = np.asarray(inst[lo:hi]).astype(np.int64)
            bad = (st != 0) & (v < 0)
            slot = b + st * np.where(st != 0, v, 0)
        bad = bad | (slot < 0) | (slot >= N)
        return dropped, bad, slot

    for f in range(F):
        lo, hi = int(off[f]), int(off[f + 1])
        ca, cb = np.asarray(a_cls[lo:hi]).astype(np.int64), np.asarray(b_cls[lo:hi]).astype(np.int64)
        inside = (ca >= 0) & (ca < a_base.shape[1]) & (cb >= 0) & (cb < b_base.shape[1])
        rej = int((~inside).sum())
        ca_c, cb_c = np.where(inside, ca, 0), np.where(inside, cb, 0)
        da, ba, sa = side(ca_c, a_inst, a_base[f], a_stride[f], NA, lo, hi)
        db, bb, sb = side(cb_c, b_inst, b_base[f], b_stride[f], NB, lo, hi)
        kept = inside & ~(da | db)
        late = kept & (ba | bb)
        rej += int(late.sum())
        ok = kept & ~late
        counts[f] = np.bincount(sa[ok] * NB + sb[ok], minlength=NA * NB).reshape(NA, NB).astype(np.int32)
        rejected[f] = rej
    return counts, rejected


def _dev_i32(t, dev, what, shape=None):
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
        raise _lib.CliftError(f"label overlap: {what} must be a contiguous CUDA int32 tensor on {dev}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.CliftError(f"label overlap: {what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def label_overlap(a_cls, a_inst, b_cls, b_inst, frame_off, a_base, a_stride, b_base, b_stride, NA, NB):
    """``clift_label_overlap`` on CUDA tensors: a_cls, b_cls (P,) int32, a_inst, b_inst (P,) int32 or None, frame_off a HOST sequence of F + 1
    offsets (checked here, uploaded as int64), the tables (F, Ca) / (F, Cb) int32.  Returns (counts (F, NA, NB), rejected (F,)) int32 on the
    device, not read back: the caller checks ``rejected``.  No host fallback: without the library or a GPU this raises."""
    off = check_frame_off(frame_off)
    F, P = off.size - 1, int(off[-1])
    if NA < 1 or NB < 1:
        raise _lib.CliftError(f"label overlap: need NA >= 1 and NB >= 1 (got {NA}, {NB})")
    check_table(F, NA, NB)
    dev = a_cls.device if torch.is_tensor(a_cls) else None
    if dev is None or dev.type != "cuda":
        raise _lib.CliftError('label overlap: backend="device" counts CUDA tensors (there is no host fallback; backend="counts" is the host function)')
    for t, what in ((a_cls, "a_cls"), (b_cls, "b_cls"), (a_inst, "a_inst"), (b_inst, "b_inst")):
        _dev_i32(t, dev, what, (P,))
    if a_base.dim() != 2 or b_base.dim() != 2 or a_base.shape[0] != F or b_base.shape[0] != F or a_base.shape[1] < 1 or b_base.shape[1] < 1:
        raise _lib.CliftError("label overlap: a_base / b_base must be (F, C) with C >= 1")
    Ca, Cb = int(a_base.shape[1]), int(b_base.shape[1])
    for t, what, C_ in ((a_base, "a_base", Ca), (a_stride, "a_stride", Ca), (b_base, "b_base", Cb), (b_stride, "b_stride", Cb)):
        _dev_i32(t, dev, what, (F, C_))
    counts = torch.empty((F, NA, NB), dtype=torch.int32, device=dev)
    rejected = torch.empty((F,), dtype=torch.int32, device=dev)
    if F == 0:
        return counts, rejected
    if P == 0:                                       # (an empty tensor has no address to hand over; the tables are the cleared ones)
        return counts.zero_(), rejected.zero_()
    with torch.cuda.device(dev):
        off_dev = torch.from_numpy(off).to(dev)
        _lib.call("clift_label_overlap", _lib.ptr(a_cls), _lib.ptr(a_inst), _lib.ptr(b_cls), _lib.ptr(b_inst), _lib.ptr(off_dev), F,
                  _lib.ptr(a_base), _lib.ptr(a_stride), Ca, _lib.ptr(b_base), _lib.ptr(b_stride), Cb, int(NA), int(NB),
                  _lib.ptr(counts), _lib.ptr(rejected), _lib.stream())
    return counts, rejected


class Counter:
    """What the scoring code needs from a count backend.  Label arrays live where the counting runs (numpy arrays for "counts", CUDA tensors
    for "device"); tables are built on the host as numpy arrays and uploaded by ``count``."""

    def __init__(self, backend, device=None):
        if backend not in ("device", "counts"):
            raise ValueError(f'a count backend is "device" or "counts", got {backend!r}')
        self.device_side = backend == "device"
        if self.device_side:
            if not torch.cuda.is_available():
                raise _lib.CliftError('label overlap: backend="device" runs on a GPU (there is no host fallback; backend="counts" is the host function)')
            self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def labels(self, x):
        """Flat label array where the counting runs, in its own integer type (``int32`` narrows it after the range check)."""
        if self.device_side:
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)).astype(np.int64))
            return t.to(self.dev).reshape(-1)
        return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(-1)

    def cat(self, parts):
        return torch.cat(parts) if self.device_side else np.concatenate(parts)

    def extremes(self, arrays):
        """[(min, max) of every array, (0, -1) for an empty one] as Python ints: one reduction pass and ONE read-back on the device."""
        if self.device_side:
            vals = []
            for x in arrays:
                if x.numel():
                    lo, hi = torch.aminmax(x)
                    vals += [lo.to(torch.int64), hi.to(torch.int64)]
                else:
                    vals += [torch.tensor(0, dtype=torch.int64, device=self.dev), torch.tensor(-1, dtype=torch.int64, device=self.dev)]
            v = torch.stack(vals).cpu().tolist()
            return [(int(v[2 * i]), int(v[2 * i + 1])) for i in range(len(arrays))]
        return [(int(x.min()), int(x.max())) if x.size else (0, -1) for x in arrays]

    def where_class_in(self, cls, classes, x):
        """x where cls is one of ``classes``, 0 elsewhere (instance ids count for thing classes only)."""
        if self.device_side:
            return torch.where(torch.isin(cls, torch.tensor(sorted(classes), dtype=cls.dtype, device=cls.device)), x, torch.zeros_like(x))
        return np.where(np.isin(cls, sorted(classes)), x, 0)

    def int32(self, x, lo, hi):
        """Narrow to contiguous int32; (lo, hi) are the array's extremes -- a value that would wrap in the cast is refused here, a negative
        one that fits is left to the counting, which rejects it."""
        if hi >= 2 ** 31 or lo < -2 ** 31:
            raise _lib.CliftError(f"label overlap: labels {lo} .. {hi} do not fit int32; score this input with backend=\"host\"")
        return x.to(torch.int32).contiguous() if self.device_side else x.astype(np.int32)

    def remap_outside(self, x, n):
        """x with every value outside [0, n) replaced by n (the confusion matrix's ignored ground truth), int32."""
        if self.device_side:
            return torch.where((x < 0) | (x >= n), torch.full_like(x, n), x).to(torch.int32).contiguous()
        return np.where((x < 0) | (x >= n), n, x).astype(np.int32)

    def count(self, a_cls, a_inst, b_cls, b_inst, frame_off, a_base, a_stride, b_base, b_stride, NA, NB):
        """Counts (F, NA, NB) where the counting runs; raises CliftError when a row was rejected."""
        if self.device_side:
            up = lambda t: torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.int32))).to(self.dev)
            counts, rejected = label_overlap(a_cls, a_inst, b_cls, b_inst, frame_off, up(a_base), up(a_stride), up(b_base), up(b_stride), NA, NB)
            rej = rejected.cpu().numpy()
        else:
            counts, rej = label_overlap_numpy(a_cls, a_inst, b_cls, b_inst, frame_off, a_base, a_stride, b_base, b_stride, NA, NB)
        if rej.any():
            f = int(np.nonzero(rej)[0][0])
            raise _lib.CliftError(f"label overlap: {int(rej.sum())} rows rejected (first in frame {f}: {int(rej[f])}): a negative class or instance "
                                  f"id, or a label outside the tables; score this input with backend=\"host\"")
        return counts

    def host(self, counts):
        """The whole table as an int64 numpy array (small tables only: the class-against-class launch)."""
        return (counts.cpu().numpy() if self.device_side else counts).astype(np.int64)

    def nonzero(self, counts):
        """The non-zero entries of a (F, NA, NB) table as host arrays (f, sa, sb, n), row-major order; only these cross to the host."""
        if self.device_side:
            idx = torch.nonzero(counts)
            vals = counts[idx[:, 0], idx[:, 1], idx[:, 2]]
            idx, vals = idx.cpu().numpy(), vals.cpu().numpy().astype(np.int64)
            return idx[:, 0], idx[:, 1], idx[:, 2], vals
        f, sa, sb = np.nonzero(counts)
        return f, sa, sb, counts[f, sa, sb].astype(np.int64)
