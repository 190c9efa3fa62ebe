"""Scene edits: oriented boxes and the host-side resolution of one edit to the plain record the edit kernels read (``clift_edit_t`` in
include/clift.h; csrc/edit.hip; ``engine.edit_forward``).

A box has axes ``A`` (3x3, ROWS are the axes), a centre ``c`` and bounds ``lo``, ``hi``: a world point p is inside iff
``lo <= A (p - c) <= hi`` component-wise, faces inclusive.  That one form covers the boxes ``points3d.fit_instance_boxes`` writes
(``EditBox.from_fitted``) and the reference's ``{"extent", "position", "orientation"}`` dictionaries (``EditBox.from_reference``).

Two families of edits:

* reference-faithful -- ``reference_delete`` / ``reference_extract`` / ``reference_duplicate`` / ``reference_manipulate`` restate the
  arithmetic of the reference's ``forward_delete`` / ``forward_extract`` / ``forward_duplicate`` / ``forward_manipulate``
  (model/renderer/panopli_tensoRF_renderer.py:303-623) exactly as it is written there, including its quirk: once the rotation is not the
  identity its maps are no rigid motion (the content is turned one way and the box the other, and the translation is subtracted after the
  rotation).  ``TensoRFRenderer.forward_*`` use these.
* rigid -- ``copy`` / ``move``: the object undergoes x -> R (x - pos) + pos + t.  The command-line tool uses these.  For R = I, ``move``
  resolves to the same record as ``reference_manipulate``.

``EditProgram`` is an ordered list of up to ``MAX_EDITS`` such edits applied in one render (``clift_edit_list_*``).

An edit may follow a SHAPE instead of its whole box (``EditShape``): a bit lattice over the source box, read from the trained
field (``EditShape.from_field``) or packed from flags; every constructor takes ``shape=``, and a program with a shaped edit runs through
the ``clift_edit_shaped_*`` entry points.
"""
import ctypes as C

import numpy as np

from . import _lib

DELETE, EXTRACT, DUPLICATE, MANIPULATE = 0, 1, 2, 3          # CLIFT_EDIT_* of include/clift.h
_MODE_NAMES = {DELETE: "delete", EXTRACT: "extract", DUPLICATE: "duplicate", MANIPULATE: "manipulate"}
MAX_EDITS = 8                                                # CLIFT_EDIT_MAX: edits in one program (EditProgram)
STATE_KILLED = 0x80                                          # CLIFT_EDIT_STATE_KILLED: the kill bit of a walk's state byte (apply_to_points)
STATE_REMAPS = 0x0f                                          # CLIFT_EDIT_STATE_REMAPS: its remap count


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def _np(x, shape):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("edit: values must be finite")
    return a


def _f32(a):
    """fp32 values of an fp64 array as a flat list (-0.0 stored as 0.0, so that equal edits pack to equal bytes)."""
    return (np.asarray(a, dtype=np.float64).astype(np.float32).reshape(-1) + np.float32(0.0)).tolist()


class EditBox:
    """Oriented box: inside iff ``lo <= axes @ (p - centre) <= hi`` (rows of ``axes`` are the box axes; faces inclusive).  fp64 on the host."""

    def __init__(self, axes, centre, lo, hi):
        self.axes, self.centre, self.lo, self.hi = _np(axes, (3, 3)), _np(centre, (3,)), _np(lo, (3,)), _np(hi, (3,))

    @classmethod
    def from_fitted(cls, entry, pad=0.0):
        """A ``bboxes.pkl`` entry of inference/fit_bboxes.py (``points3d.fit_instance_boxes``): axes = ``orientation`` (rows), centre =
        ``position``, (lo, hi) = ``bbox``.  Fitted boxes hug the filtered points: ``pad`` grows them on every side."""
        lo, hi = entry["bbox"]
        return cls(entry["orientation"], entry["position"], lo, hi).padded(pad)

    @classmethod
    def from_reference(cls, d, pad=0.0):
        """The reference's ``{"extent", "position", "orientation"}``: axes are the COLUMNS of ``orientation`` (split_points_minimal,
        renderer.py:785-797), so A = orientation^T, lo = -extent / 2, hi = +extent / 2."""
        ext = _np(d["extent"], (3,))
        return cls(_np(d["orientation"], (3, 3)).T, d["position"], -ext / 2, ext / 2).padded(pad)

    def padded(self, pad):
        pad = float(pad)
        return self if pad == 0.0 else EditBox(self.axes, self.centre, self.lo - pad, self.hi + pad)

    def local(self, points):
        """Box-frame coordinates A (p - c) of (n, 3) world points, fp64."""
        return (np.asarray(points, dtype=np.float64) - self.centre) @ self.axes.T

    def contains(self, points):
        q = self.local(points)
        return np.all((self.lo <= q) & (q <= self.hi), axis=-1)

    def _fill(self, rec):
        rec.axes[:] = _f32(self.axes)
        rec.centre[:] = _f32(self.centre)
        rec.lo[:] = _f32(self.lo)
        rec.hi[:] = _f32(self.hi)


MAX_SHAPE_DIM = 1024                                         # CLIFT_SHAPE_DIM_MAX
MAX_SHAPE_GROW = 4                                           # CLIFT_SHAPE_GROW_MAX


def _shape_dims(dims):
    d = tuple(int(g) for g in dims)
    if len(d) != 3 or not all(1 <= g <= MAX_SHAPE_DIM for g in d):
        raise ValueError(f"shape dims are three numbers in 1 .. {MAX_SHAPE_DIM}, got {dims!r}")
    return d


def _grown(f, grow):
    """f (G0, G1, G2) bool -> True where some flag within Chebyshev distance ``grow`` is set, clipped at the border (a separable maximum)."""
    for ax in range(3):
        n, out = f.shape[ax], f.copy()
        for k in range(1, min(grow, n - 1) + 1):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[ax], b[ax] = slice(k, None), slice(None, n - k)
            out[tuple(b)] |= f[tuple(a)]
            out[tuple(a)] |= f[tuple(b)]
        f = out
    return f


class EditShape:
    """The shape of an edit: a bit lattice over the edit's SOURCE box, in the box's local frame.  ``dims`` = (G0, G1, G2); cell
    i_a of axis a covers lo_a + i_a h_a .. lo_a + (i_a + 1) h_a with h_a = (hi_a - lo_a) / G_a; bits are x-major, lin = (i0 G1 + i1) G2 + i2,
    bit lin & 31 of word lin >> 5; ``words`` is a host uint32 array of ceil(G0 G1 G2 / 32) words whose unused high bits are 0 (``on`` gives
    the device copy the kernels read).  A point is part of the edit only where its cell's bit is set (``Edit``, ``EditProgram``)."""

    def __init__(self, words, dims):
        self.dims = _shape_dims(dims)
        total = self.dims[0] * self.dims[1] * self.dims[2]
        w = np.ascontiguousarray(np.asarray(_host(words)).reshape(-1))
        w = w.view(np.uint32) if w.dtype in (np.uint32, np.int32) else w.astype(np.uint32)      # (an int32 tensor holds the same bits)
        if w.shape[0] != (total + 31) // 32:
            raise ValueError(f"a shape of dims {self.dims} has {(total + 31) // 32} words, got {w.shape[0]}")
        if total % 32 and int(w[-1]) >> (total % 32):
            raise ValueError("the unused high bits of a shape's last word must be 0")
        self.words = w.copy()
        self.slot = self.n_occupied = None          # from_field: the slot the shape follows, and how many cells held density at all
        self._dev = {}

    @property
    def n_cells(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def n_set(self):
        return int(np.unpackbits(self.words.view(np.uint8)).sum())

    @classmethod
    def from_flags(cls, flags, grow=0, backend="device", device=None):
        """Pack (G0, G1, G2) flags (non-zero = set): bit = 1 iff some flag within Chebyshev distance ``grow`` (0 .. 4) of the cell is set, the
        neighbourhood clipped at the lattice border.  ``backend="device"``: clift_shape_pack (flags may be a device tensor; a host array
        goes to ``device``, default the current one); ``backend="host"``: numpy, the same words."""
        grow = int(grow)
        if not 0 <= grow <= MAX_SHAPE_GROW:
            raise ValueError(f"grow must be in 0 .. {MAX_SHAPE_GROW} (got {grow})")
        if backend == "host":
            f = np.asarray(_host(flags)) != 0
            dims = _shape_dims(f.shape)
            bits = _grown(f, grow).reshape(-1)
            padded = np.zeros((bits.shape[0] + 31) // 32 * 32, dtype=np.uint8)
            padded[:bits.shape[0]] = bits
            return cls(np.packbits(padded, bitorder="little").view(np.uint32), dims)
        if backend != "device":
            raise ValueError(f"backend is 'device' or 'host' (got {backend!r})")
        import torch
        f = flags if hasattr(flags, "detach") else torch.from_numpy(np.ascontiguousarray(np.asarray(flags) != 0))
        if not f.is_cuda:
            f = f.to(device if device is not None else "cuda")
        dims = _shape_dims(f.shape)
        f = (f != 0).to(torch.uint8).contiguous()
        words = torch.empty(((dims[0] * dims[1] * dims[2] + 31) // 32,), dtype=torch.int32, device=f.device)
        _lib.call("clift_shape_pack", _lib.ptr(f), dims[0], dims[1], dims[2], grow, _lib.ptr(words), _lib.stream())
        out = cls(words.cpu().numpy().view(np.uint32), dims)
        out._dev[str(f.device)] = words
        return out

    @classmethod
    def full(cls, dims, value=True):
        """All cells set (the plain box edit) or none."""
        dims = _shape_dims(dims)
        return cls.from_flags(np.full(dims, bool(value)), backend="host")

    def flags(self):
        """The (G0, G1, G2) bool array of the bits."""
        return np.unpackbits(self.words.view(np.uint8), bitorder="little")[:self.n_cells].astype(bool).reshape(self.dims)

    def on(self, device):
        """The words as an int32 tensor on ``device`` (the same bits), made once per device."""
        key = str(device)
        if key not in self._dev:
            import torch
            self._dev[key] = torch.from_numpy(self.words.view(np.int32).copy()).to(device)
        return self._dev[key]

    def cells(self, box, points):
        """Linear cell index of (n, 3) world points in the lattice over ``box``, fp64: per axis floor((A (x - c) - lo) G / (hi - lo)) clamped
        to 0 .. G - 1."""
        G = np.asarray(self.dims, dtype=np.float64)
        u = (box.local(points) - box.lo) * (G / (box.hi - box.lo))
        i = np.clip(np.floor(u), 0, G - 1).astype(np.int64)
        return (i[:, 0] * self.dims[1] + i[:, 1]) * self.dims[2] + i[:, 2]

    def bit(self, box, points):
        """Whether (n, 3) world points sit in a set cell of the lattice over ``box`` (fp64 on the host; no box test: the index is clamped)."""
        lin = self.cells(box, np.asarray(points, dtype=np.float64).reshape(-1, 3))
        return ((self.words[lin >> 5] >> (lin & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)

    def record(self, box, device):
        """``clift_edit_shape_t`` for an edit whose source box is ``box``: inv_cell = fp32(G / (hi - lo)), formed in fp64 from the fp32 lo and
        hi that ``Edit.record`` packs."""
        rec = _lib.EditShapeRec()
        rec.words = self.on(device).data_ptr()
        rec.dims[:] = self.dims
        rec.inv_cell[:] = self.inv_cell(box).tolist()
        return rec

    def inv_cell(self, box):
        """(3,) fp32: G_a / (hi_a - lo_a), formed in fp64 from the fp32 values of the box's bounds (a box without extent gives inf, which the
        shaped entry points refuse)."""
        lo, hi = np.asarray(_f32(box.lo), dtype=np.float64), np.asarray(_f32(box.hi), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return (np.asarray(self.dims, dtype=np.float64) / (hi - lo)).astype(np.float32)

    @classmethod
    def from_field(cls, model, renderer, box, table, slot=None, dims=(32, 32, 32), grow=1, sigma_min=10.0, use_delta=False):
        """The shape of the instance in ``box`` (an ``EditBox`` or a reference dictionary), read from the trained field: the cell centres of
        the box (fp64 on the host, fp32 world points on the device) are occupied where they are inside the aabb and the density is at least
        ``sigma_min`` (``model.compute_density``), each gets its slot under ``table`` (``engine.point_slots``), and
        flags = occupied & (slot == ``slot``), packed with ``grow``.  ``slot=None`` takes the most frequent slot >= 0 among the occupied
        cells, a tie going to the lower slot; no such cell is a ``ValueError``.  The result carries ``slot``, ``n_occupied`` and ``n_set``."""
        import torch
        from . import engine
        box, dims = _box(box), _shape_dims(dims)
        ax = [box.lo[a] + (np.arange(dims[a], dtype=np.float64) + 0.5) * ((box.hi[a] - box.lo[a]) / dims[a]) for a in range(3)]
        q = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
        dev = renderer.bbox_aabb.device
        pts = torch.from_numpy((q @ box.axes + box.centre).astype(np.float32)).to(dev)
        with torch.no_grad():
            xn = renderer.normalize_coordinates(pts)
            inside = ((pts >= renderer.bbox_aabb[0]) & (pts <= renderer.bbox_aabb[1])).all(dim=-1)
            occupied = inside & (model.compute_density(xn) >= float(sigma_min))
            slots = engine.point_slots(model, renderer, pts, table, use_delta=use_delta)
        if slot is None:
            slot = majority_slot(slots[occupied].cpu().numpy())
        flags = (occupied & (slots == int(slot))).reshape(dims)
        out = cls.from_flags(flags, grow=grow, backend="device")
        out.slot, out.n_occupied = int(slot), int(occupied.sum().item())
        return out


def majority_slot(slots):
    """The most frequent slot >= 0 of an int array, a tie going to the lower slot; none is a ``ValueError``."""
    s = np.asarray(slots).reshape(-1)
    s = s[s >= 0]
    if s.size == 0:
        raise ValueError("EditShape.from_field: no occupied cell of the box belongs to an instance slot (is the box empty, or sigma_min too high?)")
    return int(np.argmax(np.bincount(s.astype(np.int64))))


class Edit:
    """One resolved edit: kill rule (``mode``), source and destination box, the affine map p' = M p + t of samples inside the destination
    box and the matrix ``dir_inv`` applied to their view directions.  ``record()`` packs it as ``clift_edit_t``.  ``shape`` (an
    ``EditShape`` over the source box, or None) narrows the edit to the cells whose bit is set: a point is in the source only if its cell is
    set, and in the destination only if the cell of its REMAPPED point M p + t is (both read in the source frame); the record does not
    change, the shape travels beside it (``EditProgram.shapes``)."""

    def __init__(self, mode, src, dst=None, M=None, t=None, dir_inv=None, shape=None):
        if mode not in _MODE_NAMES:
            raise ValueError(f"unknown edit mode {mode!r}")
        if shape is not None and not isinstance(shape, EditShape):
            raise TypeError(f"shape is an edit.EditShape or None, got {type(shape).__name__}")
        self.shape = shape
        self.mode, self.src = mode, src
        self.dst = dst if dst is not None else src
        self.M = _np(M if M is not None else np.eye(3), (3, 3))
        self.t = _np(t if t is not None else np.zeros(3), (3,))
        self.dir_inv = _np(dir_inv if dir_inv is not None else np.eye(3), (3, 3))

    @property
    def name(self):
        return _MODE_NAMES[self.mode]

    def record(self):
        rec = _lib.EditRec()
        rec.mode = int(self.mode)
        self.src._fill(rec.src)
        self.dst._fill(rec.dst)
        rec.map_m[:] = _f32(self.M)
        rec.map_t[:] = _f32(self.t)
        rec.dir_inv[:] = _f32(self.dir_inv)
        return rec

    def record_bytes(self):
        return C.string_at(C.byref(self.record()), C.sizeof(_lib.EditRec))

    def with_shape(self, shape):
        """The same edit following ``shape`` (None: the plain box edit again)."""
        return Edit(self.mode, self.src, self.dst, self.M, self.t, self.dir_inv, shape=shape)

    def in_src(self, points):
        """Inside the source box and, with a shape, in a set cell (fp64)."""
        p = np.asarray(points, dtype=np.float64)
        src = self.src.contains(p)
        return src if self.shape is None else src & self.shape.bit(self.src, p)

    def in_dst(self, points):
        """Inside the destination box and, with a shape, the remapped point M p + t in a set cell of the SOURCE lattice (fp64)."""
        p = np.asarray(points, dtype=np.float64)
        mov = self.dst.contains(p)
        return mov if self.shape is None else mov & self.shape.bit(self.src, p @ self.M.T + self.t)

    def source_points(self, points):
        """Where (n, 3) world points are looked up: M p + t inside the destination box of a remapping edit, p elsewhere (fp64)."""
        p = np.asarray(points, dtype=np.float64)
        if self.mode < DUPLICATE:
            return p
        return np.where(self.in_dst(p)[:, None], p @ self.M.T + self.t, p)

    def killed(self, points):
        if self.mode == DUPLICATE:
            return np.zeros(np.asarray(points).shape[0], dtype=bool)
        src = self.in_src(points)
        if self.mode == DELETE:
            return src
        if self.mode == EXTRACT:
            return ~src
        return src & ~self.in_dst(points)


class EditProgram:
    """An ordered list e_1 ... e_n of resolved edits (1 <= n <= ``MAX_EDITS``) for one render: scene_i is e_i applied to scene_{i-1}, scene_0
    the trained field.  A point of scene_n is evaluated by walking the list BACKWARDS: edit i tests the current point against its boxes; a
    point its kill rule names is empty (the walk stops); a point inside its destination box continues at M_i p + t_i with the view direction
    Dinv_i d; what is left after e_1 is looked up in the field.  A program of one edit is that edit."""

    def __init__(self, edits):
        edits = tuple(edits)
        if not 1 <= len(edits) <= MAX_EDITS:
            raise ValueError(f"an edit program holds 1 to {MAX_EDITS} edits (MAX_EDITS), got {len(edits)}")
        for e in edits:
            if not isinstance(e, Edit):
                raise TypeError(f"an edit program holds edit.Edit objects, got {type(e).__name__}")
        self.edits = edits

    def __len__(self):
        return len(self.edits)

    def __iter__(self):
        return iter(self.edits)

    def __getitem__(self, i):
        return self.edits[i]

    def records(self):
        """Contiguous ctypes array of the n ``clift_edit_t`` records, in program order (the ``edits`` argument of the list entry points)."""
        return (_lib.EditRec * len(self.edits))(*(e.record() for e in self.edits))

    def record_bytes(self):
        return b"".join(e.record_bytes() for e in self.edits)

    @property
    def is_shaped(self):
        """Whether any edit follows a shape (``launch_family`` hands the program to the ``clift_edit_shaped_*`` entry points then)."""
        return any(e.shape is not None for e in self.edits)

    def launch_family(self, device):
        """How the program is passed to the four walk entry points (density_fwd, active, points, dense_sigma): -> (name pattern, leading
        arguments).  ``pattern % "points"`` is the entry point; the arguments -- the records, for a shaped program the shape records with
        their words on ``device`` right behind them, then the count -- are adjacent in every one of the four argument lists and splice in
        with ``*``.  The one place that picks between the list and the shaped family."""
        if self.is_shaped:
            return "clift_edit_shaped_%s", (self.records(), self.shapes(device), len(self.edits))
        return "clift_edit_list_%s", (self.records(), len(self.edits))

    def shapes(self, device):
        """Contiguous ctypes array of the n ``clift_edit_shape_t`` records, in program order, their words on ``device`` (the ``h_shapes``
        argument of the shaped entry points); an edit without a shape has NULL words.  None when no edit has a shape."""
        if not self.is_shaped:
            return None
        return (_lib.EditShapeRec * len(self.edits))(*(e.shape.record(e.src, device) if e.shape is not None else _lib.EditShapeRec()
                                                       for e in self.edits))

    def _walk(self, points, dirs, jac=False, origin=None):
        p = np.array(points, dtype=np.float64)
        d = None if dirs is None else np.array(dirs, dtype=np.float64)
        dead = np.zeros(p.shape[0], dtype=bool)
        hops = np.zeros(p.shape[0], dtype=np.uint8)
        J = np.tile(np.eye(3), (p.shape[0], 1, 1)) if jac else None
        for i in range(len(self.edits), 0, -1):
            e = self.edits[i - 1]
            dead |= e.killed(p)                           # (a killed point is not walked further: its p stays where the walk stopped)
            if e.mode >= DUPLICATE:
                mov = ~dead & e.in_dst(p)
                p[mov] = p[mov] @ e.M.T + e.t
                if d is not None:
                    d[mov] = d[mov] @ e.dir_inv.T
                if J is not None:
                    J[mov] = e.M @ J[mov]
                if origin is not None and e.mode == DUPLICATE:
                    origin[mov & (origin == 0)] = i
                hops[mov] += 1
        return (p, d, dead, hops, J) if jac else (p, d, dead, hops)

    def source_points(self, points, dirs=None):
        """Where (n, 3) fp64 world points are finally looked up -- and, with ``dirs``, (points, view directions).  Rows of killed points
        (``killed``) hold the position at which the walk stopped."""
        p, d = self._walk(points, dirs)[:2]
        return p if dirs is None else (p, d)

    def killed(self, points):
        return self._walk(points, None)[2]

    def jacobians(self, points):
        """The chain of the walk at (n, 3) world points, fp64 on the host: -> (source points (n, 3), J (n, 3, 3), state (n,) uint8 as
        ``apply_to_points`` gives it).  A point that the edits i_1 .. i_h remapped, in walk order, is looked up at p' = J p + b with
        J = M_{i_h} ... M_{i_1} (the identity for h = 0; for a killed point the product up to where its walk stopped).  J is piecewise
        constant in p, so the world gradient of the edited density is J^T times the field's world gradient at p' -- J^T, not an inverse:
        the maps need not be rotations."""
        p, _, dead, hops, J = self._walk(np.asarray(_host(points), dtype=np.float64).reshape(-1, 3), None, jac=True)
        return p, J, hops | np.where(dead, np.uint8(STATE_KILLED), np.uint8(0))

    def origins(self, points):
        """Which copy the content at (n, 3) world points came through, fp64 on the host: -> (source points (n, 3), origin (n,) uint8, state
        (n,) uint8 as ``apply_to_points`` gives it).  origin is the 1-based position in the program of the FIRST edit the backward walk meets
        that remaps the point and is a DUPLICATE -- the last-applied copy in whose destination the point sits -- and 0 if it meets none.  A
        copy that a later edit moves keeps its origin, for a copy of a copy the outer one wins, a killed point keeps what it had when its
        walk stopped (clift_edit_list_active_origin)."""
        origin = np.zeros(np.asarray(_host(points)).reshape(-1, 3).shape[0], dtype=np.uint8)
        p, _, dead, hops = self._walk(np.asarray(_host(points), dtype=np.float64).reshape(-1, 3), None, origin=origin)
        return p, origin, hops | np.where(dead, np.uint8(STATE_KILLED), np.uint8(0))

    def copies(self):
        """The 0-based positions of the DUPLICATE edits, in program order."""
        return [i for i, e in enumerate(self.edits) if e.mode == DUPLICATE]

    def apply_to_points(self, points, dirs=None, backend="device"):
        """The walk over arbitrary world points (n, 3), with view directions (n, 3) or without: -> (source points, source directions or
        None, state).  state (n) uint8 = the number of remaps (0 .. ``MAX_EDITS``) in the low bits, ``STATE_KILLED`` set where some edit's
        kill rule named the point; a killed row holds the position at which its walk stopped, a row no edit remaps holds its input.  No
        aabb test: the caller decides what is inside the scene.  ``backend="device"``: device fp32 tensors through
        clift_edit_list_points (one launch; tensors in, tensors out; an untouched row gets its input bits back).  ``backend="host"``:
        the fp64 walk of ``source_points`` / ``killed``, numpy arrays out."""
        if backend == "host":
            p, d, dead, hops = self._walk(np.asarray(_host(points), dtype=np.float64).reshape(-1, 3),
                                          None if dirs is None else np.asarray(_host(dirs), dtype=np.float64).reshape(-1, 3))
            return p, d, hops | np.where(dead, np.uint8(STATE_KILLED), np.uint8(0))
        if backend != "device":
            raise ValueError(f"backend is 'device' or 'host' (got {backend!r})")
        import torch
        pts = _lib.f32(points, "points").reshape(-1, 3).contiguous()
        n = pts.shape[0]
        dr = None
        if dirs is not None:
            dr = _lib.f32(dirs, "dirs").reshape(-1, 3).contiguous()
            if dr.shape[0] != n or dr.device != pts.device:
                raise ValueError(f"apply_to_points: {dr.shape[0]} directions on {dr.device} for {n} points on {pts.device}")
        out_p = torch.empty_like(pts)
        out_d = None if dr is None else torch.empty_like(dr)
        state = torch.empty(n, dtype=torch.uint8, device=pts.device)
        kernel, program = self.launch_family(pts.device)
        _lib.call(kernel % "points", *program, _lib.ptr(pts), 3, _lib.ptr(dr), 3, n, _lib.ptr(out_p), _lib.ptr(out_d), _lib.ptr(state), _lib.stream())
        return out_p, out_d, state


def as_program(x):
    """An ``EditProgram`` from an ``Edit``, an ``EditProgram`` or a sequence of ``Edit``."""
    if isinstance(x, EditProgram):
        return x
    return EditProgram([x] if isinstance(x, Edit) else x)


def _box(b, pad=0.0):
    return b.padded(pad) if isinstance(b, EditBox) else EditBox.from_reference(b, pad)


# ----------------------------------------------------------------------------- reference-faithful
def reference_delete(bbox, shape=None):
    """forward_delete (renderer.py:303-376): kill the samples inside the box (with ``shape``: inside the box and part of the shape)."""
    return Edit(DELETE, _box(bbox), shape=shape)


def reference_extract(bbox, shape=None):
    """forward_extract (renderer.py:379-453): kill the samples outside the box (with ``shape``: and those inside that are no part of it)."""
    return Edit(EXTRACT, _box(bbox), shape=shape)


def reference_duplicate(bbox, translation, rotation, shape=None):
    """forward_duplicate (renderer.py:456-536), the reference's arithmetic as written (O = orientation, R = rotation, pos = position):
    the destination box has centre R pos + t, axes = columns of R O and the same extent; samples inside it are looked up at p - t with the
    view direction R^-1 d; nothing is killed.  For R != I this is no rigid copy (the content is not turned, the box is, and it is turned
    about the origin): the quirk is reproduced on purpose."""
    O, pos, ext = _np(bbox["orientation"], (3, 3)), _np(bbox["position"], (3,)), _np(bbox["extent"], (3,))
    R, t = _np(rotation, (3, 3)), _np(translation, (3,))
    dst = EditBox((R @ O).T, R @ pos + t, -ext / 2, ext / 2)
    return Edit(DUPLICATE, _box(bbox), dst, np.eye(3), -t, np.linalg.inv(R), shape=shape)


def reference_manipulate(bbox, translation, rotation, shape=None):
    """forward_manipulate (renderer.py:539-623), the reference's arithmetic as written: the destination box has centre pos + t and axes =
    columns of R O; samples inside it are looked up at R (p - pos) + pos - t with the view direction R^-1 d; samples inside the source box
    and outside the destination box are killed.  For R != I this is no rigid motion (a rigid one looks up R^-1 (p - pos - t) + pos): the
    quirk is reproduced on purpose -- ``move`` is the rigid form."""
    O, pos, ext = _np(bbox["orientation"], (3, 3)), _np(bbox["position"], (3,)), _np(bbox["extent"], (3,))
    R, t = _np(rotation, (3, 3)), _np(translation, (3,))
    dst = EditBox((R @ O).T, pos + t, -ext / 2, ext / 2)
    return Edit(MANIPULATE, _box(bbox), dst, R, (pos - R @ pos) - t, np.linalg.inv(R), shape=shape)


# ----------------------------------------------------------------------------- rigid
def _rigid(mode, box, translation, rotation, shape=None):
    """The object undergoes x -> R (x - pos) + pos + t (pos = the box centre): the destination box has centre pos + t and axes A R^-1 (for
    a reference box: the columns of R O), a destination sample p comes from R^-1 (p - pos - t) + pos, its view direction from R^-1 d."""
    R = _np(rotation if rotation is not None else np.eye(3), (3, 3))
    t = _np(translation if translation is not None else np.zeros(3), (3,))
    Rinv = np.linalg.inv(R)
    pos = box.centre
    dst = EditBox(box.axes @ Rinv, pos + t, box.lo, box.hi)
    return Edit(mode, box, dst, Rinv, (pos - Rinv @ pos) - Rinv @ t, Rinv, shape=shape)


delete, extract = reference_delete, reference_extract          # (no motion in them: the rigid family shares the reference's forms)


def copy(box, translation=None, rotation=None, shape=None):
    """A rigid copy of the box's content at x -> R (x - pos) + pos + t; the original stays (nothing is killed).  With ``shape`` only the cells
    of the shape arrive; the rest of the destination box keeps its own content."""
    return _rigid(DUPLICATE, _box(box), translation, rotation, shape)


def move(box, translation=None, rotation=None, shape=None):
    """The box's content moved rigidly by x -> R (x - pos) + pos + t; what it leaves behind (in the source, not in the destination box) is
    killed.  With ``shape`` only the cells of the shape leave and arrive.  A rigid move keeps lo, hi and the local frame: the moved
    object is addressed at its destination (``Edit.dst``) with the same shape."""
    return _rigid(MANIPULATE, _box(box), translation, rotation, shape)


def rotation_from_euler_deg(rx, ry, rz):
    """R = Rz Ry Rx for rotations of rx, ry, rz degrees about the world x, y, z axes."""
    ax, ay, az = np.deg2rad([rx, ry, rz])
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx
