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


class Edit:
    """One resolved edit: kill rule (``mode``), source and destination box, the affine map p' = M p + t of samples inside the destination
    box and the matrix ``dir_inv`` applied to their view directions.  ``record()`` packs it as ``clift_edit_t``."""

    def __init__(self, mode, src, dst=None, M=None, t=None, dir_inv=None):
        if mode not in _MODE_NAMES:
            raise ValueError(f"unknown edit mode {mode!r}")
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

    def source_points(self, points):
        """Where (n, 3) world points are looked up: M p + t inside the destination box of a remapping edit, p elsewhere (fp64)."""
        p = np.asarray(points, dtype=np.float64)
        if self.mode < DUPLICATE:
            return p
        return np.where(self.dst.contains(p)[:, None], p @ self.M.T + self.t, p)

    def killed(self, points):
        src = self.src.contains(points)
        if self.mode == DELETE:
            return src
        if self.mode == EXTRACT:
            return ~src
        if self.mode == MANIPULATE:
            return src & ~self.dst.contains(points)
        return np.zeros(src.shape, dtype=bool)


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
                mov = ~dead & e.dst.contains(p)
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
        _lib.call("clift_edit_list_points", self.records(), len(self.edits), _lib.ptr(pts), 3, _lib.ptr(dr), 3, n, _lib.ptr(out_p),
                  _lib.ptr(out_d), _lib.ptr(state), _lib.stream())
        return out_p, out_d, state


def as_program(x):
    """An ``EditProgram`` from an ``Edit``, an ``EditProgram`` or a sequence of ``Edit``."""
    if isinstance(x, EditProgram):
        return x
    return EditProgram([x] if isinstance(x, Edit) else x)


def _box(b, pad=0.0):
    return b.padded(pad) if isinstance(b, EditBox) else EditBox.from_reference(b, pad)


# ----------------------------------------------------------------------------- reference-faithful
def reference_delete(bbox):
    """forward_delete (renderer.py:303-376): kill the samples inside the box."""
    return Edit(DELETE, _box(bbox))


def reference_extract(bbox):
    """forward_extract (renderer.py:379-453): kill the samples outside the box."""
    return Edit(EXTRACT, _box(bbox))


def reference_duplicate(bbox, translation, rotation):
    """forward_duplicate (renderer.py:456-536), the reference's arithmetic as written (O = orientation, R = rotation, pos = position):
    the destination box has centre R pos + t, axes = columns of R O and the same extent; samples inside it are looked up at p - t with the
    view direction R^-1 d; nothing is killed.  For R != I this is no rigid copy (the content is not turned, the box is, and it is turned
    about the origin): the quirk is reproduced on purpose."""
    O, pos, ext = _np(bbox["orientation"], (3, 3)), _np(bbox["position"], (3,)), _np(bbox["extent"], (3,))
    R, t = _np(rotation, (3, 3)), _np(translation, (3,))
    dst = EditBox((R @ O).T, R @ pos + t, -ext / 2, ext / 2)
    return Edit(DUPLICATE, _box(bbox), dst, np.eye(3), -t, np.linalg.inv(R))


def reference_manipulate(bbox, translation, rotation):
    """forward_manipulate (renderer.py:539-623), the reference's arithmetic as written: the destination box has centre pos + t and axes =
    columns of R O; samples inside it are looked up at R (p - pos) + pos - t with the view direction R^-1 d; samples inside the source box
    and outside the destination box are killed.  For R != I this is no rigid motion (a rigid one looks up R^-1 (p - pos - t) + pos): the
    quirk is reproduced on purpose -- ``move`` is the rigid form."""
    O, pos, ext = _np(bbox["orientation"], (3, 3)), _np(bbox["position"], (3,)), _np(bbox["extent"], (3,))
    R, t = _np(rotation, (3, 3)), _np(translation, (3,))
    dst = EditBox((R @ O).T, pos + t, -ext / 2, ext / 2)
    return Edit(MANIPULATE, _box(bbox), dst, R, (pos - R @ pos) - t, np.linalg.inv(R))


# ----------------------------------------------------------------------------- rigid
def _rigid(mode, box, translation, rotation):
    """The object undergoes x -> R (x - pos) + pos + t (pos = the box centre): the destination box has centre pos + t and axes A R^-1 (for
    a reference box: the columns of R O), a destination sample p comes from R^-1 (p - pos - t) + pos, its view direction from R^-1 d."""
    R = _np(rotation if rotation is not None else np.eye(3), (3, 3))
    t = _np(translation if translation is not None else np.zeros(3), (3,))
    Rinv = np.linalg.inv(R)
    pos = box.centre
    dst = EditBox(box.axes @ Rinv, pos + t, box.lo, box.hi)
    return Edit(mode, box, dst, Rinv, (pos - Rinv @ pos) - Rinv @ t, Rinv)


delete, extract = reference_delete, reference_extract          # (no motion in them: the rigid family shares the reference's forms)


def copy(box, translation=None, rotation=None):
    """A rigid copy of the box's content at x -> R (x - pos) + pos + t; the original stays (nothing is killed)."""
    return _rigid(DUPLICATE, _box(box), translation, rotation)


def move(box, translation=None, rotation=None):
    """The box's content moved rigidly by x -> R (x - pos) + pos + t; what it leaves behind (in the source, not in the destination box) is
    killed."""
    return _rigid(MANIPULATE, _box(box), translation, rotation)


def rotation_from_euler_deg(rx, ry, rz):
    """R = Rz Ry Rx for rotations of rx, ry, rz degrees about the world x, y, z axes."""
    ax, ay, az = np.deg2rad([rx, ry, rz])
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx
