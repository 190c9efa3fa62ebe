"""Records what contrastive_lift_amd.engine launches, on CPU stand-in tensors and without a GPU (helper of test_engine_launches.py).

``Recorder`` replaces ``engine.call`` for the duration of a ``with`` block: nothing is launched; every call is stored as
[entry point, arguments] with integers and floats as they are, pointers as None (NULL) or [buffer number, byte offset] -- buffers numbered by
first appearance in the record -- and structs (Gemm, VM, VMGrad, March, EditRec) as {field: value} in the same form, a struct inside a struct
likewise; a host array of structs (the ``edits`` of the clift_edit_list_* entry points) as the list of them, a host array of scalars (the
``c_float * 3`` box factors of the density-gradient launches) as the list of its values.  A clift_gemm launch also carries the name of the
route clift_gemm_route gives its descriptor (the real library: it loads without a GPU).

A pointer is resolved against the storages the recorder knows and keeps alive until it is dropped, so that no address is used twice within a
record: everything the engine allocates (``engine.torch`` is a proxy whose empty / zeros / empty_like / zeros_like / tensor register their
result), every tensor handed to ``engine.ptr``, and the ``roots`` of the case (parameter and gradient arenas, inputs, the field's persistent
scratch).  A pointer into none of them is an error.

Stand-ins for what the sequencing reads back from the device: clift_scan_counts / clift_scan_counts_capped write ``active`` into
ray_start[N] -- a sequence gives one count per scan, in order (the layer pass scans twice: the march's list, then its alpha-list);
``engine._rows_limit`` holds a CPU tensor so that the sync-free path never reaches torch.cuda.synchronize.
"""
import bisect
import ctypes as C

import torch

from contrastive_lift_amd import _lib, engine

_ALLOCATORS = ("empty", "zeros", "empty_like", "zeros_like", "tensor")


class _TorchProxy:
    """torch, with the allocating functions the engine uses registering what they return."""

    def __init__(self, own):
        for name in _ALLOCATORS:
            setattr(self, name, (lambda fn: lambda *a, **k: own(fn(*a, **k)))(getattr(torch, name)))

    def __getattr__(self, name):
        return getattr(torch, name)


def _f32_any_device(t, what="tensor"):
    if t.dtype != torch.float32:
        raise _lib.CliftError(f"{what}: expected a float32 tensor, got {t.dtype}")
    return t


class Recorder:
    def __init__(self, active=0, roots=lambda: (), launch=None, pointers=True):
        """``active``: the count the scan stand-ins report, or a sequence of them, one per scan.  ``roots``: callable giving tensors a pointer may point into without the engine having
        allocated them.  ``launch``: the real ``call`` to forward every launch to (GPU cross-check; no stand-ins then).  ``pointers`` False: record
        names and scalars only."""
        self.active = [int(a) for a in active] if isinstance(active, (list, tuple)) else int(active)
        self.roots, self.launch, self.pointers = roots, launch, pointers
        self.launches = []
        self._starts, self._spans, self._numbers = [], [], {}
        self._saved = None

    # ------------------------------------------------------------------ patching
    def __enter__(self):
        self._saved = (engine.call, engine.stream, engine.ptr, engine.torch, _lib.f32, dict(engine._rows_limit), engine._limit_owner)
        engine.call = self._call
        if self.launch is None:
            engine.stream = lambda: None
            engine.ptr = self._ptr
            engine.torch = _TorchProxy(self.own)
            _lib.f32 = _f32_any_device
            engine._rows_limit[("cpu", None)] = self.own(torch.tensor([engine.INT_MAX, 0], dtype=torch.int32))
            engine._limit_owner = None
        return self

    def __exit__(self, *exc):
        engine.call, engine.stream, engine.ptr, engine.torch, _lib.f32, limits, engine._limit_owner = self._saved
        engine._rows_limit.clear()
        engine._rows_limit.update(limits)
        self._starts, self._spans = [], []          # (drops the tensors kept alive)

    # ------------------------------------------------------------------ storages
    def own(self, t):
        s = t.untyped_storage()
        a, n = s.data_ptr(), s.nbytes()
        if n and a:
            i = bisect.bisect_left(self._starts, a)
            if i == len(self._starts) or self._starts[i] != a:
                self._starts.insert(i, a)
                self._spans.insert(i, (a + n, t))
        return t

    def _ptr(self, t):
        return None if t is None else C.c_void_p(self.own(t).data_ptr())

    def _find(self, p):
        i = bisect.bisect_right(self._starts, p) - 1
        if i >= 0 and p < self._spans[i][0]:
            return self._starts[i]
        return None

    def _pointer(self, p):
        if not p:
            return None
        base = self._find(p)
        if base is None:
            for t in self.roots():
                self.own(t)
            base = self._find(p)
        if base is None:
            raise AssertionError(f"launch {len(self.launches)}: pointer {p:#x} is in no tensor the recorder knows")
        return [self._numbers.setdefault(base, len(self._numbers)), p - base]

    def buffer_number(self, t):
        """The number the record gave the buffer ``t`` lives in, or -1 for one no launch has pointed into."""
        return self._numbers.get(t.untyped_storage().data_ptr(), -1)

    # ------------------------------------------------------------------ one launch
    def _struct(self, s):
        out = {}
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if ctype is C.c_void_p:
                if self.pointers:
                    out[name] = self._pointer(v)
            elif issubclass(ctype, C.Structure):
                out[name] = self._struct(v)
            elif issubclass(ctype, C.Array):
                if ctype._type_ is not C.c_void_p:
                    out[name] = list(v)
                elif self.pointers:
                    out[name] = [self._pointer(x) for x in v]
            else:
                out[name] = v
        return out

    def _call(self, name, *args):
        kinds = _lib._SIGNATURES[name][0]
        assert len(kinds) == len(args), f"{name}: {len(args)} arguments for a signature of {len(kinds)}"
        rec = []
        for kind, a in zip(kinds, args):
            if kind is not C.c_void_p:
                rec.append(float(a) if kind in (C.c_float, C.c_double) else int(a))
            elif hasattr(a, "_obj"):                     # byref(struct)
                rec.append(self._struct(a._obj))
            elif isinstance(a, C.Array) and issubclass(a._type_, C.Structure):        # host array of structs: by content, no device pointer
                rec.append([self._struct(x) for x in a])
            elif isinstance(a, C.Array):                 # host array of scalars: by content
                rec.append(list(a))
            elif self.pointers:
                rec.append(self._pointer(a.value if isinstance(a, C.c_void_p) else a))
        entry = [name, rec]
        if name == "clift_gemm" and self.pointers:
            lib = _lib.load()
            r = lib.clift_gemm_route(args[0])
            entry.append(lib.clift_gemm_route_name(r).decode() if r >= 0 else "error: " + lib.clift_last_error().decode())
        self.launches.append(entry)
        if self.launch is not None:
            self.launch(name, *args)
        elif name in ("clift_scan_counts", "clift_scan_counts_capped"):
            active = self.active.pop(0) if isinstance(self.active, list) else self.active
            C.c_int.from_address(args[2].value + 4 * int(args[1])).value = active          # ray_start[N]
