"""Kernel sequencing for the render hot path: explicit forward / backward over libclift.so entry points.

No torch autograd inside: ``render_forward`` returns the outputs plus a context holding the saved
activations, ``render_backward`` turns output gradients into parameter gradients written straight into the
caller's gradient views (the field's gradient arena in training).  ``renderer.py`` wraps this pair in a
``torch.autograd.Function`` for drop-in use.

Per chunk of N rays (reference renderer.py:80-176):
  density_fwd -> march_fwd -> scan/compact (one host read of the active count) ->
  appearance gather -> basis GEMM -> encode -> 2 GEMM+ReLU -> GEMM -> sigmoid
  xyz heads: K=3 first layer -> GEMM+ReLU chain -> narrow GEMM (-> softmax)
  composite.
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import edit as _edit
from . import layers as _layers
from ._lib import Gemm, March, VM, VMGrad, call, ptr, stream


# ----------------------------------------------------------------------------- struct builders
def march_struct(renderer, model):
    m = March()
    lo, hi = renderer.bbox_aabb_host
    inv = renderer.inv_box_extent_host
    for i in range(3):
        m.lo[i], m.hi[i], m.inv_ext2[i] = lo[i], hi[i], inv[i]
    m.step_size = renderer.step_size_host
    m.n_samples = int(renderer.n_samples)
    m.distance_scale = float(renderer.distance_scale)
    m.density_shift = float(model.splus_density_shift)
    m.weight_thres = float(renderer.raymarch_weight_thres)
    return m


def vm_struct(views, prefix, res):
    v = VM()
    for i in range(3):
        v.plane[i] = views[f"{prefix}_plane.{i}"].data_ptr()
        v.line[i] = views[f"{prefix}_line.{i}"].data_ptr()
        v.res[i] = int(res[i])
    v.comps = int(views[f"{prefix}_plane.0"].shape[1])
    return v


_GROUP_OF = {"density": "grid_density", "appearance": "grid_app", "semantic": "grid_sem", "instance": "grid_inst"}


def vm_grad_struct(model, gviews, prefix):
    """Gradient target of a scatter kernel: eight per-XCD accumulation copies (model-owned, persistent, zero between uses: XCD-local L2
    atomics) that ``vm_grad_finish`` folds into ``gviews``.  (xcd_stride = 0 in the C struct means "the final tables directly".)"""
    g = VMGrad()
    a, b = model.arena.range_of(_GROUP_OF[prefix])
    n = b - a
    work = model.xcd_workspace(prefix, 8 * n)
    base = work.data_ptr()
    for i in range(3):
        g.plane[i] = base + 4 * (model.arena.by_name[f"{prefix}_plane.{i}"].offset - a)
        g.line[i] = base + 4 * (model.arena.by_name[f"{prefix}_line.{i}"].offset - a)
    g.xcd_stride = n
    return g


def vm_grad_finish(model, gviews, prefix, g):
    if g.xcd_stride > 0:
        a, b = model.arena.range_of(_GROUP_OF[prefix])
        work = model.xcd_workspace(prefix, 8 * (b - a))
        # the tables of one group are contiguous in every arena-layout buffer, starting at plane 0
        dst = gviews[f"{prefix}_plane.0"]
        call("clift_xcd_reduce", ptr(work), g.xcd_stride, b - a, C.c_void_p(dst.data_ptr()), stream())


def grid_res(views):
    """(Rx,Ry,Rz) from the density table shapes: plane0 is (1,C,Ry,Rx), line0 is (1,C,Rz,1)."""
    p0, l0 = views["density_plane.0"], views["density_line.0"]
    return (p0.shape[3], p0.shape[2], l0.shape[2])


def _pitch(t):
    return t.stride(0) if t.dim() == 2 else 1


# MLP arithmetic of the matrix-core launches: 0 = "fp32" (exact fp32 products on the fp32 MFMA), 1 = "bf16" (operands rounded to bf16 in the
# kernel, fp32 accumulate, hidden activations bf16-stored -- BASELINE configs[2] / SURVEY 7.9), 2 = "fp32x6": every fp32 operand split
# EXACTLY into three bf16 terms (8 + 8 + 8 significant bits), the six leading cross products on v_mfma_f32_32x32x16_bf16, fp32 accumulate --
# fp32-faithful (the dropped terms are below one fp32 rounding of the product) for the 256-wide layers; narrow / 128-wide layers stay exact.
_PRECISIONS = {"fp32": 0, "f32": 0, "bf16": 1, "fp32x6": 2}
# The default since round 4 is fp32x6: fp32 results to fp32 round-off (row-max relative error against float64 2e-7 .. 8e-7, the exact kernels'
# own; whole-step gradients: no more entries outside the fp64 band than the exact path or the fp32 CPU oracle, profiles/r04_fp64_outliers.txt),
# 1.3 x the step rate of the exact-fp32 MFMA kernels.  "fp32" selects those (v_mfma_f32_32x32x2_f32: bit-identical to an fmaf chain).
DEFAULT_MLP_DTYPE = "fp32x6"
MLP_PRECISION = _PRECISIONS[os.environ.get("CLIFT_MLP_DTYPE", DEFAULT_MLP_DTYPE).lower()]


class _Precision:
    """Temporarily run the matrix-core launches at another operand precision (wave-uniform host state, restored on exit)."""

    def __init__(self, p):
        self.p = p

    def __enter__(self):
        global MLP_PRECISION
        self.prev, MLP_PRECISION = MLP_PRECISION, self.p

    def __exit__(self, *a):
        global MLP_PRECISION
        MLP_PRECISION = self.prev


def exact_fp32():
    """Context: matrix-core launches on the exact-fp32 kernels whatever mode is set or forced (tests of the exact kernels' fusions)."""
    return _Precision(0)


# bf16 mode and the 128-wide appearance MLP.  Rounds 2 - 4 kept it on the exact-fp32 persistent kernels (layer_n128.hip): faster than the TILED bf16
# kernels on these short-K layers, but bound by the fp32 matrix pipe (6 launches, 635 us of a 3.4 ms step).  Round 5: streaming bf16 kernels with
# bf16-STORED input / hidden activations / hidden gradients (csrc/layer_nb16.hip), like the xyz heads of that mode.  Tests clear APP_BF16 to get the
# old arrangement back.
APP_BF16 = True
# fp32x6 mode and the same layers.  Rounds 3 - 4 kept them exact as well (the only split kernel for their shapes was the tiled one: slower than the
# exact persistent kernels).  Round 5: persistent split kernels for the 128-wide forms (csrc/layer_n6.hip) -- 6 / 16 of the matrix time, the same
# fp32 streams.  Tests clear APP_X6 to get the exact arrangement back.
APP_X6 = True


def _app_precision():
    # fp32x6 (2): only the 256 x 256 layers have persistent split kernels; the 128-wide appearance layers would fall to the TILED split kernel
    # (gemm_split.hip), which is slower than the exact persistent kernels and -- seen with two processes sharing the GPU -- the one kernel of that
    # mode whose results were disturbed by the other process's fp32x6 launches (profiles/r03_x6_notes.txt).  Exact fp32 there.
    if MLP_PRECISION == 1 and APP_BF16 and persistent_ok():
        return _Precision(1)
    if MLP_PRECISION == 2 and APP_X6 and persistent_mode_ok():
        return _Precision(2)
    return _Precision(0)


def act_dtype():
    """Storage type of the hidden activations / hidden gradients of the xyz-MLP heads: bf16 in bf16 mode (they are only ever
    consumed as bf16 matrix-core operands or as ReLU masks there), fp32 otherwise."""
    return torch.bfloat16 if MLP_PRECISION == 1 else torch.float32


def set_mlp_precision(name):
    """'fp32', 'bf16' or 'fp32x6'; returns the previous setting's name."""
    global MLP_PRECISION
    prev = {0: "fp32", 1: "bf16", 2: "fp32x6"}[MLP_PRECISION]
    MLP_PRECISION = _PRECISIONS[str(name).lower()]
    return prev


# Kernel switches (include/clift.h, CLIFT_SWITCH_*): the library's word, set through kernel_switches() below -- or, once, at the first launch of
# a process started with one of the switch variables of include/clift.h in its environment.  The fusion conditions of this module read the
# cached copy: it changes in kernel_switches() only, so no library call is added to the launch path.
SWITCH_TILED_ONLY, SWITCH_X6_TILED, SWITCH_DENS_FWD_THREAD, SWITCH_DENS_SCATTER_WALK = 1, 2, 4, 8
_switches = None


def _switch_word():
    global _switches
    if _switches is None:
        _switches = int(_lib.load().clift_get_switches())
    return _switches


def persistent_ok():
    """Persistent / streaming / fused kernels allowed (the tiled-only switch is off)."""
    return not _switch_word() & SWITCH_TILED_ONLY


def persistent_x6_ok():
    """Persistent fp32x6 split kernels allowed (the x6-tiled switch is off)."""
    return not _switch_word() & SWITCH_X6_TILED


def persistent_mode_ok():
    """The persistent kernels of the mode that is set are allowed: persistent_ok() and, in fp32x6 mode, persistent_x6_ok()."""
    return persistent_ok() and (MLP_PRECISION != 2 or persistent_x6_ok())


@contextlib.contextmanager
def kernel_switches(tiled_only=None, x6_tiled=None, dens_fwd_thread=None, dens_scatter_walk=None):
    """Context: set (True) or clear (False) kernel switches of the library -- None leaves one as it is -- and restore the word on exit.
    The cross-checks of the test-suite and the A/B tools: the independent tiled kernels against the persistent ones on the same inputs."""
    global _switches
    prev = word = _switch_word()
    for bit, on in ((SWITCH_TILED_ONLY, tiled_only), (SWITCH_X6_TILED, x6_tiled), (SWITCH_DENS_FWD_THREAD, dens_fwd_thread),
                    (SWITCH_DENS_SCATTER_WALK, dens_scatter_walk)):
        if on is not None:
            word = (word | bit) if on else (word & ~bit)
    _lib.load().clift_set_switches(word)
    _switches = word
    try:
        yield
    finally:
        _lib.load().clift_set_switches(prev)
        _switches = prev


_x6_routes = None


def _x6_persistent_routes():
    """The clift_gemm routes of the persistent fp32x6 split kernels (they need no workspace)."""
    global _x6_routes
    if _x6_routes is None:
        routes = _lib.gemm_routes()
        _x6_routes = frozenset(routes[n] for n in ("LAYER_X6", "WGRAD_X6", "LAYER_N6", "WGRAD_N6"))
    return _x6_routes


def sign_bits_for(M, dev):
    """Scratch for the sign bytes of an (M, 256) activation written by a persistent fp32x6 forward (clift_gemm_t.sign_bits): 32 B per row."""
    return torch.empty(((M + 31) // 32 * 1024,), dtype=torch.uint8, device=dev)


def _scratch(nbytes, dev):
    """Stream-ordered scratch of one launch.  Launched on a side stream (Branches), the allocator must not recycle it before that stream is done."""
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if _lib._launch_stream is not None:
        ws.record_stream(_lib._launch_stream)
    return ws


def gemm(M, N, K, A, lda, B, ldb, Cm, ldc, a_trans=0, b_trans=0, bias=None, act=0, mask=None, ldmask=0,
         accumulate=0, split_k=1, a_off=0, c_off=0, c_trans=0, colsum=None, sign_bits=None):
    """One clift_gemm launch.  Pitches and offsets are in ELEMENTS of the respective tensor; a tensor of dtype bfloat16 is
    passed as bf16-stored (bf16 mode only: hidden activations and their gradients)."""
    g = Gemm()
    g.M, g.N, g.K = int(M), int(N), int(K)
    g.A, g.lda, g.a_trans = A.data_ptr() + A.element_size() * a_off, int(lda), int(a_trans)
    g.B, g.ldb, g.b_trans = B.data_ptr(), int(ldb), int(b_trans)
    g.C, g.ldc = Cm.data_ptr() + Cm.element_size() * c_off, int(ldc)
    g.bias = bias.data_ptr() if bias is not None else None
    g.act = int(act)
    g.mask = mask.data_ptr() if mask is not None else None
    g.ldmask = int(ldmask)
    g.accumulate, g.split_k = int(accumulate), int(split_k)
    g.c_trans = int(c_trans)
    g.colsum = colsum.data_ptr() if colsum is not None else None
    g.sign_bits = sign_bits.data_ptr() if sign_bits is not None else None
    g.a_bf16, g.b_bf16 = int(A.dtype == torch.bfloat16), int(B.dtype == torch.bfloat16)
    g.c_bf16, g.mask_bf16 = int(Cm.dtype == torch.bfloat16), int(mask is not None and mask.dtype == torch.bfloat16)
    g.precision = MLP_PRECISION
    # fp32x6 mode: the launches the library has persistent split kernels for -- the 256 x 256 hidden layers (csrc/layer_x6.hip, layer_x6w.hip) and the
    # 128-wide layers of the appearance MLP (csrc/layer_n6.hip), forward / dgrad / weight gradient -- run on them; clift_gemm_route says which those are
    route = _lib.load().clift_gemm_route(C.byref(g)) if MLP_PRECISION == 2 else None
    if MLP_PRECISION == 2 and route not in _x6_persistent_routes():
        if N == 256 and K == 256 and not a_trans and not accumulate and not c_trans:
            # a 256 x 256 forward / dgrad the persistent kernel does not take (rows not 16-byte aligned, odd output pitch, the x6-tiled switch ...)
            # goes to the library's tiled split kernel, which needs a workspace for the split weight planes
            if route != 0:      # (route 0: an empty launch, nothing runs)
                nbytes = int(_lib.load().clift_gemm_workspace_bytes(int(N), int(K)))
                g.workspace, g.workspace_bytes = _scratch(nbytes, A.device).data_ptr(), nbytes      # split weight planes
        else:
            # every other launch -- narrow layers (HBM streams), the remaining weight gradients -- stays on its exact-fp32 persistent kernel, which is
            # faster than the tiled split kernel the library would pick for it
            g.precision = 0
    call("clift_gemm", C.byref(g), stream())


def wgrad(no, ni, M, dY, ldd, X, ldx, gW, gb):
    """gW (no, ni) += dY^T X over the M samples; gb (no) += column sums of dY.  Wide layers: matrix cores, the bias sum
    fused into the GEMM (read from the A tile already staged in LDS).  Narrow layers (no <= 32): a streaming VALU
    reduction at HBM rate (clift_wgrad_narrow)."""
    if no > 32:
        gemm(no, ni, M, dY, ldd, X, ldx, gW, _pitch(gW), a_trans=1, b_trans=1, accumulate=1, split_k=_splits(no, ni, M), colsum=gb)
    else:
        if dY.dtype != torch.float32:
            raise _lib.CliftError("narrow wgrad: the output-side gradient must be fp32")
        call("clift_wgrad_narrow", ptr(dY), ldd, no, ptr(X), ldx, ni, M, ptr(gW), _pitch(gW), ptr(gb), int(X.dtype == torch.bfloat16), stream())


def _splits(out_rows, out_cols, K):
    """Split the (huge) sample-reduction of a wgrad over blockIdx.z so that the launch is ONE resident wave of workgroups
    (256 CUs x 2 blocks = 512): measured at 265 k samples, 256x256 / 128x128 / 128x152 outputs: 512 blocks 332 / 125 / 208 us,
    1024 blocks 378 / 165 / 261 us, 384 or 640 blocks worse than either (partial second wave, twice the atomics)."""
    tiles = ((out_rows + 127) // 128) * ((out_cols + 255) // 256 if out_cols > 128 else (out_cols + 127) // 128 if out_cols > 32 else 1)
    return max(1, min((K + 255) // 256, (512 + tiles - 1) // tiles))


def _lin_params(views_prefix, views):
    """[(W, b)] of an nn.Sequential MLP, fetched from a name->tensor dict (parameter or gradient views)."""
    out = []
    j = 0
    while f"{views_prefix}.{j}.weight" in views:
        out.append((views[f"{views_prefix}.{j}.weight"], views[f"{views_prefix}.{j}.bias"]))
        j += 2
    return out


# ----------------------------------------------------------------------------- concurrent head chains
MULTI_STREAM = os.environ.get("CLIFT_STREAMS", "0") == "1"   # opt-in; +4 % with the tiled kernels, -3 % with the persistent ones
_side_streams = {}


class Branches:
    """Fork/join of independent kernel chains over HIP streams.  The appearance, semantic, fast-instance and slow-instance
    heads are independent between the compaction and the compositing, and every layer-wide GEMM has a start-up phase and
    an un-overlapped output burst (see gemm.hip) that another chain's MFMA work can fill.  Launches of a branch go to a
    side stream (via _lib.set_launch_stream); ALL allocations stay on torch's current stream, and every temporary of a
    branch is kept alive in ``self.keep`` until ``join`` so that no block is recycled into another in-flight branch."""

    def __init__(self, enabled=True, model=None):
        # a head on its own VM grid (engine.grid_head_fwd / _bwd) issues torch ops -- zero fills, add_ -- which live on torch's CURRENT stream, not
        # on the branch's side stream: such a field keeps every branch on the main stream
        if model is not None and (getattr(model, "semantic_plane", None) is not None or getattr(model, "instance_plane", None) is not None):
            enabled = False
        self.enabled = enabled and MULTI_STREAM
        self.keep = []
        self.used = []
        if self.enabled:
            self.main = torch.cuda.current_stream()
            self.fork = torch.cuda.Event()
            self.fork.record(self.main)

    def run(self, idx, fn):
        if not self.enabled:
            fn(self.keep)
            return
        dev = torch.cuda.current_device()
        st = _side_streams.get((dev, idx))
        if st is None:
            st = _side_streams[(dev, idx)] = torch.cuda.Stream(device=dev)
        st.wait_event(self.fork)
        _lib.set_launch_stream(st)
        try:
            fn(self.keep)
        finally:
            _lib.set_launch_stream(None)
        self.used.append(st)

    def join(self):
        if self.enabled:
            for st in self.used:
                ev = torch.cuda.Event()
                ev.record(st)
                self.main.wait_event(ev)
        self.keep = []
        self.used = []


# ----------------------------------------------------------------------------- xyz MLP heads (semantic / instance)
def last2(M, h, W, b, Wo, bo, hidden, out, ldo, col_off):
    """One clift_xyz_head_last2_fwd launch: hidden = relu(h W^T + b) (written if not None), out[:, col_off:col_off+E] = hidden Wo^T + bo."""
    call("clift_xyz_head_last2_fwd", ptr(h), h.shape[1], ptr(W), _pitch(W), ptr(b), ptr(Wo), _pitch(Wo), ptr(bo), Wo.shape[0], M, ptr(hidden), 256,
         C.c_void_p(out.data_ptr() + 4 * col_off), ldo, stream())


def app_last2(M, H1, W2, b2, W3, b3, H2, rgb):
    """One clift_app_head_last2_fwd launch: H2 = relu(H1 W2^T + b2) (written if not None), rgb = sigmoid(H2 W3^T + b3)."""
    call("clift_app_head_last2_fwd", ptr(H1), H1.shape[1], ptr(W2), _pitch(W2), ptr(b2), ptr(W3), _pitch(W3), ptr(b3), W3.shape[0], M,
         ptr(H2), 128, None, 0, ptr(rgb), rgb.shape[1], 1, stream())


def head_bf16(M, xa, l0, l1, l2, lout, h1, h2, h3, out, ldo, col_off):
    """One clift_xyz_head_bf16_fwd launch (csrc/head_bf16.hip)."""
    (W0, b0), (W1, b1), (W2, b2) = l0, l1, l2
    Wo, bo = lout if lout is not None else (None, None)
    call("clift_xyz_head_bf16_fwd", ptr(xa), ptr(W0), _pitch(W0), ptr(b0), ptr(W1), _pitch(W1), ptr(b1), ptr(W2), _pitch(W2), ptr(b2),
         ptr(Wo), _pitch(Wo) if Wo is not None else 0, ptr(bo), Wo.shape[0] if Wo is not None else 0, M, ptr(h1), ptr(h2), ptr(h3),
         C.c_void_p(out.data_ptr() + 4 * col_off) if lout is not None else None, ldo, stream())


def first2(M, xa, W0, b0, W1, b1, h1, h2):
    """One clift_xyz_head_first2_fwd launch: h2 = relu(W1 relu(W0 x + b0) + b1); h1 (or None) receives the first layer's activation.
    (A module-level function so that bench.py can bracket these launches with events like it does engine.gemm.)"""
    call("clift_xyz_head_first2_fwd", ptr(xa), ptr(W0), _pitch(W0), ptr(b0), ptr(W1), _pitch(W1), ptr(b1), M, ptr(h1), 256, ptr(h2), 256, stream())


# The fusions of the xyz heads (xyz_head_route, _xyz_bwd_route) are not switchable one by one: their A/Bs are settled (profiles/r02_*,
# r03_ab_first2_bwd.txt, r04_ab_x6_fused_ends.txt).  The tiled-only switch -- kernel_switches(tiled_only=True), or its environment variable
# (include/clift.h) read once at start -- selects the independent tiled kernels for every layer instead (the cross-check the tests use).
APP_SCATTER_XA = True       # tests clear it: clift_app_gather_bwd without the forward's positions (xa = NULL: the lane-per-(plane, channel) walk)
DENS_BWD_SIGMA = True       # tests clear it: clift_density_bwd without the forward's sigma (sigma = NULL: the softplus derivative re-summed)
FIRST2_BF16_BWD_FUSED = True  # tests clear it: bf16 mode, the second layer's input gradient written and the K = 3 layer's weight gradient as its own launch
OUT_BWD_BF16_FUSED = True   # tests clear it: bf16 mode, output layer's weight gradient and masked input gradient as two passes over the hidden activation
COMPOSITE_ACT_FUSED = True  # tests clear it: the heads' output activations taken back by clift_rows_act_bwd launches after the compositing backward
APP_OUT_BWD_FUSED = True    # tests clear it: the appearance output layer's weight gradient and masked input gradient as two passes over the hidden activation
APP_FRONT_FUSED = True      # tests clear it: appearance gather, basis GEMM and input encoding as three launches (the form the fused front end replaced)
KEEP_FIRST_ACT = False      # tests set this to compare against the stored-activation backward (masked dgrad + K = 3 weight gradient)
SOAK_KEEP = False           # tools/determinism_soak.py sets it: a forward that retains nothing still leaves REFERENCES to the appearance chain's intermediates in ctx.soak
FUSE_HEAD_BF16 = True       # bf16 mode: first three layers (+ E <= 4 output layer) of an xyz head in one launch; tests clear it to compare with the per-layer launches


def first2_bwd(M, d, W1, W0, b0, xa, gW0, gb0):
    """One clift_xyz_head_first2_bwd launch: gW0 += ((W0 x + b0 > 0) . (d W1))^T xa[:, :3], gb0 += column sums of the same masked gradient.
    (Module-level for the same reason as first2.)"""
    call("clift_xyz_head_first2_bwd", ptr(d), d.shape[1], ptr(W1), _pitch(W1), ptr(W0), _pitch(W0), ptr(b0), ptr(xa), M, ptr(gW0), _pitch(gW0), ptr(gb0),
         stream())


def first2_x6(M, xa, W0, b0, W1, b1, h2, sign_bits=None):
    """One clift_xyz_head_first2_x6_fwd launch (fp32x6 mode): h2 = relu(W1 relu(W0 x + b0) + b1), the first activation not written;
    ``sign_bits`` (optional uint8 scratch from sign_bits_for) receives the signs of h2 for the next layer's masked dgrad."""
    call("clift_xyz_head_first2_x6_fwd", ptr(xa), ptr(W0), _pitch(W0), ptr(b0), ptr(W1), _pitch(W1), ptr(b1), M, ptr(h2), 256, ptr(sign_bits), stream())


def first2_x6_bwd(M, d, W1, W0, b0, xa, gW0, gb0):
    """One clift_xyz_head_first2_x6_bwd launch (fp32x6 mode): first2_bwd with the 256 x 256 product on the split kernels."""
    call("clift_xyz_head_first2_x6_bwd", ptr(d), d.shape[1], ptr(W1), _pitch(W1), ptr(W0), _pitch(W0), ptr(b0), ptr(xa), M, ptr(gW0), _pitch(gW0), ptr(gb0),
         stream())


def first2_x6_wgrad(M, d, W0, b0, xa, gW1, gb1):
    """One clift_xyz_head_first2_x6_wgrad launch (fp32x6 mode): first2_wgrad on the split weight-gradient kernel."""
    call("clift_xyz_head_first2_x6_wgrad", ptr(d), d.shape[1], ptr(W0), _pitch(W0), ptr(b0), ptr(xa), M, ptr(gW1), _pitch(gW1), ptr(gb1), stream())


def last2_x6(M, h, W, b, Wo, bo, hidden, out, ldo, col_off):
    """One clift_xyz_head_last2_x6_fwd launch (fp32x6 mode): last2 with the 256 x 256 layer on the split kernel; the output layer's partial
    sums travel through a stream-ordered scratch buffer (256 B per row)."""
    nbytes = 256 * M
    call("clift_xyz_head_last2_x6_fwd", ptr(h), h.shape[1], ptr(W), _pitch(W), ptr(b), ptr(Wo), _pitch(Wo), ptr(bo), Wo.shape[0], M, ptr(hidden), 256,
         C.c_void_p(out.data_ptr() + 4 * col_off), ldo, ptr(_scratch(nbytes, h.device)), nbytes, stream())


def first2_wgrad(M, d, W0, b0, xa, gW1, gb1):
    """One clift_xyz_head_first2_wgrad launch: gW1 += d^T relu(xa[:, :3] W0^T + b0), gb1 += column sums of d."""
    call("clift_xyz_head_first2_wgrad", ptr(d), d.shape[1], ptr(W0), _pitch(W0), ptr(b0), ptr(xa), M, ptr(gW1), _pitch(gW1), ptr(gb1), stream())


def out_layer_fwd(M, h, W, b, out, ldo, col_off, act):
    """One clift_out_layer_fwd launch: out[:, col_off:col_off+no] = act(h W^T + b), no <= 32, act 0 / 2 (row softmax) -- one read of h."""
    call("clift_out_layer_fwd", ptr(h), h.shape[1], ptr(W), _pitch(W), ptr(b), W.shape[0], M, C.c_void_p(out.data_ptr() + 4 * col_off), ldo, act, stream())


def _out_layer(M, h, W, K, b, out, ldo, col_off, out_act, fused=False):
    """The narrow output layer of a head over the K columns of h: out[:, col_off:col_off + n_out] = h W^T + b, then the row softmax when
    ``out_act`` is 2.  ``fused``: a hidden layer's kernel has already written the logits, only the softmax remains."""
    if not fused:
        if (MLP_PRECISION in (0, 2) and W.shape[0] <= 32 and K == 256 and h.dtype == torch.float32 and h.shape[1] == 256 and out.dtype == torch.float32
                and _pitch(W) % 4 == 0 and b is not None and persistent_ok()):
            # the E <= 32 output layer (+ the row softmax) as one stream over the hidden activation
            out_layer_fwd(M, h, W, b, out, ldo, col_off, out_act)
            return
        gemm(M, W.shape[0], K, h, h.shape[1], W, _pitch(W), out, ldo, bias=b, c_off=col_off)
    if out_act == 2:        # in place
        o = C.c_void_p(out.data_ptr() + 4 * col_off)
        call("clift_rows_act_fwd", o, ldo, M, W.shape[0], 2, o, ldo, stream())


HeadRoute = collections.namedtuple("HeadRoute", "front out_in_front tail first_stored signs")


def xyz_head_route(layers, keep, out_dtype):
    """The kernels the forward of an xyz head runs on, from the layer shapes, the precision that is set, the fusion flags and the cached switch
    word: nothing is allocated, launched or asked of the library.  xyz_mlp_fwd dispatches on it and hands it to the backward in the HeadActs.
      front         "fused3_bf16" | "first2" | "first2_x6" | "k3": what takes the K = 3 layer, with the two / the one 256 x 256 layer behind it or alone
      out_in_front  the output layer runs inside the front end as well
      tail          "last2" | "last2_x6" | None: the last hidden layer and the output layer in one launch
      first_stored  a forward that keeps its activations (``keep``) writes the K = 3 layer's; False: the backward re-derives it
      signs         the hidden activations whose signs such a forward leaves (sign_bits_for) for the next layer's masked dgrad
    A new fused kernel adds a value here, its predicate in this function and a case in xyz_mlp_fwd."""
    n, P = len(layers), MLP_PRECISION
    wide = lambda i: tuple(layers[i][0].shape) == (256, 256)
    narrow_out = layers[-1][0].shape[0] <= 4 and out_dtype == torch.float32
    gen = n >= 3 and layers[0][0].shape[0] == 256 and wide(1)       # the K = 3 layer can be generated inside the second layer's kernel
    if FUSE_HEAD_BF16 and P == 1 and gen and n >= 4 and wide(2) and persistent_ok():
        # bf16 mode: K = 3 layer + two hidden layers (+ the output layer when it is <= 4 wide and follows directly) in one launch with the
        # activations resident in LDS
        return HeadRoute("fused3_bf16", n == 4 and narrow_out, None, True, ())
    # (the first activation has no reader: first2_bwd / first2_wgrad re-derive it from the positions.  KEEP_FIRST_ACT stores it all the same,
    # which only the exact kernel can: the split kernel has no output for it)
    fused2 = P in (0, 2) and gen and persistent_mode_ok() and not (P == 2 and keep and KEEP_FIRST_ACT)
    front = ("first2_x6" if P == 2 else "first2") if fused2 else "k3"
    fused_tail = P in (0, 2) and n - 2 >= 1 + fused2 and narrow_out and wide(n - 2) and persistent_mode_ok()     # (a hidden layer is left for it)
    # fp32x6, a backward will run: the persistent kernels also leave the SIGNS of their output (32 B per row), so that the next layer's masked dgrad does
    # not stream the 1 KB-per-row activation again just to test it against zero -- but the last hidden layer's, which the output layer's backward reads as values
    signs = tuple(i for i in range(1, n - 2) if wide(i)) if (keep and P == 2 and persistent_mode_ok()) else ()
    return HeadRoute(front, False, ("last2_x6" if P == 2 else "last2") if fused_tail else None, front == "k3" or (front == "first2" and KEEP_FIRST_ACT), signs)


class HeadActs(list):
    """The hidden activations an xyz head keeps for its backward (acts[i] = output of layer i, or None where the backward re-derives it), plus
    -- fp32x6 mode -- the sign bytes a persistent forward left for activation i (``signs[i]``, from sign_bits_for): held HERE, next to the tensor
    they describe and for exactly as long, instead of as an ad-hoc attribute on the tensor object (which a view or a clone would drop silently).
    ``route``: the HeadRoute the forward ran on (None for a list built by hand: every activation stored); ``kept`` False: that forward
    retained nothing (keep_first=False), the list is [None] and a backward is refused."""

    def __init__(self, *a, route=None, kept=True):
        super().__init__(*a)
        self.signs, self.route, self.kept = {}, route, kept

    def sign_bits_of(self, i, M):
        """The sign bytes of activation i, or None; checked against the activation they were written with."""
        sb = self.signs.get(i)
        if sb is None:
            return None
        h = self[i]
        if h is None or h.shape[0] != M or sb.numel() != (M + 31) // 32 * 1024:
            raise _lib.CliftError("sign bytes and activation of an xyz head do not come from the same forward")
        return sb


def xyz_mlp_fwd(layers, xa, M, out, ldo, col_off=0, keep_first=True, out_act=0):
    """layers = [(W,b)]; xa (M,4); hidden activations returned for the backward; final layer written into
    out[:, col_off:col_off+n_out] with row pitch ldo -- as logits (``out_act`` 0) or after a softmax over the row (2: the semantic head,
    tensoRF.py:37,593; applied inside the output layer's kernel where that exists, else in place by a row-activation launch).
    ``keep_first`` = False: the caller will not run a backward through this head, so a hidden activation is written only where a following launch
    reads it and none is retained (a frame render at 65536 rays per chunk holds ~9 GiB per hidden layer otherwise)."""
    dev, n = xa.device, len(layers)
    r = xyz_head_route(layers, keep_first, out.dtype)
    acts = HeadActs(route=r)
    hdt = act_dtype()                     # bf16 mode stores the hidden activations as bf16 (half the HBM stream of these layers)
    new = lambda on=True, width=256: torch.empty((M, width), dtype=hdt, device=dev) if on else None
    signs = lambda i: acts.signs.setdefault(i, sign_bits_for(M, dev)) if i in r.signs else None
    (W0, b0), (Wo, bo) = layers[0], layers[-1]
    if r.front == "fused3_bf16":
        acts += [new(keep_first), new(keep_first), new(keep_first or not r.out_in_front)]
        head_bf16(M, xa, layers[0], layers[1], layers[2], (Wo, bo) if r.out_in_front else None, *acts, out, ldo, col_off)
    elif r.front == "first2":
        acts += [new(keep_first and r.first_stored), new()]
        first2(M, xa, W0, b0, *layers[1], *acts)
    elif r.front == "first2_x6":
        acts += [None, new()]
        first2_x6(M, xa, W0, b0, *layers[1], acts[1], signs(1))
    else:
        acts.append(new(width=W0.shape[0]))
        call("clift_linear_k3_fwd", ptr(xa), ptr(W0), _pitch(W0), ptr(b0), M, W0.shape[0], 1, ptr(acts[0]), W0.shape[0], int(hdt == torch.bfloat16), stream())
    for li in range(len(acts), n - 1):
        (W, b), h = layers[li], acts[-1]
        if r.tail and li == n - 2:
            hn = new(keep_first)
            (last2_x6 if r.tail == "last2_x6" else last2)(M, h, W, b, Wo, bo, hn, out, ldo, col_off)
        else:
            hn = new(width=W.shape[0])
            gemm(M, W.shape[0], W.shape[1], h, h.shape[1], W, _pitch(W), hn, hn.shape[1], bias=b, act=1, sign_bits=signs(li))
        acts.append(hn)
    _out_layer(M, acts[-1], Wo, Wo.shape[1], bo, out, ldo, col_off, out_act, fused=r.out_in_front or r.tail is not None)
    return acts if keep_first else HeadActs([None], route=r, kept=False)


def _xyz_bwd_route(layers, acts, li, d, M):
    """How layer ``li`` >= 1 of an xyz head is taken back.  What the forward stored is read from its record; the rest is the state at backward
    time: the fusion flags, the switches, M, type and pitch of the layer's output gradient ``d``.
      "first2" | "first2_x6" | "first2_bf16"   layers 1 and 0 together, which ends the chain: the second layer's weight gradient, then its
                         input gradient formed and consumed by the K = 3 layer's weight gradient in one launch
      "out" | "out_nh"   the output layer's weight gradient and masked input gradient in one pass over the hidden activation; _nh (bf16 mode):
                         over the bf16-stored activation, the layer's width and a bf16 flag passed, the input gradient leaves bf16-stored
      "signs" | "mask"   weight gradient, then the input gradient masked by the sign bytes the forward left / by the stored activation"""
    W, h, P, f32 = layers[li][0], acts[li - 1], MLP_PRECISION, torch.float32
    (no, ni), nh, wide = W.shape, P == 1, tuple(W.shape) == (256, 256)
    if li == 1:
        gen = wide and tuple(layers[0][0].shape) == (256, 3)
        regen = acts.route is not None and not acts.route.first_stored        # (then the forward has checked the shapes: ``gen`` holds)
        if regen and d.dtype != f32:
            raise _lib.CliftError("backward through an xyz head in bf16 mode whose forward ran in another mode and stored no first activation")
        if regen or (not KEEP_FIRST_ACT and P in (0, 2) and gen and d.dtype == f32 and h.dtype == f32 and d.shape[1] % 4 == 0 and persistent_ok()):
            return "first2_x6" if P == 2 and persistent_x6_ok() else "first2"
        if nh and FIRST2_BF16_BWD_FUSED and gen and h.dtype == d.dtype == torch.bfloat16 and d.shape[1] == h.shape[1] == 256 and M >= 4096 and persistent_ok():
            return "first2_bf16"
    if (li == len(layers) - 1 and ni == 256 and no <= 32 and d.shape[1] <= 32 and d.shape[1] % 4 == 0 and M >= 4096 and d.dtype == f32
            and h.dtype == act_dtype() and (not nh or (OUT_BWD_BF16_FUSED and h.shape[1] == 256 and _pitch(W) >= 256))):
        return "out_nh" if nh else "out"
    if acts.sign_bits_of(li - 1, M) is not None and P == 2 and wide and d.dtype == f32 and d.shape[1] % 4 == 0 and persistent_x6_ok():
        return "signs"
    return "mask"


def xyz_mlp_bwd(layers, glayers, xa, acts, dpre, M, keep=None):
    """dpre (M, ld) = gradient w.r.t. the last layer's pre-activation output (ld % 4 == 0, pad zero).
    ``keep``: list that receives every temporary (so a caller running this on a side stream controls their lifetime)."""
    if not acts.kept:
        raise _lib.CliftError("backward through an xyz head whose forward ran with keep_first=False (head not named in grad_heads)")
    dev, d, keep = xa.device, dpre, keep if keep is not None else []
    keep.append(d)
    (W0, b0), (gW0, gb0) = layers[0], glayers[0]
    for li in range(len(layers) - 1, 0, -1):
        (W, b), (gW, gb), h = layers[li], glayers[li], acts[li - 1]
        no, ni = W.shape
        how = _xyz_bwd_route(layers, acts, li, d, M)
        if how.startswith("first2"):
            if h is None:           # (over the first layer's activation regenerated from the positions)
                (first2_x6_wgrad if how == "first2_x6" else first2_wgrad)(M, d, W0, b0, xa, gW, gb)
            else:
                wgrad(no, ni, M, d, d.shape[1], h, h.shape[1], gW, gb)
            if how == "first2_bf16":
                call("clift_xyz_head_first2_bf16_bwd", ptr(d), 256, ptr(W), _pitch(W), ptr(h), 256, ptr(xa), M, ptr(gW0), _pitch(gW0), ptr(gb0), stream())
            else:
                (first2_x6_bwd if how == "first2_x6" else first2_bwd)(M, d, W, W0, b0, xa, gW0, gb0)
            return
        dn = torch.empty((M, ni), dtype=act_dtype(), device=dev)        # bf16 mode: hidden gradients are bf16-stored as well
        if how == "out":
            call("clift_out_layer_bwd", ptr(d), d.shape[1], no, ptr(W), _pitch(W), ptr(h), h.shape[1], M, ptr(dn), ni, ptr(gW), _pitch(gW), ptr(gb), stream())
        elif how == "out_nh":
            call("clift_out_layer_bwd_nh", ptr(d), d.shape[1], no, ptr(W), _pitch(W), ptr(h), h.shape[1], ni, M, ptr(dn), ni, ptr(gW), _pitch(gW), ptr(gb), 1, stream())
        else:
            wgrad(no, ni, M, d, d.shape[1], h, h.shape[1], gW, gb)
            if how == "signs":
                gemm(M, ni, no, d, d.shape[1], W, _pitch(W), dn, ni, b_trans=1, sign_bits=acts.signs[li - 1])
            else:
                gemm(M, ni, no, d, d.shape[1], W, _pitch(W), dn, ni, b_trans=1, mask=h, ldmask=h.shape[1])
        d = dn
        keep.append(d)
    call("clift_linear_k3_bwd", ptr(xa), ptr(d), d.shape[1], M, W0.shape[0], ptr(gW0), _pitch(gW0), ptr(gb0), int(d.dtype == torch.bfloat16), stream())


# ----------------------------------------------------------------------------- heads on their own VM grids (tensoRF.py:70-83,142-156)
def _grid_precision():
    # the grid heads' MLPs are short (27 -> 128 -> 128 -> C, 27 -> 256 -> 256 -> E): in bf16 mode they stay exact (no bf16-stored forms are built
    # for them); in fp32x6 mode engine.gemm sends their one 256 x 256 layer to the split kernels like any other
    return _Precision(0 if MLP_PRECISION == 1 else MLP_PRECISION)


def feat_mlp_fwd(layers, X, M, out, ldo, col_off=0, keep=True, out_act=0):
    """MLP over a feature matrix X (M, ldx) -- ldx = the first layer's row pitch, pad columns zero -- instead of over positions: hidden layers
    through engine.gemm (bias + ReLU), the last layer into out[:, col_off:col_off + n_out] (+ row softmax when ``out_act`` is 2).
    Returns the hidden activations (for feat_mlp_bwd) or None."""
    h, acts = X, []
    for W, b in layers[:-1]:
        hn = torch.empty((M, W.shape[0]), dtype=torch.float32, device=X.device)
        gemm(M, W.shape[0], _pitch(W), h, h.shape[1], W, _pitch(W), hn, hn.shape[1], bias=b, act=1)
        acts.append(hn)
        h = hn
    Wo, bo = layers[-1]
    _out_layer(M, h, Wo, _pitch(Wo), bo, out, ldo, col_off, out_act)       # (K = the row pitch, as in the hidden layers)
    return acts if keep else None


def feat_mlp_bwd(layers, glayers, X, acts, dpre, M, keep=None):
    """Backward of feat_mlp_fwd: dpre (M, ld) = gradient w.r.t. the last layer's pre-activation output (ld % 4 == 0, pad zero); accumulates the
    weight / bias gradients and returns the gradient w.r.t. X (M, ldx)."""
    keep = keep if keep is not None else []
    d = dpre
    keep.append(d)
    for li in range(len(layers) - 1, -1, -1):
        W, b = layers[li]
        gW, gb = glayers[li]
        h = acts[li - 1] if li > 0 else X
        no, kin = W.shape[0], h.shape[1]
        wgrad(no, kin, M, d, d.shape[1], h, kin, gW, gb)
        dn = torch.empty((M, kin), dtype=torch.float32, device=X.device)
        if li > 0:
            gemm(M, kin, no, d, d.shape[1], W, _pitch(W), dn, kin, b_trans=1, mask=h, ldmask=kin)
        else:
            gemm(M, kin, no, d, d.shape[1], W, _pitch(W), dn, kin, b_trans=1)
        d = dn
        keep.append(d)
    return d


def grid_head_fwd(model, views, ctx, prefix, nets, keep, out_act=0):
    """A head whose MLP reads the 27 features of its own VM grid (compute_feature, tensoRF.py:127-134, on the semantic / instance tables) for
    the chunk's active samples: product gather (the appearance head's kernel: generic in the component count), basis Linear, then every net of
    ``nets`` = [(layers, out, ldo, col_off)] on the same features (the instance head's fast and slow MLPs).  Returns what the backward needs."""
    M, dev = ctx.M, ctx.rays.device
    with _grid_precision():
        vm = vm_struct(views, prefix, ctx.res)
        nc = 3 * vm.comps
        F = torch.empty((M, nc), dtype=torch.float32, device=dev)
        call("clift_app_gather_fwd", C.byref(ctx.ms), C.byref(vm), ptr(ctx.rays), ptr(ctx.jitter), ptr(ctx.act_idx), M, ptr(F), ptr(ctx.xa), stream())
        Wb = views[f"{prefix}_basis_mat.weight"]
        nf, ldf = Wb.shape[0], (Wb.shape[0] + 3) // 4 * 4
        feat = torch.zeros((M, ldf), dtype=torch.float32, device=dev)          # (pad columns stay zero: the first layer's K is its row pitch)
        with exact_fp32():
            gemm(M, nf, nc, F, nc, Wb, _pitch(Wb), feat, ldf)
        acts = [feat_mlp_fwd(layers, feat, M, out, ldo, col_off, keep, out_act) for layers, out, ldo, col_off in nets]
    return dict(prefix=prefix, F=F if keep else None, feat=feat if keep else None, acts=acts)


def grid_head_bwd(model, views, gviews, ctx, st, nets, keep):
    """Backward of grid_head_fwd.  ``nets`` = [(layers, glayers, acts, dpre)] for the nets that receive a gradient (their input gradients add up
    on the shared features); then the basis matrix's gradient, dF = dfeat Wb and the scatter into the head's tables."""
    M, dev, prefix = ctx.M, ctx.rays.device, st["prefix"]
    with _grid_precision():
        dfeat = None
        for layers, glayers, acts, dpre in nets:
            d = feat_mlp_bwd(layers, glayers, st["feat"], acts, dpre, M, keep)
            dfeat = d if dfeat is None else dfeat.add_(d)
        Wb, gWb = views[f"{prefix}_basis_mat.weight"], gviews[f"{prefix}_basis_mat.weight"]
        nf, nc = Wb.shape
        call("clift_wgrad_narrow", ptr(dfeat), dfeat.shape[1], nf, ptr(st["F"]), nc, nc, M, ptr(gWb), _pitch(gWb), None, 0, stream())
        dF = torch.empty((M, nc), dtype=torch.float32, device=dev)
        with exact_fp32():
            gemm(M, nc, nf, dfeat, dfeat.shape[1], Wb, _pitch(Wb), dF, nc, b_trans=1)
        model.xcd_workspace_for(prefix)
        vm = vm_struct(views, prefix, ctx.res)
        g = vm_grad_struct(model, gviews, prefix)
        call("clift_app_gather_bwd", C.byref(ctx.ms), C.byref(vm), C.byref(g), ptr(ctx.rays), ptr(ctx.jitter), ptr(ctx.act_idx), M, ptr(dF),
             ptr(ctx.xa) if APP_SCATTER_XA else None, stream())
        vm_grad_finish(model, gviews, prefix, g)
        keep.extend([dfeat, dF])


# ----------------------------------------------------------------------------- forward
class RenderCtx:
    """What a forward pass leaves for its backward (and for the trainer, the bench and the tools, which read M, N, capped, soak, ...).  Every
    attribute a pass may set is declared here; one that a pass did not reach keeps its default."""

    def __init__(self):
        self.ms = self.res = self.rays = self.jitter = None                     # the march (_density_march)
        self.sigma = self.alpha = self.T = self.w = self.ray_out = self.ray_start = self.act_idx = None
        self.N = self.S = self.M = 0
        self.capped = False                  # a sync-free chunk: M is the capacity, the row count stays on the device (ray_start[N])
        self.edited = False                  # sigma came from a caller's launch (the edit renders): xa may hold remapped positions
        self.edit_program = None             # the resolved edit.EditProgram of an edit pass (a single Edit: a program of one)
        self.white_bg = self.softmax_mode = self.stop_grad = self.C = self.D = 0
        self.want = (False, False, False)    # (colour, semantic, instance) outputs composited
        self.xa = None                       # (M, 4) positions of the active samples
        self.rgb_s = self.sem_s = self.inst_s = None         # per-sample head outputs
        self.rgb_raw = self.sem_raw = None                   # per-ray sums before background / normalisation
        self.w_feat = None                   # "argmax" weights: the one-hot array the semantic and instance sums were taken with
        self.F = self.feat = self.X = self.H1 = self.H2 = None                  # the appearance chain ("app" in grad_heads)
        self.ldf = self.nf = self.ldx = 0
        self.soak = None                     # SOAK_KEEP: references to the appearance chain's intermediates
        self.sem_acts = self.inst_fast_acts = self.inst_slow_acts = None        # hidden activations of the xyz heads
        self.sem_grid = self.inst_grid = None                                   # state of a head on its own grid (grid_head_fwd)
        self.slots = self.layer_add = None   # layers_forward: the slot of every list row; with use_delta the world positions added to the features
        self.M_render = 0                    # layers_forward: the length of the march's own list (w > threshold), which its alpha-list replaced
        self.base_slots = self.origin = self.state = None  # edit_layers_forward: the slots under the base table, and which copy a row's content came through
        self.layer_rgb = self.layer_rgb_row = self.layer_dirs = None       # colour layers: the colours (Mc, 3) of the coloured list rows, the row of each list row (M; -1: none), their view directions
        self.layer_xa = None                 # edit_layers_forward with colour: the xa that clift_edit_list_active wrote beside the directions


INT_MAX = 2 ** 31 - 1
_rows_limit = {}
_limit_owner = None          # the sync-free chunk whose row count the limit currently holds


def rows_limit(dev):
    """The library's dynamic row limit of this device: int32 [limit, overflow], bound once (clift_bind_rows_limit).  limit is INT_MAX
    (no effect) except inside a sync-free pass; ``reset_rows_limit`` restores that."""
    key = (dev.type, dev.index)
    t = _rows_limit.get(key)
    if t is None:
        t = torch.tensor([INT_MAX, 0], dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        call("clift_bind_rows_limit", ptr(t))
        _rows_limit[key] = t
    return t


_grad_shard_record = {}


def grad_shard_record(dev):
    """The library's gradient-shard record of this device (5 x int64: range start, bytes, shard 0, shard stride, enabled), bound once
    (clift_bind_grad_shards).  All zero -- disabled -- except inside a trainer pass (clift_grad_shards_begin ... clift_grad_shards_fold)."""
    key = (dev.type, dev.index)
    t = _grad_shard_record.get(key)
    if t is None:
        t = torch.zeros(5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        call("clift_bind_grad_shards", ptr(t))
        _grad_shard_record[key] = t
    return t


def reset_rows_limit(dev=None):
    """Back to 'no limit' (stream-ordered).  Called at the end of every sync-free pass, and defensively by the point-wise utilities."""
    global _limit_owner
    _limit_owner = None
    for key, t in _rows_limit.items():
        if dev is None or key == (dev.type, dev.index):
            t[0:1].fill_(INT_MAX)


def _density_march(model, renderer, rays, jitter, cap=None, density_fwd=None, weight_thres=None):
    """The march prologue of every pass: densities, weights, the list of the active samples (w > threshold) and the context that holds them.
    ``density_fwd``: called as density_fwd(ms, vd, sigma) to launch what fills sigma, in place of clift_density_fwd (the edit renders);
    ``weight_thres``: in place of renderer.raymarch_weight_thres."""
    views = model.named_views()
    N = rays.shape[0]
    S = int(renderer.n_samples)
    dev = rays.device
    ms = march_struct(renderer, model)
    thres = float(renderer.raymarch_weight_thres if weight_thres is None else weight_thres)
    ms.weight_thres = thres                 # the march counts, clift_compact_fill lists: the same threshold
    res = grid_res(views)
    vd = vm_struct(views, "density", res)
    sigma = torch.empty((N, S), dtype=torch.float32, device=dev)
    alpha, T, w = torch.empty_like(sigma), torch.empty_like(sigma), torch.empty_like(sigma)
    ray_out = torch.empty((N, 8), dtype=torch.float32, device=dev)
    n_active = torch.empty((N,), dtype=torch.int32, device=dev)
    st = stream()
    if density_fwd is None:
        call("clift_density_fwd", C.byref(ms), C.byref(vd), ptr(rays), ptr(jitter), N, ptr(sigma), st)
    else:
        density_fwd(ms, vd, sigma)
    call("clift_march_fwd", C.byref(ms), ptr(rays), ptr(jitter), N, ptr(sigma), ptr(alpha), ptr(T), ptr(w), ptr(ray_out),
         ptr(n_active), st)
    ray_start = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    if cap is None:
        # a synchronising chunk inside a sync-free pass (a pass still learning its capacity, e.g. the segment term whose ray count
        # changes every step): the library-wide row limit may still hold the PREVIOUS capped chunk's count, which would silently clamp
        # every per-sample kernel of this chunk -- put "no limit" back first (stream-ordered)
        global _limit_owner
        lim_t = _rows_limit.get((dev.type, dev.index))
        if lim_t is not None and _limit_owner is not None:
            lim_t[0:1].fill_(INT_MAX)
            _limit_owner = None
        call("clift_scan_counts", ptr(n_active), N, ptr(ray_start), st)
        M = int(ray_start[N].item())        # the one host sync of the chunk: sizes the active-sample buffers
        act_idx = torch.empty((max(M, 1),), dtype=torch.int32, device=dev)
        call("clift_compact_fill", ptr(w), ptr(ray_start), N, S, thres, ptr(act_idx), st)
    else:
        # sync-free: buffers and grids are sized by the capacity, the true count stays on the device (rows_limit()[0]) where every
        # per-sample kernel clamps to it; an overflow (count > cap: samples dropped) is recorded in rows_limit()[1] for the caller
        if MLP_PRECISION == 1:
            raise _lib.CliftError("sync-free steps (cap=...) are built for the fp32 / fp32x6 paths only")
        lim = rows_limit(dev)
        M = max(int(cap), 1)
        call("clift_scan_counts_capped", ptr(n_active), N, ptr(ray_start), M, ptr(lim), C.c_void_p(lim.data_ptr() + 4), st)
        act_idx = torch.empty((M,), dtype=torch.int32, device=dev)
        call("clift_compact_fill_capped", ptr(w), ptr(ray_start), N, S, thres, ptr(act_idx), M, st)
    ctx = RenderCtx()
    ctx.ms, ctx.res, ctx.N, ctx.S, ctx.M = ms, res, N, S, M
    ctx.capped = cap is not None
    ctx.edited = density_fwd is not None
    if ctx.capped:
        _limit_owner = ctx
    ctx.rays, ctx.jitter = rays, jitter
    ctx.alpha, ctx.T, ctx.w, ctx.ray_out, ctx.ray_start, ctx.act_idx = alpha, T, w, ray_out, ray_start, act_idx
    ctx.sigma = sigma
    return ctx


def _check_rays(rays, jitter):
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"rays must be (N,8) [o,d,near,far], got {tuple(rays.shape)}")
    _lib.f32(rays, "rays")
    rays = rays.contiguous()
    if jitter is not None:
        jitter = _lib.f32(jitter, "jitter").reshape(-1).contiguous()
        if jitter.shape[0] != rays.shape[0]:
            raise ValueError("jitter must have one entry per ray")
    return rays, jitter


_HEAD_MLPS = {"app": "render_appearance_mlp.mlp", "sem": "render_semantic_mlp.mlp", "fast": "render_instance_mlp.mlp",
              "slow": "render_instance_mlp.slow_mlp"}


def _head_params(views):
    """{head: [(W, b)]} of the appearance, semantic, fast- and slow-instance MLPs (empty where the field has none), fetched once per pass from
    the parameter views -- and, by the backward, from the gradient views."""
    return {head: _lin_params(prefix, views) for head, prefix in _HEAD_MLPS.items()}


def _head_chains(model, views, ctx, params, grad_heads, want_sem):
    """The forward of the semantic head (``want_sem``) and of the instance head (ctx.D > 0) over the chunk's active samples, as
    [(Branches slot, chain)]: the heads are independent of each other and of the appearance chain.  xyz MLPs or heads on their own VM grids;
    the instance head's fast and slow nets write the two halves of ctx.inst_s.  A head named in ``grad_heads`` keeps its activations."""
    M, dev, D = ctx.M, ctx.rays.device, ctx.D
    chains = []
    if want_sem:
        def sem_chain(keep):
            Ccls = ctx.C
            sem_s = torch.empty((M, Ccls), dtype=torch.float32, device=dev)
            sm = 2 if model.render_semantic_mlp.softmax else 0
            if model.semantic_plane is not None:           # the head on its own VM grid
                ctx.sem_grid = grid_head_fwd(model, views, ctx, "semantic", [(params["sem"], sem_s, Ccls, 0)], "sem" in grad_heads, sm)
            else:
                ctx.sem_acts = xyz_mlp_fwd(params["sem"], ctx.xa, M, sem_s, Ccls, keep_first="sem" in grad_heads, out_act=sm)
            ctx.sem_s = sem_s
        chains.append((1, sem_chain))
    if D > 0:
        E = model.render_instance_mlp.output_channels
        ctx.inst_s = torch.empty((M, D), dtype=torch.float32, device=dev)
        if model.instance_plane is not None:           # the head on its own VM grid: fast and slow nets read the same features
            nets = [(params["fast"], ctx.inst_s, D, 0)] + ([(params["slow"], ctx.inst_s, D, E)] if model.slow_fast_mode else [])

            def inst_grid_chain(keep):
                ctx.inst_grid = grid_head_fwd(model, views, ctx, "instance", nets, "fast" in grad_heads or "slow" in grad_heads)
            chains.append((2, inst_grid_chain))
        else:
            def fast_chain(keep):
                ctx.inst_fast_acts = xyz_mlp_fwd(params["fast"], ctx.xa, M, ctx.inst_s, D, 0, keep_first="fast" in grad_heads)

            def slow_chain(keep):
                ctx.inst_slow_acts = xyz_mlp_fwd(params["slow"], ctx.xa, M, ctx.inst_s, D, E, keep_first="slow" in grad_heads)
            chains.append((2, fast_chain))
            if model.slow_fast_mode:
                chains.append((3, slow_chain))
    return chains


def _composite_sides(ctx, colour, feats):
    """What a compositing launch takes of the pass when the colour sums (``colour``) and / or the semantic and instance sums (``feats``) take part:
    pointer selectors for the tensors of either side, the class and instance-feature counts, softmax_mode and white_bg."""
    return ((lambda t: ptr(t) if colour else None), (lambda t: ptr(t) if feats else None), ctx.C if (feats and ctx.want[1]) else 0,
            ctx.D if feats else 0, ctx.softmax_mode if feats else 0, ctx.white_bg if colour else 0)


def _composite_fwd(ctx, w, out, colour=True, feats=True):
    """One clift_composite_fwd launch over the weight array ``w`` (None: a chunk without active samples, backgrounds and zeros only) into
    out = (rgb_raw, rgb_map, sem_raw, sem_map, inst_map)."""
    rgb_raw, rgb_map, sem_raw, sem_map, inst_map = out
    c, f, n_sem, D, softmax_mode, white_bg = _composite_sides(ctx, colour, feats)
    call("clift_composite_fwd", ptr(w), ptr(ctx.ray_start), ptr(ctx.act_idx), ctx.N, n_sem, D, c(ctx.rgb_s), f(ctx.sem_s), f(ctx.inst_s), ptr(ctx.ray_out),
         softmax_mode, white_bg, c(rgb_raw), c(rgb_map), f(sem_raw), f(sem_map), f(inst_map), stream())


def _composite_outputs(ctx, argmax, want_rgb=True, want_sem=True):
    """The per-ray outputs of a pass -- colours (``want_rgb``), semantics (``want_sem``), instance features (ctx.D > 0) -- and the compositing
    launch(es) that fill them (``argmax``: semantic_weight_mode "argmax").  Leaves the raw sums in the context; returns (rgb, sem, inst) maps."""
    N, M, Ccls, D, dev = ctx.N, ctx.M, ctx.C, ctx.D, ctx.rays.device
    # (the sum kernel writes every (ray, channel) when there are heads to sum; only a chunk without active samples needs the zeros)
    fresh = torch.empty if M > 0 else torch.zeros
    rgb_raw = fresh((N, 3), dtype=torch.float32, device=dev) if want_rgb else None
    rgb_map = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_rgb else None
    sem_raw = fresh((N, Ccls), dtype=torch.float32, device=dev) if want_sem else None
    sem_map = torch.empty((N, Ccls), dtype=torch.float32, device=dev) if want_sem else None
    inst_map = fresh((N, D), dtype=torch.float32, device=dev) if D > 0 else None
    out = (rgb_raw, rgb_map, sem_raw, sem_map, inst_map)
    if M > 0 and argmax and (want_sem or D > 0):
        # renderer.py:142-143: the semantic / instance sums take the one-hot of each ray's heaviest sample (of ALL its samples: a heaviest
        # sample below the threshold is not in the list and the ray's sums stay 0, as in the reference, whose heads are 0 there); the colours
        # keep the weights -- two passes of the compositing kernels, one per weight array
        ctx.w_feat = torch.zeros_like(ctx.w).scatter_(1, ctx.w.argmax(dim=1, keepdim=True), 1.0)
        if want_rgb:
            _composite_fwd(ctx, ctx.w, out, feats=False)
        _composite_fwd(ctx, ctx.w_feat, out, colour=False)
    else:   # (no active sample in the chunk -- reference: the `if appearance_mask.any()` branch is skipped -- no weights and no head outputs)
        _composite_fwd(ctx, ctx.w if M > 0 else None, out)
    ctx.rgb_raw, ctx.sem_raw = rgb_raw, sem_raw
    return rgb_map, sem_map, inst_map


def _app_tail(M, H1, W2, b2, W3, b3, hdt, rgb_s):
    """The last two appearance layers as their own launches: H2 = relu(H1 W2^T + b2) stored as ``hdt``, pre = H2 W3^T + b3,
    rgb_s = sigmoid(pre).  Returns (H2, pre)."""
    H2 = torch.empty((M, W2.shape[0]), dtype=hdt, device=H1.device)
    gemm(M, W2.shape[0], W2.shape[1], H1, H1.shape[1], W2, _pitch(W2), H2, H2.shape[1], bias=b2, act=1)
    pre = torch.empty((M, 3), dtype=torch.float32, device=H1.device)
    gemm(M, 3, W3.shape[1], H2, H2.shape[1], W3, _pitch(W3), pre, 3, bias=b3)
    call("clift_rows_act_fwd", ptr(pre), 3, M, 3, 1, ptr(rgb_s), 3, stream())
    return H2, pre


def app_tail_route(layers, M, hdt):
    """The launch that takes the last two appearance layers and the sigmoid together, inside _app_precision(): "last2" | "last2_x6" |
    "last2_bf16" (over the bf16-stored activation, csrc/layer_nb16.hip), or None: _app_tail's three launches.  Pure, like xyz_head_route."""
    W2, W3 = layers[1][0], layers[2][0]
    if not (tuple(W2.shape) == (128, 128) and W3.shape[0] <= 4 and W3.shape[1] == 128 and persistent_ok()):
        return None
    if MLP_PRECISION in (0, 2) and hdt == torch.float32:
        return "last2_x6" if MLP_PRECISION == 2 and persistent_x6_ok() else "last2"       # (x6: only inside _app_precision() with APP_X6)
    return "last2_bf16" if MLP_PRECISION == 1 and hdt == torch.bfloat16 and M >= 64 else None


def _app_layers(M, X, layers, hdt, keep_h2, keep):
    """The appearance MLP over its encoded input rows X (M, the first layer's row pitch), inside _app_precision(): H1 = relu(X W1^T + b1) stored as ``hdt``, then the
    last two layers fused where a kernel exists -- H2 is written only for a backward (``keep_h2``) -- else _app_tail (H2 written, ``keep``
    receives the pre-activation colours).  Returns (H1, H2, rgb_s)."""
    (W1, b1), (W2, b2), (W3, b3) = layers
    dev, ldx = X.device, _pitch(W1)
    H1 = torch.empty((M, W1.shape[0]), dtype=hdt, device=dev)
    gemm(M, W1.shape[0], ldx, X, ldx, W1, ldx, H1, H1.shape[1], bias=b1, act=1)
    rgb_s = torch.empty((M, 3), dtype=torch.float32, device=dev)
    tail = app_tail_route(layers, M, hdt)
    if tail is None:
        H2, pre = _app_tail(M, H1, W2, b2, W3, b3, hdt, rgb_s)
        keep.append(pre)
        return H1, H2, rgb_s
    H2 = torch.empty((M, 128), dtype=hdt, device=dev) if keep_h2 else None
    if tail == "last2":
        app_last2(M, H1, W2, b2, W3, b3, H2, rgb_s)
    else:
        call("clift_app_head_last2_x6_fwd" if tail == "last2_x6" else "clift_app_head_last2_bf16_fwd", ptr(H1), 128, ptr(W2), _pitch(W2), ptr(b2),
             ptr(W3), _pitch(W3), ptr(b3), W3.shape[0], M, ptr(H2), 128, ptr(rgb_s), 3, 1, stream())
    return H1, H2, rgb_s


def _app_out_bwd_route(M, W3, gW3, H2, dpre):
    """The launch that takes the appearance output layer's weight gradient and masked input gradient in one pass over the hidden activation (as in
    the xyz heads): "nh", "n128_bf16" (bf16 mode: over the bf16-stored activation, the input gradient leaves bf16-stored), or None: two passes."""
    n2 = W3.shape[1]
    if not (APP_OUT_BWD_FUSED and W3.shape[0] <= 4 and _pitch(W3) >= n2 and _pitch(gW3) >= n2 and persistent_ok()):
        return None
    if H2.dtype == torch.float32 and n2 % 32 == 0 and n2 <= 256 and M >= 4096:
        return "nh"
    return "n128_bf16" if MLP_PRECISION == 1 and H2.dtype == torch.bfloat16 and n2 == 128 and dpre.shape[1] == 4 else None


def _app_backward(model, views, gviews, ctx, layers, glayers, dpre, keep):
    """Backward of render_forward's appearance chain from ``dpre`` (M, 4), the gradient w.r.t. the pre-sigmoid colours: the three layers, the
    input encoding, the basis matrix and the scatter into the appearance tables.  ``keep`` receives every temporary."""
    M, dev = ctx.M, ctx.rays.device
    with _app_precision():
        (W1, b1), (W2, b2), (W3, b3) = layers
        (gW1, gb1), (gW2, gb2), (gW3, gb3) = glayers
        H1, H2, X, ldx = ctx.H1, ctx.H2, ctx.X, ctx.ldx
        n2 = W3.shape[1]
        dH2 = torch.empty((M, n2), dtype=H2.dtype, device=dev)
        how = _app_out_bwd_route(M, W3, gW3, H2, dpre)
        if how == "nh":
            call("clift_out_layer_bwd_nh", ptr(dpre), 4, W3.shape[0], ptr(W3), _pitch(W3), ptr(H2), n2, n2, M, ptr(dH2), n2, ptr(gW3), _pitch(gW3),
                 ptr(gb3), 0, stream())
        elif how == "n128_bf16":
            call("clift_out_layer_bwd_n128_bf16", ptr(dpre), 4, W3.shape[0], ptr(W3), _pitch(W3), ptr(H2), 128, M, ptr(dH2), 128, ptr(gW3), _pitch(gW3),
                 ptr(gb3), stream())
        else:
            wgrad(3, n2, M, dpre, 4, H2, n2, gW3, gb3)
            gemm(M, n2, 3, dpre, 4, W3, _pitch(W3), dH2, n2, b_trans=1, mask=H2, ldmask=n2)
        n1 = W2.shape[1]
        wgrad(n2, n1, M, dH2, n2, H1, n1, gW2, gb2)
        dH1 = torch.empty((M, n1), dtype=H1.dtype, device=dev)
        gemm(M, n1, n2, dH2, n2, W2, _pitch(W2), dH1, n1, b_trans=1, mask=H1, ldmask=n1)
        wgrad(n1, ldx, M, dH1, n1, X, ldx, gW1, gb1)
        dX = torch.empty((M, ldx), dtype=torch.float32, device=dev)
        gemm(M, ldx, n1, dH1, n1, W1, ldx, dX, ldx, b_trans=1)
        nf, ldf = ctx.nf, ctx.ldf
        Wb, gWb = views["appearance_basis_mat.weight"], gviews["appearance_basis_mat.weight"]
        nc = Wb.shape[1]
        va = vm_struct(views, "appearance", ctx.res)
        ga = vm_grad_struct(model, gviews, "appearance")
        dfeat = torch.empty((M, ldf), dtype=torch.float32, device=dev)
        call("clift_app_encode_bwd", ptr(ctx.feat), ldf, nf, model.pe_feat, ptr(dX), ldx, M, ptr(dfeat), ldf, stream())
        call("clift_wgrad_narrow", ptr(dfeat), ldf, nf, ptr(ctx.F), nc, nc, M, ptr(gWb), _pitch(gWb), None, 0, stream())
        dF = torch.empty((M, nc), dtype=torch.float32, device=dev)
        with exact_fp32():              # (the basis Linear is not one of the bf16 layers in any mode)
            gemm(M, nc, nf, dfeat, ldf, Wb, _pitch(Wb), dF, nc, b_trans=1)
        call("clift_app_gather_bwd", C.byref(ctx.ms), C.byref(va), C.byref(ga), ptr(ctx.rays), ptr(ctx.jitter),
             ptr(ctx.act_idx), M, ptr(dF), ptr(ctx.xa) if APP_SCATTER_XA else None, stream())
        vm_grad_finish(model, gviews, "appearance", ga)
        keep.extend([dpre, dH2, dH1, dX, dfeat, dF])


def render_forward(model, renderer, rays, jitter, white_bg, want_rgb=True, want_sem=True, want_inst=True, grad_heads=("app", "sem", "fast", "slow"),
                   cap=None, want_dist=True):
    """Full renderer.forward (reference renderer.py:80-176).  Returns dict of outputs and the backward context.
    ``grad_heads``: the heads a backward pass may be run through ("app", "sem", "fast", "slow"); a head that is not named retains
    no activations (the training main pass never differentiates the instance heads, T:155; inference none)."""
    rays, jitter = _check_rays(rays, jitter)
    views = model.named_views()
    ctx = _density_march(model, renderer, rays, jitter, cap)
    S, M, dev, st = ctx.S, ctx.M, rays.device, stream()
    Ccls = model.num_semantic_classes
    D = model.dim_feature_instance if (want_inst and model.render_instance_mlp is not None) else 0
    ctx.softmax_mode = 1 if renderer.semantic_weight_mode == "softmax" else 0
    ctx.white_bg, ctx.stop_grad = int(bool(white_bg)), int(bool(renderer.stop_semantic_grad))
    ctx.C, ctx.D = Ccls, D
    ctx.want = (want_rgb, want_sem, D > 0)
    if M > 0:
        params = _head_params(views)
        xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
        ctx.xa = xa
        front = None
        if want_rgb:       # the gather also produces xa, which every other head reads: it stays on the main stream
            va = vm_struct(views, "appearance", ctx.res)
            nc = 3 * va.comps
            Wb = views["appearance_basis_mat.weight"]
            W1 = views["render_appearance_mlp.mlp.0.weight"]
            nf, ldx = Wb.shape[0], _pitch(W1)
            if (APP_FRONT_FUSED and nf <= 28 and va.comps in (16, 32, 48) and Wb.shape[1] == nc and _pitch(Wb) % 4 == 0 and ldx % 4 == 0 and ldx <= 512
                    and persistent_ok()):
                # the appearance front end as one launch: gather -> basis -> MLP input rows (the products are written only for a backward)
                ldf = 28
                F = torch.empty((M, nc), dtype=torch.float32, device=dev) if "app" in grad_heads else None
                feat = torch.empty((M, ldf), dtype=torch.float32, device=dev)
                with _app_precision():              # bf16 mode: the MLP's input rows leave the front end bf16-stored
                    x_bf16 = MLP_PRECISION == 1 and ldx % 8 == 0
                X = torch.empty((M, ldx), dtype=torch.bfloat16 if x_bf16 else torch.float32, device=dev)
                call("clift_app_front_fwd_x", C.byref(ctx.ms), C.byref(va), ptr(rays), ptr(jitter), ptr(ctx.act_idx), M, ptr(Wb), _pitch(Wb), nf,
                     model.pe_feat, model.pe_view, ptr(xa), ptr(feat), ldf, ptr(X), ldx, ptr(F), int(x_bf16), st)
                front = (feat, ldf, X)
            else:
                F = torch.empty((M, nc), dtype=torch.float32, device=dev)
                call("clift_app_gather_fwd", C.byref(ctx.ms), C.byref(va), ptr(rays), ptr(jitter), ptr(ctx.act_idx), M, ptr(F), ptr(xa), st)
            ctx.F = F
        else:
            call("clift_active_xyz", C.byref(ctx.ms), ptr(rays), ptr(jitter), ptr(ctx.act_idx), M, ptr(xa), st)

        def app_chain(keep):
            with _app_precision():
                Wb = views["appearance_basis_mat.weight"]
                nf, nc = Wb.shape
                ldx = _pitch(params["app"][0][0])
                hdt = act_dtype() if ldx % 8 == 0 else torch.float32      # bf16 mode: encoded input and hidden activations bf16-stored
                if front is not None:
                    feat, ldf, X = front
                else:
                    ldf = (nf + 3) // 4 * 4
                    feat = torch.empty((M, ldf), dtype=torch.float32, device=dev)
                    with exact_fp32():          # (the basis Linear is not one of the bf16 layers in any mode)
                        gemm(M, nf, nc, ctx.F, nc, Wb, _pitch(Wb), feat, ldf)
                    X = torch.empty((M, ldx), dtype=hdt, device=dev)
                    call("clift_app_encode_fwd", ptr(feat), ldf, nf, model.pe_feat, model.pe_view, ptr(rays), ptr(ctx.act_idx), S, M,
                         ptr(X), ldx, int(hdt == torch.bfloat16), stream())
                H1, H2, ctx.rgb_s = _app_layers(M, X, params["app"], hdt, "app" in grad_heads, keep)
                if SOAK_KEEP:
                    ctx.soak = dict(feat=feat, X=X, H1=H1)
                if "app" in grad_heads:
                    ctx.feat, ctx.ldf, ctx.nf, ctx.X, ctx.ldx, ctx.H1, ctx.H2 = feat, ldf, nf, X, ldx, H1, H2
                else:
                    ctx.F = None

        br = Branches(model=model)
        if want_rgb:
            br.run(0, app_chain)
        for slot, chain in _head_chains(model, views, ctx, params, grad_heads, want_sem):
            br.run(slot, chain)
        br.join()
    rgb_map, sem_map, inst_map = _composite_outputs(ctx, renderer.semantic_weight_mode == "argmax", want_rgb, want_sem)
    out = dict(rgb=rgb_map, semantics=sem_map, instances=inst_map, depth=ctx.ray_out[:, 1],
               dist_reg=ctx.ray_out[:, 5].mean() if want_dist else None, opacity=ctx.ray_out[:, 0])     # (the trainer never reads the VALUE of the regulariser)
    return out, ctx


# ----------------------------------------------------------------------------- scene-editing forward
def _refuse_shaped(who, prog):
    """The passes that read ``prog.records()`` alone would silently drop the shapes of a shaped program (edit.EditShape)."""
    if prog.is_shaped:
        raise NotImplementedError(f"{who}: a shaped edit program (an edit with an EditShape) is not supported here: this pass walks the boxes "
                                  "alone and would drop the shapes; render it with edit_forward, mesh it through get_dense_sigma(edit=)")


def _edit_density_march(model, renderer, rays, edit, weight_thres):
    """The march of an edit pass.  The program (``as_program``) says which entry points take it (``EditProgram.launch_family``): the
    list family, or the shaped one when an edit follows a shape (``edit.EditShape``).  One exception is kept here: a single ``Edit``
    without a shape goes through clift_edit_density_fwd / clift_edit_active, the single-edit names.

    Returns (context, kernel-name pattern, leading edit arguments of that family).  The context keeps the resolved program
    (``edit_program``; a single edit as a program of one, whose list walk is that edit op for op)."""
    N, st = rays.shape[0], stream()
    prog = _edit.as_program(edit)
    if isinstance(edit, _edit.Edit) and edit.shape is None:
        edit_kernel, edit_args = "clift_edit_%s", (C.byref(edit.record()),)
    else:
        edit_kernel, edit_args = prog.launch_family(rays.device)

    def density_fwd(ms, vd, sigma):
        call(edit_kernel % "density_fwd", C.byref(ms), *edit_args, C.byref(vd), ptr(rays), N, ptr(sigma), st)

    ctx = _density_march(model, renderer, rays, None, density_fwd=density_fwd, weight_thres=weight_thres)
    ctx.edit_program = prog
    return ctx, edit_kernel, edit_args


def _app_points_chain(model, views, params, F, dirs, ldd, M, keep):
    """The point-wise appearance chain behind clift_vm_products_points: from the products ``F`` (M, 3 comps) and one view direction per row
    (``dirs``, row pitch ``ldd`` >= 3) the un-fused front end (the fused one recomputes positions from the rays) -- the basis Linear in exact
    fp32, clift_app_encode_points --, then render_forward's appearance layers with fp32-stored activations.  -> rgb_s (M, 3).  ``keep``
    receives every temporary (the caller may be on a side stream)."""
    dev = F.device
    with _app_precision():
        Wb = views["appearance_basis_mat.weight"]
        nf, nc = Wb.shape[0], F.shape[1]
        ldx, ldf = _pitch(params["app"][0][0]), (nf + 3) // 4 * 4
        feat = torch.empty((M, ldf), dtype=torch.float32, device=dev)
        with exact_fp32():
            gemm(M, nf, nc, F, nc, Wb, _pitch(Wb), feat, ldf)
        X = torch.empty((M, ldx), dtype=torch.float32, device=dev)
        call("clift_app_encode_points", ptr(feat), ldf, nf, model.pe_feat, model.pe_view, ptr(dirs), ldd, M, ptr(X), ldx, stream())
        H1, H2, rgb_s = _app_layers(M, X, params["app"], torch.float32, False, keep)
        keep.extend([feat, X, H1, H2, F, dirs])
    return rgb_s


@torch.no_grad()
def edit_forward(model, renderer, rays, edit, white_bg, weight_thres=0.0):
    """The reference's edit renders (renderer.py:303-623: forward_delete / _extract / _duplicate / _manipulate) for one resolved edit
    (``edit.Edit``): samples the kill rule names get sigma = 0, samples inside the destination box are looked up at the remapped position
    with the turned view direction.

    ``edit`` may also be an ``edit.EditProgram`` (or a sequence of ``Edit``): its edits are applied in order in this one render.  Every
    sample walks the list backwards (``EditProgram``) in the density_fwd / active entry points of the program's family
    (``_edit_density_march``), which take the place of the two single-edit launches; a single ``Edit`` without a shape keeps those.

    No jitter (the reference samples with perturb 0, is_train False), no activations kept, no backward, no distortion-loss value.
    Returns (dict of outputs, context) like ``render_forward``.

      edit_density_fwd -> march_fwd -> scan / compact at ``weight_thres`` -> edit_active (xa, dirs) ->
      vm_products_points -> basis GEMM -> app_encode_points -> appearance layers;  xyz heads on xa;  composite.

    ``weight_thres`` defaults to 0, not to ``renderer.raymarch_weight_thres``: the reference's edit forwards evaluate every head at every
    in-box sample instead of only where w > 1e-4, and a sample with w == 0 adds nothing to any sum, so "w > 0" reproduces them exactly.
    Pass the renderer's threshold to trade that for fewer active samples."""
    rays, _ = _check_rays(rays, None)
    if model.semantic_plane is not None or model.instance_plane is not None:
        raise NotImplementedError("edit_forward: a semantic / instance head on its own VM grid is not supported (xyz MLP heads only)")
    views = model.named_views()
    N, dev, st = rays.shape[0], rays.device, stream()
    ctx, edit_kernel, edit_args = _edit_density_march(model, renderer, rays, edit, weight_thres)
    ms, M = ctx.ms, ctx.M
    Ccls = model.num_semantic_classes
    D = model.dim_feature_instance if model.render_instance_mlp is not None else 0
    ctx.softmax_mode = 1 if renderer.semantic_weight_mode == "softmax" else 0
    ctx.white_bg, ctx.stop_grad = int(bool(white_bg)), int(bool(renderer.stop_semantic_grad))
    ctx.C, ctx.D, ctx.want = Ccls, D, (True, True, D > 0)
    if M > 0:
        params = _head_params(views)
        ctx.xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
        dirs = torch.empty((M, 4), dtype=torch.float32, device=dev)
        call(edit_kernel % "active", C.byref(ms), *edit_args, ptr(rays), ptr(ctx.act_idx), M, ptr(ctx.xa), ptr(dirs), st)
        va = vm_struct(views, "appearance", ctx.res)
        nc = 3 * va.comps
        F = torch.empty((M, nc), dtype=torch.float32, device=dev)
        call("clift_vm_products_points", C.byref(va), ptr(ctx.xa), 4, M, ptr(F), st)

        def app_chain(keep):
            ctx.rgb_s = _app_points_chain(model, views, params, F, dirs, 4, M, keep)

        br = Branches(model=model)
        br.run(0, app_chain)
        for slot, chain in _head_chains(model, views, ctx, params, (), True):
            br.run(slot, chain)
        br.join()
    rgb_map, sem_map, inst_map = _composite_outputs(ctx, renderer.semantic_weight_mode == "argmax")
    return dict(rgb=rgb_map, semantics=sem_map, instances=inst_map, depth=ctx.ray_out[:, 1], opacity=ctx.ray_out[:, 0]), ctx


# ----------------------------------------------------------------------------- backward
def _composite_bwd(ctx, w, grads, rows, colour=True, feats=True, wgrad=True):
    """One clift_composite_bwd launch over the weight array ``w``: per-sample gradients w.r.t. the heads' ACTIVATED outputs into
    rows = (d_rgb, d_sem, d_inst) and -- ``wgrad`` -- the weight and opacity gradients.  grads = (g_rgb, g_sem, g_inst, ge (scratch), g_w, g_op)."""
    (g_rgb, g_sem, g_inst, ge, g_w, g_op), (d_rgb, d_sem, d_inst) = grads, rows
    c, f, n_sem, D, softmax_mode, white_bg = _composite_sides(ctx, colour, feats)
    call("clift_composite_bwd", ptr(w), ptr(ctx.ray_start), ptr(ctx.act_idx), ctx.N, ctx.S, ctx.M, n_sem, D, c(ctx.rgb_s), f(ctx.sem_s), f(ctx.inst_s),
         c(ctx.rgb_raw), f(ctx.sem_raw), softmax_mode, white_bg, ctx.stop_grad if (feats and wgrad) else 1, c(g_rgb), f(g_sem), f(g_inst), ptr(ge),
         c(d_rgb), f(d_sem), f(d_inst), ptr(g_w) if wgrad else None, ptr(g_op) if wgrad else None, stream())


def _composite_bwd_act(ctx, w, grads, rows, sem_kind, E_inst, colour=True, feats=True, wgrad=True):
    """One clift_composite_bwd_act launch: _composite_bwd with the heads' output activations (sigmoid / ``sem_kind`` / identity) taken back in the
    same kernel.  rows = (d_rgb (M, 4), d_sem, d_inst, d_inst_slow): the zero-padded PRE-activation gradient rows the heads' backward kernels
    start from; the instance row splits into the fast and the slow net's (``E_inst`` columns each; d_inst_slow None: not wanted)."""
    (g_rgb, g_sem, g_inst, ge, g_w, g_op), (d_rgb, d_sem, d_inst, d_inst_slow) = grads, rows
    c, f, n_sem, D, softmax_mode, white_bg = _composite_sides(ctx, colour, feats)
    ldp_sem, ldp_inst = ((ctx.C + 3) // 4 * 4, (E_inst + 3) // 4 * 4) if feats else (4, 4)
    call("clift_composite_bwd_act", ptr(w), ptr(ctx.act_idx), ctx.N, ctx.S, ctx.M, n_sem, D, c(ctx.rgb_s), f(ctx.sem_s), f(ctx.inst_s),
         c(ctx.rgb_raw), f(ctx.sem_raw), softmax_mode, white_bg, ctx.stop_grad if (feats and wgrad) else 1, c(g_rgb), f(g_sem), f(g_inst), ptr(ge),
         sem_kind if feats else 0, c(d_rgb), 4, f(d_sem), ldp_sem, f(d_inst), f(d_inst_slow), ldp_inst, E_inst if feats else 0,
         ptr(g_w) if wgrad else None, ptr(g_op) if wgrad else None, stream())


def _head_dpre(fused_row, y, d, off, n, kind, M):
    """d loss / d pre-activation output of a head, (M, n padded to a multiple of 4): ``fused_row`` where the compositing backward has already
    taken the activation back (act_fused), else one clift_rows_act_bwd launch (``kind`` 0 identity / 1 sigmoid / 2 row softmax) over columns
    [off, off + n) of the gradient ``d`` w.r.t. the activated output ``y`` (None for the identity)."""
    if fused_row is not None:
        return fused_row
    ldp = (n + 3) // 4 * 4
    dpre = torch.empty((M, ldp), dtype=torch.float32, device=d.device)
    call("clift_rows_act_bwd", ptr(y), y.shape[1] if y is not None else 0, C.c_void_p(d.data_ptr() + 4 * off), d.shape[1], M, n, kind, ptr(dpre), ldp,
         stream())
    return dpre


def _kept_grid_head(st):
    if st["F"] is None:
        raise _lib.CliftError("backward through a grid head whose forward ran without keeping its activations (head not named in grad_heads)")
    return st


def render_backward(model, ctx, gviews, g_rgb=None, g_sem=None, g_inst=None, g_dist=None, density_grad=True,
                    slow_grad=False, before_density=None):
    """Accumulate parameter gradients into ``gviews`` (name -> tensor with the parameter's layout).
    g_rgb (N,3), g_sem (N,C), g_inst (N,D): output gradients or None; g_dist: device scalar tensor or None.
    ``before_density``: called once, after every head chain (MLPs, appearance tables) has been issued on the current stream and before
    the density backward -- the data-parallel trainer starts the all-reduce of those gradients there, under the density backward."""
    views = model.named_views()
    N, S, M = ctx.N, ctx.S, ctx.M
    dev = ctx.rays.device
    global _limit_owner
    if ctx.capped:
        if _limit_owner is not ctx:        # another chunk was marched since: put THIS chunk's row count back (device-to-device, 4 bytes)
            rows_limit(dev)[0:1].copy_(ctx.ray_start[N:N + 1])
            _limit_owner = ctx
    elif _limit_owner is not None:         # a synchronising chunk's backward behind a sync-free chunk: its rows are not to be clamped
        reset_rows_limit(dev)
    Ccls, D = ctx.C, ctx.D
    want_rgb, want_sem, want_inst = ctx.want
    g_rgb = g_rgb.contiguous() if (g_rgb is not None and want_rgb) else None
    g_sem = g_sem.contiguous() if (g_sem is not None and want_sem) else None
    g_inst = g_inst.contiguous() if (g_inst is not None and want_inst) else None
    if density_grad:
        # d loss / d weight (N, S) and d loss / d opacity (N): zero except at the active samples -- one fill for both
        gbuf = torch.zeros((N * S + N,), dtype=torch.float32, device=dev)
        g_w, g_op = gbuf[:N * S].view(N, S), gbuf[N * S:]
    else:       # (feature passes: the weights carry no gradient, nobody reads these)
        g_w = torch.empty((N, S), dtype=torch.float32, device=dev)
        g_op = torch.empty((N,), dtype=torch.float32, device=dev)
    if M > 0 and (g_rgb is not None or g_sem is not None or g_inst is not None):
        params, gparams = _head_params(views), _head_params(gviews)
        slow_grad = bool(slow_grad and model.slow_fast_mode)
        E_inst = model.render_instance_mlp.output_channels if (D > 0 and model.render_instance_mlp is not None) else 0
        sem_kind = 2 if (model.render_semantic_mlp is not None and model.render_semantic_mlp.softmax) else 0
        act_fused = COMPOSITE_ACT_FUSED and (D == 0 or (E_inst >= 1 and 2 * E_inst >= D))
        mk = lambda on, cols: torch.empty((M, cols), dtype=torch.float32, device=dev) if on else None
        grads = (g_rgb, g_sem, g_inst, torch.empty((N, 3 + Ccls + D), dtype=torch.float32, device=dev), g_w, g_op)
        if act_fused:
            # the heads' output activations (sigmoid / softmax / identity) are taken back inside the compositing backward: what it writes are the
            # zero-padded pre-activation gradient rows the heads' backward kernels start from
            ldp_inst = (E_inst + 3) // 4 * 4
            d_rgb, d_sem, d_inst = mk(g_rgb is not None, 4), mk(g_sem is not None, (Ccls + 3) // 4 * 4), mk(g_inst is not None, ldp_inst)
            d_inst_slow = mk(g_inst is not None and slow_grad, ldp_inst)
            pre_rgb, pre_sem, pre_fast, pre_slow = d_rgb, d_sem, d_inst, d_inst_slow
            composite = lambda w, **which: _composite_bwd_act(ctx, w, grads, (d_rgb, d_sem, d_inst, d_inst_slow), sem_kind, E_inst, **which)
        else:       # (gradients w.r.t. the activated outputs: every head chain starts with its own clift_rows_act_bwd launch)
            d_rgb, d_sem, d_inst = mk(g_rgb is not None, 3), mk(g_sem is not None, Ccls), mk(g_inst is not None, D)
            pre_rgb = pre_sem = pre_fast = pre_slow = None
            composite = lambda w, **which: _composite_bwd(ctx, w, grads, (d_rgb, d_sem, d_inst), **which)
        if ctx.w_feat is not None:
            # "argmax" weights (render_forward): the colours against the weights (with the weight / opacity gradients), then the semantic and
            # instance rows against the one-hot array, which carries no gradient
            composite(ctx.w, feats=False)
            composite(ctx.w_feat, colour=False, wgrad=False)
        else:
            composite(ctx.w)
        br = Branches(model=model)
        if density_grad:
            model.xcd_workspace_for("density")
        if d_rgb is not None:
            model.xcd_workspace_for("appearance")

        def app_chain(keep):
            _app_backward(model, views, gviews, ctx, params["app"], gparams["app"], _head_dpre(pre_rgb, ctx.rgb_s, d_rgb, 0, 3, 1, M), keep)

        # ---------------- semantic head
        def sem_chain(keep):
            dpre = _head_dpre(pre_sem, ctx.sem_s, d_sem, 0, Ccls, sem_kind, M)
            if ctx.sem_grid is not None:
                grid_head_bwd(model, views, gviews, ctx, _kept_grid_head(ctx.sem_grid), [(params["sem"], gparams["sem"], ctx.sem_grid["acts"][0], dpre)], keep)
            else:
                xyz_mlp_bwd(params["sem"], gparams["sem"], ctx.xa, ctx.sem_acts, dpre, M, keep)

        # ---------------- instance head: the fast net's half of the row, and -- slow_grad -- the slow net's
        inst_nets = [("fast", pre_fast, 0, ctx.inst_fast_acts)] + ([("slow", pre_slow, E_inst, ctx.inst_slow_acts)] if slow_grad else [])

        def inst_chain(head, fused_row, off, acts):
            def run(keep):
                xyz_mlp_bwd(params[head], gparams[head], ctx.xa, acts, _head_dpre(fused_row, None, d_inst, off, E_inst, 0, M), M, keep)
            return run

        def inst_grid_chain(keep):
            st_ = _kept_grid_head(ctx.inst_grid)
            nets = [(params[head], gparams[head], st_["acts"][i], _head_dpre(fused_row, None, d_inst, off, E_inst, 0, M))
                    for i, (head, fused_row, off, _) in enumerate(inst_nets)]
            grid_head_bwd(model, views, gviews, ctx, st_, nets, keep)

        if d_rgb is not None:
            br.run(0, app_chain)
        if d_sem is not None:
            br.run(1, sem_chain)
        if d_inst is not None and ctx.inst_grid is not None:
            br.run(2, inst_grid_chain)
        elif d_inst is not None:
            for i, net in enumerate(inst_nets):
                br.run(2 + i, inst_chain(*net))
        if density_grad:
            if before_density is not None:
                if br.enabled:
                    br.join()                 # (side-stream mode: the head chains have to be on the current stream first)
                before_density()
                before_density = None
            br.run(4, lambda keep: _density_backward(model, ctx, views, gviews, g_w, g_op, g_dist, keep))
            density_grad = False
        br.join()
    elif g_rgb is not None and ctx.white_bg:
        # no active samples but the white background still routes d rgb into the opacity
        inside = ((ctx.rgb_raw >= 0) & (ctx.rgb_raw <= 1)).to(torch.float32)
        g_op = -(g_rgb * inside).sum(-1)
    if before_density is not None:
        before_density()
    # ---------------- density path (when it was not already run as a branch above)
    if density_grad:
        _density_backward(model, ctx, views, gviews, g_w, g_op, g_dist, [])


def _density_backward(model, ctx, views, gviews, g_w, g_op, g_dist, keep):
    """Transmittance backward (needs only g_w / g_opacity from the compositing backward, so it runs concurrently with
    the MLP chains) and the scatter into the density tables."""
    N, S = ctx.N, ctx.S
    dsigma = torch.empty((N, S), dtype=torch.float32, device=ctx.rays.device)
    call("clift_march_bwd", C.byref(ctx.ms), ptr(ctx.rays), ptr(ctx.jitter), N, ptr(ctx.alpha), ptr(ctx.T), ptr(ctx.w),
         ptr(ctx.ray_out), ptr(g_w), ptr(g_op), ptr(g_dist), ptr(dsigma), stream())
    vd = vm_struct(views, "density", ctx.res)
    gd = vm_grad_struct(model, gviews, "density")
    call("clift_density_bwd", C.byref(ctx.ms), C.byref(vd), C.byref(gd), ptr(ctx.rays), ptr(ctx.jitter), N, ptr(dsigma),
         ptr(ctx.sigma) if DENS_BWD_SIGMA else None, stream())
    vm_grad_finish(model, gviews, "density", gd)
    keep.append(dsigma)


# ----------------------------------------------------------------------------- instance / segment feature passes
def feature_forward(model, renderer, rays, jitter, head, grad_heads=("app", "sem", "fast", "slow"), cap=None, want_xyz=True):
    """renderer.py:178-217 (head='instance') / :259-300 (head='semantic'): density and weights carry no gradient,
    only the head does.  ``grad_heads`` as in render_forward."""
    rays, jitter = _check_rays(rays, jitter)
    views = model.named_views()
    ctx = _density_march(model, renderer, rays, jitter, cap)
    N, M = ctx.N, ctx.M
    dev = rays.device
    ctx.white_bg, ctx.stop_grad = 0, 1
    ctx.softmax_mode = 1 if (head == "semantic" and renderer.semantic_weight_mode == "softmax") else 0
    Ccls = model.num_semantic_classes if head == "semantic" else 0
    D = model.dim_feature_instance if head == "instance" else 0
    ctx.C, ctx.D = Ccls, D
    ctx.want = (False, head == "semantic", head == "instance")
    if M > 0:
        ctx.xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
        call("clift_active_xyz", C.byref(ctx.ms), ptr(rays), ptr(jitter), ptr(ctx.act_idx), M, ptr(ctx.xa), stream())
        chains = _head_chains(model, views, ctx, _head_params(views), grad_heads, head == "semantic")
        if head == "instance" and model.instance_plane is None:       # the fast and the slow xyz net: two branches
            br = Branches(model=model)
            for slot, chain in chains:
                br.run(slot, chain)
            br.join()
        else:       # the semantic head, the instance head on its grid: one chain, on the main stream
            for _, chain in chains:
                chain([])
    fresh = torch.empty if M > 0 else torch.zeros          # (as in render_forward: the sums are written in full unless the chunk is empty)
    sem_raw = fresh((N, Ccls), dtype=torch.float32, device=dev) if Ccls else None
    sem_map = torch.empty((N, Ccls), dtype=torch.float32, device=dev) if Ccls else None
    inst_map = fresh((N, D), dtype=torch.float32, device=dev) if D else None
    _composite_fwd(ctx, ctx.w, (None, None, sem_raw, sem_map, inst_map), colour=False)
    ctx.sem_raw = sem_raw
    if head == "instance":
        # renderer.py:213-215 (the trainer asks for the points only where its loss reads them: two elementwise launches otherwise unused)
        xyz = rays[:, 0:3] + ctx.ray_out[:, 1:2] * rays[:, 3:6] if want_xyz else None
        return (inst_map, xyz), ctx
    return sem_map, ctx


def feature_backward(model, ctx, gviews, g_out, slow_grad=False):
    if ctx.want[1]:
        render_backward(model, ctx, gviews, g_sem=g_out, density_grad=False)
    else:
        render_backward(model, ctx, gviews, g_inst=g_out, density_grad=False, slow_grad=slow_grad)


# ----------------------------------------------------------------------------- point-wise utilities (reference field API)
def _points(xyz):
    x = _lib.f32(xyz, "xyz").reshape(-1, xyz.shape[-1]).contiguous()
    if x.shape[1] < 3:
        raise ValueError("xyz must have >= 3 columns")
    return x


@torch.no_grad()
def density_points(model, xyz, activation=True):
    """TensorVMSplit.compute_density / compute_density_without_activation on normalised points (no gradient)."""
    x = _points(xyz)
    reset_rows_limit(x.device)
    views = model.named_views()
    vd = vm_struct(views, "density", grid_res(views))
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    call("clift_density_points", C.byref(vd), ptr(x), x.shape[1], x.shape[0], float(model.splus_density_shift), int(bool(activation)),
         ptr(out), stream())
    return out


@torch.no_grad()
def density_grad_points(model, xyz, world=True, renderer=None):
    """(n, 4) rows [gx, gy, gz, sigma_raw] at normalised points: the analytic gradient of the density before its softplus (DESIGN.md 6g;
    right-sided on a texel line, the zero padding seen as a step at the table's edge) and that density itself, with the bits of
    ``density_points(activation=False)``.  ``world``: the gradient in world units, g_a * 2 / extent_a of ``renderer``'s box (a renderer, or the
    three factors themselves, is then required: the field does not know its box); False: with respect to the normalised coordinates."""
    x = _points(xyz)
    reset_rows_limit(x.device)
    inv2 = None
    if world:
        if renderer is None:
            raise _lib.CliftError("density_grad_points(world=True) needs the renderer whose box scales the gradient (or world=False)")
        inv2 = (C.c_float * 3)(*[float(v) for v in getattr(renderer, "inv_box_extent_host", renderer)])
    views = model.named_views()
    vd = vm_struct(views, "density", grid_res(views))
    out = torch.empty((x.shape[0], 4), dtype=torch.float32, device=x.device)
    call("clift_density_grad_points", C.byref(vd), ptr(x), x.shape[1], x.shape[0], float(model.splus_density_shift), inv2, ptr(out), stream())
    return out


def _surface_launches(model, ctx, q):
    """The two launches of the surface pass over a march context whose xa is filled: the world gradient at the active samples, then the
    per-ray median hit and normal sums."""
    q = _surface_quantile(q)
    G = None
    if ctx.M > 0:
        views = model.named_views()
        vd = vm_struct(views, "density", ctx.res)
        G = torch.empty((ctx.M, 4), dtype=torch.float32, device=ctx.rays.device)
        call("clift_density_grad_points", C.byref(vd), ptr(ctx.xa), 4, ctx.M, float(ctx.ms.density_shift), ctx.ms.inv_ext2, ptr(G), stream())
    return _ray_surface_launch(ctx, q, G)


def _surface_quantile(q):
    q = float(q)
    if not 0.0 < q < 1.0:
        raise _lib.CliftError(f"surface outputs: q must lie in (0, 1), got {q}")
    return q


def _ray_surface_launch(ctx, q, G):
    """clift_ray_surface over what the context's march stored and the world gradients G (M, 4) at its active samples (None for M = 0)."""
    N, M, dev = ctx.N, ctx.M, ctx.rays.device
    depth = torch.empty((N,), dtype=torch.float32, device=dev)
    k_med = torch.empty((N,), dtype=torch.int32, device=dev)
    nrm = torch.empty((N, 4), dtype=torch.float32, device=dev)
    call("clift_ray_surface", C.byref(ctx.ms), ptr(ctx.rays), ptr(ctx.jitter), N, ptr(ctx.T), ptr(ctx.w), ptr(ctx.ray_start),
         ptr(ctx.act_idx) if M > 0 else None, M, ptr(G), q, ptr(depth), ptr(k_med), ptr(nrm), stream())
    rays = ctx.rays
    return dict(depth_median=depth, hit=k_med >= 0, k_median=k_med, normals=nrm[:, :3],
                points=rays[:, 0:3] + depth[:, None] * rays[:, 3:6])


@torch.no_grad()
def surface_from_ctx(model, renderer, ctx, q=0.5):
    """Surface outputs of the rays of a context that ``render_forward`` or ``feature_forward`` returned, from what its march
    stored: dict(depth_median (N,), hit (N,) bool, k_median (N,) int32, normals (N, 3) = sum_k w_k n_k, un-normalised, points (N, 3) =
    o + depth_median d; depth_median and k_median are 0 and -1 where hit is False).  Two launches; the context is only read.
    Refused: a sync-free (capped) context, whose row count never reached the host, and a context of ``edit_forward``, where the gradient at a
    remapped sample has to be turned back through the edit: ``edit_surface_from_ctx`` does that."""
    if not isinstance(ctx, RenderCtx) or ctx.ms is None:
        raise _lib.CliftError("surface_from_ctx: not a context of render_forward / feature_forward")
    if ctx.capped:
        raise _lib.CliftError("surface_from_ctx: a sync-free (capped) context is not supported: its active-sample count stays on the device")
    if ctx.edited:
        raise _lib.CliftError("surface_from_ctx: a context of edit_forward is not supported here (the gradient at a remapped sample has to be "
                              "turned back through the edit): use edit_surface_from_ctx")
    if ctx.M > 0 and ctx.xa is None:
        raise _lib.CliftError("surface_from_ctx: the context holds no positions of its active samples (xa)")
    return _surface_launches(model, ctx, q)


@torch.no_grad()
def surface_forward(model, renderer, rays, jitter=None, q=0.5):
    """Geometry only: the march, the positions of the active samples and the two surface launches -- no head runs.  Returns (the dict of
    ``surface_from_ctx`` plus depth = the expected distance and opacity, context)."""
    rays, jitter = _check_rays(rays, jitter)
    ctx = _density_march(model, renderer, rays, jitter)
    if ctx.M > 0:
        ctx.xa = torch.empty((ctx.M, 4), dtype=torch.float32, device=rays.device)
        call("clift_active_xyz", C.byref(ctx.ms), ptr(rays), ptr(jitter), ptr(ctx.act_idx), ctx.M, ptr(ctx.xa), stream())
    out = _surface_launches(model, ctx, q)
    out["depth"], out["opacity"] = ctx.ray_out[:, 1], ctx.ray_out[:, 0]
    return out, ctx


# ----------------------------------------------------------------------------- amodal instance layers
def _layers_check(who, model, table, use_delta):
    """The refusals the two layer passes share; -> E, the width of the instance head's fast half."""
    if model.render_instance_mlp is None:
        raise ValueError(f"{who}: the field has no instance head")
    E = int(model.render_instance_mlp.output_channels)
    if table.num_classes != model.num_semantic_classes:
        raise ValueError(f"{who}: the table knows {table.num_classes} classes, the field {model.num_semantic_classes}")
    if table.E != E and (table.mode == 1 or table.K > 0):
        raise ValueError(f"{who}: the table expects {table.E} feature columns, the instance head gives {E}")
    if use_delta and E != 3:
        raise ValueError(f"{who}: use_delta adds world positions to the features, which needs 3 columns (the head gives {E})")
    return E


def _alpha_list(ctx, renderer, alpha_thres):
    """The march's samples listed again by alpha > threshold (the count, clift_scan_counts, clift_compact_fill): the context's list becomes
    the alpha-list, M_render keeps the length of the march's own."""
    N, S, dev, st = ctx.N, ctx.S, ctx.rays.device, stream()
    # the same fp32 threshold for the count and for the fill, however torch compares a tensor with a Python number
    thres = float(np.float32(renderer.raymarch_weight_thres if alpha_thres is None else alpha_thres))
    n_listed = (ctx.alpha > thres).sum(1, dtype=torch.int32)
    ray_start = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    call("clift_scan_counts", ptr(n_listed), N, ptr(ray_start), st)
    M = int(ray_start[N].item())
    act_idx = torch.empty((max(M, 1),), dtype=torch.int32, device=dev)
    call("clift_compact_fill", ptr(ctx.alpha), ptr(ray_start), N, S, thres, ptr(act_idx), st)
    ctx.M_render, ctx.M, ctx.ray_start, ctx.act_idx = ctx.M, M, ray_start, act_idx
    return M


def _layer_heads(model, views, ctx):
    """The semantic head and the fast instance net over the list (no appearance chain, no slow net)."""
    br = Branches(model=model)
    for slot, chain in _head_chains(model, views, ctx, _head_params(views), (), True):
        if slot != 3:                   # (3: the slow xyz net, which no slot reads)
            br.run(slot, chain)
    br.join()


def _sample_slots(ctx, renderer, table, E, use_delta):
    """clift_sample_slots over the list under ``table``'s own slots -> (M,) int32; with ``use_delta`` the world position of the looked-up
    point, de-normalised from xa, is the added term (ctx.layer_add)."""
    M, dev = ctx.M, ctx.rays.device
    cls_slots, cent = table.on(dev)
    if use_delta:
        ctx.layer_add = ((ctx.xa[:, :3] + 1.0) / renderer.inv_box_extent + renderer.bbox_aabb[0]).contiguous()
    slots = torch.empty((M,), dtype=torch.int32, device=dev)
    call("clift_sample_slots", ptr(ctx.sem_s), ctx.C, ctx.C, ptr(ctx.inst_s), ctx.D, E, ptr(ctx.layer_add), 3, ptr(cls_slots), ptr(cent), table.K_base,
         table.mode, M, ptr(slots), stream())
    ctx.inst_s = ctx.inst_s[:, :E]
    return slots


def _layer_colour_check(who, colour, colour_rest):
    if colour_rest and not colour:
        raise ValueError(f"{who}: colour_rest needs colour=True (it says which rows are coloured, not whether)")


def _layer_colour(model, views, ctx, K, colour_rest, dirs_of):
    """The colour layers of a layer pass whose slots are known -> (N, K + 1, 4) rows [R, G, B, A], premultiplied.  Coloured
    are the list rows whose column is below ``K`` -- with ``colour_rest`` every row: most listed samples of a real scene belong to stuff
    classes, and the appearance chain is the expensive part.  ``dirs_of(rows)``: the view directions (Mc, 3) of the list rows ``rows`` (int64).
    The count Mc reaches the host.  The context keeps layer_rgb (Mc, 3), layer_rgb_row (M; -1: not coloured) and layer_dirs (Mc, 3)."""
    N, M, dev, st = ctx.N, ctx.M, ctx.rays.device, stream()
    Mc = 0
    if M > 0:
        keep = torch.ones((M,), dtype=torch.bool, device=dev) if colour_rest else (ctx.slots >= 0) & (ctx.slots < K)
        rows = torch.nonzero(keep).reshape(-1)
        Mc = int(rows.shape[0])
        ctx.layer_rgb_row = torch.full((M,), -1, dtype=torch.int32, device=dev)
        ctx.layer_rgb_row[rows] = torch.arange(Mc, dtype=torch.int32, device=dev)
    ctx.layer_rgb = ctx.layer_dirs = None
    if Mc > 0:
        xc = ctx.xa[rows].contiguous()
        ctx.layer_dirs = dirs_of(rows).contiguous()
        va = vm_struct(views, "appearance", ctx.res)
        F = torch.empty((Mc, 3 * va.comps), dtype=torch.float32, device=dev)
        call("clift_vm_products_points", C.byref(va), ptr(xc), 4, Mc, ptr(F), st)
        ctx.layer_rgb = _app_points_chain(model, views, _head_params(views), F, ctx.layer_dirs, 3, Mc, [])
    out = torch.empty((N, K + 1, 4), dtype=torch.float32, device=dev)
    call("clift_ray_layer_colour", C.byref(ctx.ms), N, ptr(ctx.alpha), ptr(ctx.ray_start), ptr(ctx.act_idx) if M > 0 else None, M,
         ptr(ctx.slots) if M > 0 else None, K, ptr(ctx.layer_rgb), 3, Mc, ptr(ctx.layer_rgb_row) if M > 0 else None, ptr(out), st)
    return out


@torch.no_grad()
def point_slots(model, renderer, points, table, use_delta=False, chunk=2 ** 20):
    """The slot under ``table`` (a ``layers.SlotTable``) of arbitrary WORLD points (n, 3) on the device -> (n,) int32, -1 where the point's
    class has no slot.  The semantic head and the fast instance net through the field's point-wise methods, as ``mesh.label_vertices``
    evaluates them (xyz-MLP heads and heads on their own VM grid alike), then clift_sample_slots, ``chunk`` points at a time.  With
    ``use_delta`` the feature is output + world position.  No aabb test: what is inside the scene is the caller's decision."""
    E = _layers_check("point_slots", model, table, use_delta)
    pts = _lib.f32(points, "points").reshape(-1, 3).contiguous()
    n, dev = pts.shape[0], pts.device
    Ccls = model.num_semantic_classes
    cls_slots, cent = table.on(dev)
    slots = torch.empty((n,), dtype=torch.int32, device=dev)
    for a in range(0, n, int(chunk)):
        b = min(n, a + int(chunk))
        xyz = pts[a:b]
        xn = renderer.normalize_coordinates(xyz).contiguous()
        sem = model.render_semantic_mlp(None, model.compute_semantic_feature(xn)).float().contiguous()
        feat = model.render_instance_mlp(None, model.compute_instance_feature(xn)).float().contiguous()
        call("clift_sample_slots", ptr(sem), sem.shape[1], Ccls, ptr(feat), feat.shape[1], E, ptr(xyz) if use_delta else None, 3, ptr(cls_slots),
             ptr(cent), table.K_base, table.mode, b - a, ptr(slots[a:b]), stream())
    return slots


@torch.no_grad()
def layers_forward(model, renderer, rays, table, jitter=None, alpha_thres=None, use_delta=False, cap=None, colour=False, colour_rest=False):
    """Per ray and per instance slot of ``table`` (a ``layers.SlotTable``) what that instance covers ALONE, also behind what hides it: the march,
    its samples listed again by alpha > ``alpha_thres`` (default: renderer.raymarch_weight_thres) -- a sample behind an occluder has w ~ 0 and is
    in no render's list --, the semantic head and the fast instance net over that list (no appearance chain, no slow net, no compositing), one
    slot per row (clift_sample_slots) and the per-ray composite that keeps one transmittance per slot (clift_ray_layers).
    Returns (dict(layers (N, K + 1, 4) rows [A, V, Z, zf], column K the rest; opacity (N,), depth (N,) of the whole scene; n_listed), context).
    The context holds the alpha-list (ray_start, act_idx, M), xa, sem_s, inst_s (the fast half), slots and, with ``use_delta`` (the feature is
    output + world position; needs 3 feature columns), layer_add.  Refused: a sync-free pass (``cap``), a field without an instance head, a table
    that does not fit the field.  This pass takes no edit: the layers of an edited scene are ``edit_layers_forward``'s.

    ``colour``: the dict also holds colour (N, K + 1, 4), rows [R, G, B, A]: the premultiplied colour of every column rendered
    alone, without a background, A with the bits of layers[..., 0].  The listed rows with a slot -- with ``colour_rest`` all of them -- go
    through the point-wise appearance chain at xa with the ray's direction, and clift_ray_layer_colour composites them per column; the
    context keeps layer_rgb, layer_rgb_row and layer_dirs.  Without ``colour`` nothing of this is launched."""
    _layer_colour_check("layers_forward", colour, colour_rest)
    if cap is not None:
        raise _lib.CliftError("layers_forward: a sync-free (capped) pass is not supported: the length of the alpha-list has to reach the host")
    E = _layers_check("layers_forward", model, table, use_delta)
    rays, jitter = _check_rays(rays, jitter)
    views = model.named_views()
    ctx = _density_march(model, renderer, rays, jitter)
    N, dev, st = ctx.N, rays.device, stream()
    K = table.K
    M = _alpha_list(ctx, renderer, alpha_thres)
    ray_start, act_idx = ctx.ray_start, ctx.act_idx
    ctx.C, ctx.D = model.num_semantic_classes, model.dim_feature_instance
    ctx.want = (False, False, False)
    if M > 0:
        ctx.xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
        call("clift_active_xyz", C.byref(ctx.ms), ptr(rays), ptr(jitter), ptr(act_idx), M, ptr(ctx.xa), st)
        _layer_heads(model, views, ctx)
        ctx.slots = _sample_slots(ctx, renderer, table, E, use_delta)
    out = torch.empty((N, K + 1, 4), dtype=torch.float32, device=dev)
    call("clift_ray_layers", C.byref(ctx.ms), ptr(rays), ptr(jitter), N, ptr(ctx.alpha), ptr(ctx.w), ptr(ray_start), ptr(act_idx) if M > 0 else None,
         M, ptr(ctx.slots), K, ptr(out), st)
    res = dict(layers=out, opacity=ctx.ray_out[:, 0], depth=ctx.ray_out[:, 1], n_listed=M)
    if colour:
        # the direction the render's own appearance encoding reads for a sample: its ray's
        res["colour"] = _layer_colour(model, views, ctx, K, colour_rest,
                                      lambda rows: rays[torch.div(act_idx[rows].long(), ctx.S, rounding_mode="floor"), 3:6])
    return res, ctx


# ----------------------------------------------------------------------------- amodal instance layers of an edited scene
@torch.no_grad()
def edit_layers_forward(model, renderer, rays, edit, table, alpha_thres=None, use_delta=False, colour=False, colour_rest=False):
    """``layers_forward`` of the scene ``edit`` describes (whatever ``edit.as_program`` takes), with a column of its own for every copy:
    ``table`` (the scene's ``layers.SlotTable``) is extended by ``table.for_program`` to K + c slots, c the DUPLICATE edits of the program.

      edit march at renderer.raymarch_weight_thres (alpha, w) -> alpha-list (count, scan_counts, compact_fill) ->
      clift_edit_list_active_origin (xa where the content is looked up, origin, state) -> semantic head and fast instance net on xa ->
      clift_sample_slots under the BASE table -> retarget (a row with origin i > 0 and a slot goes to the column of copy i) ->
      clift_ray_layers with K + c.

    A killed sample has sigma exactly 0, so alpha 0: it is in no alpha-list (``alpha_thres`` < 0 is refused for that reason).  A moved
    object keeps its slot; a copy that a later edit moves keeps its column.  With ``use_delta`` the added position is the world position of
    the looked-up point.  Returns (dict(layers (N, K + c + 1, 4), opacity, depth of the edited scene, n_listed, table = the extended table),
    context); the context holds the alpha-list, xa, sem_s, inst_s, slots (retargeted), base_slots, origin, state, edit_program and edited =
    True.  The march always goes through the list kernel: a single ``Edit`` is walked as a program of one (clift_edit_list_density_fwd, whose
    walk is that edit op for op), where ``edit_forward`` keeps the single-edit launches for it.  Refused: a head on its own VM grid (as
    ``edit_forward``), and what ``layers_forward`` refuses.

    ``colour`` / ``colour_rest``: as in ``layers_forward``, with K + c + 1 columns -- a copy has a colour layer of its own.  One more launch
    of clift_edit_list_active over the alpha-list gives the turned view directions (its xa, kept as layer_xa, has the bits of the origin
    kernel's); the rows whose retargeted column is below K + c are coloured at xa with those directions."""
    _layer_colour_check("edit_layers_forward", colour, colour_rest)
    if model.semantic_plane is not None or model.instance_plane is not None:
        raise NotImplementedError("edit_layers_forward: a semantic / instance head on its own VM grid is not supported (xyz MLP heads only)")
    E = _layers_check("edit_layers_forward", model, table, use_delta)
    if alpha_thres is not None and float(alpha_thres) < 0:
        raise ValueError(f"edit_layers_forward: alpha_thres must be >= 0 (got {alpha_thres}): a killed sample has alpha 0 and stays out of the list")
    prog = _edit.as_program(edit)
    _refuse_shaped("edit_layers_forward", prog)             # (the origin walk, clift_edit_list_active_origin, reads the boxes alone)
    ext = table.for_program(prog)
    rays, _ = _check_rays(rays, None)
    views = model.named_views()
    ctx, _, _ = _edit_density_march(model, renderer, rays, prog, renderer.raymarch_weight_thres)
    N, dev, st = ctx.N, rays.device, stream()
    M = _alpha_list(ctx, renderer, alpha_thres)
    ctx.C, ctx.D = model.num_semantic_classes, model.dim_feature_instance
    ctx.want = (False, False, False)
    if M > 0:
        ctx.xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
        ctx.origin = torch.empty((M,), dtype=torch.uint8, device=dev)
        ctx.state = torch.empty((M,), dtype=torch.uint8, device=dev)
        call("clift_edit_list_active_origin", C.byref(ctx.ms), prog.records(), len(prog), ptr(rays), ptr(ctx.act_idx), M, ptr(ctx.xa),
             ptr(ctx.origin), ptr(ctx.state), st)
        _layer_heads(model, views, ctx)
        ctx.base_slots = _sample_slots(ctx, renderer, table, E, use_delta)
        ctx.slots = _layers.retarget(ctx.base_slots, ctx.origin, ext)
    out = torch.empty((N, ext.K + 1, 4), dtype=torch.float32, device=dev)
    call("clift_ray_layers", C.byref(ctx.ms), ptr(rays), None, N, ptr(ctx.alpha), ptr(ctx.w), ptr(ctx.ray_start), ptr(ctx.act_idx) if M > 0 else None,
         M, ptr(ctx.slots), ext.K, ptr(out), st)
    res = dict(layers=out, opacity=ctx.ray_out[:, 0], depth=ctx.ray_out[:, 1], n_listed=M, table=ext)
    if colour:
        dirs = None
        if M > 0:
            ctx.layer_xa = torch.empty((M, 4), dtype=torch.float32, device=dev)
            dirs = torch.empty((M, 4), dtype=torch.float32, device=dev)
            call("clift_edit_list_active", C.byref(ctx.ms), prog.records(), len(prog), ptr(rays), ptr(ctx.act_idx), M, ptr(ctx.layer_xa), ptr(dirs), st)
        res["colour"] = _layer_colour(model, views, ctx, ext.K, colour_rest, lambda rows: dirs[rows, :3])
    return res, ctx


# ----------------------------------------------------------------------------- surface outputs of an edited scene
@torch.no_grad()
def edit_density_grad_points(model, renderer, xyz_world, edit, want_state=False):
    """(n, 4) rows [gx, gy, gz, sigma_raw] at WORLD points of the scene ``edit`` describes (an ``edit.Edit``, an ``edit.EditProgram`` or a
    sequence of edits): the world gradient of the edited raw density, J^T g' with J the product of the maps of the edits that remapped the
    point and g' ``density_grad_points(world=True)`` at the point the walk ends at, and the raw density there.  A killed point gets a row
    of zeros.  No aabb test: a point (or its source) outside ``renderer``'s box reads zero padding.  ``want_state``: also the (n,) uint8
    state of ``EditProgram.apply_to_points``."""
    x = _points(xyz_world)
    reset_rows_limit(x.device)
    prog = _edit.as_program(edit)
    _refuse_shaped("edit_density_grad_points", prog)
    ms = march_struct(renderer, model)
    views = model.named_views()
    vd = vm_struct(views, "density", grid_res(views))
    n = x.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=x.device)
    state = torch.empty((n,), dtype=torch.uint8, device=x.device) if want_state else None
    call("clift_edit_list_density_grad_points", prog.records(), len(prog), C.byref(vd), ptr(x), x.shape[1], n, ms.lo, ms.inv_ext2,
         float(ms.density_shift), ptr(out), ptr(state), stream())
    return (out, state) if want_state else out


def _edit_surface_launches(model, ctx, q):
    """The surface pass of an edited march: the gradient of the EDITED density at the active samples (one launch, the walk recomputed from
    the rays -- no xa is needed), then the unchanged per-ray launch."""
    q = _surface_quantile(q)
    _refuse_shaped("edit_density_grad_active", ctx.edit_program)
    G = None
    if ctx.M > 0:
        views = model.named_views()
        vd = vm_struct(views, "density", ctx.res)
        prog = ctx.edit_program
        G = torch.empty((ctx.M, 4), dtype=torch.float32, device=ctx.rays.device)
        call("clift_edit_list_density_grad_active", C.byref(ctx.ms), prog.records(), len(prog), C.byref(vd), ptr(ctx.rays), ptr(ctx.act_idx),
             ctx.M, ptr(G), stream())
    return _ray_surface_launch(ctx, q, G)


@torch.no_grad()
def edit_surface_from_ctx(model, renderer, ctx, q=0.5):
    """``surface_from_ctx`` for a context that ``edit_forward`` returned: the same dict (depth_median, hit, k_median, normals, points), the
    normals from the gradient of the edited density -- at a remapped sample the field's gradient turned back through the edits, J^T g'
    (DESIGN.md 6h).  Two launches; the context is only read.  Any other context is refused: it belongs to ``surface_from_ctx``."""
    if not isinstance(ctx, RenderCtx) or ctx.ms is None or not ctx.edited or ctx.edit_program is None:
        raise _lib.CliftError("edit_surface_from_ctx: not a context of edit_forward (surface_from_ctx takes the context of an unedited pass)")
    if ctx.capped:
        raise _lib.CliftError("edit_surface_from_ctx: a sync-free (capped) context is not supported: its active-sample count stays on the device")
    _refuse_shaped("edit_surface_from_ctx", ctx.edit_program)
    return _edit_surface_launches(model, ctx, q)


@torch.no_grad()
def edit_surface_forward(model, renderer, rays, edit, q=0.5, weight_thres=0.0):
    """Geometry of an edited scene only: the edit's density forward, the march and the two surface launches -- no head runs and no xa is
    made, so a field whose semantic / instance head sits on its own VM grid is fine here.  ``weight_thres`` as in ``edit_forward``.
    Returns (the dict of ``edit_surface_from_ctx`` plus depth = the expected distance and opacity, context)."""
    rays, _ = _check_rays(rays, None)
    _refuse_shaped("edit_surface_forward", _edit.as_program(edit))
    ctx, _, _ = _edit_density_march(model, renderer, rays, edit, weight_thres)
    out = _edit_surface_launches(model, ctx, q)
    out["depth"], out["opacity"] = ctx.ray_out[:, 1], ctx.ray_out[:, 0]
    return out, ctx


def _basis_feature_points(model, prefix, xyz, precision):
    """VM products of the ``prefix`` tables at the points + basis Linear, the GEMM under the context ``precision``."""
    x = _points(xyz)
    reset_rows_limit(x.device)
    n = x.shape[0]
    views = model.named_views()
    vm = vm_struct(views, prefix, grid_res(views))
    nc = 3 * vm.comps
    F = torch.empty((n, nc), dtype=torch.float32, device=x.device)
    call("clift_vm_products_points", C.byref(vm), ptr(x), x.shape[1], n, ptr(F), stream())
    Wb = views[f"{prefix}_basis_mat.weight"]
    out = torch.empty((n, Wb.shape[0]), dtype=torch.float32, device=x.device)
    with precision:
        gemm(n, Wb.shape[0], nc, F, nc, Wb, _pitch(Wb), out, out.shape[1])
    return out


@torch.no_grad()
def appearance_feature_points(model, xyz):
    """TensorVMSplit.compute_appearance_feature: VM products + basis Linear (no gradient), the GEMM at the precision that is set."""
    return _basis_feature_points(model, "appearance", xyz, contextlib.nullcontext())


@torch.no_grad()
def grid_feature_points(model, prefix, xyz):
    """TensorVMSplit.compute_semantic_feature / compute_instance_feature for a head on its own VM grid: VM products + basis Linear (no gradient),
    the GEMM exact as in grid_head_fwd."""
    return _basis_feature_points(model, prefix, xyz, exact_fp32())


@torch.no_grad()
def feat_mlp_points(seq, feats):
    """Evaluate a feature-input MLP head (grid heads: MLPRenderSemanticFeature / MLPRenderInstanceFeature on 27 features) on arbitrary rows."""
    f = _lib.f32(feats, "features").reshape(-1, feats.shape[-1]).contiguous()
    reset_rows_limit(f.device)
    M = f.shape[0]
    layers = [(m.weight, m.bias) for m in seq if isinstance(m, torch.nn.Linear)]
    ldx = _pitch(layers[0][0])
    X = torch.zeros((M, ldx), dtype=torch.float32, device=f.device)
    X[:, :f.shape[1]] = f
    out = torch.empty((M, layers[-1][0].shape[0]), dtype=torch.float32, device=f.device)
    with _grid_precision():
        feat_mlp_fwd(layers, X, M, out, out.shape[1], keep=False)
    return out


@torch.no_grad()
def xyz_mlp_points(seq, xyz):
    """Evaluate an xyz MLP head on arbitrary points (inference utility, no gradient)."""
    x = _points(xyz)
    reset_rows_limit(x.device)
    M = x.shape[0]
    xa = torch.zeros((M, 4), dtype=torch.float32, device=x.device)
    xa[:, :3] = x[:, :3]
    layers = [(m.weight, m.bias) for m in seq if isinstance(m, torch.nn.Linear)]
    out = torch.empty((M, layers[-1][0].shape[0]), dtype=torch.float32, device=x.device)
    xyz_mlp_fwd(layers, xa, M, out, out.shape[1], keep_first=False)
    return out


@torch.no_grad()
def appearance_mlp_points(module, viewdirs, features):
    """MLPRenderFeature.forward(viewdirs, features) (tensoRF.py:400-411), no gradient."""
    f = _lib.f32(features, "features").reshape(-1, features.shape[-1]).contiguous()
    d = _lib.f32(viewdirs, "viewdirs").reshape(-1, 3).contiguous()
    reset_rows_limit(f.device)
    n, nf = f.shape
    (W1, b1), (W2, b2), (W3, b3) = [(m.weight, m.bias) for m in module.mlp if isinstance(m, torch.nn.Linear)]
    ldx = _pitch(W1)
    X = torch.empty((n, ldx), dtype=torch.float32, device=f.device)
    call("clift_app_encode_points", ptr(f), nf, nf, module.pe_feat, module.pe_view, ptr(d), 3, n, ptr(X), ldx, stream())
    H1 = torch.empty((n, W1.shape[0]), dtype=torch.float32, device=f.device)
    gemm(n, W1.shape[0], ldx, X, ldx, W1, ldx, H1, H1.shape[1], bias=b1, act=1)
    out = torch.empty((n, 3), dtype=torch.float32, device=f.device)
    _app_tail(n, H1, W2, b2, W3, b3, torch.float32, out)
    return out
