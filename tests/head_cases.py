"""Shared inputs of the MLP-head entry-point tests (test_head_cases_host.py on the CPU, test_gpu_head_cases.py on the GPU): the entry points of
include/clift.h that do NOT go through clift_gemm, each with a table of seeded cases that reaches the forms its launcher distinguishes, an
fp64 reference of the operation on the values as stored, and the yardstick of a case: the same operation in fp32 on the CPU with every sum
one running accumulator in the three orders of loss_cases, measured against fp64.  A device result is held, element by element, to
``(8 * yardstick + 4 * 2^-24) * S`` with S the sum of the magnitudes of that element's terms -- gemm_cases.check's rule -- and a bf16-stored
result gets 2^-8 |reference| on top.

A reference is a full image of the output BUFFER: a number where the entry point writes, NaN where it must not (pad columns, the two rows past
the output), and the comparison demands the pre-fill's bits there.  Operand rows past the row count and operand pad columns are NaN.

S of the quantities that are not plain sums (written down here because the bound depends on them):
  sigmoid      out = 1 / (1 + exp(-x)):  S = out (1 + |x|) -- the argument's rounding moves exp by |x| 2^-24 relative, and out <= exp(x);
  softmax      p_c = exp(x_c - mx) / sum:  S = p_c (1 + |x_c - mx|), the same reasoning for the subtraction x_c - mx;
  softmax over a layer's logits (clift_out_layer_fwd, act 2): d p_c = p_c (d x_c - sum_j p_j d x_j), so with |d x_j| <= f S_logit_j:
               S = p_c (1 + |x_c - mx| + S_logit_c + max_j S_logit_j);
  sigmoid' / softmax' (clift_rows_act_bwd): products and one dot over the stored `out`: S = |g| o (1 - o), S = o (|g| + sum_j |g_j| o_j).

The host test holds the tables to the entry points parsed from include/clift.h, so one added there cannot go unnoticed.  Nothing here
touches the GPU."""
import functools
import os
import re

import numpy as np

import gemm_cases as gc
from gemm_cases import BF16_HALF_SPACING, CUS, PAD_FINITE, RESERVE, SENTINEL, bf16r, cdiv, r4, row_ranges  # noqa: F401
from loss_cases import HALF_ULP, ILL_CONDITIONED, ORDERS  # noqa: F401

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "contrastive_lift_amd", "csrc")
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "clift.h")
PROBE_PRODUCTS = 1 << 19
# An element all of whose terms lie near the denormal range (one row of H = 2^-130 times a gradient) has no relative precision in ANY fp32
# arithmetic -- a product below 2^-126 keeps fewer than 24 bits, and a matrix core may flush it: such elements do not set the yardstick
# (S <= NORMAL_FLOOR), and every bound carries TINY, four times the smallest normal, on top.
NORMAL_FLOOR, TINY = 2.0 ** -100, 2.0 ** -124


def source_constant(file, name):
    """``constexpr int NAME = value`` of a kernel file: the streamed tile the row counts are built around."""
    with open(os.path.join(_CSRC, file)) as f:
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)", f.read())
    assert m, (file, name)
    return int(m.group(1))


NS_ROWS = source_constant("narrow_stream.hip", "NS_ROWS")        # k_wgrad_narrow_stream (clift_wgrad_narrow / clift_linear_k3_bwd from 4096 rows)
OF_ROWS = source_constant("narrow_stream.hip", "OF_ROWS")        # k_out_narrow_fwd


def header_entry_points():
    """The extern "C" names of the family: include/clift.h from clift_out_layer_bwd to clift_rows_act_bwd, clift_gemm itself left out, and the
    two launches of the shard bracket."""
    with open(_HEADER) as f:
        text = f.read()
    body = text[text.index("/* Backward of a narrow output layer"):text.index("/* ---- a13 compositing")]
    names = set(re.findall(r"^int (clift_\w+)\(", body, flags=re.M)) - {"clift_gemm"}
    return names | {"clift_grad_shards_begin", "clift_grad_shards_fold"}


# ---------------------------------------------------------------------------------------------------------------- the dispatchers, restated
def k3_fwd_kernel(Nout):
    """clift_linear_k3_fwd (csrc/gemm.hip): the register-resident kernel needs Nout / 4 to divide 256."""
    return "any" if Nout > 1024 or 256 % (Nout // 4) != 0 else "main"


def k3_fwd_blocks(M, Nout):
    rpi = 256 // (Nout // 4)
    return min(cdiv(M, rpi), 2048), rpi


def k3_bwd_route(M, Nout, has_db, ldh, dh_bf16):
    """clift_linear_k3_bwd: the matrix-core stream or the plain kernel (bases are 16-byte aligned in every case of the table)."""
    return "stream" if Nout == 256 and M >= 4096 and has_db and ldh % (8 if dh_bf16 else 4) == 0 else "plain"


def wgrad_narrow_route(M, no, ni, ldd, ldx, x_bf16):
    """clift_wgrad_narrow: ("stream", -) or ("plain", the NO template)."""
    if (ni == 256 or (not x_bf16 and 32 <= ni < 256 and ni % 4 == 0)) and M >= 4096 and ldd % 4 == 0 and no <= ldd <= 32 and ldx % (8 if x_bf16 else 4) == 0:
        return "stream", 0
    return "plain", next(t for t in (4, 8, 16, 24, 32) if no <= t)


def m3_rows(T, per_cu=1, first=1):
    """The smallest row count >= first at which, with RESERVE CUs held back, a block of persistent_ranges(rows, T) walks at least three tiles and
    the last block ends on a ragged tile (gemm_cases.m3 for a launcher that is not a clift_gemm route)."""
    rows = first
    while True:
        rpb = row_ranges(rows, T, CUS - RESERVE, per_cu)[1]
        if cdiv(min(rpb, rows), T) >= 3 and (rows - (cdiv(rows, rpb) - 1) * rpb) % T != 0:
            return rows
        rows += 1


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One launch of an entry point.  ``p``: its parameters, also attributes; reserve: clift_set_cu_reserve of the launch."""

    def __init__(self, entry, reserve=0, tag="", **p):
        self.entry, self.reserve, self.p, self.seed = entry, reserve, dict(p), 0
        self.__dict__.update(p)
        tag = (tag + "_" if tag else "") + "m3" if reserve else tag
        self.name = "_".join(f"{k}{v}" for k, v in p.items() if v is not None) + (f"_{tag}" if tag else "")
        self.key = (entry, self.name)

    def __repr__(self):
        return f"{self.entry}:{self.name}"

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Case) and self.key == other.key


class Entry:
    """What the tests need to know of an entry point.  T: rows of its streamed tile; fwd: the outputs whose rows correspond to sample rows --
    written with plain stores, the same bits at every launch, and under the device row limit L rows < L keep their bits; every other output is
    a reduction over the samples that ends in fp32 atomics and under the limit equals the reference of L rows; streamed: the inputs whose rows
    are samples; bf16: {buffer: the case attribute that says it is bf16-stored}; limit: the kernel honours the device row limit."""

    def __init__(self, T, draw, ref, restate, fwd, streamed, bf16=None, limit=True):
        self.T, self.draw, self.ref, self.restate, self.fwd, self.streamed, self.bf16, self.limit = T, draw, ref, restate, fwd, streamed, bf16 or {}, limit


_OB = ("clift_out_layer_bwd", "clift_out_layer_bwd_nh", "clift_out_layer_bwd_n128_bf16")
_L2 = ("clift_xyz_head_last2_fwd", "clift_app_head_last2_fwd", "clift_xyz_head_last2_x6_fwd", "clift_app_head_last2_x6_fwd", "clift_app_head_last2_bf16_fwd")
_FUSED = ("clift_xyz_head_first2_fwd", "clift_xyz_head_first2_x6_fwd") + _L2
_FB = ("clift_xyz_head_first2_bwd", "clift_xyz_head_first2_x6_bwd")
_FW = ("clift_xyz_head_first2_wgrad", "clift_xyz_head_first2_x6_wgrad")


def tile(c):
    """Rows of the streamed tile of the kernel the case goes to."""
    if c.entry == "clift_linear_k3_fwd":
        return k3_fwd_blocks(c.M, c.Nout)[1] if k3_fwd_kernel(c.Nout) == "main" else 64
    if c.entry == "clift_linear_k3_bwd":
        return NS_ROWS if k3_bwd_route(c.M, c.Nout, c.db, c.ldh, c.dh_bf16) == "stream" else 32
    if c.entry == "clift_wgrad_narrow":
        return NS_ROWS if wgrad_narrow_route(c.M, c.no, c.ni, c.ldd, c.ldx, c.x_bf16)[0] == "stream" else 64
    if c.entry.startswith("clift_rows_act"):
        return 4                                   # 256 lanes / 64-lane groups: the fewest rows a block holds
    if c.entry.startswith("clift_out_layer_bwd"):
        return ob_kind(c)[0]
    if c.entry in _FB + _FW:
        return fb_T(c)
    if c.entry == "clift_xyz_head_first2_bf16_bwd":
        return LY_ROWS
    return ENTRIES[c.entry].T


def stored_bf16(c, buf):
    if buf.startswith("_chain"):                 # a stored intermediate of a chain of bf16 roundings
        return True
    attr = ENTRIES[c.entry].bf16.get(buf)
    return bool(attr and getattr(c, attr))


def _rng(seed):
    return np.random.default_rng(9000 + seed)


def _rows(rng, M, n):
    """(M, n) ordinary values, none near zero, the rows differing in scale by 2^+-6."""
    return gc._nonzero(rng, (M, n)) * np.exp2(rng.integers(-6, 7, (M, 1))).astype(np.float32)


def _buf(logical, rows_alloc, ld, bf16=False):
    """The stored image of a logical matrix: (rows_alloc, ld), pad columns and the rows past it NaN."""
    b = np.full((rows_alloc, ld), np.nan, dtype=np.float32)
    b[:logical.shape[0], :logical.shape[1]] = bf16r(logical) if bf16 else logical
    return b


def _out(rows, ld):
    return np.full((rows + 2, ld), SENTINEL, dtype=np.float32)


def _image(shape):
    """(reference, S) images of an output buffer: NaN = not to be written."""
    return np.full(shape, np.nan), np.zeros(shape)


def _grad0(rng, out0, A, B, rows, cols):
    """Pre-fill of an accumulated-into gradient (rows x cols of out0): values of the size of the sum itself (see gemm_cases._draw)."""
    rms = np.sqrt((A.astype(np.float64) ** 2).T @ (B.astype(np.float64) ** 2))
    out0[:rows, :cols] = (rng.standard_normal((rows, cols)) * rms).astype(np.float32)


def _six(a, b, drop_middle=False):
    """The six leading products of two exactly three-way-split operands, added smallest first (gemm_cases._ksum): a (..., k), b (..., k)."""
    (a1, a2, a3), (b1, b2, b3) = gc.split3(np.ascontiguousarray(a, dtype=np.float32)), gc.split3(np.ascontiguousarray(b, dtype=np.float32))
    if drop_middle:
        a2 = np.zeros_like(a2)
    return (((a3 * b1 + a2 * b2) + a1 * b3) + (a2 * b1 + a1 * b2)) + a1 * b1


def _tsum(A, B, order, take=None, split=False, drop_middle=False):
    """sum_m A[m][i] B[m][j] in fp32 as one running sum over m in ``order``: (a, b); ``take``: only these i; split: fp32x6 products."""
    f = np.float32
    idx = np.arange(A.shape[1]) if take is None else take
    out = np.zeros((A.shape[1], B.shape[1]), f)
    Bt = np.ascontiguousarray(B.T, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in idx:
            a = np.ascontiguousarray(A[:, i], dtype=f)[None, :]
            out[i] = gc._ordered_sum(_six(np.broadcast_to(a, Bt.shape), Bt, drop_middle) if split else a * Bt, order)
    return out


def _take(n, per, edges):
    """Which of n output rows a restatement evaluates when each costs ``per`` products: all, or the edges first within PROBE_PRODUCTS."""
    return gc._take(edges, max(4, PROBE_PRODUCTS // max(per, 1)), n)


def _drop_rows(M, mistake, T):
    """Row count / source rows of the streamed-reduction mistakes."""
    if mistake == "last_m_mod_8_rows_dropped":
        return M - M % 8
    if mistake == "last_m_mod_64_rows_dropped":
        return M - M % 64
    return M


def _ragged_from_previous(X, M, T):
    """The rows of the ragged last tile replaced by the rows of the tile before."""
    first = ((M - 1) // T) * T
    if first > 0 and M % T:
        X = X.copy()
        X[first:M] = X[first - T:M - T]
    return X


# ---- clift_linear_k3_fwd: out (M, Nout) = act(W x4[:, :3] + b)
def _k3f_draw(c, rng):
    T = k3_fwd_blocks(c.M, c.Nout)[1] if k3_fwd_kernel(c.Nout) == "main" else 64
    x = _rows(rng, c.M, 3)
    W, b = gc._nonzero(rng, (c.Nout, 3)), gc._nonzero(rng, (c.Nout,)) * np.float32(0.5)
    return {"x4": _buf(x, c.M + T, 4), "W": _buf(W, c.Nout, 4), "b": b, "out": _out(c.M, c.ldo)}


def _k3f_terms(c, d, dtype):
    x, W, b = d["x4"][:c.M, :3].astype(dtype), d["W"][:, :3].astype(dtype), d["b"].astype(dtype)
    t = np.empty((c.M, c.Nout, 4), dtype)
    t[:, :, 0] = b[None, :]
    for k in range(3):
        t[:, :, k + 1] = x[:, k, None] * W[None, :, k]
    return t


def _k3f_ref(c, d, rows=None):
    t = _k3f_terms(c, d, np.float64)
    v, S = t.sum(2), np.abs(t).sum(2)
    r, s = _image(d["out"].shape)
    r[:c.M, :c.Nout], s[:c.M, :c.Nout] = (np.maximum(v, 0) if c.relu else v), S
    return {"out": (r, s)}


def _k3f_restate(c, d, order, mistake):
    t = _k3f_terms(c, d, np.float32)
    if mistake == "x4_pad_contracted":
        with np.errstate(invalid="ignore"):
            t = np.concatenate([t, (d["x4"][:c.M, 3, None] * d["W"][None, :, 3])[:, :, None]], 2)
    with np.errstate(invalid="ignore"):
        v = gc._ordered_sum(t, order)
        v = np.maximum(v, np.float32(0)) if c.relu else v
    out = d["out"].astype(np.float64)
    out[:c.M, :c.Nout] = v
    return {"out": out}


# ---- clift_linear_k3_bwd: dW (Nout, 3) += dH^T x4[:, :3], db += colsum(dH)
def _k3b_draw(c, rng):
    x, dH = _rows(rng, c.M, 3), _rows(rng, c.M, c.Nout)
    d = {"x4": _buf(x, c.M + 32, 4), "dH": _buf(dH, c.M + 32, c.ldh, c.dh_bf16), "dW": _out(c.Nout, 4), "db": _out(c.Nout, 1) if c.db else None}
    _grad0(rng, d["dW"], d["dH"][:c.M, :c.Nout], x, c.Nout, 3)
    if c.db:
        _grad0(rng, d["db"], d["dH"][:c.M, :c.Nout], np.ones((c.M, 1), np.float32), c.Nout, 1)
    return d


def _reduce_ref(d, M, left, nl, right, nr, out, with_ones=None):
    """out[:nl, :nr] += left[:M, :nl]^T right[:M, :nr] in fp64 with its S; ``with_ones``: the name of the column-sum output."""
    A, B = d[left][:M, :nl].astype(np.float64), d[right][:M, :nr].astype(np.float64)
    res = {}
    r, s = _image(d[out].shape)
    C0 = d[out][:nl, :nr].astype(np.float64)
    r[:nl, :nr], s[:nl, :nr] = A.T @ B + C0, np.abs(A).T @ np.abs(B) + np.abs(C0)
    res[out] = (r, s)
    if with_ones and d.get(with_ones) is not None:
        r, s = _image(d[with_ones].shape)
        b0 = d[with_ones][:nl, 0].astype(np.float64)
        r[:nl, 0], s[:nl, 0] = A.sum(0) + b0, np.abs(A).sum(0) + np.abs(b0)
        res[with_ones] = (r, s)
    return res


def _reduce_restate(c, d, order, mistake, M, T, left, nl, right, nr, out, with_ones=None, split=False):
    """The fp32 restatement of _reduce_ref with the streamed-reduction mistakes.  Output rows past PROBE_PRODUCTS are filled from the
    reference and left out of the yardstick (mask)."""
    A, B = d[left][:, :nl], d[right][:, :nr]
    n = _drop_rows(M, mistake, T)
    if mistake == "row_past_count_reduced":
        n = M + 1
    A, B = A[:n], B[:n]
    if mistake == "ragged_tile_rows_from_previous_tile":
        A, B = _ragged_from_previous(A, M, T), _ragged_from_previous(B, M, T)
    take = _take(nl, n * nr * (4 if split else 1), [0, nl - 1, nl - 2, 1, 3, 4, 7, 8, 31, 32, 255, 256])
    ref = d.get("_ref") or ENTRIES[c.entry].ref(c, d)
    res, mask = {}, {}
    v = _tsum(A, B, order, take, split, mistake == "x6_middle_term_dropped")
    o = ref[out][0].copy()
    o[np.isnan(o)] = d[out].astype(np.float64)[np.isnan(o)]
    C0 = d[out][:nl, :nr]
    tot = v if mistake == "accumulate_overwrites" else (v + C0).astype(np.float32)
    if mistake == "ni_tail_beyond_256_dropped":
        tot[:, 256:] = C0[:, 256:]
    o[take, :nr] = tot[take]
    mk = np.zeros(o.shape, bool)
    mk[take, :nr] = True
    res[out], mask[out] = o, mk
    if with_ones and d.get(with_ones) is not None:
        b = d[with_ones].astype(np.float64)
        with np.errstate(invalid="ignore"):
            s = gc._ordered_sum(np.ascontiguousarray(A.T, dtype=np.float32), order)
        s = s if mistake == "accumulate_overwrites" else (s + d[with_ones][:nl, 0]).astype(np.float32)
        if mistake == "gb_missing_on_last_quad":
            s[nl - (nl % 4 or 4):] = d[with_ones][nl - (nl % 4 or 4):nl, 0]
        b[:nl, 0] = s
        res[with_ones] = b
    res["_mask"] = mask
    return res


def _k3b_ref(c, d, rows=None):
    return _reduce_ref(d, c.M if rows is None else rows, "dH", c.Nout, "x4", 3, "dW", "db")


def _k3b_restate(c, d, order, mistake):
    if mistake == "x4_pad_contracted":                         # the pad column of x4 takes the place of z
        d = dict(d, x4=d["x4"][:, [0, 1, 3, 3]])
    return _reduce_restate(c, d, order, mistake, c.M, 32, "dH", c.Nout, "x4", 3, "dW", "db")


# ---- clift_wgrad_narrow: gW (no, ni) += dY^T X, gb += colsum(dY)
def _wn_draw(c, rng):
    dY, X = _rows(rng, c.M, c.no), _rows(rng, c.M, c.ni)
    d = {"dY": _buf(dY, c.M + 64, c.ldd), "X": _buf(X, c.M + 64, c.ldx, c.x_bf16), "gW": _out(c.no, c.ldw), "gb": _out(c.no, 1) if c.gb else None}
    _grad0(rng, d["gW"], dY, d["X"][:c.M, :c.ni], c.no, c.ni)
    if c.gb:
        _grad0(rng, d["gb"], dY, np.ones((c.M, 1), np.float32), c.no, 1)
    return d


def _wn_ref(c, d, rows=None):
    return _reduce_ref(d, c.M if rows is None else rows, "dY", c.no, "X", c.ni, "gW", "gb")


def _wn_restate(c, d, order, mistake):
    T = NS_ROWS if wgrad_narrow_route(c.M, c.no, c.ni, c.ldd, c.ldx, c.x_bf16)[0] == "stream" else 64
    return _reduce_restate(c, d, order, mistake, c.M, T, "dY", c.no, "X", c.ni, "gW", "gb")


# ---- clift_colsum: db (N) += colsum(dY (M, N))
def _cs_draw(c, rng):
    dY = _rows(rng, c.M, c.N)
    d = {"dY": _buf(dY, c.M + 256, c.ld), "ones": np.ones((c.M + 256, 1), np.float32), "db": _out(c.N, 1)}
    _grad0(rng, d["db"], dY, d["ones"][:c.M], c.N, 1)
    return d


def _cs_ref(c, d, rows=None):
    return _reduce_ref(d, c.M if rows is None else rows, "dY", c.N, "ones", 1, "db")


def _cs_restate(c, d, order, mistake):
    return _reduce_restate(c, d, order, mistake, c.M, 256, "dY", c.N, "ones", 1, "db")


# ---- clift_rows_act_fwd / _bwd: kind 1 sigmoid, 2 softmax over the row (bwd: 0 identity)
SPREAD, SPREAD_TOP = 80.0, 95.0            # exp(95) overflows fp32: a softmax that does not subtract the row maximum returns inf / inf


def _logits(rng, M, C, kind):
    x = (rng.standard_normal((M, C)) * 3).astype(np.float32)
    if kind == 2 and C >= 3:
        for r in range(0, M, 5):             # every fifth row: top, top - 0.5, ... down to top - 80 (the small classes underflow towards e^-80)
            x[r] = np.float32(SPREAD_TOP) - np.float32(SPREAD) * rng.permutation(np.concatenate([[0.0, 0.00625, 1.0], rng.uniform(0.05, 1, C - 3)])).astype(np.float32)
        x[min(2, M - 1)] = np.float32(1.75)   # one row of equal logits
    return x


def _act64(x, kind):
    """(value, S) in fp64."""
    if kind == 1:
        v = 1.0 / (1.0 + np.exp(-x))
        return v, v * (1 + np.abs(x))
    z = x - x.max(1, keepdims=True)
    e = np.exp(z)
    p = e / e.sum(1, keepdims=True)
    return p, p * (1 + np.abs(z))


def _act32(x, kind, order, mistake=None, C4=0):
    f = np.float32
    x = x.astype(f)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == 1:
            return f(1) / (f(1) + np.exp(x if mistake == "sigmoid_of_minus_pre" else -x, dtype=f))
        mx = np.zeros((x.shape[0], 1), f) if mistake == "softmax_without_max" else x.max(1, keepdims=True)
        e = np.exp((x - mx).astype(f), dtype=f)
        s = gc._ordered_sum(e, order)
        if mistake == "softmax_pad_lanes_exp0":
            s = (s + f(C4 - x.shape[1])).astype(f)
        return (e * (f(1) / s)[:, None]).astype(f)


def _raf_draw(c, rng):
    return {"pre": _buf(_logits(rng, c.M, c.C, c.kind), c.M + 8, c.ldp), "out": _out(c.M, c.ldo)}


def _raf_ref(c, d, rows=None):
    v, S = _act64(d["pre"][:c.M, :c.C].astype(np.float64), c.kind)
    r, s = _image(d["out"].shape)
    r[:c.M, :c.C], s[:c.M, :c.C] = v, S
    return {"out": (r, s)}


def _raf_restate(c, d, order, mistake):
    out = d["out"].astype(np.float64)
    out[:c.M, :c.C] = _act32(d["pre"][:c.M, :c.C], c.kind, order, mistake, r4(c.C))
    return {"out": out}


def _rab_draw(c, rng):
    x = _logits(rng, c.M, c.C, c.kind)
    o = _act64(x.astype(np.float64), c.kind)[0].astype(np.float32) if c.kind else np.zeros_like(x)
    return {"out": _buf(o, c.M + 8, c.ldo), "dout": _buf(_rows(rng, c.M, c.C), c.M + 8, c.lddo), "dpre": _out(c.M, c.ldd)}


def _rab_ref(c, d, rows=None):
    o, g = d["out"][:c.M, :c.C].astype(np.float64), d["dout"][:c.M, :c.C].astype(np.float64)
    if c.kind == 0:
        v, S = g, np.abs(g)
    elif c.kind == 1:
        v = g * o * (1 - o)
        S = np.abs(v)
    else:
        v, S = o * (g - (g * o).sum(1, keepdims=True)), o * (np.abs(g) + np.abs(g * o).sum(1, keepdims=True))
    r, s = _image(d["dpre"].shape)
    r[:c.M, :c.ldd], s[:c.M, :c.ldd] = 0.0, 0.0          # the alignment padding [C, ldd) is written, as zeros: it is a GEMM operand
    r[:c.M, :c.C], s[:c.M, :c.C] = v, S
    return {"dpre": (r, s)}


def _rab_restate(c, d, order, mistake):
    f = np.float32
    o, g = d["out"][:c.M, :c.C], d["dout"][:c.M, :c.C]
    if c.kind == 0:
        v = g
    elif c.kind == 1:
        v = ((g * o).astype(f) * (f(1) - o)).astype(f)
    else:
        go = (g * o).astype(f)
        dot = gc._ordered_sum(go[:, :c.C - 1] if mistake == "softmax_bwd_dot_over_c_minus_1" else go, order)
        v = (o * (g - dot[:, None]).astype(f)).astype(f)
    out = d["dpre"].astype(np.float64)
    if not (mistake == "identity_pad_columns_unwritten" and c.kind == 0):
        out[:c.M, :c.ldd] = 0.0
    out[:c.M, :c.C] = v
    return {"dpre": out}


# ---- clift_out_layer_fwd: out (M, no) = act(H W^T + b) over a 256-wide hidden activation, act 2 = softmax over the row
def _of_draw(c, rng):
    H = np.maximum(_rows(rng, c.M, 256), 0)                                            # a ReLU activation: about half of it zeros
    H[:, np.all(H == 0, 0)] = 1.0
    if c.act == 2:
        H *= np.float32(2.0 ** -6)                                                      # rows of scale 2^-12 .. 1: logits of a few units, no class saturates
    W = gc._nonzero(rng, (c.no, 256)) * np.exp2(rng.integers(-2, 3, (c.no, 1))).astype(np.float32) / np.float32(16)
    return {"H": _buf(H, c.M + OF_ROWS, c.ldh), "W": _buf(W, c.no + 2, c.ldw), "b": gc._nonzero(rng, (c.no,)), "out": _out(c.M, c.ldo)}


def _of_ref(c, d, rows=None):
    H, W, b = d["H"][:c.M, :256].astype(np.float64), d["W"][:c.no, :256].astype(np.float64), d["b"].astype(np.float64)
    x, Sx = H @ W.T + b, np.abs(H) @ np.abs(W).T + np.abs(b)
    if c.act == 2:
        p, Sp = _act64(x, 2)
        x, Sx = p, Sp + p * (Sx + Sx.max(1, keepdims=True))
    r, s = _image(d["out"].shape)
    r[:c.M, :c.no], s[:c.M, :c.no] = x, Sx
    return {"out": (r, s)}


def _of_restate(c, d, order, mistake):
    f = np.float32
    rows = _take(c.M, c.no * 257, [0, c.M - 1, ((c.M - 1) // OF_ROWS) * OF_ROWS, OF_ROWS - 1, OF_ROWS, c.M - 2, 2 * OF_ROWS, 1])
    Hs = _ragged_from_previous(d["H"], c.M, OF_ROWS) if mistake == "ragged_tile_rows_from_previous_tile" else d["H"]
    H, W, b = Hs[rows, :256], d["W"][:c.no, :256], d["b"]
    if mistake == "column_group_share_dropped":
        H = H.copy()
        H[:, 192:] = 0
    if mistake == "out_bias_added_per_column_group":
        b = (b * f(4)).astype(f)
    prod = H[:, None, :] * W[None, :, :]
    x = gc._ordered_sum(np.concatenate([np.broadcast_to(b[None, :, None], prod.shape[:2] + (1,)), prod], 2), order)
    if c.act == 2:
        x = _act32(x, 2, order)
    out = d["out"].astype(np.float64)
    out[rows, :c.no] = x
    if mistake == "columns_no_ldo_written":
        out[rows, c.no:] = 0.0
    mk = np.zeros(out.shape, bool)
    mk[rows, :c.no] = True
    ref = (d.get("_ref") or _of_ref(c, d))["out"][0]
    rest = np.setdiff1d(np.arange(c.M), rows)
    out[rest, :c.no] = ref[rest, :c.no]
    return {"out": out, "_mask": {"out": mk}}


# ---- clift_out_layer_bwd / _bwd_nh / _bwd_n128_bf16: dX = (H > 0) . (dOut W), gW += dOut^T H, gb += colsum(dOut) in one pass over H
H_SPECIALS = gc.MASK_SPECIALS[:4]          # +0, -0, +-denormal.  (+inf is left out: H is also an OPERAND of gW here, where it would make the sum inf - inf)


def ob_kind(c):
    """(T, blocks per CU, dOut pad columns: "zero" as the header demands of the narrow dgrad stream / "nan": ignored by contract)."""
    return (16, 4, "nan") if c.entry == "clift_out_layer_bwd_n128_bf16" else (NS_ROWS, 1, "zero")


def _ob_draw(c, rng):
    T, _, pad = ob_kind(c)
    dOut = _rows(rng, c.M, c.no)
    W = gc._nonzero(rng, (c.no, c.nh)) * np.exp2(rng.integers(-2, 3, (c.no, 1))).astype(np.float32)
    H = gc._nonzero(rng, (c.M, c.nh))
    flat = H.reshape(-1)
    for j, v in enumerate(H_SPECIALS):
        flat[j::11 + j] = np.float32(v)
    H[:, np.all(H == 0, 0)] = 0.5
    d = {"dOut": _buf(dOut, c.M + T, c.ldd), "W": _buf(W, c.no + 2, c.nh + 4), "H": _buf(H, c.M + T, c.ldh, c.h_bf16),
         "dX": _out(c.M, c.ldx), "gW": _out(c.no, c.nh + 4), "gb": _out(c.no, 1) if c.gb else None}
    if pad == "zero":
        d["dOut"][:c.M, c.no:] = 0.0
    _grad0(rng, d["gW"], dOut, d["H"][:c.M, :c.nh], c.no, c.nh)
    if c.gb:
        _grad0(rng, d["gb"], dOut, np.ones((c.M, 1), np.float32), c.no, 1)
    return d


def _ob_ref(c, d, rows=None):
    res = _reduce_ref(d, c.M if rows is None else rows, "dOut", c.no, "H", c.nh, "gW", "gb")
    dO, W, H = d["dOut"][:c.M, :c.no].astype(np.float64), d["W"][:c.no, :c.nh].astype(np.float64), d["H"][:c.M, :c.nh]
    r, s = _image(d["dX"].shape)
    r[:c.M, :c.nh], s[:c.M, :c.nh] = np.where(H > 0, dO @ W, 0.0), np.abs(dO) @ np.abs(W)
    res["dX"] = (r, s)
    return res


def _ob_restate(c, d, order, mistake):
    T = ob_kind(c)[0]
    res = _reduce_restate(c, d, order, mistake if mistake != "dout_pad_column_contracted" else None, c.M, T, "dOut", c.no, "H", c.nh, "gW", "gb")
    f = np.float32
    if mistake == "gb_from_masked_dout" and c.gb:
        masked = np.where(d["H"][:c.M, :c.no] > 0, d["dOut"][:c.M, :c.no], f(0))
        res["gb"][:c.no, 0] = (gc._ordered_sum(np.ascontiguousarray(masked.T), order) + d["gb"][:c.no, 0]).astype(f)
    rows = _take(c.M, c.nh * c.no, [0, c.M - 1, ((c.M - 1) // T) * T, T - 1, T, c.M - 2, 2 * T, 1])
    src = _ragged_from_previous(d["dOut"], c.M, T) if mistake == "ragged_tile_rows_from_previous_tile" else d["dOut"]
    k = c.no + (1 if mistake == "dout_pad_column_contracted" else 0)
    with np.errstate(invalid="ignore"):
        v = gc._ordered_sum(src[rows, None, :k] * np.ascontiguousarray(d["W"][:k, :c.nh].T)[None, :, :], order)
    Hp = d["H"][rows, :c.nh]
    v = np.where((Hp >= 0) if mistake == "mask_ge" else (Hp > 0), v, f(0))
    ref = (d.get("_ref") or _ob_ref(c, d))["dX"][0]
    out = d["dX"].astype(np.float64)
    out[:c.M, :c.nh] = ref[:c.M, :c.nh]
    out[rows, :c.nh] = v
    mk = np.zeros(out.shape, bool)
    mk[rows, :c.nh] = True
    res["dX"] = out
    res["_mask"]["dX"] = mk
    return res


# ---- the fused forwards in exact fp32: clift_xyz_head_first2_fwd (K = 3 layer + 256 x 256), clift_xyz_head_last2_fwd (256 x 256 + E outputs),
# clift_app_head_last2_fwd (128 x 128 + E outputs + sigmoid).  S of a second layer's sum takes the first layer's S for its inputs' magnitudes
# (S_h >= h), so the bound covers what the first layer's round-off does to the second; a sigmoid on top: S = out (1 + |pre| + S_pre).
LF_ROWS = source_constant("layer_f32.hip", "LF_ROWS")
LN_ROWS = source_constant("layer_n128.hip", "LN_ROWS")


def _layer64(A, W, b, S_A=None):
    A, W, b = A.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    return A @ W.T + b, (np.abs(A) if S_A is None else S_A) @ np.abs(W).T + np.abs(b)


def _layer32(A, W, b, order, bias_times=1, split=False, drop_middle=False):
    """act-less layer in fp32, one running sum per output with the bias a term of it; split: fp32x6 products."""
    f = np.float32
    A3, W3 = np.ascontiguousarray(A, dtype=f)[:, None, :], np.ascontiguousarray(W, dtype=f)[None, :, :]
    with np.errstate(invalid="ignore"):
        prod = _six(*np.broadcast_arrays(A3, W3), drop_middle) if split else A3 * W3
    bb = (b * f(bias_times)).astype(f)
    with np.errstate(invalid="ignore"):
        return gc._ordered_sum(np.concatenate([np.broadcast_to(bb[None, :, None], prod.shape[:2] + (1,)), prod], 2), order)


X6_ROWS = source_constant("layer_x6.hip", "X6_ROWS")
XW_ROWS = source_constant("layer_x6w.hip", "XW_ROWS")
N6_ROWS = source_constant("layer_n6.hip", "N6_ROWS")
X6 = ("clift_xyz_head_first2_x6_fwd", "clift_xyz_head_last2_x6_fwd", "clift_app_head_last2_x6_fwd", "clift_xyz_head_first2_x6_bwd", "clift_xyz_head_first2_x6_wgrad")


def m3_x6(first=1):
    """m3_rows for k_layer_x6: one row range per PAIR of CUs (csrc/layer_x6.hip)."""
    rows = first
    while True:
        nranges = min(cdiv(rows, X6_ROWS), (CUS - RESERVE) // 2)
        rpr = cdiv(cdiv(rows, nranges), X6_ROWS) * X6_ROWS
        if rpr >= 3 * X6_ROWS and (rows - (cdiv(rows, rpr) - 1) * rpr) % X6_ROWS != 0:
            return rows
        rows += 1


def m3_fixed(ranges, T):
    """... for a launcher that cuts the rows into a fixed number of ranges (the 64 x 4 quadrant weight gradient; a quarter of the CUs for fp32x6)."""
    rows = 1
    while True:
        rpr = cdiv(cdiv(rows, ranges), T) * T
        if rpr >= 3 * T and (rows - (cdiv(rows, rpr) - 1) * rpr) % T != 0:
            return rows
        rows += 1


def l2_kind(c):
    """(hidden width, T)."""
    return {"clift_app_head_last2_fwd": (128, LN_ROWS), "clift_app_head_last2_x6_fwd": (128, N6_ROWS), "clift_xyz_head_last2_x6_fwd": (256, X6_ROWS),
            "clift_app_head_last2_bf16_fwd": (128, 64)}.get(c.entry, (256, LF_ROWS))


def _l2_draw(c, rng):
    n, T = l2_kind(c)
    A = _rows(rng, c.M, n) * np.float32(2.0 ** -6 if c.p.get("sigmoid") else 1.0)          # (sigmoid: pre-activations of a few units, none saturates)
    W = gc._nonzero(rng, (n, n)) * np.exp2(rng.integers(-2, 3, (n, 1))).astype(np.float32) / np.float32(n ** 0.5)
    Wout = gc._nonzero(rng, (c.E, n)) / np.float32(n ** 0.5)
    d = {"A": _buf(A, c.M + T, c.lda), "W": _buf(W, n, n + 4), "b": gc._nonzero(rng, (n,)) * np.float32(0.25), "Wout": _buf(Wout, c.E, n + 4),
         "bout": gc._nonzero(rng, (c.E,)), "hidden": _out(c.M, c.ldh) if c.hid else None, "out": _out(c.M, c.ldo)}
    if "pre" in c.p:
        d["pre"] = _out(c.M, c.ldo + 1) if c.pre else None
    return d


def _l2_ref(c, d, rows=None):
    n, _ = l2_kind(c)
    h, Sh = _layer64(d["A"][:c.M, :n], d["W"][:, :n], d["b"])
    h = np.maximum(h, 0)
    pre, Sp = _layer64(h, d["Wout"][:, :n], d["bout"], Sh)
    res = {}
    if d.get("hidden") is not None:
        r, s = _image(d["hidden"].shape)
        r[:c.M, :n], s[:c.M, :n] = h, Sh
        res["hidden"] = (r, s)
    if d.get("pre") is not None:
        r, s = _image(d["pre"].shape)
        r[:c.M, :c.E], s[:c.M, :c.E] = pre, Sp
        res["pre"] = (r, s)
    r, s = _image(d["out"].shape)
    if c.p.get("sigmoid"):
        o = 1.0 / (1.0 + np.exp(-pre))
        r[:c.M, :c.E], s[:c.M, :c.E] = o, o * (1 + np.abs(pre) + Sp)
    else:
        r[:c.M, :c.E], s[:c.M, :c.E] = pre, Sp
    res["out"] = (r, s)
    return res


def _l2_restate(c, d, order, mistake):
    f = np.float32
    n, T = l2_kind(c)
    rows = _take(c.M, n * n * (4 if c.entry in X6 else 1), [0, c.M - 1, ((c.M - 1) // T) * T, T - 1, T, c.M - 2, 2 * T, 1])
    A = (_ragged_from_previous(d["A"], c.M, T) if mistake == "ragged_tile_rows_from_previous_tile" else d["A"])[rows, :n]
    z = _layer32(A, d["W"][:, :n], d["b"], order, split=c.entry in X6, drop_middle=mistake == "x6_middle_term_dropped")
    h = np.maximum(z, f(0))
    ho = z if mistake == "relu_missing_before_output_layer" else h
    if mistake == "column_group_share_dropped":
        ho = ho.copy()
        ho[:, 3 * n // 4:] = 0
    bout = np.full_like(d["bout"], d["bout"][0]) if mistake == "bout_of_column_0_for_all" else d["bout"]
    pre = _layer32(ho, d["Wout"][:, :n], bout, order, 4 if mistake == "out_bias_added_per_column_group" else 1)
    ref = d.get("_ref") or _l2_ref(c, d)
    res, mask = {}, {}

    def put(q, v, cols):
        o = d[q].astype(np.float64)
        o[:c.M, :cols] = ref[q][0][:c.M, :cols]
        o[rows, :cols] = v
        mk = np.zeros(o.shape, bool)
        mk[rows, :cols] = True
        res[q], mask[q] = o, mk

    if d.get("hidden") is not None:
        put("hidden", z if mistake == "hidden_stored_before_relu" else h, n)
    if d.get("pre") is not None:
        put("pre", pre, c.E)
    with np.errstate(over="ignore"):
        put("out", (f(1) / (f(1) + np.exp(pre if mistake == "sigmoid_of_minus_pre" else -pre, dtype=f))) if c.p.get("sigmoid") else pre, c.E)
    if mistake == "columns_no_ldo_written":
        res["out"][rows, c.E:] = 0.0
    res["_mask"] = mask
    return res


def _f2_draw(c, rng):
    x = _rows(rng, c.M, 3)
    W0, b0 = gc._nonzero(rng, (256, 3)), gc._nonzero(rng, (256,)) * np.float32(0.5)
    W1 = gc._nonzero(rng, (256, 256)) * np.exp2(rng.integers(-2, 3, (256, 1))).astype(np.float32) / np.float32(16)
    return {"x4": _buf(x, c.M + LF_ROWS, 4), "W0": _buf(W0, 256, 4), "b0": b0, "W1": _buf(W1, 256, 260), "b1": gc._nonzero(rng, (256,)),
            "h1": _out(c.M, c.ldh1) if c.p.get("h1") else None, "h2": _out(c.M, c.ldh2)}


def _f2_terms(d, M, dtype):
    x, W, b = d["x4"][:M, :3].astype(dtype), d["W0"][:, :3].astype(dtype), d["b0"].astype(dtype)
    return np.stack([np.broadcast_to(b[None, :], (M, 256))] + [x[:, k, None] * W[None, :, k] for k in range(3)], 2)


def _f2_ref(c, d, rows=None):
    t = _f2_terms(d, c.M, np.float64)
    h1, S1 = np.maximum(t.sum(2), 0), np.abs(t).sum(2)
    h2, S2 = _layer64(h1, d["W1"][:, :256], d["b1"], S1)
    res = {}
    if d.get("h1") is not None:
        r, s = _image(d["h1"].shape)
        r[:c.M, :256], s[:c.M, :256] = h1, S1
        res["h1"] = (r, s)
    r, s = _image(d["h2"].shape)
    r[:c.M, :256], s[:c.M, :256] = np.maximum(h2, 0), S2
    res["h2"] = (r, s)
    return res


def f2_pre(c):
    """(fp64 pre-activation of the second layer, its S): what the sign bytes of clift_xyz_head_first2_x6_fwd record the sign of."""
    d = inputs(c)
    t = _f2_terms(d, c.M, np.float64)
    return _layer64(np.maximum(t.sum(2), 0), d["W1"][:, :256], d["b1"], np.abs(t).sum(2))


def sign_unsure(c):
    """The elements of a first2_x6_fwd case whose reference pre-activation lies within its own bound of zero: their sign byte may say either,
    and the sign-byte comparison leaves them out (at most SIGN_CAP of a case; the host test counts them)."""
    pre, Sp = f2_pre(c)
    return np.abs(pre) <= factor_for(c, "h2") * Sp


SIGN_CAP = 1e-3


def _f2_restate(c, d, order, mistake):
    f = np.float32
    t = _f2_terms(d, c.M, f)
    if mistake == "x4_pad_contracted":
        with np.errstate(invalid="ignore"):
            t = np.concatenate([t, (d["x4"][:c.M, 3, None] * d["W0"][None, :, 3])[:, :, None]], 2)
    with np.errstate(invalid="ignore"):
        h1 = np.maximum(gc._ordered_sum(t, order), f(0))
    T = LF_ROWS
    rows = _take(c.M, 256 * 256 * (4 if c.entry in X6 else 1), [0, c.M - 1, ((c.M - 1) // T) * T, T - 1, T, c.M - 2, 2 * T, 1])
    src = _ragged_from_previous(h1, c.M, T) if mistake == "ragged_tile_rows_from_previous_tile" else h1
    h2 = np.maximum(_layer32(src[rows], d["W1"][:, :256], d["b1"], order, split=c.entry in X6, drop_middle=mistake == "x6_middle_term_dropped"), f(0))
    ref = d.get("_ref") or _f2_ref(c, d)
    res, mask = {}, {}
    if d.get("h1") is not None:
        o = d["h1"].astype(np.float64)
        o[:c.M, :256] = h1
        res["h1"] = o
    o = d["h2"].astype(np.float64)
    o[:c.M, :256] = ref["h2"][0][:c.M, :256]
    o[rows, :256] = h2
    mk = np.zeros(o.shape, bool)
    mk[rows, :256] = True
    res["h2"], mask["h2"] = o, mk
    res["_mask"] = mask
    return res



# ---- the backward ends of an xyz head's first two layers: clift_xyz_head_first2_bwd / _x6_bwd (gW0, gb0 through the re-derived first-layer
# sign) and clift_xyz_head_first2_wgrad / _x6_wgrad (gW1, gb1 over the regenerated first activation).  The sign of
# fmaf(w2, z, fmaf(w1, y, fmaf(w0, x, b))) is discontinuous and declared bit-faithful, so W0, b0 and the positions are DYADIC: multiples of 1/8
# (the positions times a power of two per row), every product and partial sum of the chain exact in fp32.  The pre-activation is then the
# same number in fp32, in fp64 and on the device: never within round-off of zero, and exactly zero where the draw makes it so.
# Hidden units 0 .. 3 are hand-built: pre = 0 everywhere (zero row of W0, b0 = 0); 0.5 * 1 + (-0.25) * 2 = 0 at row 0; the smallest positive
# normal 2^-126 at row 0 (the weight-gradient forms, where the first ACTIVATION is an operand and not only a sign, take 2^-60: products in the
# denormal range lose bits in any fp32 arithmetic, which is not what this unit is for); -0.
K3_SPECIAL = 4


def _dyadic_k3(rng, M, T, tiny=2.0 ** -126):
    q = lambda shape, s: np.where((r := np.round(rng.standard_normal(shape) * s) / 8) == 0, 0.125, r).astype(np.float32)
    x = q((M, 3), 8) * np.exp2(rng.integers(-6, 7, (M, 1))).astype(np.float32)
    W0, b0 = q((256, 3), 8), q((256,), 4)
    x[0] = (1.0, 2.0, -0.375)
    W0[0], b0[0] = 0.0, 0.0
    W0[1], b0[1] = (0.5, -0.25, 0.0), 0.0
    W0[2], b0[2] = (tiny, 0.0, 0.0), 0.0
    W0[3], b0[3] = (-0.0, -0.0, 0.0), -0.0                 # row 0 = (1, 2, -0.375): every product and the bias are -0
    return {"x4": _buf(x, M + T, 4), "W0": _buf(W0, 256, 4), "b0": b0}


def k3_pre(d, M, dtype=np.float32):
    """The first layer's pre-activation as the fmaf chain forms it (exact for the dyadic draws, whatever the dtype)."""
    x, W, b = d["x4"][:M, :3].astype(dtype), d["W0"][:, :3].astype(dtype), d["b0"].astype(dtype)
    return ((b[None, :] + x[:, 0, None] * W[None, :, 0]) + x[:, 1, None] * W[None, :, 1]) + x[:, 2, None] * W[None, :, 2]


def fb_T(c):
    return {"clift_xyz_head_first2_bwd": LF_ROWS, "clift_xyz_head_first2_x6_bwd": X6_ROWS, "clift_xyz_head_first2_wgrad": 64, "clift_xyz_head_first2_x6_wgrad": XW_ROWS}[c.entry]


def _fb_draw(c, rng):
    T = fb_T(c)
    d = _dyadic_k3(rng, c.M, T)
    dH2 = _rows(rng, c.M, 256)
    W1 = gc._nonzero(rng, (256, 256)) * np.exp2(rng.integers(-2, 3, (256, 1))).astype(np.float32) / np.float32(16)
    d.update({"dH2": _buf(dH2, c.M + T, c.ldd), "W1": _buf(W1, 256, 260), "gW0": _out(256, 4), "gb0": _out(256, 1)})
    on = (k3_pre(d, c.M) > 0).astype(np.float32)
    rms = np.sqrt((dH2.astype(np.float64) ** 2) @ (W1.astype(np.float64) ** 2)) * on          # the size of dH1
    x = d["x4"][:c.M, :3]
    d["gW0"][:256, :3] = (rng.standard_normal((256, 3)) * np.sqrt((rms ** 2).T @ (x.astype(np.float64) ** 2))).astype(np.float32)
    d["gb0"][:256, 0] = (rng.standard_normal(256) * np.sqrt((rms ** 2).sum(0))).astype(np.float32)
    return d


def _fb_ref(c, d, rows=None):
    M = c.M if rows is None else rows
    on = k3_pre(d, M, np.float64) > 0
    dH2, W1, x = d["dH2"][:M, :256].astype(np.float64), d["W1"][:, :256].astype(np.float64), d["x4"][:M, :3].astype(np.float64)
    dH1, S1 = np.where(on, dH2 @ W1, 0.0), np.where(on, np.abs(dH2) @ np.abs(W1), 0.0)
    res = {}
    for q, v, S in (("gW0", dH1.T @ x, S1.T @ np.abs(x)), ("gb0", dH1.sum(0)[:, None], S1.sum(0)[:, None])):
        r, s = _image(d[q].shape)
        n = v.shape[1]
        C0 = d[q][:256, :n].astype(np.float64)
        r[:256, :n], s[:256, :n] = v + C0, S + np.abs(C0)
        res[q] = (r, s)
    return res


def _fb_restate(c, d, order, mistake):
    f = np.float32
    T, M = fb_T(c), c.M
    n = _drop_rows(M, mistake, T) + (1 if mistake == "row_past_count_reduced" else 0)
    with np.errstate(invalid="ignore"):
        pre = k3_pre(d, n)
        if mistake == "first_layer_sign_without_b0":
            pre = k3_pre(dict(d, b0=np.zeros_like(d["b0"])), n)
    units = _take(256, n * 256 * (4 if c.entry in X6 else 1), [0, 1, 2, 3, 255, 4, 31, 32, 128, 127])
    dH2, x = d["dH2"][:n, :256], d["x4"][:n, [0, 1, 3] if mistake == "x4_pad_contracted" else [0, 1, 2]]
    if mistake == "ragged_tile_rows_from_previous_tile":
        dH2, x, pre = _ragged_from_previous(dH2, M, T), _ragged_from_previous(x, M, T), _ragged_from_previous(pre, M, T)
    W1u = np.ascontiguousarray(d["W1"][:, units].T)                                   # (units, 256)
    with np.errstate(invalid="ignore"):
        prod = dH2[:, None, :] * W1u[None, :, :] if c.entry not in X6 else _six(*np.broadcast_arrays(dH2[:, None, :], W1u[None, :, :]), mistake == "x6_middle_term_dropped")
        dH1 = gc._ordered_sum(prod, order)                                             # (n, units)
    on = pre[:, units]
    on = {"mask_ge": on >= 0, "mask_from_second_layer": dH2[:, units] > 0}.get(mistake, on > 0)
    dH1 = np.where(on, dH1, f(0))
    ref = d.get("_ref") or _fb_ref(c, d)
    res, mask = {}, {}
    with np.errstate(invalid="ignore"):
        sums = {"gW0": gc._ordered_sum(np.ascontiguousarray((dH1[:, :, None] * x[:, None, :]).transpose(1, 2, 0)), order),
                "gb0": gc._ordered_sum(np.ascontiguousarray(dH1.T), order)[:, None]}
    for q, v in sums.items():
        cols = v.shape[1]
        o = ref[q][0].copy()
        o[np.isnan(o)] = d[q].astype(np.float64)[np.isnan(o)]
        C0 = d[q][units, :cols]
        tot = v if mistake == "accumulate_overwrites" else (v + C0).astype(f)
        if mistake == "gb_missing_on_last_quad" and q == "gb0":
            tot = np.where((units >= 252)[:, None], C0, tot)
        o[units, :cols] = tot
        mk = np.zeros(o.shape, bool)
        mk[units, :cols] = True
        res[q], mask[q] = o, mk
    res["_mask"] = mask
    return res


def _fw_draw(c, rng):
    T = fb_T(c)
    d = _dyadic_k3(rng, c.M, T, 2.0 ** -60)
    dH2 = _rows(rng, c.M, 256)
    d.update({"dH2": _buf(dH2, c.M + T, c.ldd), "gW1": _out(256, c.ldg), "gb1": _out(256, 1) if c.gb else None})
    d["_h1"] = np.full((c.M + T, 256), np.nan, np.float32)
    d["_h1"][:c.M] = np.maximum(k3_pre(d, c.M), 0)
    _grad0(rng, d["gW1"], dH2, d["_h1"][:c.M], 256, 256)
    if c.gb:
        _grad0(rng, d["gb1"], dH2, np.ones((c.M, 1), np.float32), 256, 1)
    return d


def _fw_ref(c, d, rows=None):
    return _reduce_ref(d, c.M if rows is None else rows, "dH2", 256, "_h1", 256, "gW1", "gb1")


def _fw_restate(c, d, order, mistake):
    if mistake in ("first_layer_sign_without_b0", "x4_pad_contracted"):
        h = d["_h1"].copy()
        with np.errstate(invalid="ignore"):
            if mistake == "x4_pad_contracted":
                h[:c.M] = np.maximum(k3_pre(dict(d, x4=d["x4"][:, [0, 1, 3, 3]]), c.M), 0)
            else:
                h[:c.M] = np.where(k3_pre(dict(d, b0=np.zeros_like(d["b0"])), c.M) > 0, k3_pre(d, c.M), 0)
        d = dict(d, _h1=h)
    return _reduce_restate(c, d, order, mistake, c.M, fb_T(c), "dH2", 256, "_h1", 256, "gW1", "gb1", split=c.entry in X6)



# ---- clift_app_head_last2_bf16_fwd: a chain of bf16 roundings.  hidden = bf16(relu(bf16(A) bf16(W)^T + b)) is held to the fp64 reference with the
# bf16 allowance; the output layer reads the STORED hidden, and a hidden value at a rounding boundary may land on either neighbour, which the
# output layer amplifies beyond any yardstick -- so `out` is held to the fp64 output layer over the hidden activation that was actually
# stored ("_chain": the device's own, or the restatement's own), and a launch that does not store it must give the bits of one that does.
NB_ROWS = source_constant("layer_nb16.hip", "NB_ROWS")
CHAINED = ("clift_app_head_last2_bf16_fwd",)


def _lb_draw(c, rng):
    A = _rows(rng, c.M, 128) * np.float32(2.0 ** -6 if c.sigmoid else 1.0)
    W = gc._nonzero(rng, (128, 128)) * np.exp2(rng.integers(-2, 3, (128, 1))).astype(np.float32) / np.float32(128 ** 0.5)
    Wout = gc._nonzero(rng, (c.E, 128)) / np.float32(128 ** 0.5)
    return {"A": _buf(A, c.M + NB_ROWS, c.lda, True), "W": _buf(W, 128, 132), "b": gc._nonzero(rng, (128,)) * np.float32(0.25), "Wout": _buf(Wout, c.E, 132),
            "bout": gc._nonzero(rng, (c.E,)), "hidden": _out(c.M, c.ldh) if c.hid else None, "out": _out(c.M, c.ldo)}


def _lb_ref(c, d, rows=None, chain=None):
    if "_h64" not in d:
        h, Sh = _layer64(d["A"][:c.M, :128], bf16r(d["W"][:, :128]), d["b"])
        d["_h64"] = (np.maximum(h, 0), Sh)
    h, Sh = d["_h64"]
    hs = bf16r(h) if chain is None else chain
    pre, Sp = _layer64(hs, d["Wout"][:, :128], d["bout"])
    res = {}
    if d.get("hidden") is not None:
        r, s = _image(d["hidden"].shape)
        r[:c.M, :128], s[:c.M, :128] = h, Sh
        res["hidden"] = (r, s)
    r, s = _image(d["out"].shape)
    o = 1.0 / (1.0 + np.exp(-pre))
    r[:c.M, :c.E], s[:c.M, :c.E] = (o, o * (1 + np.abs(pre) + Sp)) if c.sigmoid else (pre, Sp)
    res["out"] = (r, s)
    if chain is not None:                    # the stored hidden itself, wherever it was read from, against its own reference
        res["_chain"] = (h, Sh)
    return res


def _lb_restate(c, d, order, mistake):
    f = np.float32
    T = NB_ROWS
    rows = _take(c.M, 128 * 128, [0, c.M - 1, ((c.M - 1) // T) * T, T - 1, T, c.M - 2, 2 * T, 1])
    A = (_ragged_from_previous(d["A"], c.M, T) if mistake == "ragged_tile_rows_from_previous_tile" else d["A"])[rows, :128]
    z = _layer32(A, bf16r(d["W"][:, :128]), d["b"], order)
    h = np.maximum(z, f(0))
    hs = bf16r(h)
    ho = h if mistake == "bf16_hidden_rounded_after_output_layer" else (z if mistake == "relu_missing_before_output_layer" else hs)
    if mistake == "column_group_share_dropped":
        ho = ho.copy()
        ho[:, 96:] = 0
    bout = np.full_like(d["bout"], d["bout"][0]) if mistake == "bout_of_column_0_for_all" else d["bout"]
    pre = _layer32(ho, d["Wout"][:, :128], bout, order, 4 if mistake == "out_bias_added_per_column_group" else 1)
    if "_chain0" not in d:
        _lb_ref(c, d)
        d["_chain0"] = bf16r(d["_h64"][0]).astype(np.float64)
    chain = d["_chain0"].copy()
    chain[rows] = hs
    ref = _lb_ref(c, d, chain=chain)
    res, mask = {"_chain": chain}, {}

    def put(q, v, cols):
        o = d[q].astype(np.float64)
        o[:c.M, :cols] = ref[q][0][:c.M, :cols]
        o[rows, :cols] = v
        mk = np.zeros(o.shape, bool)
        mk[rows, :cols] = True
        res[q], mask[q] = o, mk

    if d.get("hidden") is not None:
        put("hidden", z if mistake == "hidden_stored_before_relu" else h, 128)
    with np.errstate(over="ignore"):
        put("out", (f(1) / (f(1) + np.exp(pre if mistake == "sigmoid_of_minus_pre" else -pre, dtype=f))) if c.sigmoid else pre, c.E)
    if mistake == "columns_no_ldo_written":
        res["out"][rows, c.E:] = 0.0
    res["_mask"] = mask
    return res



# ---- clift_xyz_head_first2_bf16_bwd: gW0 += ((h1 > 0) . bf16(dH2 W1))^T x4[:, :3], gb0 += its column sums.  include/clift.h: the second layer's
# input gradient is "formed, rounded to bf16 and masked exactly as clift_gemm would store it", so the sums are held over the bf16 dH1 that was
# actually stored ("_chain": on the device, what the LAYER_BF16 masked dgrad of clift_gemm writes for the same operands), and that dH1 to its
# own fp64 reference with the bf16 allowance.  h1 is an input: a mask with +-0, +-denormals and +inf (gemm_cases.MASK_SPECIALS), NaN-free.
LY_ROWS = source_constant("layer_bf16.hip", "LY_ROWS")
HB_ROWS = source_constant("head_bf16.hip", "HB_ROWS")
HB_XROWS = source_constant("head_bf16.hip", "HB_XROWS")
CHAINED = CHAINED + ("clift_xyz_head_first2_bf16_bwd", "clift_xyz_head_bf16_fwd")


def _bb_draw(c, rng):
    T = LY_ROWS
    x, dH2 = _rows(rng, c.M, 3), _rows(rng, c.M, 256)
    W1 = gc._nonzero(rng, (256, 256)) * np.exp2(rng.integers(-2, 3, (256, 1))).astype(np.float32) / np.float32(16)
    h1 = gc._nonzero(rng, (c.M, 256))
    flat = h1.reshape(-1)
    for j, v in enumerate(gc.MASK_SPECIALS):
        flat[j::11 + j] = np.float32(v)
    d = {"x4": _buf(x, c.M + T, 4), "dH2": _buf(dH2, c.M + T, c.ldd, True), "W1": _buf(W1, 256, 260), "h1": _buf(h1, c.M + T, c.ldm, True),
         "gW0": _out(256, 4), "gb0": _out(256, 1)}
    rms = np.sqrt((d["dH2"][:c.M, :256].astype(np.float64) ** 2) @ (W1.astype(np.float64) ** 2)) * (d["h1"][:c.M, :256] > 0)
    d["gW0"][:256, :3] = (rng.standard_normal((256, 3)) * np.sqrt((rms ** 2).T @ (x.astype(np.float64) ** 2))).astype(np.float32)
    d["gb0"][:256, 0] = (rng.standard_normal(256) * np.sqrt((rms ** 2).sum(0))).astype(np.float32)
    return d


def _bb_dh1(c, d):
    if "_dh1" not in d:
        on = d["h1"][:c.M, :256] > 0
        dH2, W1 = d["dH2"][:c.M, :256].astype(np.float64), bf16r(d["W1"][:, :256]).astype(np.float64)
        d["_dh1"] = (np.where(on, dH2 @ W1, 0.0), np.where(on, np.abs(dH2) @ np.abs(W1), 0.0))
    return d["_dh1"]


def _bb_ref(c, d, rows=None, chain=None):
    M = c.M if rows is None else rows
    v1, S1 = _bb_dh1(c, d)
    ch = (bf16r(v1).astype(np.float64) if chain is None else np.asarray(chain, dtype=np.float64))[:M]
    x = d["x4"][:M, :3].astype(np.float64)
    res = {}
    for q, v, S in (("gW0", ch.T @ x, np.abs(ch).T @ np.abs(x)), ("gb0", ch.sum(0)[:, None], np.abs(ch).sum(0)[:, None])):
        r, s = _image(d[q].shape)
        n = v.shape[1]
        C0 = d[q][:256, :n].astype(np.float64)
        r[:256, :n], s[:256, :n] = v + C0, S + np.abs(C0)
        res[q] = (r, s)
    if chain is not None:
        res["_chain"] = (v1, S1)
    return res


def _bb_restate(c, d, order, mistake):
    f = np.float32
    T, M = LY_ROWS, c.M
    units = _take(256, M * 256, [0, 1, 2, 3, 255, 4, 31, 32, 128, 127])
    v1, _ = _bb_dh1(c, d)
    chain = bf16r(v1).astype(np.float64)
    dH2, W1u = d["dH2"][:M, :256], np.ascontiguousarray(bf16r(d["W1"][:, :256])[:, units].T)
    with np.errstate(invalid="ignore"):
        dH1 = gc._ordered_sum(dH2[:, None, :] * W1u[None, :, :], order)
    h1 = d["h1"][:M, units]
    dH1 = np.where((h1 >= 0) if mistake == "mask_ge" else (h1 > 0), dH1, f(0))
    chain[:, units] = bf16r(dH1)
    use = dH1 if mistake == "bf16_hidden_rounded_after_output_layer" else chain[:, units].astype(f)       # (here: dH1 consumed unrounded)
    n = _drop_rows(M, mistake, T)
    x = d["x4"][:, [0, 1, 3] if mistake == "x4_pad_contracted" else [0, 1, 2]]
    if mistake == "row_past_count_reduced":
        n, use = M + 1, np.concatenate([use, np.full((1, len(units)), np.nan, f)])
    use, x = use[:n], x[:n]
    if mistake == "ragged_tile_rows_from_previous_tile":
        use, x = _ragged_from_previous(use, M, T), _ragged_from_previous(x, M, T)
    ref = _bb_ref(c, d, chain=chain)
    res, mask = {"_chain": chain}, {}
    with np.errstate(invalid="ignore"):
        sums = {"gW0": gc._ordered_sum(np.ascontiguousarray((use[:, :, None] * x[:, None, :]).transpose(1, 2, 0)), order),
                "gb0": gc._ordered_sum(np.ascontiguousarray(use.T), order)[:, None]}
    for q, v in sums.items():
        cols = v.shape[1]
        o = ref[q][0].copy()
        o[np.isnan(o)] = d[q].astype(np.float64)[np.isnan(o)]
        C0 = d[q][units, :cols]
        o[units, :cols] = v if mistake == "accumulate_overwrites" else (v + C0).astype(f)
        mk = np.zeros(o.shape, bool)
        mk[units, :cols] = True
        res[q], mask[q] = o, mk
    res["_mask"] = mask
    return res


# ---- clift_xyz_head_bf16_fwd: h1 = bf16(relu(W0 x + b0)) (the fmaf chain in fp32), h2 = bf16(relu(bf16(W1) h1 + b1)), h3 likewise, and for E > 0
# out = bf16(Wout) h3 + bout in fp32.  Layer by layer: h1 to its fp64 reference with the bf16 allowance, h2 over the STORED h1, h3 over the stored
# h2, out over the stored h3 ("_chain": {h1, h2, h3} of a launch that stores all three -- every other NULL / non-NULL combination must give the
# same bits for what it writes).  ``_rows``: the refill case is evaluated on a probe of its rows only (see head_refill_probe).
def head_refill_rows():
    return (CUS - RESERVE) * HB_XROWS + HB_ROWS + 1


def head_refill_probe(M):
    """First and last row of each block's first and second staged 2048 positions, and the ragged end, under RESERVE."""
    rpb = row_ranges(M, HB_ROWS, CUS - RESERVE)[1]
    rows = set()
    for b in range(0, M, rpb):
        rows |= {b, b + HB_XROWS - 1, b + HB_XROWS, min(b + rpb, M) - 1}
    rows |= {M - 1, M - 2, ((M - 1) // HB_ROWS) * HB_ROWS, ((M - 1) // HB_ROWS) * HB_ROWS - 1}
    return np.array(sorted(r for r in rows if 0 <= r < M), dtype=np.int64)


def _hb_draw(c, rng):
    x = _rows(rng, c.M, 3)
    W = lambda n: gc._nonzero(rng, (n, 256)) * np.exp2(rng.integers(-2, 3, (n, 1))).astype(np.float32) / np.float32(16)
    d = {"x4": _buf(x, c.M + HB_ROWS, 4), "W0": _buf(gc._nonzero(rng, (256, 3)), 256, 4), "b0": gc._nonzero(rng, (256,)) * np.float32(0.5),
         "W1": _buf(W(256), 256, 260), "b1": gc._nonzero(rng, (256,)), "W2": _buf(W(256), 256, 260), "b2": gc._nonzero(rng, (256,)),
         "Wout": _buf(W(max(c.E, 1)), max(c.E, 1), 260), "bout": gc._nonzero(rng, (max(c.E, 1),)) if c.bout else None}
    rows = head_refill_probe(c.M) if c.p.get("probe") else np.arange(c.M)
    d["_rows"] = rows
    for q, on in (("h1", c.h1), ("h2", c.h2), ("h3", c.h3)):
        d[q] = _out(len(rows), 256) if on else None
    d["out"] = _out(len(rows), c.ldo) if c.E else None
    return d


def _hb_layers64(c, d, chain):
    """[(value, S)] of h1, h2, h3, out in fp64, each over the stored (``chain``) or the reference's own bf16-rounded predecessor.  With a chain
    only the rows whose stored predecessor differs from the reference's own are evaluated again."""
    rows = d["_rows"]
    if chain and "_l64" not in d:
        d["_l64"] = _hb_layers64(c, d, None)
    base = d.get("_l64") if chain else None
    x, W0, b0 = d["x4"][rows, :3].astype(np.float64), d["W0"][:, :3].astype(np.float64), d["b0"].astype(np.float64)
    if base is None:
        t = np.stack([np.broadcast_to(b0[None, :], (len(rows), 256))] + [x[:, k, None] * W0[None, :, k] for k in range(3)], 2)
        out = [(np.maximum(t.sum(2), 0), np.abs(t).sum(2))]
    else:
        out = [base[0]]
    layers = [("h1", "W1", "b1", True), ("h2", "W2", "b2", True)] + ([("h3", "Wout", "bout", False)] if c.E else [])
    for i, (q, W, b, relu) in enumerate(layers):
        n = 256 if relu else c.E
        bias = d[b] if d[b] is not None else np.zeros(n, np.float32)
        if base is None:
            own = bf16r(out[-1][0]).astype(np.float64)
            d.setdefault("_own", {})[q] = own
        else:
            own = d["_own"][q]
        if base is None:
            v, S = _layer64(own, bf16r(d[W][:n, :256]), bias[:n])
        else:
            src = np.asarray(chain[q], dtype=np.float64) if q in chain else bf16r(out[-1][0]).astype(np.float64)
            v, S = base[i + 1][0].copy(), base[i + 1][1].copy()
            redo = np.flatnonzero(np.any(src != own, axis=1))
            if redo.size:
                v2, S2 = _layer64(src[redo], bf16r(d[W][:n, :256]), bias[:n])
                v[redo], S[redo] = (np.maximum(v2, 0) if relu else v2), S2
            out.append((v, S))
            continue
        out.append((np.maximum(v, 0) if relu else v, S))
    return out


def _hb_ref(c, d, rows=None, chain=None):
    if chain is None and "_l64" in d:
        L = d["_l64"]
    else:
        L = _hb_layers64(c, d, chain)
        if chain is None:
            d["_l64"] = L
    n = len(d["_rows"])
    res = {}
    for i, q in enumerate(("h1", "h2", "h3")):
        if d.get(q) is not None:
            r, s = _image(d[q].shape)
            r[:n, :256], s[:n, :256] = L[i]
            res[q] = (r, s)
        if chain is not None:
            res["_chain:" + q] = L[i]
    if c.E:
        r, s = _image(d["out"].shape)
        r[:n, :c.E], s[:n, :c.E] = L[3]
        res["out"] = (r, s)
    return res


def _hb_restate(c, d, order, mistake):
    f = np.float32
    rows_all = d["_rows"]
    n = len(rows_all)
    sub = _take(n, 2 * 256 * 256, [0, n - 1, ((n - 1) // HB_ROWS) * HB_ROWS, HB_ROWS - 1, HB_ROWS, n - 2, 1])      # positions within _rows
    base = _hb_ref(c, d) and d["_l64"]
    chain = {q: (d["_own"][q] if q in d["_own"] else bf16r(base[i][0]).astype(np.float64)).copy() for i, q in enumerate(("h1", "h2", "h3"))}
    xs = d["x4"][rows_all]
    if mistake == "ragged_tile_rows_from_previous_tile" and not c.p.get("probe"):
        xs = _ragged_from_previous(xs, n, HB_ROWS)
    x, W0, b0 = xs[sub], d["W0"], d["b0"]
    k = [0, 1, 3] if mistake == "x4_pad_contracted" else [0, 1, 2]
    with np.errstate(invalid="ignore"):
        t = np.stack([np.broadcast_to(b0[None, :], (len(sub), 256))] + [x[:, j, None] * W0[None, :, j] for j in k], 2).astype(f)
        h = [np.maximum(gc._ordered_sum(t, order), f(0))]
        for W, b in (("W1", "b1"), ("W2", "b2")):
            h.append(np.maximum(_layer32(bf16r(h[-1]), bf16r(d[W][:, :256]), d[b], order), f(0)))
        for i, q in enumerate(("h1", "h2", "h3")):
            chain[q][sub] = bf16r(h[i])
        if c.E:
            src = h[2] if mistake == "bf16_hidden_rounded_after_output_layer" else bf16r(h[2])
            bout = d["bout"] if d["bout"] is not None else np.zeros(c.E, f)
            bout = np.full_like(bout, bout[0]) if mistake == "bout_of_column_0_for_all" else bout
            o = _layer32(src, bf16r(d["Wout"][:c.E, :256]), bout, order)
    ref = _hb_ref(c, d, chain=chain)
    res, mask = {"_chain": chain}, {}
    for i, q in enumerate(("h1", "h2", "h3")):
        if d.get(q) is not None:
            img = d[q].astype(np.float64)
            img[:n, :256] = ref[q][0][:n, :256]
            img[sub, :256] = h[i]
            mk = np.zeros(img.shape, bool)
            mk[sub, :256] = True
            res[q], mask[q] = img, mk
    if c.E:
        img = d["out"].astype(np.float64)
        img[:n, :c.E] = ref["out"][0][:n, :c.E]
        img[sub, :c.E] = o
        mk = np.zeros(img.shape, bool)
        mk[sub, :c.E] = True
        res["out"], mask["out"] = img, mk
    res["_mask"] = mask
    return res



ENTRIES = {
    "clift_linear_k3_fwd": Entry(0, _k3f_draw, _k3f_ref, _k3f_restate, ("out",), ("x4",), {"out": "out_bf16"}),
    "clift_linear_k3_bwd": Entry(32, _k3b_draw, _k3b_ref, _k3b_restate, (), ("x4", "dH"), {"dH": "dh_bf16"}),
    "clift_wgrad_narrow": Entry(64, _wn_draw, _wn_ref, _wn_restate, (), ("dY", "X"), {"X": "x_bf16"}),
    "clift_colsum": Entry(256, _cs_draw, _cs_ref, _cs_restate, (), ("dY",)),
    "clift_rows_act_fwd": Entry(0, _raf_draw, _raf_ref, _raf_restate, ("out",), ("pre",)),
    "clift_rows_act_bwd": Entry(0, _rab_draw, _rab_ref, _rab_restate, ("dpre",), ("out", "dout")),
    "clift_out_layer_fwd": Entry(OF_ROWS, _of_draw, _of_ref, _of_restate, ("out",), ("H",)),
    "clift_out_layer_bwd": Entry(NS_ROWS, _ob_draw, _ob_ref, _ob_restate, ("dX",), ("dOut", "H"), {"H": "h_bf16", "dX": "h_bf16"}),
    "clift_out_layer_bwd_nh": Entry(NS_ROWS, _ob_draw, _ob_ref, _ob_restate, ("dX",), ("dOut", "H"), {"H": "h_bf16", "dX": "h_bf16"}),
    "clift_out_layer_bwd_n128_bf16": Entry(16, _ob_draw, _ob_ref, _ob_restate, ("dX",), ("dOut", "H"), {"H": "h_bf16", "dX": "h_bf16"}, limit=False),
    "clift_xyz_head_first2_fwd": Entry(LF_ROWS, _f2_draw, _f2_ref, _f2_restate, ("h1", "h2"), ("x4",)),
    "clift_xyz_head_last2_fwd": Entry(LF_ROWS, _l2_draw, _l2_ref, _l2_restate, ("hidden", "out"), ("A",)),
    "clift_app_head_last2_fwd": Entry(LN_ROWS, _l2_draw, _l2_ref, _l2_restate, ("hidden", "pre", "out"), ("A",)),
    "clift_xyz_head_first2_x6_fwd": Entry(X6_ROWS, _f2_draw, _f2_ref, _f2_restate, ("h2",), ("x4",)),
    "clift_xyz_head_last2_x6_fwd": Entry(X6_ROWS, _l2_draw, _l2_ref, _l2_restate, ("hidden", "out"), ("A",)),
    "clift_app_head_last2_x6_fwd": Entry(N6_ROWS, _l2_draw, _l2_ref, _l2_restate, ("hidden", "out"), ("A",)),
    "clift_xyz_head_first2_bwd": Entry(LF_ROWS, _fb_draw, _fb_ref, _fb_restate, (), ("x4", "dH2")),
    "clift_xyz_head_first2_x6_bwd": Entry(X6_ROWS, _fb_draw, _fb_ref, _fb_restate, (), ("x4", "dH2")),
    "clift_xyz_head_first2_wgrad": Entry(64, _fw_draw, _fw_ref, _fw_restate, (), ("x4", "dH2")),
    "clift_xyz_head_first2_x6_wgrad": Entry(XW_ROWS, _fw_draw, _fw_ref, _fw_restate, (), ("x4", "dH2")),
    "clift_app_head_last2_bf16_fwd": Entry(NB_ROWS, _lb_draw, _lb_ref, _lb_restate, ("hidden", "out"), ("A",), {"A": "one", "hidden": "one"}, limit=False),
    "clift_xyz_head_first2_bf16_bwd": Entry(LY_ROWS, _bb_draw, _bb_ref, _bb_restate, (), ("x4", "dH2", "h1"), {"dH2": "one", "h1": "one"}, limit=False),
    "clift_xyz_head_bf16_fwd": Entry(HB_ROWS, _hb_draw, _hb_ref, _hb_restate, ("h1", "h2", "h3", "out"), ("x4",), {"h1": "one", "h2": "one", "h3": "one"}, limit=False),
}
# the two launches of the shard bracket have no case table: their model is shards_fold below, their device test runs them around the stream
# routes of clift_wgrad_narrow and clift_linear_k3_bwd (the kernels of this table that call grad_target)
TABLE = set(ENTRIES) | {"clift_grad_shards_begin", "clift_grad_shards_fold"}
K3_CAP_ROWS = 3 * 2048 * 256 + 300            # Nout = 4: 2048 blocks x 256 rows per sweep; the four-rows-in-flight loop runs only past three sweeps


# (E, hidden stored) of the two cases per row count of the xyz last2 forms: every combination over the five row counts
_E_HID = (((1, 0), (2, 1)), ((3, 0), (4, 1)), ((1, 1), (2, 0)), ((3, 1), (4, 0)), ((3, 0), (2, 1)))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda entry, **p: out.append(Case(entry, **p))
    # ---- clift_linear_k3_fwd
    for i, Nout in enumerate((4, 64, 256, 12, 1028)):
        T = 256 // (Nout // 4) if k3_fwd_kernel(Nout) == "main" else 64
        for j, M in enumerate(sorted({1, max(T - 1, 1), T, T + 1, 2 * T + 1})):
            add("clift_linear_k3_fwd", M=M, Nout=Nout, relu=(i + j // 2) % 2, out_bf16=j % 2, ldo=Nout + (8 if j % 3 else 0))
        add("clift_linear_k3_fwd", M=2 * T + 1, Nout=Nout, relu=1, out_bf16=1, ldo=Nout + 8, tag="relu")
        add("clift_linear_k3_fwd", M=2 * T + 1, Nout=Nout, relu=0, out_bf16=0, ldo=Nout, tag="plain")
    add("clift_linear_k3_fwd", M=K3_CAP_ROWS, Nout=4, relu=1, out_bf16=0, ldo=4, tag="cap")
    # ---- clift_linear_k3_bwd
    for j, M in enumerate((1, 7, 8, 9, 31, 32, 33, 39, 40, 41, 63, 65, 511, 512, 513, 1057)):
        add("clift_linear_k3_bwd", M=M, Nout=256, ldh=264, dh_bf16=j % 2, db=1)
    for bf in (0, 1):
        add("clift_linear_k3_bwd", M=4097, Nout=256, ldh=256, dh_bf16=bf, db=0, tag="no_db")
        add("clift_linear_k3_bwd", M=545, Nout=64, ldh=72, dh_bf16=bf, db=1)
        add("clift_linear_k3_bwd", M=545, Nout=260, ldh=264, dh_bf16=bf, db=1)
        for M in (4095, 4096, 4097, 4096 + NS_ROWS - 1):
            add("clift_linear_k3_bwd", M=M, Nout=256, ldh=256 + 8 * bf, dh_bf16=bf, db=1)
        add("clift_linear_k3_bwd", M=m3_rows(NS_ROWS, first=4096), Nout=256, ldh=264, dh_bf16=bf, db=1, reserve=RESERVE)
    # ---- clift_wgrad_narrow
    wn = lambda M, no, ni, x_bf16=0, gb=1, ldd=None, ldx=None, **kw: add(
        "clift_wgrad_narrow", M=M, no=no, ni=ni, ldd=r4(no) + 4 if ldd is None else ldd, ldx=(gc.r8(ni) + 8 if x_bf16 else r4(ni) + 4) if ldx is None else ldx,
        ldw=r4(ni) + 4, x_bf16=x_bf16, gb=gb, **kw)
    nis, Ms = (3, 36, 256, 260, 515), (1, 63, 64, 65, 71, 129)
    for i, no in enumerate((1, 4, 5, 8, 9, 16, 22, 24, 25, 32)):
        wn(Ms[i % 6], no, nis[i % 5], x_bf16=i % 2)
        wn(Ms[(i + 3) % 6], no, nis[(i + 2) % 5], x_bf16=(i + 1) % 2)
    for ni in nis:
        for bf in (0, 1):
            wn(129, 22, ni, x_bf16=bf, tag="ni")
    for M in Ms:
        wn(M, 3, 36, tag="rows")
    wn(129, 22, 260, gb=0, tag="no_gb")
    wn(4095, 22, 256, ldd=24)
    for M in (4096, 4097, 4096 + NS_ROWS - 1):
        wn(M, 22, 256, ldd=24)
        wn(M, 3, 256, x_bf16=1, ldd=4)
    wn(4096, 22, 28, ldd=24)                    # ni < 32: the plain kernel
    wn(4096, 22, 32, ldd=24)                    # the stream, one wave's columns
    wn(4096, 22, 34, ldd=24, ldx=36)            # ni % 4 != 0: plain
    wn(4096, 9, 36, ldd=12)                     # the stream with a ragged last column group
    wn(4096, 4, 128, x_bf16=1, ldd=4)           # bf16-stored with ni != 256: plain
    wn(4096, 22, 256, ldd=24, gb=0, tag="no_gb")
    wn(4096, 22, 256, ldd=36, tag="ldd36")      # ldd > 32: plain
    wn(m3_rows(NS_ROWS, first=4096), 22, 256, ldd=24, reserve=RESERVE)
    wn(m3_rows(NS_ROWS, first=4096), 4, 256, x_bf16=1, ldd=4, reserve=RESERVE)
    # ---- clift_colsum
    for N, M in ((1, 257), (255, 1), (256, 255), (257, 256), (22, 513)):
        add("clift_colsum", M=M, N=N, ld=N)
        add("clift_colsum", M=M, N=N, ld=r4(N) + 4, tag="padded")
    # ---- clift_rows_act_fwd / _bwd
    for C_ in (1, 2, 3, 5, 22, 32, 33, 64):
        for kind in (1, 2):
            add("clift_rows_act_fwd", M=37, C=C_, kind=kind, ldp=C_, ldo=C_)
            add("clift_rows_act_fwd", M=515, C=C_, kind=kind, ldp=r4(C_) + 4, ldo=C_ + 3)
        for kind in (0, 1, 2):
            add("clift_rows_act_bwd", M=37, C=C_, kind=kind, ldo=C_, lddo=C_, ldd=C_)
            add("clift_rows_act_bwd", M=515, C=C_, kind=kind, ldo=C_ + 3, lddo=C_ + 1, ldd=r4(C_ + 1) if C_ < 64 else 64)
    # ---- clift_out_layer_fwd
    for i, no in enumerate((1, 3, 4, 5, 22, 29, 32)):
        for j, M in enumerate((1, OF_ROWS - 1, OF_ROWS, OF_ROWS + 1, 2 * OF_ROWS + 1)):
            add("clift_out_layer_fwd", M=M, no=no, act=2 * ((i + j) % 2), ldo=no + (5 if j % 2 else 0), ldh=(256, 260)[j % 2], ldw=(260, 256)[j % 2])
        add("clift_out_layer_fwd", M=2 * OF_ROWS + 1, no=no, act=2 * ((i + 1) % 2), ldo=no + 5, ldh=260, ldw=260, tag="other_act")
    for no, act in ((22, 2), (3, 0)):
        add("clift_out_layer_fwd", M=m3_rows(OF_ROWS), no=no, act=act, ldo=no + 2, ldh=256, ldw=256, reserve=RESERVE)
    # ---- clift_out_layer_bwd / _nh / _n128_bf16
    ob = lambda entry, M, no, nh, ldd, h_bf16=0, gb=1, **kw: add(entry, M=M, no=no, nh=nh, ldd=ldd, ldh=nh + (8 if h_bf16 else 4), ldx=nh + (8 if h_bf16 else 4),
                                                                 h_bf16=h_bf16, gb=gb, **kw)
    Ms = (1, NS_ROWS - 1, NS_ROWS, NS_ROWS + 1, 2 * NS_ROWS + 1)
    for i, no in enumerate((3, 9, 22, 29)):                   # cdiv(no, 8) = 1 .. 4
        for j, M in enumerate(Ms):
            ob("clift_out_layer_bwd", M, no, 256, (r4(no), 32)[(i + j) % 2])
        ob("clift_out_layer_bwd", 2 * NS_ROWS + 1, no, 256, (r4(no), 32)[i % 2], tag="other_ldd")
    ob("clift_out_layer_bwd", 2 * NS_ROWS + 1, 22, 256, 24, gb=0, tag="no_gb")
    ob("clift_out_layer_bwd", m3_rows(NS_ROWS), 22, 256, 24, reserve=RESERVE)
    for nh, hb, no, ldd in ((32, 0, 3, 4), (128, 0, 3, 4), (128, 0, 4, 32), (256, 1, 22, 24), (256, 1, 3, 32)):
        for M in Ms:
            ob("clift_out_layer_bwd_nh", M, no, nh, ldd, hb)
    ob("clift_out_layer_bwd_nh", 2 * NS_ROWS + 1, 3, 128, 4, gb=0, tag="no_gb")
    ob("clift_out_layer_bwd_nh", m3_rows(NS_ROWS), 3, 128, 4, reserve=RESERVE)
    ob("clift_out_layer_bwd_nh", m3_rows(NS_ROWS), 22, 256, 24, 1, reserve=RESERVE)
    for j, M in enumerate((1, 15, 16, 17, 33)):
        for no in (1, 3, 4):
            ob("clift_out_layer_bwd_n128_bf16", M, no, 128, (4, 8)[(j + no) % 2], 1)
    ob("clift_out_layer_bwd_n128_bf16", 33, 3, 128, 8, 1, gb=0, tag="no_gb")
    ob("clift_out_layer_bwd_n128_bf16", 33, 3, 128, 4, 1, tag="ldd4")
    ob("clift_out_layer_bwd_n128_bf16", m3_rows(16, 4), 3, 128, 8, 1, reserve=RESERVE)
    # ---- clift_xyz_head_first2_fwd
    for j, M in enumerate((1, LF_ROWS - 1, LF_ROWS, LF_ROWS + 1, 2 * LF_ROWS + 1)):
        add("clift_xyz_head_first2_fwd", M=M, h1=j % 2, ldh1=(256, 264)[(j // 2) % 2], ldh2=(264, 256)[j % 2])
        add("clift_xyz_head_first2_fwd", M=M, h1=(j + 1) % 2, ldh1=(264, 256)[(j // 2) % 2], ldh2=(256, 264)[j % 2], tag="b")
    for h1 in (0, 1):
        add("clift_xyz_head_first2_fwd", M=m3_rows(LF_ROWS), h1=h1, ldh1=264, ldh2=264, reserve=RESERVE)
    # ---- clift_xyz_head_last2_fwd / clift_app_head_last2_fwd
    for j, M in enumerate((1, LF_ROWS - 1, LF_ROWS, LF_ROWS + 1, 2 * LF_ROWS + 1)):
        for E, hid in _E_HID[j]:
            add("clift_xyz_head_last2_fwd", M=M, E=E, hid=hid, lda=(256, 260)[j % 2], ldh=(260, 256)[j % 2], ldo=E + (E + j) % 3)
    for hid in (0, 1):
        add("clift_xyz_head_last2_fwd", M=m3_rows(LF_ROWS), E=3, hid=hid, lda=256, ldh=256, ldo=4, reserve=RESERVE)
    for j, M in enumerate((1, LN_ROWS - 1, LN_ROWS, LN_ROWS + 1, 2 * LN_ROWS + 1)):
        for i, E in enumerate((1, 3, 4)):
            k = i + j
            add("clift_app_head_last2_fwd", M=M, E=E, hid=k % 2, pre=(k // 2) % 2, sigmoid=(k // 4 + j) % 2, lda=(128, 160)[j % 2], ldh=(160, 128)[j % 2], ldo=E + k % 2)
    for hid, pre, sg in ((0, 0, 1), (1, 1, 1), (1, 0, 0), (0, 1, 0)):
        add("clift_app_head_last2_fwd", M=2 * LN_ROWS + 1, E=3, hid=hid, pre=pre, sigmoid=sg, lda=160, ldh=160, ldo=4, tag="forms")
    add("clift_app_head_last2_fwd", M=m3_rows(LN_ROWS), E=3, hid=1, pre=1, sigmoid=1, lda=128, ldh=128, ldo=4, reserve=RESERVE)
    add("clift_app_head_last2_fwd", M=m3_rows(LN_ROWS), E=3, hid=0, pre=0, sigmoid=1, lda=128, ldh=128, ldo=3, reserve=RESERVE)
    # ---- the fp32x6 forwards
    Ms = (1, X6_ROWS - 1, X6_ROWS, X6_ROWS + 1, 2 * X6_ROWS + 1)
    for j, M in enumerate(Ms):
        add("clift_xyz_head_first2_x6_fwd", M=M, signs=j % 2, ldh2=(264, 256)[j % 2])
        for E, hid in _E_HID[j]:
            add("clift_xyz_head_last2_x6_fwd", M=M, E=E, hid=hid, lda=(256, 260)[j % 2], ldh=(260, 256)[j % 2], ldo=E + (E + j) % 3)
        for i, E in enumerate((1, 3, 4)):
            add("clift_app_head_last2_x6_fwd", M=M, E=E, hid=(i + j) % 2, sigmoid=((i + j) // 2) % 2, lda=(128, 160)[j % 2], ldh=(160, 128)[j % 2], ldo=E + (i + j) % 2)
    for sg in (0, 1):
        add("clift_xyz_head_first2_x6_fwd", M=2 * X6_ROWS + 1, signs=sg, ldh2=264, tag="forms")
        add("clift_xyz_head_first2_x6_fwd", M=m3_x6(), signs=sg, ldh2=256, reserve=RESERVE)
        add("clift_xyz_head_last2_x6_fwd", M=m3_x6(), E=3, hid=sg, lda=256, ldh=256, ldo=4, reserve=RESERVE)
        if sg:
            add("clift_app_head_last2_x6_fwd", M=m3_rows(N6_ROWS, 2), E=3, hid=1, sigmoid=1, lda=128, ldh=128, ldo=4, reserve=RESERVE)
    for hid, sg in ((0, 0), (0, 1), (1, 0), (1, 1)):
        add("clift_app_head_last2_x6_fwd", M=2 * N6_ROWS + 1, E=3, hid=hid, sigmoid=sg, lda=160, ldh=160, ldo=4, tag="forms")
    # ---- the backward ends of the first two layers
    for entry, T, big in (("clift_xyz_head_first2_bwd", LF_ROWS, m3_rows(LF_ROWS)), ("clift_xyz_head_first2_x6_bwd", X6_ROWS, m3_x6())):
        for j, M in enumerate((1, T - 1, T, T + 1, 2 * T + 1)):
            add(entry, M=M, ldd=(256, 260)[j % 2])
        add(entry, M=big, ldd=260, reserve=RESERVE)
    for entry, T, big in (("clift_xyz_head_first2_wgrad", 64, m3_fixed(64, 64)), ("clift_xyz_head_first2_x6_wgrad", XW_ROWS, m3_fixed((CUS - RESERVE) // 4, XW_ROWS))):
        for j, M in enumerate((1, T - 1, T, T + 1, 2 * T + 1)):
            add(entry, M=M, ldd=(256, 260)[j % 2], ldg=(264, 256)[j % 2], gb=int(j != 3))
        add(entry, M=2 * T + 1, ldd=260, ldg=264, gb=0, tag="no_gb")
        add(entry, M=big, ldd=260, ldg=264, gb=1, reserve=RESERVE)
    # ---- clift_app_head_last2_bf16_fwd
    for j, M in enumerate((1, NB_ROWS - 1, NB_ROWS, NB_ROWS + 1, 2 * NB_ROWS + 1)):
        for i, E in enumerate((1, 3, 4)):
            add("clift_app_head_last2_bf16_fwd", M=M, E=E, hid=(i + j) % 2, sigmoid=((i + j) // 2) % 2, lda=(128, 160)[j % 2], ldh=(160, 128)[j % 2], ldo=E + (i + j) % 2, one=1)
    for hid, sg in ((0, 0), (0, 1), (1, 0), (1, 1)):
        add("clift_app_head_last2_bf16_fwd", M=2 * NB_ROWS + 1, E=3, hid=hid, sigmoid=sg, lda=160, ldh=160, ldo=4, one=1, tag="forms")
    add("clift_app_head_last2_bf16_fwd", M=m3_rows(NB_ROWS, 2), E=3, hid=1, sigmoid=1, lda=128, ldh=128, ldo=4, one=1, reserve=RESERVE)
    # ---- clift_xyz_head_first2_bf16_bwd
    for j, M in enumerate((1, LY_ROWS - 1, LY_ROWS, LY_ROWS + 1, 2 * LY_ROWS + 1)):
        add("clift_xyz_head_first2_bf16_bwd", M=M, ldd=(256, 264)[j % 2], ldm=(264, 256)[j % 2], one=1)
    add("clift_xyz_head_first2_bf16_bwd", M=gc.m3("LAYER_BF16", "dgrad_masked"), ldd=264, ldm=264, one=1, reserve=RESERVE)
    # ---- clift_xyz_head_bf16_fwd
    hb = lambda M, E, h, bout=1, **kw: add("clift_xyz_head_bf16_fwd", M=M, E=E, h1=h[0], h2=h[1], h3=h[2], bout=bout, ldo=E + (M % 2), one=1, **kw)
    combos = [(a, b, c_) for a in (0, 1) for b in (0, 1) for c_ in (0, 1)]
    for j, M in enumerate((1, HB_ROWS - 1, HB_ROWS, HB_ROWS + 1, 2 * HB_ROWS + 1)):
        hb(M, j, combos[j] if j else (0, 0, 1))
        hb(M, 4 - j if j < 4 else 2, combos[7 - j])
    for h in combos:
        hb(2 * HB_ROWS + 1, 3, h, tag="forms")
    hb(2 * HB_ROWS + 1, 0, (1, 1, 1), tag="e0")
    hb(2 * HB_ROWS + 1, 3, (0, 0, 0), bout=0, tag="no_bout")
    hb(m3_rows(HB_ROWS), 3, (0, 0, 0), reserve=RESERVE, tag="nostore")
    hb(head_refill_rows(), 3, (0, 0, 0), reserve=RESERVE, probe=1, tag="refill")
    for i, c in enumerate(out):
        c.seed = i + 1
    keys = [c.key for c in out]
    assert len(set(keys)) == len(keys), "case names must be unique"
    return tuple(out)


def groups():
    out = {}
    for c in cases():
        out.setdefault(c.entry, []).append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs, yardsticks
@functools.lru_cache(maxsize=4)
def inputs(c):
    """{buffer: float32 image (None: a NULL argument)} plus "_ref" and "_yard".  A draw whose yardstick is ill-conditioned is redrawn."""
    seed, e = c.seed, ENTRIES[c.entry]
    for _ in range(8):
        d = e.draw(c, _rng(seed))
        d["_ref"] = e.ref(c, d)
        d["_yard"] = _yardsticks(c, d)
        if max(d["_yard"].values()) <= ILL_CONDITIONED:
            return d
        seed += 1000
    raise AssertionError(f"{c}: no well-conditioned draw")


def reference(c):
    """{output buffer: (fp64 image, S image)}: NaN in the image where the entry point must not write."""
    return inputs(c)["_ref"]


def reference_of(c, rows):
    """... of the first ``rows`` sample rows (the device row limit; the reductions only)."""
    return ENTRIES[c.entry].ref(c, inputs(c), rows)


def _yardsticks(c, d):
    out = {q: 0.0 for q in d["_ref"]}
    d["_plain"] = {}
    for order in ORDERS:
        r = d["_plain"][order] = ENTRIES[c.entry].restate(c, d, order, None)
        refs = ENTRIES[c.entry].ref(c, d, chain=r["_chain"]) if "_chain" in r else d["_ref"]
        for q, (ref, S) in refs.items():
            if q.startswith("_chain"):
                continue
            on = ~np.isnan(ref) & (S > NORMAL_FLOOR)
            if "_mask" in r and q in r["_mask"]:
                on &= r["_mask"][q]
            if on.any():
                out[q] = max(out[q], float(np.max(np.abs(r[q][on] - ref[on]) / S[on])))
    return out


def yardsticks(c):
    return dict(inputs(c)["_yard"])


def restate(c, order="natural", mistake=None):
    """{output buffer: image}: the operation in fp32, sums running in ``order``, optionally with a mistake built in; as stored."""
    d = inputs(c)
    r = dict(d["_plain"][order]) if mistake is None else ENTRIES[c.entry].restate(c, d, order, mistake)     # (the plain ones: made for the yardstick)
    r.pop("_mask", None)
    for q in r:
        if not q.startswith("_chain") and stored_bf16(c, q):         # (a chain is made of bf16 values already)
            r[q] = bf16r(r[q]).astype(np.float64)
    return r


# Bounds that had to be widened on the device for a reason that is not a bug: (entry, case name, buffer): (largest error / S measured, the
# reason read from the kernel); the new factor is twice the measured one.
WIDENED = {}


def factor_for(c, q):
    y = yardsticks(c)
    f = gc.bound_factor(y[q] if not q.startswith("_chain") else max(y.values()))
    entry = WIDENED.get((c.entry, c.name, q))
    return max(f, 2.0 * entry[0]) if entry is not None else f


def check(got, c, ref=None, prefill=None, base=None):
    """gemm_cases.check for buffer images.  got: {buffer: image as float64}; where the reference image is NaN the buffer must hold the bits of
    its pre-fill (``prefill``, default: the case's inputs).  Returns (ok, worst error / bound, worst error / S, text)."""
    d = inputs(c)
    if ref is None and "_chain" in got:          # a chain of bf16 roundings: the later layers over the intermediate that was actually stored
        ref = ENTRIES[c.entry].ref(c, d, chain=got["_chain"])
    ref = reference(c) if ref is None else ref
    worst, worst_s, notes = 0.0, 0.0, []
    for q, (r, S) in ref.items():
        if q.startswith("_chain:") and q[7:] in ref:          # stored by the case itself: held as that output
            continue
        g = np.asarray(got["_chain"][q[7:]] if q.startswith("_chain:") else got[q], dtype=np.float64).reshape(r.shape)
        pre = (np.zeros(r.shape) if q.startswith("_chain") else (d[q] if prefill is None else prefill[q]).astype(np.float64).reshape(r.shape))
        off = np.isnan(r)
        if not np.array_equal(g[off], pre[off]):
            at = np.argwhere(off & (g != pre))[0]
            notes.append(f"{q}{tuple(int(i) for i in at)} was written: {g[tuple(at)]!r}")
        bnd = factor_for(c, q) * S + np.where(S > 0, TINY, 0.0)
        if stored_bf16(c, q):
            bnd = bnd + BF16_HALF_SPACING * np.abs(np.nan_to_num(r))
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(off, 0.0, np.abs(g - np.nan_to_num(r)))
            ratio = np.where(err <= bnd, err / np.maximum(bnd, 1e-300), np.inf)
            rel = np.where((S > 0) & ~off, err / np.maximum(S, 1e-300), 0.0)
        w = float(ratio.max()) if ratio.size else 0.0
        worst, worst_s = max(worst, w), max(worst_s, float(np.nanmax(rel)) if rel.size else 0.0)
        if not w <= 1.0:
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            notes.append(f"{q}{tuple(int(i) for i in at)}: got {g[at]!r}, reference {r[at]!r}, bound {bnd[at]:.3e}")
    return not notes, worst, worst_s, f"{c}: " + ("; ".join(notes) if notes else f"worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- mistakes
# mistake: the entry points whose restatement can make it
MISTAKES = {
    "x4_pad_contracted": ("clift_linear_k3_fwd", "clift_linear_k3_bwd", "clift_xyz_head_first2_fwd", "clift_xyz_head_first2_x6_fwd") + _FB + _FW,
    "mask_ge": _OB + _FB + ("clift_xyz_head_first2_bf16_bwd",),
    "mask_from_second_layer": _FB,
    "first_layer_sign_without_b0": _FB + _FW,
    "x6_middle_term_dropped": X6,
    "gb_from_masked_dout": _OB,
    "dout_pad_column_contracted": _OB,
    "bout_of_column_0_for_all": _L2 + ("clift_xyz_head_bf16_fwd",),
    "relu_missing_before_output_layer": _L2,
    "hidden_stored_before_relu": _L2,
    "last_m_mod_8_rows_dropped": ("clift_linear_k3_bwd", "clift_wgrad_narrow") + _OB + _FB + _FW,
    "last_m_mod_64_rows_dropped": ("clift_wgrad_narrow", "clift_colsum"),
    "ragged_tile_rows_from_previous_tile": ("clift_linear_k3_bwd", "clift_wgrad_narrow", "clift_out_layer_fwd") + _OB + _FUSED,
    "row_past_count_reduced": ("clift_linear_k3_bwd", "clift_wgrad_narrow", "clift_colsum") + _OB + _FB + _FW,
    "gb_missing_on_last_quad": ("clift_wgrad_narrow", "clift_linear_k3_bwd") + _OB + _FB + _FW,
    "accumulate_overwrites": ("clift_linear_k3_bwd", "clift_wgrad_narrow", "clift_colsum") + _OB + _FB + _FW,
    "ni_tail_beyond_256_dropped": ("clift_wgrad_narrow",),
    "out_bias_added_per_column_group": ("clift_out_layer_fwd",) + _L2,
    "column_group_share_dropped": ("clift_out_layer_fwd",) + _L2,
    "columns_no_ldo_written": ("clift_out_layer_fwd",) + _L2,
    "sigmoid_of_minus_pre": ("clift_rows_act_fwd", "clift_app_head_last2_fwd", "clift_app_head_last2_x6_fwd", "clift_app_head_last2_bf16_fwd"),
    "bf16_hidden_rounded_after_output_layer": ("clift_app_head_last2_bf16_fwd", "clift_xyz_head_first2_bf16_bwd", "clift_xyz_head_bf16_fwd"),
    "softmax_without_max": ("clift_rows_act_fwd",),
    "softmax_pad_lanes_exp0": ("clift_rows_act_fwd",),
    "softmax_bwd_dot_over_c_minus_1": ("clift_rows_act_bwd",),
    "identity_pad_columns_unwritten": ("clift_rows_act_bwd",),
}
FOLD_MISTAKES = ("fold_takes_seven_copies", "fold_does_not_clear", "fold_ignores_first")


def shards_fold(grad, shards, first, n, mistake=None):
    """clift_grad_shards_fold in fp32 on copies: grad[first : first + n) += the eight shards in shard order, which are cleared.  Returns
    (grad, shards)."""
    grad, shards = grad.astype(np.float32).copy(), shards.astype(np.float32).copy()
    at = 0 if mistake == "fold_ignores_first" else first
    acc = np.zeros(n, np.float32)
    for x in range(7 if mistake == "fold_takes_seven_copies" else 8):
        acc = (acc + shards[x, at:at + n]).astype(np.float32)
        if mistake != "fold_does_not_clear":
            shards[x, at:at + n] = 0
    grad[at:at + n] = (grad[at:at + n] + acc).astype(np.float32)
    return grad, shards
