"""Shared inputs of the clift_gemm tests (test_gemm_cases_host.py on the CPU, test_gpu_gemm_cases.py on the GPU): a table of seeded cases
that reaches every route of clift_gemm_route (csrc/gemm.hip) in every form its predicate admits, an fp64 reference of the operation on the
values as stored, and the yardstick of a case: the same operation in fp32 on the CPU with the k-sum in the three orders of loss_cases,
measured against fp64.  The k-sum of the restatement is a running sum -- one fp32 accumulator that takes the terms one after the other, the
bias among them -- because that is what the kernels are: an MFMA accumulator chain is bit-identical to an fmaf chain over k (csrc/gemm.hip),
and the persistent forward kernels enter the bias as one more contraction step (csrc/layer_f32.hip).  A pairwise tree, whose error grows with
log K, would measure an arithmetic no kernel here performs.

    C[m][n] (+)= act( sum_k A(m,k) B(n,k) + bias[n] ) * (mask[m][n] > 0),   colsum[m] += sum_k A(m,k)

A device result is held, element by element, to ``(8 * yardstick + 4 * 2^-24) * S`` with S = |A| |B| + |bias| + |C0| of that element and the
yardstick the largest |fp32 restatement - fp64| / S of the case -- the form of loss_cases.bound.  A bf16-stored result gets 2^-8 |reference|
on top, half the spacing of an 8-bit significand: what its one rounding may move it by (see ``check``).

What the table poisons: operand rows past the row count are NaN (T more rows than the launch names are allocated, T the kernel's streamed
tile, so nothing a kernel may touch lies outside an allocation); output pad columns [N, ldc) and two rows past the last hold SENTINEL and
must keep it; operand pad columns [K, lda) / [K, ldb) are NaN where the route's kernel does not read them (ROUTES[..].pad == "unread") and
the finite PAD_FINITE where it reads them against zero weights ("times_zero": k_dgrad_narrow_stream) -- the contract include/clift.h
states at clift_gemm_t.  Masks hold +0.0, -0.0, a positive and a negative denormal and +inf among ordinary values; NaN masks are outside the
contract.

The fp32 restatement is evaluated on a PROBE of a large case -- the output rows / columns at the tile edges, the ragged last tile and a few
more, at most PROBE_PRODUCTS products -- since M N K elementwise fp32 products of a 30 000-row case do not fit a test; the reference and the
device comparison always cover every element.  Nothing here touches the GPU."""
import functools

import numpy as np
import torch

import loss_cases as lc
from loss_cases import HALF_ULP, ILL_CONDITIONED, ORDERS

SENTINEL = -7.25                 # exactly representable in bf16
PAD_FINITE = 9.5e8
RESERVE = 128                    # clift_set_cu_reserve of the M3 cases: 256 - 128 CUs
CUS = 256
SW_TILED_ONLY, SW_X6_TILED = 1, 2
PROBE_PRODUCTS = 1 << 22
BF16_HALF_SPACING = 2.0 ** -8


class Route:
    """What the tests need to know of a route's kernel, read from its source.
    T: rows of the streamed tile (the tiled kernels: rows of the block tile); rows: "every" M, "m64" (>= 64) or "m4096" (>= 4096; the wgrads: K);
    plan: how the launcher divides the rows (None: a grid of tiles); pad: operand pad columns "unread" or "times_zero"; rounds: operands are
    rounded to bf16 (RNE) on their way in; split: fp32x6 arithmetic; atomics: the result is accumulated with fp32 atomics (bits may differ from
    launch to launch); limit: the kernel calls limit_rows."""

    def __init__(self, T, rows, plan, pad="unread", rounds=False, split=False, atomics=False, limit=True):
        self.T, self.rows, self.plan, self.pad, self.rounds, self.split, self.atomics, self.limit = T, rows, plan, pad, rounds, split, atomics, limit


ROUTES = {
    # precision 2
    "LAYER_X6": Route(32, "every", ("ranges", 1, 2), split=True),                     # X6_ROWS; one row range per PAIR of CUs
    "WGRAD_X6": Route(32, "m4096", ("quarter",), split=True, atomics=True),           # XW_ROWS; a quarter of the CUs row ranges, whatever K
    "LAYER_N6": Route(32, "every", ("ranges", 2, 1), split=True),                     # N6_ROWS; two blocks per CU (the 160-wide dgrad: one)
    "WGRAD_N6": Route(32, "every", ("ranges", 1, 1), split=True, atomics=True),
    "SPLIT_TILED": Route(128, "every", None, split=True, limit=False),                # gemm_split.hip does not clamp and need not
    # precision 0
    "LAYER_F32_FWD": Route(32, "every", ("ranges", 1, 1)),                            # LF_ROWS
    "LAYER_F32_DGRAD": Route(32, "m4096", ("ranges", 1, 1)),
    "DGRAD_NARROW": Route(32, "m4096", ("ranges", 1, 1), pad="times_zero"),           # narrow_stream.hip: fragments past K re-read LDS against zero weights
    "WGRAD_F32_QUADS": Route(64, "m4096", ("fixed", 64), atomics=True),               # 64 row ranges x 4 quadrants, whatever the reserve
    "WGRAD_N128": Route(64, "m4096", ("fixed", 256), atomics=True),
    "LAYER_N128": Route(64, "every", ("ranges", 1, 1)),                               # LN_ROWS
    "DGRAD_N160_PAIR": Route(64, "m4096", ("ranges", 1, 1)),
    "TILED_128X256": Route(128, "every", None),
    "TILED_128X128": Route(128, "every", None),
    "TILED_256X32": Route(256, "every", None),
    # precision 1
    "LAYER_BF16": Route(64, "m64", ("bf16",), rounds=True, limit=False),              # LY_ROWS; ranges balanced to 32 rows
    "WGRAD_BF16": Route(64, "m64", ("wgrad_bf16",), rounds=True, atomics=True, limit=False),     # K < 4096: one range per CU; else 64 x 4 slices
    "DGRAD_NARROW_BF16": Route(32, "m4096", ("ranges", 1, 1), pad="times_zero"),      # fp32 products of fp32 operands: nothing is rounded
    "LAYER_NB16": Route(64, "m64", ("ranges", 2, 1), rounds=True, limit=False),       # NB_ROWS
    "WGRAD_NB16": Route(64, "m64", ("ranges", 1, 1), rounds=True, atomics=True, limit=False),
    "TILED_BF16_128X256": Route(128, "every", None, rounds=True, limit=False),
    "TILED_BF16_128X128": Route(128, "every", None, rounds=True, limit=False),
    "TILED_BF16_256X32": Route(256, "every", None, rounds=True, limit=False),
}
PERSISTENT = tuple(r for r, info in ROUTES.items() if info.plan is not None)


# ---------------------------------------------------------------------------------------------------------------- row ranges, M3
def cdiv(a, b):
    return (a + b - 1) // b


def row_ranges(rows, ROWS, cus, per_cu=1):
    """csrc/row_ranges.h restated: (blocks, rows per block, grid)."""
    tiles, want = cdiv(rows, ROWS), per_cu * cus
    if rows <= 0 or want <= 0:
        return 0, 0, 0
    blocks = min(tiles, want)
    rpb = cdiv(cdiv(rows, blocks), ROWS) * ROWS
    return blocks, rpb, cdiv(rows, rpb)


def rows_per_block(route, form, rows, cus):
    """Rows of a block (row range) of a persistent route's launch over ``rows`` rows with ``cus`` CUs, as its launcher sizes it."""
    info = ROUTES[route]
    T, plan = info.T, info.plan
    if plan[0] == "ranges":
        per_cu = 1 if (route == "LAYER_N6" and form == "dgrad_unmasked") else plan[1]
        rpb = row_ranges(rows, T, cus // plan[2], per_cu)[1]
    elif plan[0] == "fixed" or (plan[0] == "wgrad_bf16" and rows >= 4096):
        rpb = cdiv(cdiv(rows, plan[1] if plan[0] == "fixed" else 64), T) * T
    elif plan[0] == "wgrad_bf16":
        rpb = row_ranges(rows, T, cus)[1]
    elif plan[0] == "quarter":
        rpb = cdiv(cdiv(rows, max(cus // 4, 1)), T) * T
    else:                        # "bf16": k_layer_bf16 balances its ranges to 32 rows and walks them in 64-row tiles
        rpb = cdiv(cdiv(rows, min(cdiv(rows, T), cus)), 32) * 32
    return rpb


def block_rows(route, form, rows, cus):
    """[(first row, end row)] of those blocks."""
    rpb = rows_per_block(route, form, rows, cus)
    return [(b, min(rows, b + rpb)) for b in range(0, rows, rpb)]


def walks_three_tiles_and_ends_ragged(route, form, rows, cus=CUS - RESERVE):
    """Some block walks at least three tiles (the first is never shorter than another) and the last block ends on a ragged tile."""
    T, rpb = ROUTES[route].T, rows_per_block(route, form, rows, cus)
    return cdiv(min(rpb, rows), T) >= 3 and (rows - (cdiv(rows, rpb) - 1) * rpb) % T != 0


MIN_ROWS = {"every": 1, "m64": 64, "m4096": 4096}


@functools.lru_cache(maxsize=None)
def m3(route, form):
    """The smallest row count the route admits at which, with RESERVE CUs held back, some block walks at least three tiles and the last block
    ends on a ragged tile."""
    rows = MIN_ROWS[ROUTES[route].rows]
    while not walks_three_tiles_and_ends_ragged(route, form, rows):
        rows += 1
    return rows


def sizes(route, form):
    """[(rows, reserve)]: the smallest row counts at which the kernel can still go wrong."""
    info = ROUTES[route]
    T = info.T
    plain = {"every": (1, T - 1, T, T + 1, 2 * T + 1), "m64": (64, 65, 64 + T + 1), "m4096": (4096, 4097, 4096 + T - 1)}[info.rows]
    out = [(r, 0) for r in plain]
    if route == "WGRAD_BF16":                     # the second kernel of the route, from K = 4096 on
        out += [(4096, 0), (4097, 0), (4096 + T - 1, 0)]
    if info.plan is not None:
        out.append((m3(route, form), RESERVE))
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def r4(x):
    return (x + 3) // 4 * 4


def r8(x):
    return (x + 7) // 8 * 8


class Case:
    """One clift_gemm launch.  form: fwd, dgrad_masked, dgrad_unmasked or wgrad (a label: the transposes are fields of their own);
    switches: the library's switch word; c_mis: bytes the C base lies off 16-byte alignment; reserve: clift_set_cu_reserve of the launch;
    signs: the LAYER_X6 forms that write ("write") / read ("read") sign bytes."""

    def __init__(self, route, form, M, N, K, precision=0, switches=0, a_trans=None, b_trans=None, lda=None, ldb=None, ldc=None, ldmask=None,
                 bias=0, act=0, accumulate=0, split_k=1, c_trans=0, colsum=0, signs=None, a_bf16=0, b_bf16=0, c_bf16=0, mask_bf16=0,
                 c_mis=0, reserve=0, seed=0, tag=""):
        self.route, self.form, self.M, self.N, self.K, self.precision, self.switches = route, form, M, N, K, precision, switches
        self.a_trans = int(form == "wgrad") if a_trans is None else a_trans
        self.b_trans = int(form != "fwd") if b_trans is None else b_trans
        self.mask = int(form == "dgrad_masked" and signs is None)
        self.bias, self.act, self.accumulate, self.split_k, self.c_trans, self.colsum, self.signs = bias, act, accumulate, split_k, c_trans, colsum, signs
        self.sign_bits = int(signs is not None)
        self.a_bf16, self.b_bf16, self.c_bf16, self.mask_bf16, self.c_mis, self.reserve, self.seed, self.tag = a_bf16, b_bf16, c_bf16, mask_bf16, c_mis, reserve, seed, tag
        ra, rb, rc = (r8 if a_bf16 else r4), (r8 if b_bf16 else r4), (r8 if c_bf16 else r4)
        # default pitches leave pad columns: one 16-byte chunk past the row
        self.lda = ra(self.a_cols) + (8 if a_bf16 else 4) if lda is None else lda
        self.ldb = rb(self.b_cols) + (8 if b_bf16 else 4) if ldb is None else ldb
        self.ldc = rc(M if c_trans else N) + (8 if c_bf16 else 4) if ldc is None else ldc
        self.ldmask = ((r8(N) + 8 if mask_bf16 else r4(N) + 4) if ldmask is None else ldmask) if self.mask else 0
        self.tag = tag = (tag + "_" if tag else "") + "m3" if reserve else tag
        self.name = f"M{M}_N{N}_K{K}" + (f"_{tag}" if tag else "")

    # stored shapes: A is (a_rows, lda) with a_cols meaningful columns, B likewise
    a_rows = property(lambda s: s.K if s.a_trans else s.M)
    a_cols = property(lambda s: s.M if s.a_trans else s.K)
    b_rows = property(lambda s: s.K if s.b_trans else s.N)
    b_cols = property(lambda s: s.N if s.b_trans else s.K)
    c_rows = property(lambda s: s.N if s.c_trans else s.M)
    c_cols = property(lambda s: s.M if s.c_trans else s.N)
    rows = property(lambda s: s.K if s.a_trans else s.M)          # the streamed (sample) rows: K in the weight-gradient forms
    key = property(lambda s: (s.route, s.form, s.name))

    def __repr__(self):
        return f"{self.route}:{self.form}:{self.name}"

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Case) and self.key == other.key


NARROW_KLDA = ((3, 4), (9, 12), (22, 24), (27, 28), (32, 32))      # cdiv(K, 8) = 1, 2, 3, 4, 4


def _sized(out, route, form, N, K, out_rows=None, **kw):
    """One case per row count of the route's size rule (the weight-gradient forms: K is the row count, ``out_rows`` is M)."""
    for rows, reserve in sizes(route, form):
        M_, K_ = (out_rows, rows) if form == "wgrad" else (rows, K)
        out.append(Case(route, form, M_, N, K_, reserve=reserve, seed=len(out) + 1, **kw))


def _tiled(out, route, N, precision, store):
    """The options of the tiled kernels (gemm.hip / gemm_bf16.hip), N picks the block tile.  ``store``: bf16 storage of the forward / dgrad forms
    and of the wgrad form."""
    T = ROUTES[route].T
    fs, ws = store
    K0, M0 = 40, T + 3
    add = lambda form, M, N_, K, **kw: out.append(Case(route, form, M, N_, K, precision=precision, seed=len(out) + 1, **kw))
    for rows, _ in sizes(route, "fwd"):                                                      # forward: bias, ReLU; every tile edge of M
        add("fwd", rows, N, K0, bias=1, act=1, **fs)
    add("fwd", M0, N, K0, bias=1, act=1, tag="masked", **fs)                                   # bias, ReLU and mask in one epilogue
    out[-1].mask, out[-1].ldmask = 1, (r8(N) + 8 if fs.get("c_bf16") else r4(N) + 4)
    out[-1].mask_bf16 = int(bool(fs.get("c_bf16")))
    add("dgrad_masked", M0, N, K0, mask_bf16=int(bool(fs.get("c_bf16"))), **fs)
    add("dgrad_unmasked", M0, N, K0, **fs)
    add("fwd", M0, N, 1, bias=1, tag="k1", **fs)                                               # K = 1
    add("fwd", M0, N, 33, bias=1, tag="k33", **fs)                                             # one k-tile and a ragged one
    add("dgrad_unmasked", M0, N, 33, tag="k33", **fs)
    if N >= 32 and N % 4:                                                                      # vector epilogue with its scalar tail
        add("fwd", M0, N, K0, bias=1, act=1, ldc=(r8(N) if fs.get("c_bf16") else r4(N)), tag="tail", **fs)
    else:
        add("fwd", M0, N - 2, K0, bias=1, act=1, tag="n_minus_2", **fs)                        # N not a multiple of 4
    add("fwd", M0, N, K0, bias=1, act=1, ldc=N + 1 + N % 2, tag="odd_ldc", **fs)               # odd pitch: the scalar epilogue
    add("fwd", M0, N, K0, bias=1, act=1, c_mis=4, tag="c_off4", **{k: v for k, v in fs.items() if k != "c_bf16"})
    nob = {k: v for k, v in fs.items() if k != "c_bf16"}                                       # (a bf16-stored C is neither transposed nor accumulated into)
    add("fwd", M0, N, K0, bias=1, c_trans=1, tag="c_trans", **nob)
    add("fwd", M0, N, K0, bias=1, act=1, accumulate=1, tag="accumulate", **nob)
    for sk in (1, 3):                                                                          # weight-gradient forms: K = the sample rows
        add("wgrad", 67, N, 200, accumulate=1, split_k=sk, colsum=1, tag=f"split{sk}", **ws)
    add("wgrad", 67, N, 200, accumulate=1, tag="no_colsum", **ws)
    add("wgrad", 131, N, 33, tag="overwrite", **ws)
    if not ws:                                                                                  # (a_trans, !b_trans): no instantiation for a bf16-stored A
        add("wgrad", 67, N, 200, b_trans=0, accumulate=1, split_k=3, colsum=1, tag="at_only")
        add("wgrad", 67, N, 33, b_trans=0, tag="at_only_overwrite")


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # ---- precision 2: fp32x6
    _sized(out, "LAYER_X6", "fwd", 256, 256, precision=2, bias=1, act=1)
    _sized(out, "LAYER_X6", "fwd", 256, 256, precision=2, bias=1, act=1, signs="write", tag="signs")
    _sized(out, "LAYER_X6", "dgrad_masked", 256, 256, precision=2)
    _sized(out, "LAYER_X6", "dgrad_masked", 256, 256, precision=2, signs="read", tag="signs")
    for cs in (1, 0):
        _sized(out, "WGRAD_X6", "wgrad", 256, None, precision=2, out_rows=256, accumulate=1, colsum=cs, tag=f"colsum{cs}")
    _sized(out, "LAYER_N6", "fwd", 128, 128, precision=2, bias=1, act=1)
    _sized(out, "LAYER_N6", "fwd", 128, 160, precision=2, bias=1, act=1)
    _sized(out, "LAYER_N6", "dgrad_masked", 128, 128, precision=2)
    _sized(out, "LAYER_N6", "dgrad_unmasked", 160, 128, precision=2)
    for N in (128, 160):
        for cs in (1, 0):
            _sized(out, "WGRAD_N6", "wgrad", N, None, precision=2, out_rows=128, accumulate=1, colsum=cs, tag=f"colsum{cs}")
    for rows, _ in sizes("SPLIT_TILED", "fwd"):
        out.append(Case("SPLIT_TILED", "fwd", rows, 72, 40, precision=2, bias=1, act=1, seed=len(out) + 1))
        out.append(Case("SPLIT_TILED", "fwd", rows, 256, 256, precision=2, switches=SW_X6_TILED, bias=1, act=1, seed=len(out) + 1, tag="x6_tiled"))
        out.append(Case("SPLIT_TILED", "dgrad_masked", rows, 256, 256, precision=2, switches=SW_X6_TILED, seed=len(out) + 1, tag="x6_tiled"))
    # ---- precision 0: exact fp32
    _sized(out, "LAYER_F32_FWD", "fwd", 256, 256, bias=1, act=1)
    _sized(out, "LAYER_F32_DGRAD", "dgrad_masked", 256, 256)
    for (K, lda), (form, N) in zip(NARROW_KLDA, (("dgrad_masked", 128), ("dgrad_unmasked", 36), ("dgrad_masked", 256), ("dgrad_unmasked", 144),
                                                 ("dgrad_unmasked", 256))):
        _sized(out, "DGRAD_NARROW", form, N, K, lda=lda, tag=f"lda{lda}")
    for cs in (1, 0):
        _sized(out, "WGRAD_F32_QUADS", "wgrad", 256, None, out_rows=256, accumulate=1, colsum=cs, tag=f"colsum{cs}")
    for N in (128, 160):
        for cs in (1, 0):
            _sized(out, "WGRAD_N128", "wgrad", N, None, out_rows=128, accumulate=1, colsum=cs, tag=f"colsum{cs}")
    _sized(out, "LAYER_N128", "fwd", 128, 128, bias=1, act=1)
    _sized(out, "LAYER_N128", "fwd", 128, 160, bias=1, act=1)
    _sized(out, "LAYER_N128", "dgrad_masked", 128, 128)
    _sized(out, "DGRAD_N160_PAIR", "dgrad_unmasked", 160, 128)
    for route, N in (("TILED_256X32", 32), ("TILED_128X128", 33), ("TILED_128X128", 128), ("TILED_128X256", 129)):
        _tiled(out, route, N, 0, ({}, {}))
    # ---- precision 1: bf16 operands
    st = dict(a_bf16=1, c_bf16=1)
    _sized(out, "LAYER_BF16", "fwd", 256, 256, precision=1, bias=1, act=1, **st)
    _sized(out, "LAYER_BF16", "dgrad_masked", 256, 256, precision=1, mask_bf16=1, **st)
    for cs in (1, 0):
        _sized(out, "WGRAD_BF16", "wgrad", 256, None, precision=1, out_rows=256, accumulate=1, colsum=cs, a_bf16=1, b_bf16=1, tag=f"colsum{cs}")
    for K, lda in ((3, 4), (22, 24)):
        _sized(out, "DGRAD_NARROW_BF16", "dgrad_masked", 256, K, precision=1, lda=lda, c_bf16=1, mask_bf16=1, tag=f"lda{lda}")
    _sized(out, "LAYER_NB16", "fwd", 128, 128, precision=1, bias=1, act=1, **st)
    _sized(out, "LAYER_NB16", "fwd", 128, 160, precision=1, bias=1, act=1, **st)
    _sized(out, "LAYER_NB16", "dgrad_masked", 128, 128, precision=1, mask_bf16=1, **st)
    _sized(out, "LAYER_NB16", "dgrad_unmasked", 160, 128, precision=1, tag="c_bf16", **st)
    _sized(out, "LAYER_NB16", "dgrad_unmasked", 160, 128, precision=1, a_bf16=1, tag="c_f32")
    for N in (128, 160):
        for cs in (1, 0):
            _sized(out, "WGRAD_NB16", "wgrad", N, None, precision=1, out_rows=128, accumulate=1, colsum=cs, a_bf16=1, b_bf16=1, tag=f"colsum{cs}")
    for route, N in (("TILED_BF16_256X32", 32), ("TILED_BF16_128X128", 33), ("TILED_BF16_128X128", 128), ("TILED_BF16_128X256", 129)):
        for tag, store in (("f32", ({}, {})), ("ac16", (dict(a_bf16=1, c_bf16=1), dict(a_bf16=1, b_bf16=1))), ("c16", (dict(c_bf16=1), {}))):
            first = len(out)
            _tiled(out, route, N, 1, store)
            if tag != "f32":                      # the storage variants: the forms that storage touches, at one M
                out[first:] = [c for c in out[first:] if c.M == ROUTES[route].T + 3 or (c.form == "wgrad" and store[1])]
            for c in out[first:]:
                c.tag = (c.tag + "_" if c.tag else "") + tag
                c.name = f"M{c.M}_N{c.N}_K{c.K}_{c.tag}"
    keys = [c.key for c in out]
    assert len(set(keys)) == len(keys), "case names must be unique"
    return tuple(out)


def groups():
    """{(route, form): [cases]} in table order."""
    out = {}
    for c in cases():
        out.setdefault((c.route, c.form), []).append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def bf16r(x):
    """Round to bf16 (RNE), as float32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _nonzero(rng, shape):
    """Ordinary values, none of them near zero: a dropped column or row always shows."""
    x = rng.standard_normal(shape).astype(np.float32)
    return np.where(np.abs(x) < 0.05, np.float32(0.05) * np.where(x < 0, np.float32(-1), np.float32(1)), x)


MASK_SPECIALS = (0.0, -0.0, 2.0 ** -130, -(2.0 ** -130), float("inf"))         # 2^-130: a denormal of fp32 and of bf16


def _store(logical, rows_alloc, ld, trans, pad_value, bf16):
    """The stored image of a logical (r, c) matrix: (rows_alloc, ld), transposed if ``trans``, pad columns = pad_value, rows past it NaN."""
    x = logical.T if trans else logical
    buf = np.full((rows_alloc, ld), np.nan, dtype=np.float32)
    buf[:x.shape[0], :] = pad_value
    buf[:x.shape[0], :x.shape[1]] = x
    return bf16r(buf) if bf16 else buf


def _draw(c, seed):
    rng = np.random.default_rng(7000 + seed)
    info = ROUTES[c.route]
    M, N, K, T = c.M, c.N, c.K, info.T
    A = _nonzero(rng, (M, K)) * np.exp2(rng.integers(-6, 7, (M, 1))).astype(np.float32)        # rows differ in scale
    B = _nonzero(rng, (N, K)) * np.exp2(rng.integers(-2, 3, (N, 1))).astype(np.float32) / np.float32(max(K, 1) ** 0.5)
    if c.a_bf16:
        A = bf16r(A)
    if c.b_bf16:
        B = bf16r(B)
    a_pad = PAD_FINITE if info.pad == "times_zero" else np.nan
    d = {"A": _store(A, c.a_rows + T, c.lda, c.a_trans, a_pad, c.a_bf16), "B": _store(B, c.b_rows + T, c.ldb, c.b_trans, np.nan, c.b_bf16)}
    d["bias"] = _nonzero(rng, (N,)) if c.bias else None
    C0 = np.full((c.c_rows + 2, c.ldc), SENTINEL, dtype=np.float32)
    if c.accumulate:
        # accumulated into: values of the size of the product itself (its root-mean-square over the signs of the terms), as a gradient
        # buffer holds them -- not of the size of S = |A| |B|, which would put the bound's |C0| term above every error of the k-sum
        rms = np.sqrt((A.astype(np.float64) ** 2) @ (B.astype(np.float64) ** 2).T)
        pre = (rng.standard_normal((M, N)) * rms).astype(np.float32)
        C0[:c.c_rows, :c.c_cols] = pre.T if c.c_trans else pre
    d["C0"] = C0
    if c.mask or c.signs == "read":
        mk = _nonzero(rng, (M, N))
        flat = mk.reshape(-1)
        for j, v in enumerate(MASK_SPECIALS):
            flat[j::11 + j] = np.float32(v)
        if c.signs == "read":                     # the sign bytes of a forward: its activation, relu(.) >= 0
            mk = np.maximum(mk, 0).astype(np.float32)
            mk[np.isinf(mk)] = 1.0
        d["mask"] = _store(mk, M + T, c.ldmask if c.mask else r4(N), 0, np.nan, c.mask_bf16)
    else:
        d["mask"] = None
    if c.colsum:
        cs = np.full((M + 2,), SENTINEL, dtype=np.float32)
        cs[:M] = (rng.standard_normal(M) * np.sqrt((A.astype(np.float64) ** 2).sum(1))).astype(np.float32)
        d["colsum0"] = cs
    else:
        d["colsum0"] = None
    return d


@functools.lru_cache(maxsize=2)
def inputs(c):
    """Stored arrays of the case as float32 numpy (a bf16-stored tensor holds bf16-representable values): A, B, C0 (the output's pre-fill:
    sentinels, and the accumulated-into values), bias, mask, colsum0.  A draw whose yardstick is ill-conditioned is redrawn."""
    seed = c.seed
    for _ in range(8):
        d = _draw(c, seed)
        d["_ref"] = _reference(c, d)
        d["_yard"] = _yardsticks(c, d)
        if max(d["_yard"].values()) <= ILL_CONDITIONED:
            return d
        seed += 1000
    raise AssertionError(f"{c}: no well-conditioned draw")


def logical(c, d, rows=None):
    """(A (M, K), B (N, K), bias, mask (M, N) or None, C0 (M, N), colsum0 (M)) as stored, untransposed; ``rows``: only the first rows of the
    streamed dimension."""
    M, N, K = c.M, c.N, c.K
    if rows is not None:
        M, K = (M, rows) if c.a_trans else (rows, K)
    A = d["A"][:K, :M].T if c.a_trans else d["A"][:M, :K]
    B = d["B"][:K, :N].T if c.b_trans else d["B"][:N, :K]
    mask = None if d["mask"] is None else d["mask"][:M, :N]
    C0 = d["C0"][:N, :M].T if c.c_trans else d["C0"][:M, :N]
    cs0 = None if d["colsum0"] is None else d["colsum0"][:M]
    return A, B, d["bias"], mask, C0, cs0


def _operands(c, A, B):
    """The operands as the kernel multiplies them: rounded to bf16 where the route's kernel rounds them (a bf16-stored one already is)."""
    if ROUTES[c.route].rounds:
        return bf16r(A), bf16r(B)
    return A, B


# ---------------------------------------------------------------------------------------------------------------- reference, restatement
def _reference(c, d, rows=None, mask=None):
    A, B, bias, mk, C0, cs0 = logical(c, d, rows)
    mk = mk if mask is None else mask
    Ar, Br = _operands(c, A, B)
    A64, B64 = Ar.astype(np.float64), Br.astype(np.float64)
    v = A64 @ B64.T
    S = np.abs(A64) @ np.abs(B64).T
    if bias is not None:
        v, S = v + bias.astype(np.float64), S + np.abs(bias.astype(np.float64))
    if c.act == 1:
        v = np.maximum(v, 0.0)
    if mk is not None:
        v = np.where(mk > 0, v, 0.0)
    if c.accumulate:
        v, S = v + C0.astype(np.float64), S + np.abs(C0.astype(np.float64))
    out = {"C": v, "S_C": S}
    if c.colsum:
        out["colsum"] = cs0.astype(np.float64) + A64.sum(1)
        out["S_colsum"] = np.abs(cs0.astype(np.float64)) + np.abs(A64).sum(1)
    return out


def reference(c):
    """fp64 on the values as stored: {"C": (M, N), "colsum": (M), and the elementwise scales "S_C", "S_colsum"} (C before any bf16 rounding of a
    bf16-stored output: ``check`` rounds it)."""
    return inputs(c)["_ref"]


def reference_of(c, rows=None, mask=None):
    """... of the first ``rows`` streamed rows only (the device row limit), or under another mask (the sign bytes a forward wrote)."""
    return _reference(c, inputs(c), rows, mask)


def probe(c):
    """(rows, columns) of the output elements the fp32 restatement is evaluated on: everything for a small case, else the tile edges, the
    ragged last tile and the column edges, at most PROBE_PRODUCTS products."""
    M, N, K, T = c.M, c.N, c.K, ROUTES[c.route].T
    if M * N * K <= PROBE_PRODUCTS:
        return np.arange(M), np.arange(N)
    budget = max(PROBE_PRODUCTS // K, 16)
    col_edges = [0, N - 1, N - 4, 31, 32, N - 2, 1, N - 3, 127, 128, 63, 64, 33, 129, 3, 4, N - 5]
    row_edges = [0, M - 1, ((M - 1) // T) * T, T - 1, T, M - 2, T + 1, 2 * T, 2 * T - 1, 1, M // 2]
    ncol = N if c.form != "wgrad" else max(4, min(N, int(budget ** 0.5)))
    return _take(row_edges, max(4, budget // ncol), M), _take(col_edges, ncol, N)


def _take(edges, n, lim):
    """n of range(lim), the edges first (in their order of importance), sorted."""
    if n >= lim:
        return np.arange(lim)
    seen = []
    for e in list(edges) + list(range(lim)):
        if 0 <= e < lim and e not in seen:
            seen.append(e)
            if len(seen) == n:
                break
    return np.array(sorted(seen), dtype=np.int64)


def split3(x):
    """x = x1 + x2 + x3 exactly, each term a bf16 (gemm_split.hip)."""
    x1 = bf16r(x)
    r1 = (x - x1).astype(np.float32)
    x2 = bf16r(r1)
    return x1, x2, bf16r((r1 - x2).astype(np.float32))


MISTAKES = ("k_last_chunk_dropped", "ragged_tile_rows_from_previous_tile", "mask_one_tile_late", "mask_ge", "bias_missing_on_last_quad",
            "relu_after_mask", "accumulate_overwrites", "colsum_overwrites", "c_trans_ignored", "pad_column_contracted",
            "row_past_count_reduced", "x6_middle_term_dropped")


def _ordered_sum(terms, order):
    """Running fp32 sum over the last axis, the terms taken in ``order``: one rounding per addition, as an accumulator chain adds them."""
    n = terms.shape[-1]
    if n == 0:
        return np.zeros(terms.shape[:-1], np.float32)
    if order != "natural" and n > 1:
        terms = terms[..., lc._index(n, order).numpy()]
    return np.cumsum(terms, axis=-1, dtype=np.float32)[..., -1]


def _ksum(Ap, Bp, order, c, mistake, bias=None):
    """bias[j] + sum_k Ap[i][k] Bp[j][k] in fp32 as ONE running sum in ``order`` -- the bias is a term of the sum like the products (the
    persistent forward kernels enter it as one more contraction step; "natural" has it first, "reversed" last); fp32x6 routes: three bf16 terms
    per operand, the six leading products (each exact in fp32) added smallest first."""
    f = np.float32
    Ap, Bp = np.ascontiguousarray(Ap, dtype=f), np.ascontiguousarray(Bp, dtype=f)
    pr = lambda a, b: a[:, None, :] * b[None, :, :]
    if ROUTES[c.route].split:
        (a1, a2, a3), (b1, b2, b3) = split3(Ap), split3(Bp)
        if mistake == "x6_middle_term_dropped":
            a2 = np.zeros_like(a2)
        prod = (((pr(a3, b1) + pr(a2, b2)) + pr(a1, b3)) + (pr(a2, b1) + pr(a1, b2))) + pr(a1, b1)
    else:
        prod = pr(Ap, Bp)
    if bias is not None:
        prod = np.concatenate([np.broadcast_to(bias.astype(f)[None, :, None], prod.shape[:2] + (1,)), prod], 2)
    return _ordered_sum(prod, order)


def _restate(c, d, order, mistake, stored=True):
    A, B, bias, mk, C0, cs0 = logical(c, d)
    M, N, K, T = c.M, c.N, c.K, ROUTES[c.route].T
    ri, ci = probe(c)
    A, B = _operands(c, A, B)
    streamed_k = bool(c.a_trans)                   # the sample rows run along k
    if mistake == "ragged_tile_rows_from_previous_tile":
        n = K if streamed_k else M
        first = ((n - 1) // T) * T
        if first > 0 and n % T:
            if streamed_k:
                A, B = A.copy(), B.copy()
                A[:, first:], B[:, first:] = A[:, first - T:n - T], B[:, first - T:n - T]
            else:
                A = A.copy()
                A[first:] = A[first - T:M - T]
    if mistake == "k_last_chunk_dropped":
        keep = K - min(4, K)
        A, B = A[:, :keep], B[:, :keep]
    Ap, Bp = A[ri], B[ci]
    if mistake == "pad_column_contracted":         # column K of both stored rows joins the sum
        if not c.a_trans and c.lda > K and (c.b_trans or c.ldb > K):
            pa, pb = d["A"][:M, K][ri], (d["B"][K, :N] if c.b_trans else d["B"][:N, K])[ci]
            Ap, Bp = np.concatenate([Ap, pa[:, None]], 1), np.concatenate([Bp, pb[:, None]], 1)
    if mistake == "row_past_count_reduced" and streamed_k:
        Ap = np.concatenate([Ap, d["A"][K, :M][ri][:, None]], 1)
        Bp = np.concatenate([Bp, (d["B"][K, :N] if c.b_trans else d["B"][:N, K] if c.ldb > K else np.full(N, np.nan, np.float32))[ci][:, None]], 1)
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        b = None
        if bias is not None:
            b = bias[ci].copy()
            if mistake == "bias_missing_on_last_quad":
                b[ci >= N - (N % 4 or 4)] = 0
        on = None
        if mk is not None:
            mrows = np.maximum(ri - T, 0) if mistake == "mask_one_tile_late" else ri
            mp = mk[mrows][:, ci]
            on = (mp >= 0) if mistake == "mask_ge" else (mp > 0)
        if mistake == "relu_after_mask" and on is not None:          # the mask falls on the sum, the bias and the ReLU come after it
            v = np.where(on, _ksum(Ap, Bp, order, c, mistake), f(0))
            v, on = (v if b is None else (v + b[None, :]).astype(f)), None
        else:
            v = _ksum(Ap, Bp, order, c, mistake, b)
        if c.act == 1:
            v = np.maximum(v, f(0))
        if on is not None:
            v = np.where(on, v, f(0))
        if mistake == "c_trans_ignored" and c.c_trans:
            full = (A.astype(f) @ B.astype(f).T + (0 if bias is None else bias[None, :])).astype(f)
            v = np.array([[full[n, m] if (n < M and m < N) else f(SENTINEL) for n in ci] for m in ri], dtype=f)
        raw = v.astype(np.float64)
        if c.accumulate and mistake != "accumulate_overwrites":
            v = (v + C0[ri][:, ci]).astype(f)
            raw = v.astype(np.float64)
        if c.c_bf16 and stored:
            v = bf16r(v)
        out = {"C": v, "raw_C": raw}
        if c.colsum:
            s = _ordered_sum(np.ascontiguousarray(Ap, dtype=f), order)
            out["colsum"] = s if mistake == "colsum_overwrites" else (cs0[ri] + s).astype(f)
    return out


def restate(c, order="natural", mistake=None):
    """{"C": fp32 (probe rows, probe columns), "colsum": (probe rows)}: the operation in fp32 with one rounding per operation, the k-sum in
    ``order``, optionally with one of MISTAKES built in; as stored (a bf16-stored output rounded once)."""
    out = _restate(c, inputs(c), order, mistake)
    out.pop("raw_C")
    return out


def _yardsticks(c, d):
    ref = d["_ref"]
    ri, ci = probe(c)
    out = {"C": 0.0, "colsum": 0.0}
    for order in ORDERS:
        r = _restate(c, d, order, None)
        out["C"] = max(out["C"], float(np.max(np.abs(r["raw_C"] - ref["C"][ri][:, ci]) / ref["S_C"][ri][:, ci])))
        if c.colsum:
            out["colsum"] = max(out["colsum"], float(np.max(np.abs(r["colsum"].astype(np.float64) - ref["colsum"][ri]) / ref["S_colsum"][ri])))
    return out


@functools.lru_cache(maxsize=None)
def yardsticks(c):
    """{"C", "colsum"}: the largest |fp32 restatement - fp64| / S over the probe and the three orders (before the rounding of a bf16-stored output)."""
    return dict(inputs(c)["_yard"])


def bound_factor(yard):
    return 8.0 * yard + 4.0 * HALF_ULP


# Bounds that had to be widened on the device for a reason that is not a bug: (route, form, case name, quantity): (largest error / S measured
# over repeated launches of that case, the plain factor 8 * yardstick + 4 * 2^-24 it missed); the new factor is twice the measured one.
WIDENED = {}


def factor_for(c, quantity):
    f = bound_factor(yardsticks(c)[quantity])
    entry = WIDENED.get((c.route, c.form, c.name, quantity))
    return max(f, 2.0 * entry[0]) if entry is not None else f


def check(got, c, ref=None, rows=None):
    """The one comparison of both test files.  got: {"C": (M, N) logical, or (probe rows, probe columns) of a restatement; "colsum": likewise}.
    Returns (ok, worst error / bound, text).  ``ref``: another reference than reference(c) (``reference_of``); ``rows``: the output rows
    compared (row-limit test)."""
    ref = reference(c) if ref is None else ref
    ri, ci = probe(c)
    worst, notes = 0.0, []
    for q in ("C", "colsum"):
        if q not in ref:
            continue
        g = np.asarray(got[q], dtype=np.float64)
        r, S = ref[q], ref["S_" + q]
        if g.shape != r.shape:                     # a restatement: the probe's elements
            r, S = (r[ri][:, ci], S[ri][:, ci]) if q == "C" else (r[ri], S[ri])
        if g.shape != r.shape:
            return False, float("inf"), f"{c}: {q} has shape {g.shape}, expected {r.shape}"
        if rows is not None and q == "C":
            g, r, S = g[:rows], r[:rows], S[:rows]
        bnd = factor_for(c, q) * S
        if q == "C" and c.c_bf16:
            # One bf16 rounding moves a value by at most half the spacing of an 8-bit significand, 2^-8 |value|.  The allowance is taken around
            # the reference itself, not around its bf16 rounding: a value within the fp32 bound of a rounding boundary may round to either
            # neighbour, and the two neighbours are a whole spacing apart -- up to 2^-7 |value|, which no correct kernel could be held to from
            # the far side (the fp32 restatement itself lands there in about one element of a few hundred).
            bnd = bnd + BF16_HALF_SPACING * np.abs(r)
        with np.errstate(invalid="ignore"):
            err = np.abs(g - r)
            ratio = np.where(err <= bnd, err / np.maximum(bnd, 1e-300), np.inf)      # a NaN error breaks the bound
        w = float(ratio.max()) if ratio.size else 0.0
        worst = max(worst, w)
        if not w <= 1.0:
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            notes.append(f"{q}{tuple(int(i) for i in at)}: got {g[at]!r}, reference {r[at]!r}, bound {bnd[at]:.3e}")
    return not notes, worst, f"{c}: " + ("; ".join(notes) if notes else f"worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- the descriptor
def descriptor(c, addr):
    """The clift_gemm_t of a case.  addr: {A, B, C, bias, mask, colsum, sign_bits, workspace: address} -- 16-byte-aligned bases; the case's
    misalignment of C is added here."""
    from contrastive_lift_amd._lib import Gemm
    g = Gemm()
    g.M, g.N, g.K = c.M, c.N, c.K
    g.A, g.lda, g.a_trans = addr["A"], c.lda, c.a_trans
    g.B, g.ldb, g.b_trans = addr["B"], c.ldb, c.b_trans
    g.C, g.ldc = addr["C"] + c.c_mis, c.ldc
    g.bias, g.act = (addr["bias"] if c.bias else None), c.act
    g.mask, g.ldmask = (addr["mask"] if c.mask else None), c.ldmask
    g.accumulate, g.split_k, g.c_trans = c.accumulate, c.split_k, c.c_trans
    g.colsum = addr["colsum"] if c.colsum else None
    g.sign_bits = addr["sign_bits"] if c.sign_bits else None
    g.a_bf16, g.b_bf16, g.c_bf16, g.mask_bf16 = c.a_bf16, c.b_bf16, c.c_bf16, c.mask_bf16
    g.precision = c.precision
    if addr.get("workspace"):
        g.workspace, g.workspace_bytes = addr["workspace"], addr.get("workspace_bytes", 1 << 40)
    return g
