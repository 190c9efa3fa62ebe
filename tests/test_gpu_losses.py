"""Every entry point of csrc/losses.hip against the fp64 references of tests/loss_cases.py, called through _lib.call with raw pointers (null
arguments and pitches are reachable that way) and, where one exists, through its Python wrapper.

A device result is held to |device - fp64| <= 8 * yardstick + 4 * 2^-24 * scale (loss_cases.bound; loss_cases.WIDENED lists the three
sums of clift_tv_fwd_bwd over hundreds of blocks that need more, and why); each test prints
``yardstick | device error | bound`` per case and quantity.  Refusals are tested only where CLIFT_REQUIRE rejects on the host, before any
launch."""
import ctypes as C

import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SENTINEL = 123.0


def _L():
    from contrastive_lift_amd import _lib
    _lib.load()
    return _lib


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


class Table:
    """Rows of ``yardstick | device error | bound``; ``hold`` records a row and remembers a break."""

    def __init__(self):
        self.rows, self.broken = [], []

    def hold(self, case, q, dev, how="raw"):
        self.add(case, q, how, lc.yardstick(case, q), lc.max_error(dev, lc.reference(case)[q]), lc.bound_for(case, q, how))

    def add(self, case, q, how, yard, err, bnd):
        self.rows.append(f"{case.kernel:11s} {case.name:34s} {q:6s} {how:7s} | {yard:9.3e} | {err:9.3e} | {bnd:9.3e}")
        if lc.exceeds(err, bnd):
            self.broken.append(self.rows[-1])

    def fail(self, case, what):
        self.broken.append(f"{case}: {what}")

    def close(self, capsys):
        with capsys.disabled():
            print("\nkernel      case                               what   call    | yardstick | dev error | bound\n" + "\n".join(self.rows))
        assert not self.broken, "outside the bound:\n" + "\n".join(self.broken)


# ---------------------------------------------------------------------------------------------------------------- contrastive
def _contrastive(L, c, want_grad):
    f, y = _d(c.f), _d(c.y.to(torch.int32))
    B, E = f.shape
    loss = torch.full((1,), SENTINEL, device=DEV)
    g = torch.full_like(f, SENTINEL) if want_grad else None
    work = torch.empty((max(4 * B, 4),), device=DEV)
    L.call("clift_contrastive", L.ptr(f), L.ptr(y), B, E, c.temperature, L.ptr(loss), L.ptr(g), L.ptr(work), L.stream())
    return loss[0].cpu(), None if g is None else g.cpu()


def test_contrastive(capsys):
    from contrastive_lift_amd import loss as closs
    L, t = _L(), Table()
    for c in lc.contrastive_cases():
        loss, g = _contrastive(L, c, True)
        t.hold(c, "loss", loss)
        t.hold(c, "grad", g)
        loss, _ = _contrastive(L, c, False)                  # g_feat == NULL: the same loss
        t.hold(c, "loss", loss, "nograd")
        loss, g = closs.contrastive_loss(_d(c.f), _d(c.y), c.temperature, return_grad=True)
        t.hold(c, "loss", loss.cpu(), "wrapper")
        t.hold(c, "grad", g.cpu(), "wrapper")
        if c.labels == "distinct":
            assert float(loss) == 0.0 and float(g.abs().max()) == 0.0, c
    t.close(capsys)


def test_instance_losses_refuse_e_above_32():
    L = _L()
    f, y = torch.zeros((4, lc.CL_MAXE + 1), device=DEV), torch.zeros((4,), dtype=torch.int32, device=DEV)
    loss, g, work = torch.zeros((1,), device=DEV), torch.zeros_like(f), torch.zeros((16,), device=DEV)
    with pytest.raises(L.CliftError):
        L.call("clift_contrastive", L.ptr(f), L.ptr(y), 4, lc.CL_MAXE + 1, 100.0, L.ptr(loss), L.ptr(g), L.ptr(work), L.stream())
    with pytest.raises(L.CliftError):
        L.call("clift_slow_fast", L.ptr(f), L.ptr(y), L.ptr(loss), 4, lc.CL_MAXE + 1, L.ptr(loss), None, L.ptr(work), L.stream())


# ---------------------------------------------------------------------------------------------------------------- slow-fast
def test_slow_fast(capsys):
    from contrastive_lift_amd import loss as closs
    L, t = _L(), Table()
    for c in lc.slow_fast_cases():
        x, y, conf = _d(c.inst), _d(c.y.to(torch.int32)), _d(c.conf)
        B, E = x.shape[0], x.shape[1] // 2
        H = B // 2
        loss, g = torch.full((1,), SENTINEL, device=DEV), torch.full_like(x, SENTINEL)
        work = torch.empty((8 * B + 2 * B * E + 8,), device=DEV)
        L.call("clift_slow_fast", L.ptr(x), L.ptr(y), L.ptr(conf), B, E, L.ptr(loss), L.ptr(g), L.ptr(work), L.stream())
        wl, wg = closs.slow_fast_loss(x, _d(c.y), conf, return_grad=True)
        for how, lo, gr in (("raw", loss[0].cpu(), g.cpu()), ("wrapper", wl.cpu(), wg.cpu())):
            t.hold(c, "loss", lo, how)                       # (a NaN reference -- no label in common -- needs a NaN here: lc.max_error)
            t.hold(c, "grad", gr, how)
            if float(gr[H:].abs().max()) != 0.0:
                t.fail(c, f"{how}: gradient rows of the slow ray set are not exactly zero")
            if float(gr[:, E:].abs().max()) != 0.0:
                t.fail(c, f"{how}: the slow column half is not exactly zero")
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- pixel losses
def test_pixel_losses(capsys):
    L, t = _L(), Table()
    for c in lc.pixel_cases():
        ins = [_d(getattr(c, k)) for k in ("rgb", "gt", "sem", "probs", "conf", "class_w", "maskf")]
        out2 = _d(c.prefill.clone())
        g_rgb = torch.full((c.N, 3), SENTINEL, device=DEV) if c.want_g_rgb else None
        g_sem = torch.full((c.N, c.C), SENTINEL, device=DEV) if c.want_g_sem else None
        head = [L.ptr(x) for x in ins] + [c.N, c.C, c.w_rgb, c.w_sem]
        tail = [L.ptr(out2), L.ptr(g_rgb), L.ptr(g_sem), L.stream()]
        if c.sce:
            L.call("clift_pixel_losses_sce", *head, c.alpha, c.beta, *tail)
        else:
            L.call("clift_pixel_losses", *head, *tail)
        out2 = out2.cpu()
        t.hold(c, "out0", out2[0])
        t.hold(c, "out1", out2[1])
        ref = lc.reference(c)
        for q, g in (("g_rgb", g_rgb), ("g_sem", g_sem)):
            if q in ref:
                t.hold(c, q, g.cpu())
            elif g is not None and not bool((g == SENTINEL).all()):          # its input pair is null: nothing may be written
                t.fail(c, f"{q} was written although its inputs are null")
    t.close(capsys)


def test_semantic_loss_rows(capsys):
    from contrastive_lift_amd import loss as closs
    L, t = _L(), Table()
    for c in lc.rows_cases():
        x, p, cw = _d(c.pred), _d(c.probs), _d(c.class_w)
        rows = torch.full((c.N,), SENTINEL, device=DEV)
        g = torch.full_like(x, SENTINEL) if c.want_grad else None
        L.call("clift_semantic_loss_rows", L.ptr(x), L.ptr(p), L.ptr(cw), c.N, c.C, c.sce, c.alpha, c.beta, L.ptr(rows), L.ptr(g), L.stream())
        t.hold(c, "rows", rows.cpu())
        if c.want_grad:
            t.hold(c, "grad", g.cpu())
            xw = x.clone().requires_grad_(True)
            fn = closs.SCELoss(c.alpha, c.beta, cw) if c.sce else closs.SoftTargetCrossEntropy(cw)
            wr = fn(xw, p)
            t.hold(c, "rows", wr.detach().cpu(), "wrapper")
            t.hold(c, "grad", torch.autograd.grad(wr.sum(), xw)[0].cpu(), "wrapper")
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- segment consistency
def test_segment_loss(capsys):
    L, t = _L(), Table()
    for c in lc.segment_cases():
        feats = torch.full((c.B, c.ld), 9.0, device=DEV)
        feats[:, :c.C] = _d(c.feats)
        group, conf, cw = _d(c.group.to(torch.int32)), _d(c.conf), _d(c.class_w)
        work = torch.full((c.G * c.C + c.G,), SENTINEL, device=DEV)          # (the call zeroes it)
        loss = _d(c.prefill.reshape(1).clone())
        g = torch.full((c.B, c.ldg), SENTINEL, device=DEV) if c.want_grad else None
        L.call("clift_segment_loss", L.ptr(feats), c.ld, L.ptr(group), L.ptr(conf), L.ptr(cw), c.B, c.C, c.G, c.scale, L.ptr(work), L.ptr(loss),
               L.ptr(g), c.ldg, L.stream())
        t.hold(c, "loss", loss[0].cpu())
        if c.want_grad:
            g = g.cpu()
            t.hold(c, "grad", g[:, :c.C])
            if not bool((g[:, c.C:] == SENTINEL).all()):
                t.fail(c, "the padding of the gradient rows was written")
        if c.exact:          # first maximum: the sums are exact, so the kernel's work buffer holds the reference's, bit for bit
            assert torch.equal(work[:c.G * c.C].cpu().reshape(c.G, c.C).to(F64), lc.segment_sums(c)), c
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- total variation
def _tv_single(L, x, weight, grad, loss):
    H, W, Cc = x.shape
    L.call("clift_tv_fwd_bwd", L.ptr(x), H, W, Cc, weight, L.ptr(grad), L.ptr(loss), L.stream())


def test_tv(capsys):
    from contrastive_lift_amd import loss as closs
    L, t = _L(), Table()
    for c in lc.tv_cases():
        x, g, loss = _d(c.planes[0]), _d(c.grad_prefill[0]), _d(c.loss_prefill.reshape(1).clone())
        if g is not None:
            g = g.clone()
        _tv_single(L, x, c.weights[0], g, loss)
        t.hold(c, "loss", loss[0].cpu())
        if g is not None:
            t.hold(c, "grad0", g.cpu())
        elif c.weights[0] == 1.0 and float(c.loss_prefill) == 0.0:
            t.hold(c, "loss", closs.TVLoss()(x.permute(2, 0, 1)[None]).cpu(), "wrapper")
    t.close(capsys)


def _tv_set(L, planes, grads, weights):
    ts = L.TVSet()
    ts.n = len(planes)
    for i, (x, g, w) in enumerate(zip(planes, grads, weights)):
        ts.plane[i], ts.grad[i] = x.data_ptr(), (g.data_ptr() if g is not None else None)
        ts.H[i], ts.W[i], ts.C[i], ts.weight[i] = x.shape[0], x.shape[1], x.shape[2], w
    return ts


def test_tv_multi(capsys):
    """One launch for a set of planes; the same planes through the single-plane kernel are held to the same bound."""
    L, t = _L(), Table()
    for c in lc.tv_multi_cases():
        planes = [_d(x) for x in c.planes]
        for how in ("multi", "single"):
            grads = [None if g is None else _d(g).clone() for g in c.grad_prefill]
            loss = _d(c.loss_prefill.reshape(1).clone())
            if how == "multi":
                ts = _tv_set(L, planes, grads, c.weights)
                L.call("clift_tv_fwd_bwd_multi", C.byref(ts), L.ptr(loss), L.stream())
            else:
                for x, g, w in zip(planes, grads, c.weights):
                    _tv_single(L, x, w, g, loss)
            t.hold(c, "loss", loss[0].cpu(), how)
            for i, g in enumerate(grads):
                if g is not None:
                    t.hold(c, f"grad{i}", g.cpu(), how)
    t.close(capsys)


def test_tv_multi_planes_below_four_elements():
    """A set whose planes all have fewer than four elements used to size its grid to zero blocks: an error return, where the answer is
    loss += weight * TV (zero for the (1, 1, 3) plane, not zero for the (1, 3, 1) plane)."""
    L = _L()
    x = torch.tensor([1.0, -2.0, 0.5], device=DEV)
    for shape, want in (((1, 1, 3), 0.0), ((1, 3, 1), 2.0 * (9.0 + 6.25) / (2.0 + 1e-4))):
        loss, g = torch.full((1,), 0.25, device=DEV), torch.zeros((3,), device=DEV)
        ts = _tv_set(L, [x.reshape(shape)], [g.reshape(shape)], [0.5])
        L.call("clift_tv_fwd_bwd_multi", C.byref(ts), L.ptr(loss), L.stream())
        assert abs(float(loss[0]) - (0.25 + 0.5 * want)) <= 1e-6 * (0.25 + 0.5 * want), (shape, float(loss[0]))
        assert (float(g.abs().max()) == 0.0) == (want == 0.0), (shape, g)


def test_tv_multi_refusals():
    L = _L()
    x, loss = torch.zeros((4, 4, 8), device=DEV), torch.zeros((1,), device=DEV)
    ts = _tv_set(L, [x], [None], [1.0])
    ts.n = lc.TV_MAX + 1
    with pytest.raises(L.CliftError):
        L.call("clift_tv_fwd_bwd_multi", C.byref(ts), L.ptr(loss), L.stream())
    ts = _tv_set(L, [x], [None], [1.0])
    ts.plane[0] = x.data_ptr() + 4                           # not 16-byte aligned
    ts.H[0] = 3
    with pytest.raises(L.CliftError):
        L.call("clift_tv_fwd_bwd_multi", C.byref(ts), L.ptr(loss), L.stream())
    assert float(loss[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------- Adam / EMA
def _padded(t, off):
    """A device buffer with sentinels on both sides of ``t``, and the view that holds t (at an odd element offset for off = 3)."""
    buf = torch.full((off + t.numel() + 5,), SENTINEL, device=DEV)
    buf[off:off + t.numel()] = t.to(DEV)
    return buf, buf[off:off + t.numel()]


def _sentinels_intact(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


class Worst:
    """Per kind of quantity (the first letter of its name), the step and element that came closest to its bound, or went furthest past it."""

    def __init__(self):
        self.kept = {}

    def offer(self, q, yard, err, bnd):
        """err: |device - fp64| per element; bnd: one bound, or one per element.  A NaN error counts as past any bound."""
        bnd = torch.as_tensor(bnd, dtype=F64).expand_as(err)
        ratio = (err / bnd.clamp(min=1e-300)).nan_to_num(nan=float("inf"))
        ratio = torch.where((err == 0) & (bnd == 0), torch.zeros_like(ratio), ratio)
        i = int(torch.argmax(ratio))
        if q[0] not in self.kept or float(ratio[i]) > self.kept[q[0]][0]:
            self.kept[q[0]] = (float(ratio[i]), q, yard, float(err[i]), float(bnd[i]))

    def rows(self):
        return [row[1:] for _, row in sorted(self.kept.items())]


def test_adam(capsys):
    """m, v and p after each of steps 1..5 and then step 1000 against torch.optim.Adam in fp64.  p is held through its step
    p<k> - p<k-1> (per element: half an fp32 ulp at |p| plus the bound of the step) and, summed over the steps so far, on p itself."""
    L, t = _L(), Table()
    for ci, c in enumerate(lc.adam_cases()):
        off = 3 if ci % 2 == 0 else 0
        ref = lc.reference(c)
        bufs = [_padded(x, off) for x in (c.p0, torch.zeros(c.n), torch.zeros(c.n))]
        (pb, p), (mb, m), (vb, v) = bufs
        before, allowed = c.p0.to(F64), torch.zeros(c.n, dtype=F64)
        worst = Worst()
        for k, step in enumerate(lc.ADAM_STEPS):
            g = _d(c.grads[k])
            L.call("clift_adam", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), c.n, c.lr, c.beta1, c.beta2, lc.ADAM_EPS, c.wd, step, L.stream())
            now = p.cpu().to(F64)
            for q, dev in ((f"m{k}", m.cpu()), (f"v{k}", v.cpu())):
                worst.offer(q, lc.yardstick(c, q), (dev.to(F64) - ref[q]).abs(), lc.bound_for(c, q))
            bnd = lc.adam_step_bound(c, k)
            allowed = allowed + bnd
            worst.offer(f"d{k}", lc.yardstick(c, f"d{k}"), ((now - before) - ref[f"d{k}"]).abs(), bnd)
            worst.offer(f"p{k}", lc.yardstick(c, f"d{k}"), (now - ref[f"p{k}"]).abs(), allowed)
            before = now
        for q, yard, err, bnd in worst.rows():
            t.add(c, q, "raw", yard, err, bnd)
        if not all(_sentinels_intact(b, off, c.n) for b in (pb, mb, vb)):
            t.fail(c, "elements outside the range were written")
    t.close(capsys)


def test_adam_refuses_step_zero():
    L = _L()
    p, g, m, v = (torch.zeros((8,), device=DEV) for _ in range(4))
    with pytest.raises(L.CliftError):
        L.call("clift_adam", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 8, 1e-2, 0.9, 0.99, 1e-8, 0.0, 0, L.stream())


def test_ema(capsys):
    from contrastive_lift_amd import loss as closs
    L, t = _L(), Table()
    for ci, c in enumerate(lc.ema_cases()):
        off = 3 if ci % 2 == 0 else 0
        (sb, s), (fb, f) = _padded(c.slow, off), _padded(c.fast, off)
        L.call("clift_ema", L.ptr(s), L.ptr(f), c.n, c.momentum, L.stream())
        t.hold(c, "slow", s.cpu())
        if not (_sentinels_intact(sb, off, c.n) and torch.equal(f.cpu(), c.fast)):
            t.fail(c, "elements outside the range, or the fast operand, were written")
    gen = torch.Generator().manual_seed(5)
    for shape in ((5, 7), (5,)):
        s0, f0 = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        ps, pf = torch.nn.Parameter(s0.to(DEV)), torch.nn.Parameter(f0.to(DEV))
        c = lc.Case("ema", f"ema_update_{'x'.join(map(str, shape))}", n=s0.numel(), slow=s0.reshape(-1), fast=f0.reshape(-1), momentum=lc.f32r(0.9))
        closs.ema_update(torch.nn.ParameterList([ps]), torch.nn.ParameterList([pf]), 0.9)
        t.hold(c, "slow", ps.detach().cpu().reshape(-1), "wrapper")
    t.close(capsys)


# ---------------------------------------------------------------------------------------------------------------- nearest centroid
def test_nearest_centroid():
    """Labels equal the fp64 reference's wherever its top-two distance gap is at least 1e-4 relative (every row of the exact cases): lowest
    index on a tie, -1 for an invalid row and for a NaN row."""
    from contrastive_lift_amd import inference
    L = _L()
    for c in lc.centroid_cases():
        feat, cent, valid = _d(c.feat), _d(c.cent), _d(c.valid)
        lab = torch.full((c.n,), -7, dtype=torch.int32, device=DEV)
        L.call("clift_nearest_centroid", L.ptr(feat), c.ldf, c.E, L.ptr(cent), c.K, L.ptr(valid), c.n, L.ptr(lab), L.stream())
        want, sure = lc.centroid_reference(c)
        got = lab.cpu().to(torch.int64)
        assert int((~sure).sum()) <= lc.CENTROID_LEFT_OUT * c.n, c
        assert torch.equal(got[sure], want[sure]), (c, int((got[sure] != want[sure]).sum()))
        assert bool(((got >= -1) & (got < c.K)).all()), c
        if c.valid is None and c.ldf == c.E:
            w = torch.from_numpy(inference._nearest_centroid(c.feat.numpy(), c.cent.numpy(), DEV))
            assert torch.equal(w[sure], want[sure]), c
