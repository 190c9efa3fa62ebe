"""The fp64 references, cases and bounds of tests/loss_cases.py, checked without a GPU: the references reproduce the committed goldens and
the oracle in fp64, every case meets the conditions its GPU test relies on, and the bound catches a list of plausible kernel mistakes."""
import math

import numpy as np
import torch

import loss_cases as lc
from conftest import load_golden, T, rel_close
from oracle import losses as olosses, params as op

F64 = torch.float64


def _all_cases():
    return [c for make in lc.CASES.values() for c in make()]


# ---------------------------------------------------------------------------------------------------------------- goldens
def test_references_reproduce_g8_losses():
    g = load_golden("g8_losses")
    for tag in "abcd":
        c = lc.Case("contrastive", f"g8_{tag}", f=T(g[f"con_{tag}.f"]), y=T(g[f"con_{tag}.y"]).to(torch.int64), temperature=100.0)
        r = lc.reference(c)
        rel_close(r["loss"], g[f"con_{tag}.loss"], 2e-5, atol=1e-7, what=f"contrastive {tag}")
        rel_close(r["grad"], g[f"con_{tag}.grad"], 1e-4, what=f"contrastive grad {tag}")
        c = lc.Case("slow_fast", f"g8_{tag}", inst=T(g[f"sf_{tag}.feats"]), y=T(g[f"sf_{tag}.y"]).to(torch.int64), conf=T(g[f"sf_{tag}.conf"]))
        r = lc.reference(c)
        rel_close(r["loss"], g[f"sf_{tag}.loss"], 2e-5, atol=1e-7, what=f"slow_fast {tag}")
        rel_close(r["grad"], g[f"sf_{tag}.grad"], 1e-4, what=f"slow_fast grad {tag}")


def test_references_reproduce_g9_tv():
    g = load_golden("g9_tv")
    P = op.make_params(int(g["seed"]), tuple(int(x) for x in g["res"]), 2, 3)
    x = P["density_plane.1"][0].permute(1, 2, 0).contiguous()          # (1, C, H, W) -> (H, W, C)
    c = lc.Case("tv", "g9", planes=[x], weights=[1.0], grad_prefill=[torch.zeros_like(x)], loss_prefill=torch.tensor(0.0))
    r = lc.reference(c)
    rel_close(r["loss"], g["tv_plane1"], 2e-5, what="tv")
    rel_close(r["grad0"].permute(2, 0, 1)[None], g["tv_plane1_grad"], 1e-4, what="tv grad")


def test_references_reproduce_g18_sce():
    g = load_golden("g18_sce")
    for tag in "abcd":
        a, b = (float(x) for x in g[f"{tag}.ab"])
        pred, conf = T(g[f"{tag}.pred"]), T(g[f"{tag}.conf"])
        N, C = pred.shape
        c = lc.Case("rows", f"g18_{tag}", N=N, C=C, pred=pred, probs=T(g[f"{tag}.p"]), class_w=T(g[f"{tag}.w"]), sce=1, alpha=a, beta=b,
                    want_grad=True)
        r = lc.reference(c)
        rel_close(r["rows"], g[f"{tag}.rows"], 1e-5, atol=1e-6, what=f"sce rows {tag}")
        # the golden is fp32 work: where softmax(w x) is 0.998, its 1 - q has lost three digits (4.6e-7 against this reference in case d,
        # 8e-7 of the largest entry), so the absolute term is a few fp32 ulp of the gradient's scale
        rel_close(r["grad"] * (conf.to(F64) / N)[:, None], g[f"{tag}.grad"], 1e-4, atol=1e-6 * float(np.abs(g[f"{tag}.grad"]).max()),
                  what=f"sce grad {tag}")


# ---------------------------------------------------------------------------------------------------------------- the oracle in fp64
def _close64(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err, tol = lc.max_error(a, b), 1e-10 * max(lc.scale_of(b), 1e-30)
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def test_references_agree_with_the_oracle_in_fp64():
    for c in lc.contrastive_cases():
        f = c.f.to(F64).requires_grad_(True)
        L = olosses.contrastive(f, c.y, c.temperature)
        r = lc.reference(c)
        _close64(r["loss"], L.detach(), f"{c} loss")
        _close64(r["grad"], lc._grad(L, f), f"{c} grad")
    for c in lc.slow_fast_cases():
        B = c.inst.shape[0]
        if B < 2 or c.kind == "no_common":          # (B = 1: the oracle returns a constant; no common label: NaN, held by the GPU test)
            continue
        x = c.inst.to(F64).requires_grad_(True)
        L = olosses.slow_fast(x, c.y, c.conf.to(F64))
        r = lc.reference(c)
        # torch.cdist takes its matrix-multiply path above 25 rows: |a|^2 + |b|^2 - 2ab loses ~1e-16 / d absolute in a distance d
        tol = 1e-9
        assert lc.max_error(r["loss"], L.detach()) <= tol * abs(float(L.detach())), f"{c} loss"
        assert lc.max_error(r["grad"], lc._grad(L, x)) <= tol * lc.scale_of(r["grad"]) + 1e-300, f"{c} grad"
    for c in lc.rows_cases():
        cw = torch.ones(c.C, dtype=F64) if c.class_w is None else c.class_w.to(F64)
        x = c.pred.to(F64)
        want = olosses.sce_rows(x, c.probs.to(F64), cw, c.alpha, c.beta) if c.sce else \
            torch.nn.functional.cross_entropy(x, c.probs.to(F64), weight=cw, reduction="none")
        _close64(lc.reference(c)["rows"], want, f"{c} rows")
    for c in lc.pixel_cases():
        if c.sem is None or c.sce:
            continue
        mk = lc._opt(c.maskf, F64, c.N)
        cw = lc._opt(c.class_w, F64, c.C)
        want = olosses.semantic_ce(c.sem.to(F64), c.probs.to(F64), lc._opt(c.conf, F64, c.N) * mk, cw)
        _close64(lc.reference(c)["out1"], c.prefill[1].to(F64) + want, f"{c} out1")
        if c.rgb is not None:
            mse = torch.nn.functional.mse_loss(c.rgb.to(F64) * mk[:, None], c.gt.to(F64) * mk[:, None])
            _close64(lc.reference(c)["out0"], c.prefill[0].to(F64) + mse, f"{c} out0")
    for c in lc.segment_cases():
        # (the oracle's scatter buffers are fp32: it is evaluated in fp32 here, and held to 1e-5 of each quantity's scale)
        f = c.feats.clone().requires_grad_(True)
        L = olosses.segment_consistency(f, c.group, c.conf, c.class_w, c.G)
        r = lc.reference(c)
        assert lc.max_error(c.prefill + L.detach(), r["loss"]) <= 1e-5 * lc.scale_of(r["loss"]), f"{c} loss"
        if c.want_grad:
            assert lc.max_error(c.scale * lc._grad(L, f), r["grad"]) <= 1e-5 * lc.scale_of(r["grad"]), f"{c} grad"
    for c in lc.tv_cases() + lc.tv_multi_cases():
        want = c.loss_prefill.to(F64)
        for x, w in zip(c.planes, c.weights):
            want = want + w * olosses.tv_plane(x.to(F64).permute(2, 0, 1)[None])
        _close64(lc.reference(c)["loss"], want, f"{c} loss")
    for c in lc.ema_cases():
        s = [c.slow.to(F64).clone()]
        olosses.ema_(s, [c.fast.to(F64)], c.momentum)
        _close64(lc.reference(c)["slow"], s[0], f"{c}")


def test_adam_restatement_is_torch_adam_in_fp64():
    for c in lc.adam_cases():
        if c.n > 100000:
            continue
        want, got = lc.adam_torch(c), lc._eval_adam(c, F64, "natural", None)
        for q in want:
            _close64(got[q], want[q], f"{c} {q}")


# ---------------------------------------------------------------------------------------------------------------- conditions
def test_the_cases_cover_what_the_issue_lists():
    con = lc.contrastive_cases()
    assert {(c.f.shape[0], c.f.shape[1]) for c in con} >= {(B, E) for B in (1, 2, 255, 256, 257, 513) for E in (1, 3, 16, 32)}
    assert {c.temperature for c in con} == {100.0, 0.5} and {c.labels for c in con} == {"zipf", "equal", "distinct"}
    for c in con:
        cnt = torch.unique(c.y, return_counts=True)[1]
        B = c.y.numel()
        if c.labels == "zipf" and B >= 3:
            assert int(cnt.min()) == 1 and int(cnt.max()) >= 2, c              # singletons (p == 0 rows) next to real classes
        if c.labels == "distinct":
            r = lc.reference(c)
            assert float(r["loss"]) == 0.0 and float(r["grad"].abs().max()) == 0.0, c
        if "outlier" in c.name:
            d2 = ((c.f[5] - c.f[6]) ** 2).sum()
            assert float(torch.exp(-d2 / max(c.temperature, 1.0))) == 0.0, c
    sf = lc.slow_fast_cases()
    assert {(c.inst.shape[0], c.inst.shape[1] // 2) for c in sf} >= {(B, E) for B in (1, 2, 3, 256, 511, 513, 1026) for E in (1, 3, 16, 32)}
    for c in sf:
        B, E = c.inst.shape[0], c.inst.shape[1] // 2
        H = B // 2
        fast, slow = set(c.y[:H].tolist()), set(c.y[H:].tolist())
        if c.kind == "zipf" and B > 3:
            assert fast - slow and slow - fast and fast & slow, c
            assert torch.equal(c.inst[0, :E], c.inst[H, E:]) and int((c.conf == 0).sum()) > 0, c
        if c.kind == "many_labels":
            nf = torch.unique(c.y[:H], return_counts=True)[1]
            assert len(fast & slow) > 200 and set(nf.tolist()) == {1, 3, 7}, c
        if c.kind == "no_common":
            assert not fast & slow and math.isnan(float(lc.reference(c)["loss"])), c
        g = lc.reference(c)["grad"]
        assert float(g[H:].abs().max()) == 0.0 and float(g[:, E:].abs().max()) == 0.0, c
    px = lc.pixel_cases()
    assert {(c.N, c.C) for c in px} == set(lc.PIXEL_SHAPES) and {c.null for c in px} == set(lc.PIXEL_NULLS)
    assert {(c.sce, c.alpha, c.beta) for c in px} == set(lc.SEM_MODES) and {c.onehot for c in px} == {True, False}
    for c in list(px) + list(lc.rows_cases()):
        x, w = (c.sem, c.class_w) if c.kernel == "pixel" else (c.pred, c.class_w)
        if x is not None and c.C > 1 and c.N > 1:                                          # row 0: the clamp of the reverse term is active
            z = x[0].to(F64) * (1.0 if w is None else w.to(F64))
            assert float(torch.softmax(z, 0).min()) < 1e-9, c
            assert w is None or float(w[0]) == 0.0, c
        if x is not None and c.C == 22 and c.N == 1 and w is not None:                    # the lone row: nineteen classes just below the clamp
            q = torch.softmax(x[0].to(F64) * w.to(F64), 0)
            assert int(((q > 5e-9) & (q < 1e-8)).sum()) == 19 and int((c.probs[0] == 0).sum()) == 20, c
    for c in lc.segment_cases():
        assert float(lc.segment_gaps(c).min()) >= 1e-3 or c.exact, (c, float(lc.segment_gaps(c).min()))
    tie = [c for c in lc.segment_cases() if c.exact][0]
    s = lc.segment_sums(tie)[0]
    assert float(s[1]) == float(s[3]) == float(s.max()) and float(s[0]) < float(s[1])
    assert any(c.G > int(torch.unique(c.group).numel()) for c in lc.segment_cases())
    assert {tuple(c.planes[0].shape) for c in lc.tv_cases()} == set(lc.TV_SHAPES)
    assert {len(c.planes) for c in lc.tv_multi_cases()} >= {1, 6, lc.TV_MAX}
    ad = lc.adam_cases()
    assert {c.n for c in ad} == set(lc.ADAM_N)
    for n in lc.ADAM_N:
        assert {c.beta2 for c in ad if c.n == n} == {lc.f32r(0.99), lc.f32r(0.999)}
        assert {c.wd for c in ad if c.n == n} == {lc.f32r(w) for w in (lc.ADAM_WD if n < 100000 else lc.ADAM_WD[:2])}
    for c in ad:
        g = torch.cat(c.grads)
        assert int((g == 0).sum()) > 0 or c.n < 4
        assert float(c.p0.abs().max()) < 1e-3
    assert {(c.n, c.momentum) for c in lc.ema_cases()} == {(n, lc.f32r(m)) for n in lc.EMA_N for m in (0.0, 0.9, 1.0)}
    for c in lc.centroid_cases():
        lab, sure = lc.centroid_reference(c)
        assert int((~sure).sum()) <= lc.CENTROID_LEFT_OUT * c.n, (c, int((~sure).sum()))
    nan = [c for c in lc.centroid_cases() if c.name == "nan_rows"][0]
    lab, _ = lc.centroid_reference(nan)
    assert int(lab[3]) == -1 and int(lab[200]) == -1 and int((lab >= 0).sum()) == nan.n - 2
    ties = [c for c in lc.centroid_cases() if c.name == "integer_ties"][0]
    assert lc.centroid_reference(ties)[0].tolist() == [0, 0, 1, 0, 1, 2, 3]


def test_every_case_is_well_conditioned(capsys):
    """yardstick <= 1e-5 * scale for every quantity of every case; the table is printed."""
    rows, bad = [], []
    for c in _all_cases():
        ref = lc.reference(c)
        for q, y in lc.yardsticks(c).items():
            if c.kernel == "adam" and q[0] == "p":          # Adam's p is held through its step d<k> (lc.adam_step_bound), not on its own scale
                continue
            s = lc.scale_of(ref[q])
            rows.append(f"{c.kernel:12s} {c.name:34s} {q:6s} scale {s:10.3e}  yardstick {y:10.3e}  ({y / s if s else 0.0:8.1e} of scale)")
            if y > lc.ILL_CONDITIONED * s:
                bad.append(rows[-1])
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert not bad, "ill-conditioned cases (redraw them):\n" + "\n".join(bad)


def test_widened_bounds_stay_inside_the_parity_tolerance():
    """Every entry of lc.WIDENED names a case, a loss and calls of clift_tv_fwd_bwd only, and stays below 1e-4 relative; every other call of
    the case -- the one launch of clift_tv_fwd_bwd_multi above all -- keeps the plain bound."""
    by_name = {(c.kernel, c.name): c for c in _all_cases()}
    for (kernel, name, q), (measured, missed, calls) in lc.WIDENED.items():
        c = by_name[(kernel, name)]
        s = lc.scale_of(lc.reference(c)[q])
        plain = lc.bound(lc.yardstick(c, q), s)
        assert q == "loss" and measured > missed and calls and set(calls) <= {"raw", "wrapper", "single"}, (kernel, name)
        for call in calls:
            assert 2.0 * measured <= lc.bound_for(c, q, call) <= 1e-4 * s, (kernel, name, call, lc.bound_for(c, q, call), s)
        for call in {"raw", "wrapper", "single", "multi", "nograd"} - set(calls):
            assert lc.bound_for(c, q, call) == plain, (kernel, name, call)
    for c in lc.tv_multi_cases():
        for q in lc.reference(c):
            assert lc.bound_for(c, q, "multi") == lc.bound(lc.yardstick(c, q), lc.scale_of(lc.reference(c)[q])), (c, q)


# ---------------------------------------------------------------------------------------------------------------- the bounds have teeth
def test_bounds_catch_known_mistakes():
    """Each mistake of lc.MISTAKES, built into the fp32 restatement (never into the library), must break the bound of at least one quantity
    of at least one case of its kernel."""
    missed = []
    for kernel, names in lc.MISTAKES.items():
        cases = [c for c in lc.CASES[kernel]() if not (kernel == "adam" and c.n > 100000)]
        if kernel == "pixel":
            cases = cases + list(lc.rows_cases())
        if kernel == "tv":
            cases = cases + list(lc.tv_multi_cases())
        for m in names:
            caught = 0
            for c in cases:
                ref, wrong = lc.reference(c), lc.restate(c, "natural", m)
                for q in ref:
                    if kernel == "adam" and q[0] == "p":
                        continue
                    if q.startswith("d") and kernel == "adam":
                        brk = bool(((wrong[q].to(F64) - ref[q]).abs() > lc.adam_step_bound(c, int(q[1:]))).any()) or \
                            bool(torch.isnan(wrong[q]).any())
                    else:
                        brk = lc.exceeds(lc.max_error(wrong[q], ref[q]), lc.bound(lc.yardstick(c, q), lc.scale_of(ref[q])))
                    caught += brk
                if caught:
                    break
            if not caught:
                missed.append(f"{kernel}: {m}")
    assert not missed, f"mistakes the bounds would let through: {missed}"


def test_the_unmistaken_restatement_is_inside_its_bound():
    """The other half of the test above: without a mistake, the fp32 restatement in any order is inside every bound (by construction of the
    yardstick), so a break there is caused by the mistake alone."""
    for c in _all_cases():
        if c.kernel in ("adam", "ema") and c.n > 100000:
            continue
        ref, got = lc.reference(c), lc.restate(c, "permuted")
        for q in ref:
            if c.kernel == "adam" and q[0] == "p":
                continue
            assert not lc.exceeds(lc.max_error(got[q], ref[q]), lc.bound(lc.yardstick(c, q), lc.scale_of(ref[q]))), (c, q)
