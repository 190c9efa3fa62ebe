"""GPU tests of the device backend of the linear-assignment instance loss (ABI 27, csrc/assign.hip): the solver alone against scipy, the
fused per-image pass against the CPU oracle (matching, virtual labels, active flag, loss, gradient), its determinism, and the trainer with
``assignment_backend="device"`` against the reference's recorded steps and the CPU oracle.  Inputs: tests/lsap_cases.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_close
import lsap_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ============================================================================ 1. the solver alone
def _solve(cost):
    from contrastive_lift_amd.loss import linear_sum_assignment_device
    col, total = linear_sum_assignment_device(torch.from_numpy(cost).to(DEV))
    return col.cpu().numpy(), float(total.cpu())


def test_solver_against_scipy():
    for name, kind, cost in lsap_cases.solver_cases():
        L, E = cost.shape
        col, total = _solve(cost)
        want_col, want_total = lsap_cases.optimum(cost)
        assert col.shape == (L,) and len(set(col.tolist())) == L and col.min() >= 0 and col.max() < E, name
        clean = np.nan_to_num(cost.astype(np.float64))
        assert total == float(sum(clean[r, col[r]] for r in range(L))), name          # the value of the assignment returned, in row order
        if kind in ("integer", "product"):
            assert total == want_total, (name, total, want_total)
        else:
            assert abs(total - want_total) <= 1e-12 * L, (name, total, want_total)
        if kind in ("random", "nan"):
            assert np.array_equal(col, want_col), name


def test_solver_batched_with_a_padded_stride():
    """One call on three problems that sit in a larger buffer (row stride 70 > E, batch stride > L * ld) equals the three single calls."""
    from contrastive_lift_amd.loss import linear_sum_assignment_device
    rng = np.random.default_rng(5)
    L, E = 30, 65
    buf = torch.full((3, L + 3, 70), float("nan"))
    mats = [rng.uniform(-1, 0, (L, E)).astype(np.float32) for _ in range(3)]
    for b in range(3):
        buf[b, :L, :E] = torch.from_numpy(mats[b])
    view = buf.to(DEV)[:, :L, :E]
    assert view.stride(0) > L * view.stride(1) and view.stride(1) == 70
    col, total = linear_sum_assignment_device(view)
    assert col.shape == (3, L) and total.shape == (3,)
    for b in range(3):
        c1, t1 = _solve(mats[b])
        assert np.array_equal(col[b].cpu().numpy(), c1) and float(total[b].cpu()) == t1
        assert np.array_equal(c1, lsap_cases.optimum(mats[b])[0])


def test_solver_error_returns():
    from contrastive_lift_amd import CliftError, _lib
    from contrastive_lift_amd.loss import linear_sum_assignment_device
    with pytest.raises(CliftError, match="L = 5"):
        linear_sum_assignment_device(torch.zeros(5, 4, device=DEV))
    with pytest.raises(CliftError, match="512"):
        linear_sum_assignment_device(torch.zeros(2, 513, device=DEV))
    c = torch.zeros(2, 8, device=DEV)
    col = torch.zeros(2, dtype=torch.int32, device=DEV)
    for args, word in (((_lib.ptr(c), 8, 0, 1, 9, 8, _lib.ptr(col), None), "L = 9"), ((_lib.ptr(c), 513, 0, 1, 2, 513, _lib.ptr(col), None), "512"),
                       ((_lib.ptr(c), 7, 0, 1, 2, 8, _lib.ptr(col), None), "ld = 7")):
        with pytest.raises(CliftError, match=word):
            _lib.call("clift_lsap", *args, _lib.stream())
    col0, total0 = linear_sum_assignment_device(torch.zeros(0, 4, device=DEV))          # L == 0: nothing to match, value 0
    assert col0.shape == (0,) and float(total0.cpu()) == 0.0


# ============================================================================ 2.-4. the fused pass
def _conf(n, k):
    return torch.rand(n, generator=torch.Generator().manual_seed(100 + k)) * 0.8 + 0.2          # uniform in (0.2, 1)


def _fused(y, f, conf):
    """One clift_assign_loss call; every output on the host."""
    from contrastive_lift_amd.loss import _assign_loss_device
    out = _assign_loss_device(f.to(DEV), y.to(DEV), conf.to(DEV), want_grad=True, want_cost=True)
    return {k: v.cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _results():
    """Device outputs and oracle quantities of every matching case, computed once for the tests below and not changed by them."""
    from oracle import losses as olosses
    res = []
    for k, (name, y, f) in enumerate(lsap_cases.matching_cases()):
        conf = _conf(y.shape[0], k)
        ids, cost = lsap_cases.oracle_cost(y, f)
        res.append(dict(name=name, y=y, f=f, conf=conf, dev=_fused(y, f, conf), ids=ids, cost=cost, margin=lsap_cases.margin(cost),
                        target=olosses.virtual_labels_linear_assignment(y, f)))
    return tuple(res)


def test_fused_matching_against_the_oracle():
    fallouts = 0
    for r in _results():
        d, L, E = r["dev"], len(r["ids"]), r["f"].shape[1]
        assert int(d["n_ids"]) == L and d["ids"][:L].tolist() == r["ids"], r["name"]
        delta = float(np.abs(d["cost"][:L].double().numpy() - r["cost"]).max())
        print(f"{r['name']}: L {L}, delta {delta:.3e} ({delta * 2 ** 24:.2f} x 2^-24), margin {r['margin']:.3e}")
        # the oracle adds fp32 probabilities in fp32 over at most 1024 rays: (log2 n + 3) 2^-24 < 2^-20; the device adds one rounding and one division
        assert delta <= 2.0 ** -20, (r["name"], delta)
        slot = d["slot_of_id"][:L].numpy()
        assert len(set(slot.tolist())) == L and slot.min() >= 0 and slot.max() < E, r["name"]
        value = float(sum(r["cost"][l, slot[l]] for l in range(L)))
        assert value <= lsap_cases.optimum(r["cost"])[1] + 2 * L * delta, (r["name"], value)          # rigorous whatever the margin
        if r["margin"] > 2 * L * delta:
            assert torch.equal(d["target"].to(torch.int64), r["target"]), r["name"]
        else:
            fallouts += 1
    print(f"cases outside the equality check (margin <= 2 L delta): {fallouts} of {len(_results())}")
    assert fallouts <= 2


def test_fused_loss_and_gradient_against_the_oracle(monkeypatch):
    """Tolerances: the loss as tests/test_gpu_parity.py::test_pixel_losses_adam_ema_vs_torch holds clift_pixel_losses' cross entropy (rtol
    1e-4), the gradient as tests/test_gpu_round2.py::test_sce_loss_callable_golden_g18 holds clift_semantic_loss_rows' per-row gradient (rtol
    1e-3, atol 1e-6 on d CE_i / d scores_i) -- so the device gradient is divided by its conf_i / n first, in fp64."""
    from oracle import losses as olosses
    for r in _results():
        d, n = r["dev"], r["y"].shape[0]
        target = d["target"].to(torch.int64)
        L, delta = len(r["ids"]), float(np.abs(d["cost"][:len(r["ids"])].double().numpy() - r["cost"]).max())
        if r["margin"] > 2 * L * delta:
            target = r["target"]          # (asserted equal above; the oracle's own matching, evaluated in fp32 like everywhere else)
        assert int(d["active"]) == int(bool(torch.any(d["target"].to(torch.int64) != r["f"].argmax(-1)))), r["name"]
        f64 = r["f"].double().requires_grad_(True)
        monkeypatch.setattr(olosses, "virtual_labels_linear_assignment", lambda y, s, t=target: t)
        want, active = olosses.linear_assignment(f64, r["y"], r["conf"].double())
        assert int(d["active"]) == int(active), r["name"]
        if not active:
            assert float(d["loss"][0]) == 0.0 and float(d["grad"].abs().max()) == 0.0, r["name"]
            continue
        rel_close(d["loss"][0], want.detach(), 1e-4, what=f"{r['name']} loss")
        g_rows = torch.autograd.grad(F.cross_entropy(f64, target, reduction="none").sum(), f64)[0]
        unscaled = d["grad"].double() * (n / r["conf"].double())[:, None]
        rel_close(unscaled, g_rows, 1e-3, atol=1e-6, what=f"{r['name']} per-row gradient")
        g_full = torch.autograd.grad(want, f64)[0]          # torch autograd of the oracle's loss: the per-row gradient times conf_i / n
        assert torch.allclose(g_full, g_rows * (r["conf"].double() / n)[:, None], rtol=1e-12, atol=0.0), r["name"]


def _inactive_image(E=6, n=64, seed=21):
    """Peaked scores whose argmax already is the matched slot: id k sits on slot k (non-zero), every ray's score has +8 there."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, 5, (n,), generator=g)
    f = torch.randn(n, E, generator=g)
    f[torch.arange(n), y] += 8
    return y, f


def test_fused_inactive_image_writes_zeros():
    from contrastive_lift_amd import _lib
    from contrastive_lift_amd.loss import linear_assignment_loss
    from oracle import losses as olosses
    y, f = _inactive_image()
    conf = _conf(y.shape[0], 50)
    want, active = olosses.linear_assignment(f, y, conf)
    assert not active and float(want) == 0.0
    assert torch.equal(olosses.virtual_labels_linear_assignment(y, f), f.argmax(-1))
    n, E = f.shape
    fd, yd, cd = f.to(DEV), y.to(torch.int32).to(DEV), conf.to(DEV)
    ints = torch.full((2 * E + 2 + n,), 77, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), 5.0, device=DEV)
    grad = torch.ones((n, E), device=DEV)          # must be overwritten, not left as it was
    nbytes = int(_lib.load().clift_assign_work_bytes(n, E))
    work = torch.empty((nbytes // 8 + 2,), dtype=torch.int64, device=DEV)
    _lib.call("clift_assign_loss", _lib.ptr(fd), E, _lib.ptr(yd), _lib.ptr(cd), n, E, _lib.ptr(ints[:E]), _lib.ptr(ints[2 * E:]), None,
              _lib.ptr(ints[E:2 * E]), _lib.ptr(ints[2 * E + 2:]), _lib.ptr(loss), _lib.ptr(grad), E, _lib.ptr(ints[2 * E + 1:]), _lib.ptr(work),
              nbytes, _lib.stream())
    assert int(ints[2 * E + 1]) == 0 and int(ints[2 * E]) == 4
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    assert torch.equal(ints[2 * E + 2:].cpu().to(torch.int64), f.argmax(-1))
    l2, g2, a2 = linear_assignment_loss(fd, y.to(DEV), cd, return_grad=True, backend="device")
    assert l2.is_cuda and a2.is_cuda and a2.dtype == torch.int32 and g2 is not None
    assert int(a2) == 0 and float(l2) == 0.0 and float(g2.abs().max()) == 0.0


def test_python_entry_points():
    """create_virtual_gt_with_linear_assignment(backend="device") returns the oracle's labels in the labels' dtype; the autograd form of the
    loss hands the kernel's gradient back; strided scores (a column slice) are accepted."""
    from contrastive_lift_amd.loss import create_virtual_gt_with_linear_assignment, linear_assignment_loss
    r = _results()[0]
    got = create_virtual_gt_with_linear_assignment(r["y"].to(DEV), r["f"].to(DEV), backend="device")
    assert got.dtype == r["y"].dtype and torch.equal(got.cpu(), r["target"])
    wide = torch.zeros((r["f"].shape[0], r["f"].shape[1] + 3), device=DEV)
    wide[:, :r["f"].shape[1]] = r["f"].to(DEV)
    x = wide[:, :r["f"].shape[1]].requires_grad_(True)
    loss = linear_assignment_loss(x, r["y"].to(DEV), r["conf"].to(DEV), backend="device")
    (g,) = torch.autograd.grad(2.0 * loss, x)
    assert torch.equal(loss.detach().cpu(), r["dev"]["loss"][0]) and torch.equal(g.cpu(), 2.0 * r["dev"]["grad"])


def test_fused_pass_is_deterministic():
    for r in _results():
        if r["name"] in ("E64_ids64_n1024_0", "E500_ids30_n256_0"):
            again = _fused(r["y"], r["f"], r["conf"])
            for k in ("cost", "target", "loss", "grad", "ids", "slot_of_id", "active"):
                assert torch.equal(again[k], r["dev"][k]), (r["name"], k)


def test_large_n_takes_the_selection_path():
    """n > 8192 extracts the ids one reduction at a time instead of sorting them: same ids, same matching as the oracle."""
    from oracle import losses as olosses
    g = torch.Generator().manual_seed(8)
    n, E = 8200, 5
    y = torch.randint(-3, 4, (n,), generator=g) * 1000          # seven ids, five slots
    f = 3 * torch.randn(n, E, generator=g)
    d = _fused(y, f, torch.ones(n))
    ids, cost = lsap_cases.oracle_cost(y, f)
    assert int(d["n_ids"]) == 5 and d["ids"].tolist() == ids
    delta = float(np.abs(d["cost"].double().numpy() - cost).max())
    assert delta <= 2.0 ** -20 and lsap_cases.margin(cost) > 2 * 5 * delta          # ((log2 1200 + 3) 2^-24 per id's sum)
    assert torch.equal(d["target"].to(torch.int64), olosses.virtual_labels_linear_assignment(y, f))


def test_limits():
    from contrastive_lift_amd import CliftError
    from contrastive_lift_amd.loss import create_virtual_gt_with_linear_assignment, linear_assignment_loss
    y, conf = torch.ones(8, dtype=torch.int64, device=DEV), torch.ones(8, device=DEV)
    for E in (513, 1):
        with pytest.raises(CliftError, match="512"):
            linear_assignment_loss(torch.zeros(8, E, device=DEV), y, conf, return_grad=True, backend="device")
        with pytest.raises(CliftError, match="512"):
            create_virtual_gt_with_linear_assignment(y, torch.zeros(8, E, device=DEV), backend="device")


# ============================================================================ 5. the trainer on the reference's recorded steps
def test_trainer_replays_the_reference_fixture_on_the_device_backend(monkeypatch):
    """golden G12l (two training_step()s recorded from the REFERENCE trainer, instance_loss_mode "linear_assignment") through the replay of
    tests/gpu_scenes.py (replay_g12) with assignment_backend="device": the same tolerances as the host replay; clift_assign_loss ran, scipy did not."""
    import scipy.optimize
    import contrastive_lift_amd.trainer as trainer_mod
    from contrastive_lift_amd import _lib
    from gpu_scenes import replay_g12
    base = trainer_mod.default_config
    monkeypatch.setattr(trainer_mod, "default_config", lambda **over: base(**dict(over, assignment_backend="device")))

    def no_scipy(*a, **k):
        raise AssertionError("scipy.optimize.linear_sum_assignment was called with assignment_backend='device'")

    monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", no_scipy)
    names, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    replay_g12("g12l_training_steps_linear_assignment")
    assert names.count("clift_assign_loss") == 2, names.count("clift_assign_loss")          # one image per step, two steps


# ============================================================================ 6. the trainer with a wide instance layer
def _wide_setup(backend="device"):
    """The set-up of tests/test_gpu_round5.py::test_linear_assignment_mode_with_a_wide_instance_layer_against_the_oracle."""
    from gpu_scenes import _import, build_model, scene
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    cl, op, orender, ofld, olosses, orays = _import()
    res, C_, E, Bi = (20, 24, 28), 3, 40, 512
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    _, rays, rng = scene(op, orays, 91, res, C_, 3, Bi)
    P = op.add_blob(op.make_params(91, res, C_, E, slow_fast=False), res, 2.5, 0.45)
    m = build_model(cl, P, res, C_, E, -3.0, slow_fast=False)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    cfg = default_config(chunk=0, instance_optimization_epoch=0, late_semantic_optimization=0, instance_loss_mode="linear_assignment", max_instances=E,
                         assignment_backend=backend)
    tr = HotPathTrainer(m, r, cfg, current_epoch=4)
    return dict(P=P, m=m, r=r, tr=tr, rays=rays, rng=rng, res=res, aabb=aabb, E=E, Bi=Bi, orender=orender)


def test_trainer_wide_instance_layer_against_the_oracle_on_the_device_backend():
    """E = 40, 60 ids, three steps of the HIP trainer with assignment_backend="device" against the CPU oracle's: loss to 1e-3, every
    instance-head parameter within 10 % of a learning-rate step (the tolerances of the host-backend test)."""
    from oracle.train_step import CpuTrainer
    s = _wide_setup()
    tr, m, rays, rng, Bi = s["tr"], s["m"], s["rays"], s["rng"], s["Bi"]
    assert tr.assignment_backend == "device"
    ct = CpuTrainer(s["P"], s["orender"].RenderCfg(s["aabb"], s["res"], density_shift=-3.0), chunk=4096, epoch=4, instance_loss_mode="linear_assignment")
    labels = torch.from_numpy(rng.integers(1, 61, size=(Bi,)))               # more ids than slots: the ids past the 40th stay unmatched (class 0)
    conf = torch.from_numpy(rng.uniform(0.2, 1, Bi).astype(np.float32))
    for step in range(3):
        jit = torch.from_numpy(rng.uniform(0, 1, Bi).astype(np.float32))
        oi = ct.instance_pass(rays, labels, conf, jit)
        tr.losses.zero_()
        tr.instance_pass([dict(rays=rays.to(DEV), instances=labels.to(DEV), confidences=conf.to(DEV))], jitter=jit.to(DEV))
        rel_close(tr.losses[3], oi["loss"], 1e-3, what=f"step {step} linear-assignment loss")
        sd = m.state_dict()
        for k, v in ct.P.items():
            if k.startswith("render_instance_mlp."):
                diff = float((sd[k].cpu() - v.detach()).abs().max())
                assert diff <= 0.1 * 5e-4 * (step + 1) + 1e-7, (step, k, diff)


def test_trainer_inactive_image_beside_an_active_one():
    """Two images in one pass, one of them already on its slots: its zero gradient adds exact zeros, so the parameters after the step equal
    (1e-7: what remains is the order of the two additions into the loss) those of a pass fed the active image alone.  A pass fed only the
    inactive image changes nothing: no optimiser step, no step count."""
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.loss import linear_assignment_loss
    a, b, c = _wide_setup(), _wide_setup(), _wide_setup()
    rays, rng, Bi = a["rays"].to(DEV), a["rng"], a["Bi"]
    labels = torch.from_numpy(rng.integers(1, 61, size=(Bi,))).to(DEV)
    conf = torch.from_numpy(rng.uniform(0.2, 1, Bi).astype(np.float32)).to(DEV)
    jit = torch.from_numpy(rng.uniform(0, 1, Bi).astype(np.float32)).to(DEV)
    # the inactive image: the same rays, every ray labelled by its own argmax slot (+ 1000): id 1000 + s is matched to slot s
    (inst, _), _ = engine.feature_forward(c["m"], c["r"], rays, jit, "instance", grad_heads=("fast",), cap=c["tr"]._capacity("inst", Bi), want_xyz=False)
    inst = inst.clone()
    quiet = inst.argmax(-1) + 1000
    _, g, act = linear_assignment_loss(inst, quiet, conf, return_grad=True, backend="device")
    assert int(act) == 0 and float(g.abs().max()) == 0.0
    _, _, act = linear_assignment_loss(inst, labels, conf, return_grad=True, backend="device")
    assert int(act) == 1
    img_active = dict(rays=rays, instances=labels, confidences=conf)
    img_quiet = dict(rays=rays, instances=quiet, confidences=conf)
    before = {k: v.detach().clone() for k, v in c["m"].state_dict().items()}
    steps_before = dict(c["tr"].opt_inst.t)
    c["tr"].instance_pass([img_quiet], jitter=jit)
    assert c["tr"].opt_inst.t == steps_before
    for k, v in c["m"].state_dict().items():
        assert torch.equal(v, before[k]), k
    a["tr"].instance_pass([img_quiet, img_active], jitter=jit)
    b["tr"].instance_pass([img_active], jitter=jit)
    assert a["tr"].opt_inst.t == b["tr"].opt_inst.t and any(t == 1 for t in a["tr"].opt_inst.t.values())
    moved = 0.0
    sa, sb = a["m"].state_dict(), b["m"].state_dict()
    for k in sa:
        assert float((sa[k] - sb[k]).abs().max()) <= 1e-7, k
        moved = max(moved, float((sa[k] - before[k]).abs().max()))
    assert moved > 1e-5          # the active image did train
    rel_close(a["tr"].losses[3], b["tr"].losses[3], 1e-6, what="loss of the pass")
