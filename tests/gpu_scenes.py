"""Shared set-up of the GPU parity suites (not collected by pytest): the oracle import, a product model built from oracle parameters, the seeded
scene and its rays, one forward + backward through the product path, the first-two-layers case and the synthetic scene that two suites
each use, and ``replay_g12``, the replay of the reference trainer's recorded steps (golden G12) that three suites run.
tools/ab_persistent.py imports from here too.  A helper that only one suite uses lives in that suite, next to its tests."""
import numpy as np
import torch

from conftest import load_golden, rel_close, T

DEV = "cuda"


def _import():
    import contrastive_lift_amd as cl
    from oracle import params as op, render as orender, field as ofld, losses as olosses, rays as orays
    return cl, op, orender, ofld, olosses, orays


def build_model(cl, P, res, C_, E, shift, mode="softmax", slow_fast=True):
    m = cl.TensorVMSplit(list(res), num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=C_,
                         dim_feature_instance=(2 * E if slow_fast else E), splus_density_shift=shift,
                         output_mlp_semantics=(torch.nn.Softmax(dim=-1) if mode == "softmax" else torch.nn.Identity()),
                         use_semantic_mlp=True, use_instance_mlp=True, slow_fast_mode=slow_fast, device=DEV)
    missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
    assert not missing and not unexpected
    return m


def scene(op, orays, seed, res, C_, E, n_rays, img=48, amp=2.5, sg=0.45):
    P = op.add_blob(op.make_params(seed, res, C_, E), res, amplitude=amp, sigma_g=sg)
    rng = np.random.default_rng(seed + 1)
    K = torch.tensor([[img * 1.25, 0, img / 2], [0, img * 1.25, img / 2], [0, 0, 1]])

    def look_at(eye):
        eye = np.asarray(eye, np.float64)
        f = -eye / np.linalg.norm(eye)
        r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
        d = np.cross(f, r)
        M = np.eye(4); M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = r, d, f, eye
        return torch.tensor(M, dtype=torch.float32)
    tabs = [orays.ray_table(img, img, K, look_at(e)) for e in ((0.0, 0.1, -0.9), (0.7, -0.4, 0.3), (-0.5, 0.6, 0.4))]
    allr = torch.cat(tabs, 0)
    pick = torch.from_numpy(rng.choice(allr.shape[0], size=n_rays, replace=False))
    return P, allr[pick].contiguous(), rng


def _run_forward_backward(cl, m, r, rays, jitter, white, cots):
    for p in m.parameters():
        p.requires_grad_(True)
    rgb, sem, inst, depth, feats, dreg = r.forward(m, rays.to(DEV), 1.0, white, True, jitter=jitter.to(DEV), white_bg_resolved=white)
    L = (rgb * cots[0].to(DEV)).sum() + (sem * cots[1].to(DEV)).sum() + (inst * cots[2].to(DEV)).sum()
    if len(cots) > 3:
        L = L + cots[3] * dreg
    grads = torch.autograd.grad(L, list(m.parameters()), allow_unused=True)
    return (rgb, sem, inst, depth, feats, dreg), {n: g for (n, _), g in zip(m.named_parameters(), grads)}


def _first2_case(M, seed, cap=None):
    from contrastive_lift_amd._lib import call, ptr, stream
    R = cap or M
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(R, 256, generator=g) * (torch.rand(R, 256, generator=g) > 0.4)
    W1 = torch.randn(256, 256, generator=g) / 16
    W0, b0 = torch.randn(256, 3, generator=g), 0.5 * torch.randn(256, generator=g)
    x4 = torch.cat([torch.rand(R, 3, generator=g) * 2 - 1, torch.zeros(R, 1)], 1).contiguous()
    dev = {k: v.to(DEV) for k, v in dict(d=d, W1=W1, W0=W0, b0=b0, x4=x4).items()}
    h1 = torch.empty(R, 256, device=DEV)          # the forward's first-layer activation (its sign is what the fused kernel has to reproduce)
    call("clift_linear_k3_fwd", ptr(dev["x4"]), ptr(dev["W0"]), 3, ptr(dev["b0"]), R, 256, 1, ptr(h1), 256, 0, stream())
    dH1 = (d[:M].double() @ W1.double()) * (h1[:M].cpu() > 0)
    return dev, h1, dH1.t() @ x4[:M, :3].double(), dH1.sum(0)


def _scene(C_=22, res=64):
    from contrastive_lift_amd import synthetic
    model, renderer, pool = synthetic.make_scene(grid=res, num_classes=C_, max_instances=3, seed=0, device=DEV, image=128)
    return model, renderer, pool


def replay_g12(fixture):
    """The product trainer (HIP kernels, arena Adam) replays the three training_step()s recorded from the REFERENCE trainer
    class (golden G12: chunked forwards with chunk = 40, masked pixels, recorded jitter / white-background draws, slow-fast
    instance pass with the EMA between forward and loss): losses to 1e-3, every parameter after every step to 10 % of a
    learning-rate step (Adam moves a weight by ~lr whatever the gradient size, so gradient round-off on |g| ~ eps elements
    is amplified to that scale) and norms to 1e-3."""
    cl, op, orender, ofld, olosses, orays = _import()
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    g = load_golden(fixture)          # second fixture: instance_loss_mode "contrastive" + use_delta on a single instance MLP
    res = tuple(int(x) for x in g["res"])
    C_, E = int(g["C"]), int(g["E"])
    mode = str(g["mode"]) if "mode" in g else "slow_fast"
    sf = mode == "slow_fast"
    grids = "grid_heads" in fixture                # sixth fixture: both heads on their own VM grids (the allgrid overlay), plain contrastive loss
    wmode = str(g["weight_mode"]) if "weight_mode" in g else "softmax"      # seventh fixture: semantic_weight_mode "argmax" (R:142-143)
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E, slow_fast=sf, sem_grid=grids, inst_grid=grids), res, 2.5, 0.45)
    if grids:
        m = cl.TensorVMSplit(list(res), num_semantics_comps=(32, 32, 32), num_instance_comps=(32, 32, 32), num_semantic_classes=C_,
                             dim_feature_instance=(2 * E if sf else E),
                             splus_density_shift=float(g["shift"]), use_semantic_mlp=False, use_instance_mlp=False, slow_fast_mode=sf, device=DEV)
        missing, unexpected = m.load_state_dict({k: v.to(DEV) for k, v in P.items()}, strict=True)
        assert not missing and not unexpected
    else:
        m = build_model(cl, P, res, C_, E, float(g["shift"]), mode=wmode, slow_fast=sf)
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode=wmode).to(DEV)
    cfg = default_config(chunk=int(g["chunk"]), semantic_weight_mode=wmode, probabilistic_ce_mode=str(g["ce_mode"]) if "ce_mode" in g else "TTAConf", late_semantic_optimization=1, instance_optimization_epoch=3, instance_loss_mode=mode,
                         use_delta=bool(int(g["use_delta"])) if "use_delta" in g else False, max_instances=E)
    if "sce" in g and float(g["sce"][1]) != 0.0:          # fourth fixture: config.use_symmetric_ce (SCELoss, T:74-77)
        cfg.use_symmetric_ce, cfg.ce_alpha, cfg.ce_beta = True, float(g["sce"][0]), float(g["sce"][1])
    tr = HotPathTrainer(m, r, cfg, class_weights=T(g["class_weights"]), current_epoch=int(g["epoch"]))
    rel_close(tr.current_lambda_dist_reg, g["lambda_dist"], 1e-6, what="dist-reg ramp")
    d = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(DEV)
    for st in range(int(g["steps"])):
        white = [bool(x) for x in g[f"s{st}.white"]]
        assert len(set(white)) == 1          # the recorded coin flips of one step happen to agree: one flag per main pass
        batch0 = dict(rays=d(g[f"s{st}.rays"]), rgbs=d(g[f"s{st}.rgbs"]), probabilities=d(g[f"s{st}.probs"]),
                      confidences=d(g[f"s{st}.confs"]), mask=d(g[f"s{st}.mask"]), semantics=d(g[f"s{st}.probs"]).argmax(-1))
        seg, sjit = None, None
        if f"s{st}.srays" in g:          # third fixture: the segment-consistency term (batch[2], T:185-197)
            seg = dict(rays=d(g[f"s{st}.srays"]), group=d(g[f"s{st}.sgroup"]), confidences=d(g[f"s{st}.sconf"]), n_groups=6)
            sjit = d(g[f"s{st}.sjitter"])
        tr.main_pass(batch0, jitter=d(g[f"s{st}.jitter"]), white_bg=white[0], segments=seg, segment_jitter=sjit)
        if seg is not None:
            rel_close(tr.loss_segment[0], g[f"s{st}.loss_segment"], 1e-3, what=f"step {st} loss_segment")
        rel_close(tr.losses[0], g[f"s{st}.loss_rgb"], 1e-3, what=f"step {st} loss_rgb")
        rel_close(tr.losses[1], g[f"s{st}.loss_sem"], 1e-3, what=f"step {st} loss_sem")
        tr.instance_pass([dict(rays=d(g[f"s{st}.irays"]), instances=d(g[f"s{st}.labels"]), confidences=d(g[f"s{st}.iconf"]))],
                         jitter=d(g[f"s{st}.ijitter"]))
        rel_close(tr.losses[3], g[f"s{st}.loss_clustering"], 1e-3, what=f"step {st} loss_clustering")
        sd = m.state_dict()
        for k in P:
            flat = sd[k].detach().cpu().reshape(-1)
            sub = flat if flat.numel() <= 4096 else flat[::17]
            lr = 1e-2 if k.split(".")[0].endswith(("_plane", "_line")) else 5e-4
            rel_close(flat.norm(), g[f"s{st}.pnorm.{k}"], 1e-3, atol=1e-6, what=f"step {st} |{k}|")
            diff = float((sub - T(g[f"s{st}.psub.{k}"]).reshape(-1)).abs().max())
            assert diff <= 0.1 * lr * (st + 1) + 1e-7, f"step {st} param {k}: max |diff| {diff:.3e} vs lr {lr}"
