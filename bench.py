#!/usr/bin/env python3
"""bench.py -- ray-samples/sec of a train step of the Contrastive-Lift render hot path on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times the K steps, writes outputs with --dump-outputs DIR and prints the line.  The dump is the timed step
run once more, untimed, from the set-up state with the last timed step's batch (rendered rgb / semantics of the main pass, the four losses,
the gradient arena, the parameter arena after Adam): its inputs are the same in every run, whereas the state the timed steps reach is
not -- their gradients are sums through floating-point atomics, and Adam carries the last-bit differences into the parameters.  --full
adds, after the timed region, what the headline does not need: the roofline replays, the per-pass split, the other arithmetics and shapes, the frame
render, the CPU baseline, and with N > 1 the exchange timed alone and the data-parallel self-check.

Step = one full ``training_step`` of the reference (trainer/train_panopli_tensorf.py:148-228) at steady state:
main pass over 4096 rays (forward of all heads, MSE + TV + confidence-weighted CE + dist-reg, backward, Adam)
followed by the instance pass over 1024 rays (EMA, forward_instance_feature, slow-fast loss, backward, Adam).
Workload = BASELINE.json configs[1] ("ScanNet scene0423_02, 4096 rays/batch, fp32") as a synthetic stand-in of
the same shapes (no dataset offline): C = 22 classes, E = 3 (D = 6), grid 128^3 => S = 440 samples/ray.
Unit = nominal ray-sample (rays x S); value = world * (4096 + 1024) * S / step time, weak scaling
(every rank renders its own rays; one RCCL all-reduce of the gradient arena range per backward).
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PMC_RECORD = "profiles/r03_pmc_k_layer_f32.json"        # exact-fp32 dominant kernel
PMC_RECORD_X6 = "profiles/r05_pmc_k_layer_x6.json"      # fp32x6 dominant kernel (the default arithmetic)
PEAK_BF16_MFMA_TFLOPS = 2500.0       # /opt/skills/guides/MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)
PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~8 TB/s
PEAK_FP32_MFMA_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense fp32


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--inst-rays", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--chunk", type=int, default=0, help="rays per renderer call; 0 = whole batch (reference: 2048)")
    ap.add_argument("--lean", action="store_true", help="skip the instance heads in the main pass (their output is discarded)")
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp32x6"], default="fp32x6",
                    help="arithmetic of the 256-wide MLP layers: fp32x6 (default = the library's default: fp32-faithful three-way bf16 split, six "
                         "products, fp32 accumulate; BASELINE configs[1]), fp32 (exact fp32 MFMA; also measured as an extra of the default run) "
                         "or bf16 operands / fp32 accumulate (configs[2])")
    ap.add_argument("--inference-probe", action="store_true",
                    help="also report frame-render throughput and the lean main-pass time (both change the launch mix of the dominant "
                         "kernel: keep them out of profiled runs)")
    ap.add_argument("--global-rays", type=int, default=0,
                    help="strong scaling (BASELINE configs[3]: 8192 rays per step over the job): rays per GPU = global / world, "
                         "instance rays stay per-GPU (one instance image per rank, as the reference's DDP)")
    ap.add_argument("--nosync", action="store_true",
                    help="sync-free steps: the active-sample count is never read back; buffers sized by a learnt capacity, kernels clamp to the "
                         "device-side count (exact fp32 only)")
    ap.add_argument("--inference-sharded", action="store_true",
                    help="BASELINE configs[4]: time full 1296x968 frames through inference.render_rays_sharded (row tiles over the ranks, one "
                         "all-gather per frame) instead of training steps; a 'step' is one frame, value = rays/s over the job")
    ap.add_argument("--launch-check", action="store_true",
                    help="only launch the ranks, form the process group, all-reduce one number and print the line's n_gpus / rccl_ranks "
                         "fields (no render work; runs without a GPU over gloo)")
    ap.add_argument("--soak", type=int, default=0,
                    help="after the timed region: K replays of one full training step from the timed region's snapshot with the asynchronous "
                         "gradient exchange ON (RCCL kernels beside the persistent MFMA kernels), every replay's rendered outputs bit-compared "
                         "with the first one's and its gradients compared within the noise of the floating-point atomics; counts in `soak`")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline, after the timed region: the roofline replays of the timed steps, "
                         "the per-pass split, the extras (unless --no-extras), the CPU baseline (unless --no-cpu-baseline), with N > 1 the exchange "
                         "timed alone and the data-parallel self-check, with --inference-sharded the frame's roofline.  Without it a run sets up, "
                         "warms up, times the steps, writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, run the timed step once more from the set-up state with the last timed step's batch (the same "
                         "inputs in every run) and write what it computed as float32 DIR/<name>.npy (at most 64 MB in all: a larger array is cut "
                         "to a fixed, seeded sample of its rows); with --inference-sharded, the last timed frame")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the bf16-mode and frame-render extras measured after the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-budget-s", type=float, default=30.0)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def self_launch(a):
    """``python bench.py --gpus N`` without a launcher: re-exec this command under torch.distributed.run with N ranks on this node
    (one per GPU, RCCL).  On a box with fewer devices than ranks (the 1-GPU test box) the ranks share devices and the process group
    falls back to gloo -- the line then says so (`dist_backend`, `rccl_ranks: 0`)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if ndev < a.gpus:
        env.setdefault("CLIFT_DIST_BACKEND", "gloo")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def launch_check(a, world, rank):
    """The launcher path alone: process group + one collective, no render work (CPU-runnable)."""
    backend = os.environ.get("CLIFT_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
    total, check = 1.0, None
    if world > 1:
        if backend == "nccl":
            local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            t = torch.ones(1, device="cuda")
        else:
            dist.init_process_group(backend)
            t = torch.ones(1)
        dist.all_reduce(t)
        total = float(t.item())
        # the self-check's comparison across ranks (data_parallel_self_check), on tensors whose answer is known: equal on every rank / not
        cdev = "cuda" if backend == "nccl" else "cpu"
        same = torch.arange(1000, dtype=torch.float32)
        check = {"identical_tensor_delta": max_delta_across_ranks(same, cdev),
                 "rank_dependent_tensor_delta": max_delta_across_ranks(same + (rank == world - 1) * (same == 7.0), cdev)}
        # the reduction `--soak` reports through (soak_replays): counts and the worst delta MAX-reduced over the ranks
        sk = torch.tensor([float(rank == world - 1), 0.0, 0.5 * rank], dtype=torch.float64, device=cdev)
        dist.all_reduce(sk, op=dist.ReduceOp.MAX)
        check["soak_reduction"] = [float(x) for x in sk.tolist()]
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "requested_gpus": a.gpus, "dist_backend": backend if world > 1 else None,
                          "rccl_ranks": (dist.get_world_size() if (world > 1 and backend == "nccl") else 0), "allreduce_of_ones": total,
                          "self_check_primitive": check}))
    if world > 1:
        dist.destroy_process_group()


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.launch_check:
        return launch_check(a, world, rank)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the render path has no CPU fallback")
    local = local % torch.cuda.device_count()       # (lets a 2-rank gloo smoke test share one GPU; a no-op on a real node)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend = None
    if world > 1:
        backend = os.environ.get("CLIFT_DIST_BACKEND", "nccl")      # "nccl" is RCCL on ROCm
        if backend == "nccl" and torch.cuda.device_count() < world:
            backend = "gloo"                                        # ranks share a device (1-GPU test box): RCCL wants one device per rank
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    if a.global_rays:
        a.rays = max(1, a.global_rays // world)
    import contrastive_lift_amd as cl
    from contrastive_lift_amd import engine, synthetic
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config

    engine.set_mlp_precision(a.dtype)
    model, renderer, pool = synthetic.make_scene(grid=a.grid, num_classes=a.classes, max_instances=3, seed=0, device=dev)
    S = int(renderer.n_samples)
    if a.inference_sharded:
        return bench_inference_sharded(a, model, renderer, dev, world, rank, backend)
    cfg = default_config(chunk=a.chunk, instance_optimization_epoch=0, late_semantic_optimization=0, mlp_dtype=a.dtype, nosync=a.nosync)
    tr = HotPathTrainer(model, renderer, cfg, current_epoch=4)
    n_batches = 4
    batches = [synthetic.make_batches(pool, a.rays, a.inst_rays, a.classes, 25, seed=100 + rank * 17 + i, device=dev) for i in range(n_batches)]

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # Everything the measurement itself uses for the first time -- a device-to-host copy (the generator state in the snapshot), timing
    # events, their read-back -- is used once BEFORE the warm-up: the runtime creates queues / signal pools lazily, and in the first GPU
    # process on a fresh box that one-off cost (44-51 ms) landed in the first timed step.
    _ = tr._rng_state()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); torch.zeros(8, device=dev).cpu(); ev[1].record(); torch.cuda.synchronize(); _ = ev[0].elapsed_time(ev[1])
    # ... and so are the buffers of the state snapshot (only the replays after the timed region use it: --full, --soak) and the per-step events of
    # the timed loop: allocated / created (and recorded once) HERE, so that the caching allocator and the runtime's event pool are in the same
    # state during the warm-up as during the timed steps
    need_snap = a.full or a.soak > 0
    snap_bufs = [torch.empty_like(model.param_flat) for _ in range(5)] if need_snap else None
    # --dump-outputs: the set-up state, taken before any step -- the only training state that is the same in every run (every step sums
    # gradients through floating-point atomics, and Adam carries their last-bit differences into the parameters, so the state after the
    # warm-up and the timed steps differs between runs)
    init = state_snapshot(model, tr, [torch.empty_like(model.param_flat) for _ in range(5)]) if a.dump_outputs else None
    # ... and so is the interpreter's first FULL garbage collection: it traverses everything the imports and the set-up created (35 - 60 ms) and
    # fell at a fixed position of the run -- timed step 19 of 20 in seven runs out of eight once this round's edits had shifted the allocation
    # count.  Collected once here and frozen (gc.freeze: the set-up's objects are not traversed again); the step itself allocates little.
    import gc
    gc.collect()
    gc.freeze()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    for m_ in marks:
        m_.record()
    torch.cuda.synchronize()
    if world > 1 and tr.overlap_allreduce == "auto":
        # data-parallel: the trainer decides by measurement whether the asynchronous exchange (early range all-reduced under the density
        # backward, CUs reserved for RCCL) beats the synchronous one -- its 2 + 2 x 4 calibration passes synchronise the device, so
        # they run here, before the warm-up
        for i in range(tr.CAL_WARMUP + 2 * tr.CAL_STEPS):
            tr.training_step(batches[i % n_batches], lean=a.lean)
    for i in range(a.warmup):
        tr.training_step(batches[i % n_batches], lean=a.lean)
    # snapshot of the training state at the start of the timed region (parameters + both Adam states): the roofline pass below
    # replays exactly these steps with per-launch events
    snap = state_snapshot(model, tr, snap_bufs) if need_snap else None
    sync_all()
    # one event per step boundary (recorded, never waited on inside the loop): the per-step GPU times afterwards show whether the K steps were
    # uniform or whether one of them carried a one-off stall (seen: ~40 ms once in the first GPU process on a fresh box)
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        tr.training_step(batches[i % n_batches], lean=a.lean)
        marks[i + 1].record()
    sync_all()
    dt = time.perf_counter() - t0
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)]
    if os.environ.get("CLIFT_BENCH_DUMP"):
        print("[steps] " + " ".join(f"{x:.2f}" for x in step_ms), file=sys.stderr)
    step_ms_timed = list(step_ms)
    step_ms.sort()
    if a.dump_outputs:
        # the timed path's step once more, untimed, on inputs that are the same in every run: the set-up state and generators, the batch of
        # the last timed step (every rank takes part: the step all-reduces its gradients)
        restore_state(model, tr, init)
        tr.training_step(batches[(a.steps - 1) % n_batches], lean=a.lean)
        if rank == 0:
            lo = tr.last_outputs
            dump_outputs(a.dump_outputs, {"rgb": lo[0], "semantics": lo[1], "losses": tr.losses, "grads": model.grad_flat,
                                          "params": model.param_flat})
    rec_mean, rec, rec_all = roofline_replays(a, tr, batches, snap, sync_all) if a.full else (None, None, None)
    ar_ms, rank_ms, dp_check = None, None, None
    if world > 1:
        cdev = dev if backend == "nccl" else "cpu"
        t = torch.tensor([dt, -dt], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rank_ms = [-float(t[1]) / a.steps * 1e3, float(t[0]) / a.steps * 1e3]       # fastest / slowest rank's wall time per step
        dt = float(t[0])
    if world > 1 and a.full:
        # the exchange by itself: the main pass's gradient range (what every backward all-reduces), 5 times, event-bracketed on this stream
        r0, r1 = tr.main_range
        gbuf = model.grad_flat[r0:r1]
        dist.all_reduce(gbuf); sync_all()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            dist.all_reduce(gbuf)
        e1.record(); sync_all()
        ar_ms = {"main_range_bytes": 4 * (r1 - r0), "ms": e0.elapsed_time(e1) / 5, "backend": backend,
                 "note": "one all-reduce of the main pass's gradient range alone (no compute beside it), mean of 5"}
        dp_check = data_parallel_self_check(tr, model, batches[0], snap, a.lean, cdev, sync_all)
    soak = None
    if a.soak > 0:
        soak = soak_replays(tr, model, batches[0], snap, a.soak, a.lean, (dev if backend == "nccl" else "cpu") if world > 1 else None, sync_all)
    ms_step = dt / a.steps * 1e3
    samples_step = world * (a.rays + a.inst_rays) * S
    value = samples_step / (dt / a.steps)

    extra = {}
    roof = None
    cpu = None
    if a.full and rank == 0:
        roof = roofline(rec_mean, rec_all, a.steps, engine, a.dtype, ms_step, rec_min=rec)
    if a.full and rank == 0 and world == 1:
        # ---- per-pass split and sample statistics (outside the timed region)
        def timed(fn, n=n_batches):          # cycles through the same batches as the timed loop
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(n):
                fn(batches[i % n_batches])
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n
        t_main = timed(lambda b: tr.main_pass(b[0], lean=a.lean))
        t_inst = timed(lambda b: tr.instance_pass(b[1]))
        ctxs = tr.main_pass(batches[0][0], lean=a.lean)
        M = sum((int(c.ray_start[-1]) if getattr(c, "capped", False) else c.M) for c in ctxs)
        inbox = sum(int((c.alpha > 0).sum()) for c in ctxs)
        extra = dict(main_pass_ms=round(t_main * 1e3, 3), instance_pass_ms=round(t_inst * 1e3, 3),
                     main_pass_samples_per_s=a.rays * S / t_main, instance_pass_samples_per_s=a.inst_rays * S / t_inst,
                     f_active=M / (a.rays * S), f_inbox_alpha_gt0=inbox / (a.rays * S), samples_per_ray=S)
        extra["active_samples_per_s_main_pass"] = M / t_main            # cost follows the ACTIVE samples; comparable across scenes
        if not a.no_extras and a.dtype in ("fp32", "fp32x6"):
            # the reference's main pass computes the instance heads and discards their output (T:155); without that dead work:
            t_lean = timed(lambda b: tr.main_pass(b[0], lean=True))
            extra["lean_main_pass_ms"] = round(t_lean * 1e3, 3)
            extra["lean_step_ms_estimate"] = round((t_lean + t_inst) * 1e3, 3)
            # The other arithmetics and shapes on the same scene, AFTER the timed region, so that the driver-run record carries them: the other
            # fp32 arithmetic (exact fp32 MFMA when the run is the default fp32x6, and vice versa) with its own roofline, BASELINE configs[2]
            # (bf16 MLP operands), configs[3]'s per-GPU shape with the strong-scaling projection, configs[4] (frame render): same step
            # definition, 10 steps after 3 warm-up steps / one 262144-ray tile
            extra.update(inference_probe(cl, model, renderer, pool))
            extra.update(bf16_probe(a, dev, batches, S))
            extra.update(other_fp32_probe(a, dev, batches, S, "fp32" if a.dtype == "fp32x6" else "fp32x6"))
            extra.update(small_batch_probe(a, dev, pool, S, tr.model.arena.range_of("grid_density", "grid_app", "net_app", "net_sem")))
        if "bf16_ms_per_step" in extra:
            extra["bf16"] = {"mlp_arithmetic": MLP_ARITHMETIC["bf16"], "ms_per_step": extra["bf16_ms_per_step"], "ray_samples_per_s": extra["bf16_ray_samples_per_s"],
                             "roofline": {k: v for k, v in (extra.get("bf16_roofline") or {}).items() if k != "families"}}
        if roof is not None:
            # (the driver's record keeps `roofline`, `config` and `cpu_baseline` whole and only the NAMES of other keys: what a reader of that
            # record should see of the extras rides inside `roofline`)
            if "rays1024_ms_per_step" in extra:
                extra["rays1024"] = {"ms_per_step": extra["rays1024_ms_per_step"], "nosync_ms_per_step": extra.get("rays1024_nosync_ms_per_step"),
                                     "shape": "1024 main-pass rays + 1024 instance rays (configs[3] per-GPU shape)"}
            for k in ("exact_fp32", "fp32x6", "bf16", "rays1024", "configs3_strong_scaling_projection", "inference_roofline"):
                if k in extra:
                    roof.setdefault("other_measurements", {})[k] = extra[k]
    rccl_ranks = dist.get_world_size() if (world > 1 and backend == "nccl") else 0
    if world > 1:
        # every rank has left the timed region, the replays and the collectives: the group is done with.  Rank 0 then times the CPU path ALONE
        # (the other ranks have exited; `cores` = what this process may use) and prints the line.
        dist.barrier()
        dist.destroy_process_group()
    if a.full and rank == 0 and not a.no_cpu_baseline:
        cpu = cpu_baseline(model, renderer, batches[0], a, S)
    if rank == 0:
        line = {"metric": "ray-samples/sec (train step) at 4096 rays", "value": value, "unit": "ray-samples/s",
                "main_pass_samples_per_s": extra.get("main_pass_samples_per_s"), "n_gpus": world,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_step, "higher_is_better": True, "scaling": ("strong" if a.global_rays else "weak"),
                "vs_baseline": None, "full": a.full,
                "value_definition": "nominal ray-samples of one full training_step = (main-pass rays + instance-pass rays) x S, over all ranks, / step time; the "
                                    "main pass alone (the 4096 rays of the metric's name) is `main_pass_samples_per_s`, and because cost follows the ACTIVE "
                                    "samples (f_active of the nominal ones) `active_samples_per_s_main_pass` is the scene-independent figure",
                "dtype": {"fp32": "f32", "bf16": "bf16", "fp32x6": "f32"}[a.dtype],
                "data": "synthetic",
                "config": {"workload": ("BASELINE configs[1] stand-in: ScanNet-shaped scene (C=22, E=3/D=6, grid 128^3, S=440), "
                                        "full training_step = main pass 4096 rays + slow-fast instance pass 1024 rays, fp32") if a.dtype != "bf16" else
                                       (f"BASELINE configs[2]-style bf16 mode on the configs[1] shapes (C={a.classes}, E=3/D=6, grid {a.grid}^3): MLP "
                                        "operands bf16 (weights rounded in-kernel, hidden activations / gradients bf16-stored), fp32 accumulate; everything else fp32"),
                           "mlp_arithmetic": MLP_ARITHMETIC[a.dtype],
                           "main_pass_samples_per_s": extra.get("main_pass_samples_per_s"),
                           "rays_per_gpu": a.rays, "instance_rays_per_gpu": a.inst_rays, "grid": a.grid, "classes": a.classes,
                           "samples_per_ray": S, "chunk": a.chunk or a.rays, "lean_main_pass": bool(a.lean), "sync_free": bool(a.nosync),
                           "parallelism": f"dp{world} (rays sharded, 1 all-reduce per backward)"},
                "roofline": roof, "cpu_baseline": cpu,
                "dist_backend": backend, "rccl_ranks": rccl_ranks,
                "devices_visible": torch.cuda.device_count(),
                "allreduce_overlap": (tr.overlap_decision or {"overlap": tr.overlap_allreduce}) if world > 1 else None,
                "allreduce_cu_reserve": tr.allreduce_cu_reserve if world > 1 else None,
                "allreduce_ms": ar_ms, "rank_ms_per_step_min_max": rank_ms, "data_parallel_self_check": dp_check, "soak": soak,
                "scaling_note": ("`value` is BASELINE's metric (ray-samples/s of the whole job: every rank renders its own 4096 + 1024 rays -- N ranks "
                                 "render N instance images per step where one rank renders one); the driver's efficiency = value(N) / (N value(1)), and "
                                 "north_star's '>= 6x at 8 GPUs' is read against THIS ratio.  The step-TIME ratio of a fixed global batch "
                                 "(--global-rays, configs[3]) is the other reading: see configs3_strong_scaling_projection")}
        line.update(extra)
        #  the arithmetic of the headline number at the top level, with the exact-fp32 step of the same run beside it when it was measured
        line["arithmetic"] = {"fp32x6": "fp32x6 (fp32-faithful: six bf16 MFMA products of exactly three-way-split fp32 operands, fp32 accumulate)",
                              "fp32": "exact fp32 (fp32 MFMA)", "bf16": "bf16 operands, fp32 accumulate"}[a.dtype]
        if a.dtype == "fp32x6" and isinstance(extra.get("exact_fp32"), dict):
            line["exact_fp32_ms_per_step"] = extra["exact_fp32"].get("ms_per_step")
        line["step_ms_median"] = step_ms[len(step_ms) // 2]
        line["step_ms_min_max"] = [step_ms[0], step_ms[-1]]
        line["step_ms"] = step_ms_timed                 # GPU time of every timed step, in order (events at the step boundaries)
        print(json.dumps(line))


def state_snapshot(model, tr, bufs):
    """Training state (parameters, both Adam states, the step's generators) copied into five arena-sized buffers."""
    for buf, src in zip(bufs, (model.param_flat, tr.opt_main.m, tr.opt_main.v, tr.opt_inst.m, tr.opt_inst.v)):
        buf.copy_(src)
    return (bufs[0], {"m": bufs[1], "v": bufs[2], "t": dict(tr.opt_main.t), "lr_scale": tr.opt_main.lr_scale},
            {"m": bufs[3], "v": bufs[4], "t": dict(tr.opt_inst.t), "lr_scale": tr.opt_inst.lr_scale}, tr._rng_state())


def restore_state(model, tr, snap):
    model.param_flat.copy_(snap[0])
    tr.opt_main.load_state_dict(snap[1])
    tr.opt_inst.load_state_dict(snap[2])
    tr.load_rng_state(snap[3])


def roofline_replays(a, tr, batches, snap, sync_all):
    """--full: replays of the timed steps from their snapshot with matrix-core launches bracketed by HIP events; returns the records
    ``roofline`` is built from (dominant family: per-launch median and minimum of the replays; every launch: one replay)."""
    from contrastive_lift_amd import engine
    model, n_batches = tr.model, len(batches)
    # ---- roofline pass: the SAME steps again from the same state (the active-sample count drifts while the field trains, so
    # any other step would see a different launch mix), every clift_gemm launch bracketed by two HIP events on its launch
    # stream (torch's current stream; the side-stream mode is off by default).  Kept out of the timed region because creating
    # and recording ~80 events per step makes the step host-bound (+20 %); kernel durations are unaffected by that.
    real_gemm, real_first2, real_last2, real_app_last2, real_first2_bwd, real_first2_wgrad = (engine.gemm, engine.first2, engine.last2, engine.app_last2,
                                                                                              engine.first2_bwd, engine.first2_wgrad)
    real_first2_x6, real_last2_x6, real_first2_x6_bwd, real_first2_x6_wgrad = engine.first2_x6, engine.last2_x6, engine.first2_x6_bwd, engine.first2_x6_wgrad

    def replay(select):
        """Re-run the timed steps from the snapshot with the selected matrix-core launches bracketed by HIP events.  Two launch sites:
        engine.gemm (clift_gemm) and engine.first2 (clift_xyz_head_first2_fwd: the K = 3 layer generated inside the persistent kernel
        of the first 256 x 256 layer -- kind "fwd_gen", FLOPs of both layers)."""
        restore_state(model, tr, snap)          # (the generators too: the per-ray jitter -- same samples, same launch sizes)
        out = []

        def bracket(kind, M, N, K, extra_flops, nbytes, fn):
            """nbytes = ALGORITHMIC HBM bytes of the launch: every operand row read once, every result row written once, weights once."""
            if not select(kind, N):
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            out.append((kind, M, N, K, e0, e1, extra_flops, nbytes))
        WB = 256 * 256 * 4.0                                # one 256 x 256 fp32 weight matrix

        def recorded_gemm(M, N, K, *args, **kw):
            kind = "wgrad" if kw.get("a_trans") else "dgrad" if kw.get("b_trans") else "fwd"
            if kind == "wgrad":
                nb = 4.0 * K * (M + N) + 4.0 * M * N
            else:
                nb = 4.0 * M * (K + N) + 4.0 * N * K + (4.0 * M * N if kw.get("mask") is not None else 0.0)
            return bracket(kind, M, N, K, 0.0, nb, lambda: real_gemm(M, N, K, *args, **kw))

        def recorded_first2(M, *args):                     # args = (xa, W0, b0, W1, b1, h1, h2)
            return bracket("fwd_gen", M, 256, 256, 2.0 * M * 256 * 3, M * (16.0 + 1024.0 * (2 if args[5] is not None else 1)) + WB, lambda: real_first2(M, *args))

        def out_bytes(M, E, hidden, x6):                   # last hidden layer + output layer: row in, E outputs out, hidden if kept, x6: 256 B of partial sums out and back
            return M * (1024.0 + 4.0 * E + (1024.0 if hidden is not None else 0.0) + (512.0 if x6 else 0.0)) + WB

        def recorded_last2(M, h, W, b, Wo, bo, hidden, *args):        # last hidden layer + narrow output layer (clift_xyz_head_last2_fwd)
            return bracket("fwd_out", M, 256, 256, 2.0 * M * 256 * Wo.shape[0], out_bytes(M, Wo.shape[0], hidden, False), lambda: real_last2(M, h, W, b, Wo, bo, hidden, *args))
        def recorded_app_last2(M, H1, W2, b2, W3, *args):  # appearance: last hidden layer + output layer + sigmoid (clift_app_head_last2_fwd)
            return bracket("fwd_out", M, 128, 128, 2.0 * M * 128 * W3.shape[0], M * 1036.0, lambda: real_app_last2(M, H1, W2, b2, W3, *args))
        def recorded_first2_bwd(M, *args):                 # second layer's masked dgrad + the K = 3 layer's weight gradient (clift_xyz_head_first2_bwd)
            return bracket("dgrad", M, 256, 256, 2.0 * M * 256 * 4, M * 1040.0 + WB, lambda: real_first2_bwd(M, *args))
        def recorded_first2_wgrad(M, *args):               # second layer's weight gradient over the regenerated first activation (clift_xyz_head_first2_wgrad)
            return bracket("wgrad", 256, 256, M, 2.0 * M * 256 * 3, M * 1040.0 + WB, lambda: real_first2_wgrad(M, *args))
        engine.gemm, engine.first2, engine.last2, engine.app_last2 = recorded_gemm, recorded_first2, recorded_last2, recorded_app_last2
        engine.first2_bwd, engine.first2_wgrad = recorded_first2_bwd, recorded_first2_wgrad

        def recorded_first2_x6(M, *args):                  # fp32x6 mode: the same fusion on the split kernel (clift_xyz_head_first2_x6_fwd)
            return bracket("fwd_gen", M, 256, 256, 2.0 * M * 256 * 3, M * 1040.0 + WB, lambda: real_first2_x6(M, *args))
        engine.first2_x6 = recorded_first2_x6
        real_out_fwd = engine.out_layer_fwd               # E <= 32 output layer + row softmax as one stream (clift_out_layer_fwd)
        engine.out_layer_fwd = lambda M, h, W, *args: bracket("fwd", M, W.shape[0], 256, 0.0, M * (1024.0 + 4.0 * W.shape[0]), lambda: real_out_fwd(M, h, W, *args))
        # ... and the other fused ends of the mode (ABI 14)
        engine.last2_x6 = lambda M, h, W, b, Wo, bo, hidden, *args: bracket("fwd_out", M, 256, 256, 2.0 * M * 256 * Wo.shape[0], out_bytes(M, Wo.shape[0], hidden, True),
                                                                            lambda: real_last2_x6(M, h, W, b, Wo, bo, hidden, *args))
        engine.first2_x6_bwd = lambda M, *args: bracket("dgrad", M, 256, 256, 2.0 * M * 256 * 4, M * 1040.0 + WB, lambda: real_first2_x6_bwd(M, *args))
        engine.first2_x6_wgrad = lambda M, *args: bracket("wgrad", 256, 256, M, 2.0 * M * 256 * 3, M * 1040.0 + WB, lambda: real_first2_x6_wgrad(M, *args))
        try:
            for i in range(a.steps):
                tr.training_step(batches[i % n_batches], lean=a.lean)
            sync_all()
        finally:
            engine.gemm, engine.first2, engine.last2, engine.app_last2 = real_gemm, real_first2, real_last2, real_app_last2
            engine.first2_bwd, engine.first2_wgrad, engine.first2_x6 = real_first2_bwd, real_first2_wgrad, real_first2_x6
            engine.last2_x6, engine.first2_x6_bwd, engine.first2_x6_wgrad = real_last2_x6, real_first2_x6_bwd, real_first2_x6_wgrad
            engine.out_layer_fwd = real_out_fwd
        return out
    # pass 1: only the dominant kernel's launches (k_layer_f32 forward: the 11 256 x 256 forward layers of a step, in its three
    # instantiations -- plain, K = 3 input generated in-kernel, narrow output layer fused) -- few enough events that the step stays
    # GPU-bound, so an event pair measures the kernel and not a host gap; pass 2: every matrix-core launch, for the informational all_gemm
    # split (the ~60 events per step make that pass host-bound, so its per-launch times are upper bounds).
    # The pass runs TWICE and each launch keeps the shorter of its two measurements: an event pair also contains any moment the GPU
    # sat idle between the two records, and a single host hiccup (seen: 40 ms inside one bracket of the first process on a fresh box)
    # would otherwise pass for kernel time.  The replays are deterministic (same state, same batches), so launch i is the same work.
    def resolve(recs):
        return [(kind, M, N, K, e0.elapsed_time(e1), xf, nb) for kind, M, N, K, e0, e1, xf, nb in recs]
    dom_sel = lambda kind, N: kind in ("fwd", "fwd_gen", "fwd_out") and N > 128
    rec, rec_b, rec_c = resolve(replay(dom_sel)), resolve(replay(dom_sel)), resolve(replay(dom_sel))
    # (same launch = same kind and shape at the same position; the row count may differ by a few samples between replays -- the gradient
    # atomics are not order-deterministic, so a later step's active-sample count can move by one or two)
    same = lambda x, y: x[0] == y[0] and x[2:4] == y[2:4] and abs(x[1] - y[1]) <= 0.01 * max(x[1], y[1])
    # what `roofline.frac` is built from: per launch the MEDIAN of three dominant-only replays.  (Round 3 reported the minimum -- optimistic, VERDICT r3
    # item 10; the mean of two that followed is at the mercy of one stall: a run right behind the 17-minute test session read 0.22 where the same
    # kernels' rocprofv3 average gives 0.46 -- one replay's brackets of one instantiation were 3.6 x too long.)
    rec_mean = rec
    if len(rec) == len(rec_b) == len(rec_c) and all(same(x, y) and same(x, z) for x, y, z in zip(rec, rec_b, rec_c)):
        rec_mean = [x[:4] + (sorted((x[4], y[4], z[4]))[1],) + x[5:] for x, y, z in zip(rec, rec_b, rec_c)]
        rec = [x[:4] + (min(x[4], y[4], z[4]),) + x[5:] for x, y, z in zip(rec, rec_b, rec_c)]
    rec_all = resolve(replay(lambda kind, N: True))
    # every bracket is an UPPER bound of its kernel's time (it also contains any moment the GPU idled between the two records), and the third
    # replay bracketed the same launches once more: keep the shortest of the three per launch (seen once: all OUTV brackets of both dominant
    # passes 3x too long in a run right behind a 20-minute test session -- 0.45 instead of 0.77 -- while the all-launch pass read 111 TFLOP/s)
    sub = [x for x in rec_all if dom_sel(x[0], x[2])]
    if len(sub) == len(rec) and all(same(x, y) for x, y in zip(rec, sub)):
        rec = [x[:4] + (min(x[4], y[4]),) + x[5:] for x, y in zip(rec, sub)]
    return rec_mean, rec, rec_all


def max_delta_across_ranks(t, cdev):
    """max over the elements of (MAX over ranks - MIN over ranks) of a tensor every rank holds: 0.0 iff all ranks hold the same values."""
    import torch.distributed as dist
    hi, lo = t.to(cdev).clone(), t.to(cdev).clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return float((hi - lo).abs().max())


def soak_replays(tr, model, batch, snap, K, lean, cdev, sync_all):
    """--soak K: K replays of ONE full training step (main pass + instance pass, Adam) from the snapshot of the timed region,
    same batch / jitter / background, asynchronous gradient exchange forced ON when there is more than one rank (the RCCL kernels then run
    beside the persistent MFMA kernels -- a co-residency that has never run on hardware, and the sharing history of csrc/layer_x6.hip:24-28
    is the reason to check).  Deterministic by construction: the rendered rgb / semantics of the main pass and the instance features' loss
    inputs (no atomics on that path) -- bit-compared with the first replay.  Order-dependent in the last bits: gradients and updated
    parameters (floating-point atomics) -- compared within 10 x the difference two identical single-rank passes show, floor 1e-6 of the
    largest entry.  Counts are MAX-reduced over the ranks."""
    import torch.distributed as dist
    g = torch.Generator(device="cpu").manual_seed(4321)
    dev = model.param_flat.device
    jit = torch.rand(batch[0]["rays"].shape[0], generator=g).to(dev)
    ijit = [torch.rand(img["rays"].shape[0], generator=g).to(dev) for img in batch[1]]
    keep = tr.overlap_allreduce
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        tr.overlap_allreduce = True
    r0, r1 = tr.main_range
    first, bad_out, bad_grad, worst = None, 0, 0, 0.0
    try:
        for k in range(K):
            with torch.no_grad():
                model.param_flat.copy_(snap[0])
            tr.opt_main.load_state_dict(snap[1])
            tr.opt_inst.load_state_dict(snap[2])
            tr.main_pass(batch[0], jitter=jit, white_bg=False, lean=lean)
            outs = [t.detach().clone() for t in tr.last_outputs]
            grad = model.grad_flat[r0:r1].detach().clone()
            for img, ij in zip(batch[1], ijit):
                tr.instance_pass([img], jitter=ij)
            sync_all()
            par = model.param_flat.detach().clone()
            if first is None:
                first = (outs, grad, par)
                scale = max(float(grad.abs().max()), 1e-30)
                continue
            if not all(torch.equal(x, y) for x, y in zip(outs, first[0])):
                bad_out += 1
            d = float((grad - first[1]).abs().max()) / scale
            worst = max(worst, d)
            if d > 1e-5 or not bool(torch.isfinite(par).all()):
                bad_grad += 1
    finally:
        tr.overlap_allreduce = keep
    res = {"replays": K, "overlap_forced_on": bool(tr.world > 1), "replays_with_different_outputs": bad_out,
           "replays_with_gradients_beyond_atomics_noise": bad_grad, "worst_gradient_delta_rel": worst,
           "note": "outputs bit-compared, gradients within 1e-5 of the largest entry (sums through floating-point atomics differ in the last bits between any two passes)"}
    if cdev is not None:
        t = torch.tensor([float(bad_out), float(bad_grad), worst], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        res.update(replays_with_different_outputs=int(t[0]), replays_with_gradients_beyond_atomics_noise=int(t[1]), worst_gradient_delta_rel=float(t[2]))
    return res


def data_parallel_self_check(tr, model, batch, snap, lean, cdev, sync_all):
    """N > 1 only: is the exchange CORRECT under the real collective, not only fast?
    * `param_max_abs_delta_across_ranks`: after all the steps of this run, element-wise MAX and MIN of the flat parameter arena over the ranks
      (two all-reduces); every rank applied the same all-reduced gradients to the same initial state, so the difference must be exactly 0.
    * `overlap_grad`: from the snapshot of the timed region, the main pass of one step with the asynchronous exchange (early range all-reduced
      beside the density backward, CUs reserved for the collective) and with the synchronous one, same batch / jitter / background; the
      all-reduced gradients are compared.  A rank's own sums go through floating-point atomics, so two passes differ in the last bits even
      with the same setting: the same-setting difference is measured too and `equal` means 'no further than 10 x that noise (floor 1e-6 of
      the largest gradient entry)'.  The verdicts are MAX-reduced over the ranks."""
    import torch.distributed as dist
    out = {}
    out["param_max_abs_delta_across_ranks"] = max_delta_across_ranks(model.param_flat.detach(), cdev)
    out["params_identical_across_ranks"] = out["param_max_abs_delta_across_ranks"] == 0.0
    r0, r1 = tr.main_range
    g = torch.Generator(device="cpu").manual_seed(1234)
    jit = torch.rand(batch[0]["rays"].shape[0], generator=g).to(model.param_flat.device)
    keep = tr.overlap_allreduce

    def grads(overlap):
        with torch.no_grad():
            model.param_flat.copy_(snap[0])
        tr.opt_main.load_state_dict(snap[1])
        tr.opt_inst.load_state_dict(snap[2])
        tr.overlap_allreduce = overlap
        tr.main_pass(batch[0], jitter=jit, white_bg=False, lean=lean)
        sync_all()
        return model.grad_flat[r0:r1].detach().clone()
    try:
        g_sync, g_sync2, g_over = grads(False), grads(False), grads(True)
    finally:
        tr.overlap_allreduce = keep
    scale = max(float(g_sync.abs().max()), 1e-30)
    noise = float((g_sync - g_sync2).abs().max()) / scale
    delta = float((g_sync - g_over).abs().max()) / scale
    t = torch.tensor([noise, delta], dtype=torch.float64, device=cdev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    noise, delta = float(t[0]), float(t[1])
    out["overlap_grad"] = {"max_abs_delta_over_max_entry": delta, "same_setting_noise": noise, "equal": bool(delta <= max(10.0 * noise, 1e-6)),
                           "finite": bool(torch.isfinite(g_over).all())}
    out["overlap_grad_equal"] = out["overlap_grad"]["equal"] and out["overlap_grad"]["finite"]
    return out


MLP_ARITHMETIC = {
    "fp32x6": "fp32 in, fp32 out, fp32-FAITHFUL products on the bf16 matrix cores for the 256-wide layers (forward, input gradient, weight gradient): every "
              "fp32 operand is split exactly into three bf16 terms (8 + 8 + 8 significant bits), the six leading cross products run on "
              "v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the three dropped terms are below one fp32 rounding of the product (row-max relative "
              "error vs float64 2e-7 .. 8e-7 = the exact-fp32 kernels' own; tests/test_gpu_round3.py, test_gpu_round4.py); since round 5 the 128-wide "
              "appearance layers likewise (csrc/layer_n6.hip, tests/test_gpu_round5b.py); K = 3 / E <= 32 layers, activations, losses, tables and the "
              "optimizer are plain fp32",
    "fp32": "exact fp32 products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, bit-identical to an fmaf chain), fp32 accumulate",
    "bf16": "MLP operands rounded to bf16 (RNE) in the kernels, hidden activations / hidden gradients bf16-stored, fp32 accumulate; everything else fp32",
}
FRAME_W, FRAME_H = 1296, 968             # BASELINE configs[4]: ScanNet colour frame


def head_flops_per_active_sample(model):
    """Forward matrix-core FLOPs of all heads per ACTIVE sample: 2 x (sum of in x out over every Linear of the appearance MLP + basis,
    the semantic MLP and both instance MLPs)."""
    tot = 0
    for name, t in model.named_views().items():
        if name.endswith(".weight") and t.dim() == 2 and ("mlp" in name or "basis_mat" in name):
            tot += 2 * t.shape[0] * t.shape[1]
    return float(tot)


def bench_inference_sharded(a, model, renderer, dev, world, rank, backend):
    """configs[4]: full 1296 x 968 frames (is_train=False, step ratio halved as RP:104, chunked like RP:114-120) through
    ``inference.render_rays_sharded``: contiguous row tiles, one per rank, ONE all-gather of the packed outputs per frame.  A step is one
    frame; value = rays/s over the job (strong scaling: the frame is fixed)."""
    import numpy as np
    from contrastive_lift_amd import inference as inf, synthetic
    from contrastive_lift_amd.rays import generate_ray_table
    K = np.array([[1170.0, 0, 647.75], [0, 1170.0, 483.75], [0, 0, 1]], np.float32)
    rays = generate_ray_table(FRAME_H, FRAME_W, K, synthetic.look_at((0.0, 0.0, -0.9)), device=dev)
    renderer.update_step_ratio(renderer.step_ratio * 0.5)
    S = int(renderer.n_samples)
    chunk = a.chunk or 65536

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()
    for _ in range(max(1, a.warmup)):
        out = inf.render_rays_sharded(model, renderer, rays, chunk)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = inf.render_rays_sharded(model, renderer, rays, chunk)
    sync_all()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, dict(zip(("rgb", "semantics", "instances", "distance"), out)))
    if rank == 0:
        P = rays.shape[0]
        t_frame = dt / a.steps
        roof = None
        if a.full:
            # active samples of the frame (cost follows them): counted once on this rank's tile, outside the timed region
            b = inf.tile_bounds(P, world)
            mine = rays[b[0]:b[1]]
            act = 0
            for i in range(0, mine.shape[0], chunk):
                _, ctx = engine_render_forward(model, renderer, mine[i:i + chunk])
                act += int(ctx.M)
            fl = head_flops_per_active_sample(model)
            tf = act * world * fl / t_frame / 1e12          # tiles are equal-sized; this rank's active fraction stands for the frame
            roof = inference_roofline_object(tf, a.dtype, act * world / P, fl)
        print(json.dumps({"metric": "rays/sec (full-frame 1296x968 render, row tiles sharded over the ranks)", "value": P / t_frame,
                          "unit": "rays/s", "n_gpus": world, "steps": a.steps, "warmup": max(1, a.warmup), "ms_per_step": t_frame * 1e3,
                          "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": {"fp32": "f32", "fp32x6": "f32"}.get(a.dtype, a.dtype),
                          "data": "synthetic",
                          "config": {"workload": "BASELINE configs[4] stand-in: one 1296x968 frame (1,254,528 rays), is_train=False, S=%d, "
                                                 "chunk %d rays, rgb/semantics/instances/distance outputs" % (S, chunk),
                                     "mlp_arithmetic": MLP_ARITHMETIC[a.dtype],
                                     "rays_per_frame": P, "samples_per_ray": S, "classes": a.classes, "grid": a.grid,
                                     "parallelism": f"row tiles over {world} rank(s), 1 all-gather per frame"},
                          "ray_samples_per_s": P * S / t_frame,
                          "inference_roofline": roof, "full": a.full,
                          "dist_backend": backend, "rccl_ranks": (dist.get_world_size() if backend == "nccl" else 0),
                          "devices_visible": torch.cuda.device_count()}))
    if world > 1:
        dist.destroy_process_group()


DUMP_BUDGET_BYTES = 64 * 2 ** 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs DIR: every array as float32 DIR/<name>.npy.  When they add up to more than DUMP_BUDGET_BYTES, an array larger than its
    equal share of the budget is cut to a sample of its leading-dimension rows that fits the share: numpy default_rng(0), sorted, so the same
    arguments give the same rows in every run and every build."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {name: t.detach().to(torch.float32).cpu().numpy() for name, t in arrays.items()}
    share = DUMP_BUDGET_BYTES // len(host)
    over = sum(x.nbytes for x in host.values()) > DUMP_BUDGET_BYTES
    for name, x in host.items():
        if over and x.nbytes > share:
            rows = x.shape[0]
            keep = max(1, share // (x.nbytes // rows))
            x = x[np.sort(np.random.default_rng(0).choice(rows, keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(x))


def inference_roofline_object(tf, mode, act_per_ray, fl):
    """Whole-render figure: forward head FLOPs (fp32-equivalent 2MNK) of the active samples / render time, against the matrix-core peak of the
    arithmetic in use (fp32x6: 6 bf16 products per fp32 product of the 256-wide layers, ~92 % of the FLOPs, against the dense bf16 peak)."""
    if mode == "fp32x6":
        return {"bound": "mfma", "achieved": 6.0 * tf, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s (bf16 MFMA FLOPs = 6 x the fp32-equivalent head FLOPs)",
                "frac": 6.0 * tf / PEAK_BF16_MFMA_TFLOPS, "fp32_equivalent_tflops": tf, "fp32_equivalent_vs_exact_fp32_mfma_peak": tf / PEAK_FP32_MFMA_TFLOPS,
                "active_samples_per_ray": act_per_ray, "flops_per_active_sample": fl,
                "note": "head FLOPs of the active samples / render time (includes every non-MLP kernel of the render)"}
    return {"bound": "mfma", "achieved": tf, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS,
            "active_samples_per_ray": act_per_ray, "flops_per_active_sample": fl,
            "note": "head FLOPs of the active samples / render time / exact-fp32 MFMA peak"}


def engine_render_forward(model, renderer, rays):
    from contrastive_lift_amd import engine
    with torch.no_grad():
        return engine.render_forward(model, renderer, rays, None, False, grad_heads=())


def bf16_probe(a, dev, batches, S, steps=10, warmup=3):
    """The same training_step in bf16 mode (mlp_dtype "bf16": bf16 MLP operands, bf16-stored hidden activations, fp32 accumulate;
    everything else fp32) on a fresh copy of the scene."""
    from contrastive_lift_amd import engine, synthetic
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    prev = engine.set_mlp_precision("bf16")
    try:
        model, renderer, pool = synthetic.make_scene(grid=a.grid, num_classes=a.classes, max_instances=3, seed=0, device=dev)
        tr = HotPathTrainer(model, renderer, default_config(chunk=a.chunk, instance_optimization_epoch=0, late_semantic_optimization=0,
                                                            mlp_dtype="bf16"), current_epoch=4)
        for i in range(warmup):
            tr.training_step(batches[i % len(batches)], lean=a.lean)
        torch.cuda.synchronize()
        dt = extras_step_time(tr, batches, steps, a.lean)
        bf16_roof = bf16_roofline_pass(tr, batches, a.lean)
        # frame render in bf16 mode (the xyz heads run as one fused kernel each: csrc/head_bf16.hip)
        from contrastive_lift_amd import inference as inf
        ratio = renderer.step_ratio
        renderer.update_step_ratio(ratio * 0.5)
        try:
            rays = pool[:262144].contiguous()
            inf.render_rays(model, renderer, rays[:32768], 32768)
            torch.cuda.synchronize()
            t = time.perf_counter()
            inf.render_rays(model, renderer, rays, 32768)
            torch.cuda.synchronize()
            inf_rate = rays.shape[0] / (time.perf_counter() - t)
        finally:
            renderer.update_step_ratio(ratio)
    finally:
        engine.set_mlp_precision(prev)
    return dict(bf16_ms_per_step=round(dt * 1e3, 3), bf16_ray_samples_per_s=(a.rays + a.inst_rays) * S / dt, bf16_inference_rays_per_s=inf_rate,
                bf16_roofline=bf16_roof)


def extras_step_time(tr, batches, steps, lean):
    """Seconds per training_step for the EXTRAS (not the headline, whose contract is wall time over all K steps): per-step GPU times from events
    recorded at the step boundaries, MEDIAN -- a one-off stall of a few ms inside a ten-step probe (seen: fp32x6 reported 6.98 instead of 6.5 ms
    once) would otherwise pass for the mode's speed."""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        tr.training_step(batches[i % len(batches)], lean=lean)
        marks[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return ts[steps // 2] * 1e-3


def forward_family_pass(tr, batches, lean, steps=3):
    """Event brackets around the dominant family's launches (the 256 x 256 forward layers of the xyz heads, every instantiation) over `steps`
    training steps of `tr`'s arithmetic: returns (fp32-equivalent FLOPs, ms, launches)."""
    from contrastive_lift_amd import engine
    names = ("gemm", "first2", "last2", "first2_x6", "last2_x6")
    real = {n: getattr(engine, n) for n in names}
    rec = []

    def bracket(flops, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        rec.append((flops, e0, e1))

    def gemm(M, N, K, *args, **kw):
        if N == 256 and K == 256 and not kw.get("a_trans") and not kw.get("b_trans"):
            return bracket(2.0 * M * N * K, lambda: real["gemm"](M, N, K, *args, **kw))
        return real["gemm"](M, N, K, *args, **kw)
    wrap_gen = lambda fn: (lambda M, *args: bracket(2.0 * M * 256 * (256 + 3), lambda: fn(M, *args)))
    wrap_out = lambda fn: (lambda M, h, W, b, Wo, *args: bracket(2.0 * M * 256 * (256 + Wo.shape[0]), lambda: fn(M, h, W, b, Wo, *args)))
    engine.gemm = gemm
    engine.first2, engine.first2_x6 = wrap_gen(real["first2"]), wrap_gen(real["first2_x6"])
    engine.last2, engine.last2_x6 = wrap_out(real["last2"]), wrap_out(real["last2_x6"])
    try:
        for i in range(steps):
            tr.training_step(batches[i % len(batches)], lean=lean)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(engine, n, real[n])
    return sum(f for f, _, _ in rec), sum(e0.elapsed_time(e1) for _, e0, e1 in rec), len(rec) // steps


def other_fp32_probe(a, dev, batches, S, mode, steps=10, warmup=3):
    """The same training_step in the OTHER fp32 arithmetic (exact fp32 MFMA when the timed run is the default fp32x6, and vice versa) on a fresh
    copy of the scene, with the roofline of its own dominant kernel family (the 256 x 256 forward layers) and its frame-render rate."""
    from contrastive_lift_amd import engine, synthetic
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    prev = engine.set_mlp_precision(mode)
    try:
        model, renderer, pool = synthetic.make_scene(grid=a.grid, num_classes=a.classes, max_instances=3, seed=0, device=dev)
        tr = HotPathTrainer(model, renderer, default_config(chunk=a.chunk, instance_optimization_epoch=0, late_semantic_optimization=0,
                                                            mlp_dtype=mode), current_epoch=4)
        for i in range(warmup):
            tr.training_step(batches[i % len(batches)], lean=a.lean)
        torch.cuda.synchronize()
        dt = extras_step_time(tr, batches, steps, a.lean)
        fl, ms, per_step = forward_family_pass(tr, batches, a.lean)
        from contrastive_lift_amd import inference as inf
        ratio = renderer.step_ratio
        renderer.update_step_ratio(ratio * 0.5)
        try:
            rays = pool[:262144].contiguous()
            inf.render_rays(model, renderer, rays[:32768], 32768)
            torch.cuda.synchronize()
            t = time.perf_counter()
            inf.render_rays(model, renderer, rays, 32768)
            torch.cuda.synchronize()
            inf_rate = rays.shape[0] / (time.perf_counter() - t)
        finally:
            renderer.update_step_ratio(ratio)
    finally:
        engine.set_mlp_precision(prev)
    tfl = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    if mode == "fp32":
        roof = {"bound": "mfma", "kernel": "k_layer_f32<false, *, *, false> (csrc/layer_f32.hip, v_mfma_f32_32x32x2_f32)", "achieved": tfl, "peak": PEAK_FP32_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": tfl / PEAK_FP32_MFMA_TFLOPS, "launches_per_step": per_step}
        key = "exact_fp32"
    else:
        roof = {"bound": "mfma", "kernel": "k_layer_x6<false, *> (csrc/layer_x6.hip, v_mfma_f32_32x32x16_bf16 x 6)", "achieved": 6.0 * tfl, "peak": PEAK_BF16_MFMA_TFLOPS,
                "unit": "TFLOP/s (bf16 MFMA FLOPs = 6 x the fp32-equivalent 2MNK)", "frac": 6.0 * tfl / PEAK_BF16_MFMA_TFLOPS, "fp32_equivalent_tflops": tfl,
                "launches_per_step": per_step}
        key = "fp32x6"
    return {key: {"mlp_arithmetic": MLP_ARITHMETIC[mode], "ms_per_step": round(dt * 1e3, 3), "ray_samples_per_s": (a.rays + a.inst_rays) * S / dt,
                  "inference_rays_per_s": inf_rate, "roofline": roof,
                  "note": f"same scene, same batches, {steps} steps after {warmup} warm-up steps (median of per-step GPU times); the roofline brackets are taken over 3 further steps"},
            f"{key}_ms_per_step": round(dt * 1e3, 3)}


def small_batch_probe(a, dev, pool, S, main_range, rays=1024, steps=10, warmup=3):
    """BASELINE configs[3] per-GPU shape: 8192 rays per step over 8 GPUs = 1024 main-pass rays per rank (+ one 1024-ray instance image per rank,
    as the reference's DDP), in the library's default arithmetic, on this one GPU -- and the same step at the job's whole 8192 rays on this GPU:
    their ratio, with the gradient all-reduce priced in, projects the strong-scaling figure of configs[3] on 8 GPUs."""
    from contrastive_lift_amd import synthetic
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    out = {}
    for n in (rays, 8 * rays):
        model, renderer, _ = synthetic.make_scene(grid=a.grid, num_classes=a.classes, max_instances=3, seed=0, device=dev)
        tr = HotPathTrainer(model, renderer, default_config(chunk=a.chunk, instance_optimization_epoch=0, late_semantic_optimization=0, mlp_dtype=a.dtype), current_epoch=4)
        bs = [synthetic.make_batches(pool, n, a.inst_rays, a.classes, 25, seed=300 + i, device=dev) for i in range(4)]
        for i in range(warmup):
            tr.training_step(bs[i % 4], lean=a.lean)
        torch.cuda.synchronize()
        out[n] = extras_step_time(tr, bs, steps, a.lean)
    # the same 1024 + 1024 step in the sync-free mode (no read-back of the active-sample count; VERDICT r4 item 5 / weak point 8: at this shape --
    # ~45 % of the step in sub-50-us launches -- the gaps around the two read-backs are a larger share than at 4096 rays)
    nosync_ms = None
    if a.dtype in ("fp32", "fp32x6"):
        model, renderer, _ = synthetic.make_scene(grid=a.grid, num_classes=a.classes, max_instances=3, seed=0, device=dev)
        tr = HotPathTrainer(model, renderer, default_config(chunk=a.chunk, instance_optimization_epoch=0, late_semantic_optimization=0, mlp_dtype=a.dtype, nosync=True),
                            current_epoch=4)
        bs = [synthetic.make_batches(pool, rays, a.inst_rays, a.classes, 25, seed=300 + i, device=dev) for i in range(4)]
        for i in range(warmup + 3):          # (+ the two capacity-learning steps of the mode)
            tr.training_step(bs[i % 4], lean=a.lean)
        torch.cuda.synchronize()
        nosync_ms = extras_step_time(tr, bs, steps, a.lean) * 1e3
        overflow = tr.overflow_steps
    nbytes = 4 * (main_range[1] - main_range[0])
    # ring all-reduce over the 8 GPUs of a node: 2 (N-1)/N of the buffer per link direction; RCCL reaches ~150 GB/s bus bandwidth at this
    # message size on xGMI (7 links x ~50 GB/s per direction shared by the ring's two neighbours), + ~40 us of launch / sync latency per collective
    ar_ms = 2.0 * 7 / 8 * nbytes / 150e9 * 1e3 + 0.04 + 0.04
    t1, t8 = out[8 * rays] * 1e3, out[rays] * 1e3
    return {"rays1024_ms_per_step": round(t8, 3), "rays1024_ray_samples_per_s": (rays + a.inst_rays) * S / out[rays],
            "rays8192_ms_per_step": round(t1, 3),
            "rays1024_nosync_ms_per_step": (round(nosync_ms, 3) if nosync_ms is not None else None),
            "rays1024_nosync_note": (f"the same step with config.nosync (no host read-back; capacities instead of counts): {nosync_ms:.3f} ms against {t8:.3f} ms with "
                                     f"the two read-backs; {overflow} capacity overflows" if nosync_ms is not None else None),
            "rays1024_note": f"configs[3] per-GPU shape (8192 global rays / 8 ranks): 1024 main-pass rays + 1024 instance rays per step, {a.dtype}",
            "configs3_strong_scaling_projection": {
                "projected_strong_scaling_8gpu": t1 / (t8 + ar_ms), "one_gpu_8192_rays_ms": round(t1, 3), "per_gpu_1024_rays_ms": round(t8, 3),
                "projected_scaling_in_metric_unit_8gpu": (8 * (rays + a.inst_rays) / (t8 + ar_ms)) / ((8 * rays + a.inst_rays) / t1),
                "which_ratio_the_6x_target_means": "north_star's '>= 6x at 8 GPUs' is a THROUGHPUT statement in BASELINE's metric (ray-samples/s): "
                                                   "`projected_scaling_in_metric_unit_8gpu` (eight ranks render eight instance images per step, one rank "
                                                   "renders one) is the figure to hold against it; `projected_strong_scaling_8gpu` is the step-time ratio",
                "allreduce_ms_estimate": round(ar_ms, 3), "allreduce_bytes": nbytes,
                "ideal_given_the_per_rank_instance_pass": "every rank renders its OWN 1024-ray instance image whatever the rank count (the reference's DDP): with a "
                                                          "perfectly linear main pass the ratio is (8 m + i) / (m + i) -- it only reaches 8 when i = 0",
                "note": "(one GPU at 8192 + 1024 rays) / (one GPU at 1024 + 1024 rays + an ESTIMATED all-reduce of the main gradient range + the instance range): "
                        "both step times measured here, the all-reduce priced at 150 GB/s ring bus bandwidth + 40 us per collective (no multi-GPU node in this run)"}}


def bf16_roofline_pass(tr, batches, lean, steps=3):
    """bf16 mode is HBM-bound (bf16 MFMAs run 16x the fp32 rate): per kernel family of the xyz heads, ALGORITHMIC bytes per launch / launch
    time from HIP events around the launch sites (engine.head_bf16 = the fused whole-head forward, engine.gemm = per-layer forward / dgrad
    / wgrad launches), over `steps` training steps after the timed ones.  The family with the largest time share is reported as the
    dominant kernel, against the 8 TB/s peak and the ~6.3 TB/s a pure stream reaches on this chip (MI355X_MICROARCH.md)."""
    from contrastive_lift_amd import engine
    real_head, real_gemm = engine.head_bf16, engine.gemm
    rec = []

    def bracket(kind, nbytes, flops, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        rec.append((kind, nbytes, flops, e0, e1))

    def head(M, xa, l0, l1, l2, lout, h1, h2, h3, out, ldo, col_off):
        kept = sum(x is not None for x in (h1, h2, h3))
        nb = M * (16.0 + (4.0 * lout[0].shape[0] if lout is not None else 0.0) + kept * 512.0) + 3 * 256 * 256 * 4.0
        fl = 2.0 * M * (3 * 256 + 2 * 256 * 256 + (256 * lout[0].shape[0] if lout is not None else 0))
        return bracket("k_head_bf16_fwd (whole xyz head forward)", nb, fl, lambda: real_head(M, xa, l0, l1, l2, lout, h1, h2, h3, out, ldo, col_off))

    def gemm(M, N, K, A, lda, B, ldb, Cm, ldc, **kw):
        es = lambda t: float(t.element_size())
        if kw.get("a_trans"):       # wgrad: both operands streamed over K rows, result (M x N) accumulated
            kind, nb = "wgrad", K * (M * es(A) + N * es(B)) + M * N * 4.0
        else:
            kind = "dgrad" if kw.get("b_trans") else "fwd"
            nb = M * K * es(A) + M * N * es(Cm) + N * K * es(B) + (M * N * es(kw["mask"]) if kw.get("mask") is not None else 0.0)
        kind = f"{kind} {N}x{K}" if not kw.get("a_trans") else f"wgrad {M}x{N}"
        return bracket(kind, nb, 2.0 * M * N * K, lambda: real_gemm(M, N, K, A, lda, B, ldb, Cm, ldc, **kw))
    engine.head_bf16, engine.gemm = head, gemm
    try:
        for i in range(steps):
            tr.training_step(batches[i % len(batches)], lean=lean)
        torch.cuda.synchronize()
    finally:
        engine.head_bf16, engine.gemm = real_head, real_gemm
    fam = {}
    for kind, nb, fl, e0, e1 in rec:
        f = fam.setdefault(kind, [0.0, 0.0, 0, 0.0])
        f[0] += nb; f[1] += e0.elapsed_time(e1); f[2] += 1; f[3] += fl
    if not fam:
        return None
    table = {k: {"GBps": v[0] / (v[1] * 1e-3) / 1e9, "tflops": v[3] / (v[1] * 1e-3) / 1e12, "ms_per_step": v[1] / steps,
                 "launches_per_step": v[2] / steps} for k, v in fam.items() if v[1] > 0}
    dom = max(table, key=lambda k: table[k]["ms_per_step"])
    g, tfl = table[dom]["GBps"], table[dom]["tflops"]
    hbm_frac, mfma_frac = g / PEAK_HBM_GBS, tfl / 2500.0
    # The fused head forward moves 16 B in / 4 E B out per row (+ 512 B per kept activation): it is NOT a stream -- its ceiling is the bf16
    # matrix pipe / LDS (every wave re-reads the 64-row tile from LDS); the per-layer launches (activations through HBM) are streams.
    return {"bound": "hbm" if hbm_frac >= mfma_frac else "mfma", "kernel": dom,
            "achieved": g if hbm_frac >= mfma_frac else tfl, "peak": PEAK_HBM_GBS if hbm_frac >= mfma_frac else 2500.0,
            "unit": "GB/s" if hbm_frac >= mfma_frac else "TFLOP/s (dense bf16 MFMA)", "frac": max(hbm_frac, mfma_frac),
            "hbm_GBps": g, "hbm_frac": hbm_frac, "hbm_frac_of_achievable_stream_6300": g / 6300.0, "mfma_tflops": tfl, "mfma_frac": mfma_frac,
            "families": table,
            "note": "algorithmic bytes per launch (operands + results as stored: bf16 activations, fp32 weights / narrow tensors) / HIP-event time "
                    "(events make the step host-bound, so per-launch times are upper bounds)"}


def inference_probe(cl, model, renderer, pool, n_rays=262144, chunk=32768):
    """Frame-render throughput (BASELINE configs[4] shape: is_train=False, halved step ratio as RP:104, chunked like
    RP:114-120) on a bounded 262144-ray tile -- reported beside the training metric, outside the timed region."""
    from contrastive_lift_amd import inference as inf
    ratio = renderer.step_ratio
    renderer.update_step_ratio(ratio * 0.5)
    try:
        rays = pool[:n_rays].contiguous()
        inf.render_rays(model, renderer, rays[:chunk], chunk)
        torch.cuda.synchronize()
        t = time.perf_counter()
        inf.render_rays(model, renderer, rays, chunk)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        S = int(renderer.n_samples)
        act = 0
        for i in range(0, rays.shape[0], chunk):
            act += int(engine_render_forward(model, renderer, rays[i:i + chunk])[1].M)
    finally:
        renderer.update_step_ratio(ratio)
    fl = head_flops_per_active_sample(model)
    tf = act * fl / dt / 1e12
    from contrastive_lift_amd import engine
    mode = {0: "fp32", 1: "bf16", 2: "fp32x6"}[engine.MLP_PRECISION]
    return dict(inference_roofline=inference_roofline_object(tf, mode, act / rays.shape[0], fl),
                inference_rays_per_s=rays.shape[0] / dt, inference_ray_samples_per_s=rays.shape[0] * S / dt,
                inference_samples_per_ray=S, inference_probe=f"{rays.shape[0]} rays, chunk {chunk}, fp32 outputs rgb/sem/inst/dist")


def measured_traffic_ratio(record=None):
    """HBM bytes of the dominant kernel from counters, as a ratio to its algorithmic bytes: profiles/r03_pmc_k_layer_f32.json holds
    the rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE in separate runs, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for
    16-byte-per-lane streaming reads on gfx950) over this very command and over the torch-free single-kernel harness."""
    try:
        with open(os.path.join(REPO, record or PMC_RECORD)) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def roofline(rec_dom, rec, nb, engine, dtype="fp32x6", ms_step=None, rec_min=None):
    """Roofline object of the dominant kernel family of the timed steps.

    ``rec`` = (kind, M, N, K, ms, extra FLOPs, algorithmic bytes) of EVERY matrix-core launch of the ``nb`` replayed steps (informational
    ``all_gemm`` split; ~60 events per step make that replay host-bound, so its times are upper bounds); ``rec_dom`` = the same for the
    dominant family only -- the 256 x 256 FORWARD layers of the xyz heads, 11 launches per step: k_layer_x6<false, *> in the default
    fp32x6 arithmetic (csrc/layer_x6.hip), k_layer_f32<false, *> in exact fp32 (csrc/layer_f32.hip) -- as the per-launch MEDIAN of three
    replays in which only those launches carry events (the step stays GPU-bound); ``rec_min`` = per-launch minimum over all four replays
    (reported as `frac_best_of_4_brackets`).  achieved = algorithmic FLOPs (2 M N K per launch, M = active samples of the pass; x 6 bf16
    products in fp32x6) / summed launch durations.  The active-sample count drifts while the field trains, which is why the records come
    from replays of exactly the timed steps."""
    tf = lambda f, ms: f / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    tot_f, tot_ms, by = 0.0, 0.0, {}
    for kind, M, N, K, ms, xf, _ in rec:
        fl = 2.0 * M * N * K + xf
        tot_f += fl; tot_ms += ms
        b = by.setdefault(kind, [0.0, 0.0, 0])
        b[0] += fl; b[1] += ms; b[2] += 1

    def family(records):
        """Sums over the dominant family: [main FLOPs (2MNK), extra exact FLOPs, ms, launches, bytes] in total and per instantiation."""
        tot, inst = [0.0, 0.0, 0.0, 0, 0.0], {}
        for kind, M, N, K, ms, xf, nbytes in records:
            for acc in (tot, inst.setdefault(kind, [0.0, 0.0, 0.0, 0, 0.0])):
                acc[0] += 2.0 * M * N * K; acc[1] += xf; acc[2] += ms; acc[3] += 1; acc[4] += nbytes or 0.0
        return tot, inst
    dom, inst = family(rec_dom)
    dom_best, _ = family(rec_min if rec_min is not None else rec_dom)
    if os.environ.get("CLIFT_BENCH_DUMP"):
        for kind, M, N, K, ms, xf, _ in rec_dom:
            print(f"[dom] {kind} M={M} N={N} K={K} {ms:.4f} ms", file=sys.stderr)
    ach = tf(dom[0] + dom[1], dom[2])                      # fp32-equivalent TFLOP/s of the family
    all_gemm = {"fp32_equiv_tflops": tf(tot_f, tot_ms), "launches_per_step": len(rec) // nb, "ms_per_step": tot_ms / nb, "gflop_per_step": tot_f / 1e9 / nb,
                "by_kind": {k: {"tflops": tf(v[0], v[1]), "ms": v[1] / nb, "launches": v[2] // nb} for k, v in by.items()}}
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    if dtype == "bf16":
        # bf16 operands run the same layers at 16x the MFMA rate: the dominant kernel is then bound by streaming its activations
        # (bf16-stored: half the bytes the fp32 brackets counted for the activation rows).
        esz = 2.0 if engine.act_dtype() == torch.bfloat16 else 4.0
        dom_b = sum(esz * M * K + esz * M * N + 4.0 * N * K for kind, M, N, K, _, _, _ in rec_dom)
        g = gbs(dom_b, dom[2])
        return {"bound": "hbm", "kernel": "k_layer_bf16<false,3> (persistent streamed 256x256 forward layers: weights in registers, LDS-DMA ring, v_mfma_f32_32x32x16_bf16; bf16-stored activations)",
                "achieved": g, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": g / PEAK_HBM_GBS, "traffic": None,
                "launches_per_step": dom[3] // nb, "avg_launch_ms": dom[2] / max(1, dom[3]), "mfma_tflops_of_same_kernel": ach, "all_gemm": all_gemm}
    if dtype == "fp32x6":
        # Two ceilings, both reported: the bf16 matrix pipe (6 bf16 products per fp32 product: 6 x 2MNK FLOPs against the 2.5 PFLOP/s dense
        # peak; the K = 3 / output layers' exact VALU FLOPs counted once) and HBM (algorithmic bytes per launch against 8 TB/s).
        x6tf = lambda v: tf(6.0 * v[0] + v[1], v[2])
        bf16_tf, g = x6tf(dom), gbs(dom[4], dom[2])
        pmc = measured_traffic_ratio(PMC_RECORD_X6)
        names = {"fwd": "k_layer_x6<false, false, 0> (input streamed, output written)", "fwd_gen": "k_layer_x6<false, true, 0> (K = 3 input layer generated in-kernel)",
                 "fwd_out": "k_layer_x6<false, false, 1|2> + k_x6_out_sum (E <= 4 output layer applied in-kernel)"}
        out = {"bound": "mfma",
               "kernel": "k_layer_x6<false, *> (csrc/layer_x6.hip: persistent fp32-faithful split kernel -- the 256x256 forward layers of the xyz heads, 11 launches per "
                         "step in three instantiations; pair of workgroups per row range, the weights' three bf16 planes in registers, cooperative activation split "
                         "through LDS-DMA staging, v_mfma_f32_32x32x16_bf16, eight waves = 4 column groups x 2 k-halves meeting through LDS)",
               "achieved": bf16_tf, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s (bf16 MFMA FLOPs = 6 x the fp32-equivalent 2MNK)", "frac": bf16_tf / PEAK_BF16_MFMA_TFLOPS,
               "frac_is": "per launch the median of three event-bracketed replays of the timed steps (rocprofv3 average of the same command: profiles/r05_kernel_stats_fp32x6.txt)",
               "frac_best_of_4_brackets": x6tf(dom_best) / PEAK_BF16_MFMA_TFLOPS,
               "fp32_equivalent_tflops": ach, "fp32_equivalent_vs_exact_fp32_mfma_peak": ach / PEAK_FP32_MFMA_TFLOPS,
               "hbm": {"achieved": g, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": g / PEAK_HBM_GBS,
                       "bytes": "algorithmic: 1 KB per activation row read / written, 16 B per generated row, 256 B per row of output-layer partial sums written "
                                "and read back, 256 KB weights per launch"},
               "traffic": (dom[4] / max(1, dom[3]) * pmc["bench_ratio"]) if pmc else None,
               "traffic_unit": "bytes/launch (average launch of this run)", "traffic_algorithmic": dom[4] / max(1, dom[3]),
               "traffic_over_algorithmic": pmc["bench_ratio"] if pmc else None,
               "traffic_is": ("ESTIMATE = this run's algorithmic bytes x the counter/algorithmic ratio RECORDED in " + PMC_RECORD_X6 + " (rocprofv3 --pmc FETCH_SIZE / "
                              "WRITE_SIZE, separate passes, FETCH_SIZE x2 as MI355X_MICROARCH.md prescribes for gfx950; not re-measured by this run)") if pmc else None,
               "note": "a bare stream of these MFMAs (no memory, no VALU) runs 113 us per 249 k-row launch on this chip = 1.73 PFLOP/s at the ~1.7 GHz it holds "
                       "under that load (profiles/r03_x6_notes.txt): the 2.5 PFLOP/s peak assumes 2.4 GHz",
               "launches_per_step": dom[3] // nb, "avg_launch_ms": dom[2] / max(1, dom[3]),
               "instantiations": {names[k]: {"bf16_mfma_tflops": x6tf(v), "frac": x6tf(v) / PEAK_BF16_MFMA_TFLOPS, "hbm_GBps": gbs(v[4], v[2]),
                                             "launches_per_step": v[3] // nb, "avg_launch_ms": v[2] / max(1, v[3])} for k, v in inst.items()},
               "all_gemm": all_gemm}
        if ms_step:
            out["step_gflop_fp32_equiv"] = tot_f / 1e9 / nb
            out["step_fp32_equiv_tflops"] = (tot_f / nb) / (ms_step * 1e-3) / 1e12
        return out
    # exact fp32
    plain = inst.get("fwd", dom)
    alg_bytes = plain[4] / max(1, plain[3])
    pmc = measured_traffic_ratio(PMC_RECORD)
    names = {"fwd": "k_layer_f32<false, false, false, false>", "fwd_gen": "k_layer_f32<false, true, false, false>", "fwd_out": "k_layer_f32<false, false, true, false>"}
    etf = lambda v: tf(v[0] + v[1], v[2])
    out = {"bound": "mfma", "kernel": "k_layer_f32<false, *, *, false> (persistent fp32 v_mfma_f32_32x32x2_f32 kernel: the 256x256 forward MLP layers of the xyz heads, "
                                      "11 launches per step in three instantiations -- input streamed from memory / K = 3 input layer generated in-kernel / narrow "
                                      "output layer applied in-kernel; rocprofv3 lists them separately: see `instantiations`)",
           "instantiations": {names[k]: {"tflops": etf(v), "frac": etf(v) / PEAK_FP32_MFMA_TFLOPS, "launches_per_step": v[3] // nb,
                                         "avg_launch_ms": v[2] / max(1, v[3])} for k, v in inst.items()},
           "achieved": ach, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP32_MFMA_TFLOPS,
           "frac_is": "per launch the median of three event-bracketed replays of the timed steps", "frac_best_of_4_brackets": etf(dom_best) / PEAK_FP32_MFMA_TFLOPS,
           "traffic": (alg_bytes * pmc["bench_ratio"]) if pmc else None,
           "traffic_is": "ESTIMATE = this run's algorithmic bytes (plain instantiation) x the counter/algorithmic ratio RECORDED in " + PMC_RECORD,
           "traffic_unit": "bytes/launch (average plain launch of this run)", "traffic_algorithmic": alg_bytes,
           "traffic_over_algorithmic": pmc["bench_ratio"] if pmc else None,
           "mfma_busy_frac_counters": pmc.get("mfma_busy_frac") if pmc else None,
           "launches_per_step": dom[3] // nb, "avg_launch_ms": dom[2] / max(1, dom[3]), "gflop_per_launch_avg": (dom[0] + dom[1]) / max(1, dom[3]) / 1e9,
           "all_gemm": dict(all_gemm, achieved=all_gemm["fp32_equiv_tflops"], frac=all_gemm["fp32_equiv_tflops"] / PEAK_FP32_MFMA_TFLOPS)}
    if ms_step:
        # whole-step fraction of the fp32-MFMA roof: every matrix-core FLOP of a step / the step's wall time / peak
        out["step_gflop"] = tot_f / 1e9 / nb
        out["step_frac"] = (tot_f / nb) / (ms_step * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS
    return out


def usable_cores():
    """Host cores this process may actually use: min(affinity mask, cgroup v2 cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(model, renderer, batch, a, S):
    """The oracle (CPU-PyTorch restatement of the reference path, same ATen ops / shapes / chunk 2048) timed on the
    host cores of this box: 1 warm-up + up to 3 full-size steps within the budget."""
    from oracle import render as orender
    from oracle.train_step import CpuTrainer
    cores = usable_cores()
    torch.set_num_threads(cores)
    P = {k: v.detach().cpu() for k, v in model.export_state_dict().items()}
    cfg = orender.RenderCfg(renderer.bbox_aabb.cpu(), tuple(int(x) for x in renderer.grid_dim.tolist()), density_shift=-3.0)
    ct = CpuTrainer(P, cfg, chunk=2048, epoch=4)
    b0, b1 = batch[0], batch[1][0]
    rays, rgbs, probs, conf = (b0[k].cpu() for k in ("rays", "rgbs", "probabilities", "confidences"))
    ir, il, ic = b1["rays"].cpu(), b1["instances"].cpu(), b1["confidences"].cpu()
    g = torch.Generator().manual_seed(1)

    def step():
        jit = torch.rand(rays.shape[0], generator=g)
        ct.main_pass(rays, rgbs, probs, conf, jit, [False] * ((rays.shape[0] + 2047) // 2048))
        ct.instance_pass(ir, il, ic, torch.rand(ir.shape[0], generator=g))
    t0 = time.perf_counter()
    step()
    warm = time.perf_counter() - t0
    ts = []
    while len(ts) < 3 and (time.perf_counter() - t0) + warm < a.cpu_budget_s:
        t = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t)
    if not ts:
        ts = [warm]
    ts.sort()
    med = ts[len(ts) // 2]
    return {"value": (a.rays + a.inst_rays) * S / med, "unit": "ray-samples/s", "cores": cores, "kind": "port",
            "sample": f"{len(ts)} full-size training_step(s) after 1 warm-up ({a.rays}+{a.inst_rays} rays x S={S}, chunk 2048, "
                      f"torch {torch.__version__} CPU, {cores} threads), median {med:.2f} s/step",
            "s_per_step": med,
            "port_vs_reference": "build container, 8 threads, same step: oracle port 6.28 s, imported reference trainer 5.22 s (port / reference time "
                                 "= 1.20; tools/cpu_port_vs_reference.py, profiles/r02_cpu_port_vs_reference.json) -- the reference's own CPU "
                                 "path is ~1.2x FASTER than this port number"}


if __name__ == "__main__":
    main()
