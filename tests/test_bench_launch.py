"""bench.py --gpus N must occupy N ranks by itself (the flag was parsed and ignored, so a driver-run
`python bench.py --gpus 8` produced a 1-rank record).  CPU: the launcher path alone (`--launch-check`: process group over gloo,
one all-reduce, the line's n_gpus).  GPU: the real bench with two ranks sharing the one device of the test box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel_close


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_gpus_flag_self_launches_that_many_ranks():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                       timeout=300, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["requested_gpus"] == 2
    assert line["allreduce_of_ones"] == 2.0          # both ranks took part in the collective
    # the comparison the N > 1 bench line's `data_parallel_self_check` is built on tells equal from unequal ranks
    assert line["self_check_primitive"] == {"identical_tensor_delta": 0.0, "rank_dependent_tensor_delta": 1.0, "soak_reduction": [1.0, 0.0, 0.5]}


def test_gpus_8_launch_check_reports_eight_ranks_over_gloo():
    """The configs[3] / configs[4] launch shape without a node: `--gpus 8 --launch-check` forms an 8-rank group (gloo here) and says so."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--launch-check"], capture_output=True, text=True,
                       timeout=600, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 8 and line["requested_gpus"] == 8 and line["allreduce_of_ones"] == 8.0
    assert line["dist_backend"] == "gloo" and line["rccl_ranks"] == 0


def test_single_rank_needs_no_launcher():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--launch-check"], capture_output=True, text=True, timeout=300,
                       env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _last_json(r.stdout)["n_gpus"] == 1


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_reports_two():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--rays", "1024",
                        "--inst-rays", "256", "--grid", "64", "--no-extras", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900,
                       env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["dist_backend"] in ("gloo", "nccl")
    assert line["value"] > 0 and line["allreduce_overlap"] is not None
    # the N > 1 record is complete: dominant-kernel roofline, the exchange timed by itself, per-rank step times
    assert line["roofline"]["frac"] > 0 and line["allreduce_ms"]["ms"] > 0 and len(line["rank_ms_per_step_min_max"]) == 2
    # ... and self-validating: the ranks end the run with identical parameters, overlapped and synchronous exchange agree
    chk = line["data_parallel_self_check"]
    assert chk["params_identical_across_ranks"] and chk["param_max_abs_delta_across_ranks"] == 0.0, chk
    assert chk["overlap_grad_equal"] and chk["overlap_grad"]["finite"], chk
    assert line["dtype"] == "f32" and "three bf16 terms" in line["config"]["mlp_arithmetic"]
    assert "6x" in line["scaling_note"]


@pytest.mark.gpu
def test_bench_soak_two_ranks_on_one_gpu():
    """`--soak K`: K replays of one training step with the asynchronous exchange forced on; the rendered outputs of every
    replay are bit-identical to the first one's on every rank, the gradients within the noise of the floating-point atomics."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--rays", "1024",
                        "--inst-rays", "256", "--grid", "64", "--no-extras", "--no-cpu-baseline", "--soak", "6"], capture_output=True, text=True,
                       timeout=900, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sk = _last_json(r.stdout)["soak"]
    assert sk["replays"] == 6 and sk["overlap_forced_on"] and sk["replays_with_different_outputs"] == 0, sk
    assert sk["replays_with_gradients_beyond_atomics_noise"] == 0, sk


@pytest.mark.gpu
def test_bench_two_ranks_line_carries_the_cpu_baseline():
    """... and, run without --no-cpu-baseline, rank 0 times the CPU path after the group is torn down (bounded here to one small step)."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--rays", "256",
                        "--inst-rays", "128", "--grid", "32", "--no-extras", "--cpu-budget-s", "5", "--full"], capture_output=True, text=True, timeout=900,
                       env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"


@pytest.mark.gpu
def test_bench_inference_sharded_two_ranks():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--inference-sharded", "--steps", "1", "--warmup", "1",
                        "--grid", "64", "--full"], capture_output=True, text=True, timeout=900, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["config"]["rays_per_frame"] == 1296 * 968
    assert 0 < line["inference_roofline"]["frac"] < 1


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    """A plain run (no --full) times exactly --steps steps and carries none of the --full measurements.  --dump-outputs writes, as float32
    .npy within 64 MB, the timed step replayed from the set-up state with the last timed step's batch: a second run with the same arguments
    writes the same values (the rendered outputs bit for bit; losses, gradients and parameters -- sums through floating-point atomics --
    within rounding), they are what that step computes when it is run here from a freshly set-up scene, and the pixel losses are those
    of the dumped rendering against the batch's targets."""
    import torch
    from contrastive_lift_amd import synthetic
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    steps, rays, inst_rays, grid, classes = 3, 1024, 256, 64, 22
    names = ["grads.npy", "losses.npy", "params.npy", "rgb.npy", "semantics.npy"]
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rays", str(rays),
                            "--inst-rays", str(inst_rays), "--grid", str(grid), "--dump-outputs", str(d)], capture_output=True, text=True,
                           timeout=600, env=_env(), cwd=REPO)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        line = _last_json(r.stdout)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f32" and line["full"] is False
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["main_pass_samples_per_s"] is None
        # the GPU time between the step-boundary events of exactly `steps` timed steps, against the wall time the line reports for them
        assert len(line["step_ms"]) == steps and 0.5 <= sum(line["step_ms"]) / (steps * line["ms_per_step"]) <= 1.1, line["step_ms"]
        assert sorted(os.listdir(d)) == names
        arrs = {f: np.load(d / f) for f in names}
        assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in arrs.values())
        assert sum(x.nbytes for x in arrs.values()) <= 64 * 2 ** 20
        assert arrs["rgb.npy"].shape == (rays, 3) and arrs["semantics.npy"].shape == (rays, classes) and arrs["losses.npy"].shape == (4,)
        outs.append(arrs)
    a, b = outs

    def rounding(x, y, f):
        rel_close(x, y, rtol=1e-5, atol=1e-6 * float(np.abs(y).max()), what=f)
    for f in ("rgb.npy", "semantics.npy"):
        assert np.array_equal(a[f], b[f]), f
    for f in ("losses.npy", "grads.npy", "params.npy"):
        rounding(a[f], b[f], f)
    # the same step here: bench.py's scene, trainer and batch of the last timed step, from the set-up state and generators
    dev = torch.device("cuda", 0)
    model, renderer, pool = synthetic.make_scene(grid=grid, num_classes=classes, max_instances=3, seed=0, device=dev)
    tr = HotPathTrainer(model, renderer, default_config(chunk=0, instance_optimization_epoch=0, late_semantic_optimization=0, mlp_dtype="fp32x6"),
                        current_epoch=4)
    batch = synthetic.make_batches(pool, rays, inst_rays, classes, 25, seed=100 + (steps - 1) % 4, device=dev)
    assert not np.array_equal(model.param_flat.cpu().numpy(), a["params.npy"])        # the dump is the state AFTER the step's Adam update
    tr.training_step(batch, lean=False)
    torch.cuda.synchronize()
    here = {"rgb.npy": tr.last_outputs[0], "semantics.npy": tr.last_outputs[1], "losses.npy": tr.losses, "grads.npy": model.grad_flat,
            "params.npy": model.param_flat}
    here = {f: t.detach().cpu().numpy() for f, t in here.items()}
    for f in ("rgb.npy", "semantics.npy"):
        assert np.array_equal(here[f], a[f]), f
    for f in ("losses.npy", "grads.npy", "params.npy"):
        rounding(here[f], a[f], f)
    # the pixel losses from the dumped rendering: MSE against the targets, confidence-weighted cross entropy against the soft labels
    b0 = {k: v.cpu().double().numpy() for k, v in batch[0].items() if k != "mask"}
    rgb, sem = a["rgb.npy"].astype(np.float64), a["semantics.npy"].astype(np.float64)
    mse = np.mean((rgb - b0["rgbs"]) ** 2)
    z = sem - sem.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    cw = tr.class_weights.cpu().double().numpy()
    ce = np.mean(b0["confidences"] * -(cw * b0["probabilities"] * logp).sum(1))
    rel_close(a["losses.npy"][:2], np.array([mse, ce]), rtol=1e-5, atol=0.0, what="pixel losses")


@pytest.mark.gpu
def test_bench_frame_render_dump(tmp_path):
    """--inference-sharded --dump-outputs on one rank: the last timed frame's outputs within 64 MB (rgb and distance whole, the wider
    arrays as a seeded sample of rows), the same in a second run, and equal to the frame's first chunk rendered here."""
    import torch
    from contrastive_lift_amd import inference as inf, synthetic
    from contrastive_lift_amd.rays import generate_ray_table
    P = 1296 * 968
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--inference-sharded", "--steps", "1", "--warmup", "1",
                            "--grid", "64", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=_env(), cwd=REPO)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert _last_json(r.stdout)["inference_roofline"] is None
        names = sorted(os.listdir(d))
        assert names == ["distance.npy", "instances.npy", "rgb.npy", "semantics.npy"], names
        arrs = {f: np.load(d / f) for f in names}
        assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in arrs.values())
        assert sum(x.nbytes for x in arrs.values()) <= 64 * 2 ** 20
        assert arrs["rgb.npy"].shape == (P, 3) and arrs["distance.npy"].shape == (P,)
        assert arrs["semantics.npy"].shape[1] == 22 and 0 < arrs["semantics.npy"].shape[0] < P
        outs.append(arrs)
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f
    dev = torch.device("cuda", 0)
    model, renderer, _ = synthetic.make_scene(grid=64, num_classes=22, max_instances=3, seed=0, device=dev)
    K = np.array([[1170.0, 0, 647.75], [0, 1170.0, 483.75], [0, 0, 1]], np.float32)
    rays = generate_ray_table(968, 1296, K, synthetic.look_at((0.0, 0.0, -0.9)), device=dev)
    renderer.update_step_ratio(renderer.step_ratio * 0.5)
    n = 65536                                                   # bench.py's chunk: the frame's first chunk
    rgb, _, _, dist = inf.render_rays(model, renderer, rays[:n].contiguous(), n)
    assert np.array_equal(rgb.cpu().numpy(), outs[0]["rgb.npy"][:n]) and np.array_equal(dist.cpu().numpy(), outs[0]["distance.npy"][:n])
