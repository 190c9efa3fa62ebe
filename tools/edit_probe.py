#!/usr/bin/env python3
"""Frame-render probe of the scene-editing path: one 262144-ray frame of the bench scene (tools/inference_probe.py's set-up) rendered
plainly (inference.render_rays) and under a ``move`` edit (inference.render_rays_edit) at weight_thres 0 and 1e-4, alternating, with the
active-sample count M of each.  Prints one line per variant: median / min / max seconds per frame over the repeats and M.

    python tools/edit_probe.py [fp32x6|fp32|bf16] [chunk] [repeats] [--n_edits K]

``--n_edits K`` (1 .. 8) renders the edit variants through the edit-program path (clift_edit_list_*): K - 1 deletes of small boxes in the
thin space outside the blob -- they change next to nothing in the frame, and every sample pays their box tests -- followed by the same move.  Without it the
single-edit path runs.

Run under rocprofv3 --kernel-trace --stats (a run of its own) for the per-kernel split."""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from contrastive_lift_amd import edit, engine, inference as inf, synthetic     # noqa: E402

argv, n_edits = sys.argv[1:], 0
if "--n_edits" in argv:
    i = argv.index("--n_edits")
    n_edits = int(argv[i + 1])
    del argv[i:i + 2]
dtype = argv[0] if len(argv) > 0 else engine.DEFAULT_MLP_DTYPE
chunk = int(argv[1]) if len(argv) > 1 else 32768
repeats = int(argv[2]) if len(argv) > 2 else 7
engine.set_mlp_precision(dtype)
model, renderer, pool = synthetic.make_scene(grid=128, num_classes=22, max_instances=3, seed=0, device="cuda")
renderer.update_step_ratio(renderer.step_ratio * 0.5)
rays = pool[:262144].contiguous()
# the blob is opaque from r ~ 0.5 inwards and the first camera looks along +z from z = -0.9: a box over the part of the blob's surface that
# faces the camera, moved into the empty space beside it and turned, so that what is removed and what appears are both seen
box = edit.EditBox(edit.rotation_from_euler_deg(0, 0, 20), [0.1, 0.05, -0.45], [-0.25, -0.25, -0.25], [0.25, 0.25, 0.25])
the_edit = edit.move(box, [-0.5, 0.25, -0.1], edit.rotation_from_euler_deg(10, 0, 35))
if n_edits:
    # small boxes on a ring of radius 0.8 about the blob's centre, inside the aabb and clear of the blob and of the move's two boxes
    ring = [edit.delete(edit.EditBox(edit.rotation_from_euler_deg(15 * i, 0, 10 * i), [0.8 * math.cos(0.7 * i + 1.2), 0.8 * math.sin(0.7 * i + 1.2), 0.3],
                                     [-0.04, -0.04, -0.04], [0.04, 0.04, 0.04])) for i in range(n_edits - 1)]
    the_edit = edit.EditProgram(ring + [the_edit])

def count(fn):
    return sum(int(fn(rays[i:i + chunk])[1].M) for i in range(0, rays.shape[0], chunk))


variants = {
    "plain render_rays (thres 1e-4)": (lambda: inf.render_rays(model, renderer, rays, chunk),
                                       lambda r: engine.render_forward(model, renderer, r, None, False, grad_heads=())),
    "edit move, weight_thres 0": (lambda: inf.render_rays_edit(model, renderer, rays, chunk, edit=the_edit, weight_thres=0.0),
                                  lambda r: engine.edit_forward(model, renderer, r, the_edit, False, weight_thres=0.0)),
    "edit move, weight_thres 1e-4": (lambda: inf.render_rays_edit(model, renderer, rays, chunk, edit=the_edit, weight_thres=1e-4),
                                     lambda r: engine.edit_forward(model, renderer, r, the_edit, False, weight_thres=1e-4)),
}
M = {name: count(fwd) for name, (_, fwd) in variants.items()}       # (also the warm-up of every shape)
for run, _ in variants.values():
    run()
times = {name: [] for name in variants}
for _ in range(repeats):                                            # alternate the variants inside every repeat
    for name, (run, _) in variants.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t)
base = statistics.median(times["plain render_rays (thres 1e-4)"])
path = f"edit program of {n_edits} (list kernels)" if n_edits else "single edit"
print(f"{dtype}, {rays.shape[0]} rays in chunks of {chunk}, S = {renderer.n_samples}, {repeats} repeats, {path}")
for name, ts in times.items():
    med = statistics.median(ts)
    print(f"{name:32s} median {med * 1e3:8.2f} ms  (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})  x{med / base:.2f} of plain   M = {M[name]:,}")
d_edit = inf.render_rays_edit(model, renderer, rays, chunk, edit=the_edit)[3]
d_plain = inf.render_rays(model, renderer, rays, chunk)[3]
print(f"the edit shows: max depth change {float((d_edit - d_plain).abs().max()):.3f}, {int(((d_edit - d_plain).abs() > 0.01).sum()):,} of {rays.shape[0]:,} rays change by more than 0.01")
