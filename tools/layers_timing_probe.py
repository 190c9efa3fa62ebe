#!/usr/bin/env python3
"""Time of the amodal instance layers on one frame of the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob;
rows x cols rays of the first camera, rendered in chunks like inference.render_rays):

    python tools/layers_timing_probe.py [--grid 128] [--rows 256] [--cols 384] [--chunk 32768] [--repeats 7] [--slots 24]
                                        [--only render] [--out profiles/layers_timing.txt]

  render           inference.render_rays: the plain frame render
  layers           inference.render_rays_layers: march, alpha-list, semantic head and fast instance net over it, slots, per-ray composite
  the two kernels  clift_sample_slots and clift_ray_layers alone, launched again over every chunk's kept context

Device events around each, after one untimed warm-up; the median and the spread of the repeats are printed, with the length of the
alpha-list against the render's list.  ``--only render`` times the first row alone (it runs on a checkout without the layers, for the
row of the commit before them).  The table has ``--slots`` made-up centroids spread over the first thing classes.  Recorded in
profiles/layers_timing.txt, not gated.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import engine, synthetic    # noqa: E402
from contrastive_lift_amd import inference as inf      # noqa: E402


def timed(fn, repeats):
    fn()                                                         # warm-up
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return out, ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=384)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slots", type=int, default=24)
    ap.add_argument("--only", choices=("render",), default=None)
    ap.add_argument("--label", type=str, default="render")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.cols)
    P = a.rows * a.cols
    rays = pool[:P].contiguous()
    lines = [f"grid {a.grid}, one frame of {a.rows} x {a.cols} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}; {a.repeats} repeats after "
             f"one warm-up; ms (device events)", f"{'stage':<28}{'median':>10}{'min':>10}{'max':>10}"]
    _, *t_plain = timed(lambda: inf.render_rays(model, renderer, rays, a.chunk), a.repeats)
    lines.append(f"{a.label:<28}{t_plain[0]:>10.3f}{t_plain[1]:>10.3f}{t_plain[2]:>10.3f}")
    if a.only is None:
        from contrastive_lift_amd import _lib
        from contrastive_lift_amd.layers import SlotTable
        C_, E = model.num_semantic_classes, model.render_instance_mlp.output_channels
        rng = np.random.default_rng(0)
        per = max(a.slots // max(C_ - 1, 1), 1)
        cents = {c: (0.5 * rng.standard_normal((per, E))).astype(np.float32) for c in range(1, C_)}
        cents = {c: v for i, (c, v) in enumerate(cents.items()) if i * per < a.slots}
        table = SlotTable.from_centroids(cents, list(cents), C_)
        lay, *t_lay = timed(lambda: inf.render_rays_layers(model, renderer, rays, a.chunk, table=table), a.repeats)
        lines.append(f"{'layers':<28}{t_lay[0]:>10.3f}{t_lay[1]:>10.3f}{t_lay[2]:>10.3f}")
        ctxs = [engine.layers_forward(model, renderer, rays[i:i + a.chunk], table)[1] for i in range(0, P, a.chunk)]
        cls_slots, cent = table.on(rays.device)
        K = table.K

        def slots_again():
            for c in ctxs:
                if c.M > 0:
                    _lib.call("clift_sample_slots", _lib.ptr(c.sem_s), c.C, c.C, _lib.ptr(c.inst_s), c.D, E, None, 3, _lib.ptr(cls_slots), _lib.ptr(cent),
                              K, table.mode, c.M, _lib.ptr(c.slots), _lib.stream())

        def layers_again():
            for c in ctxs:
                out = torch.empty((c.N, K + 1, 4), dtype=torch.float32, device=rays.device)
                _lib.call("clift_ray_layers", ctypes.byref(c.ms), _lib.ptr(c.rays), None, c.N, _lib.ptr(c.alpha), _lib.ptr(c.w), _lib.ptr(c.ray_start),
                          _lib.ptr(c.act_idx) if c.M > 0 else None, c.M, _lib.ptr(c.slots), K, _lib.ptr(out), _lib.stream())
        _, *t_s = timed(slots_again, a.repeats)
        _, *t_l = timed(layers_again, a.repeats)
        lines.append(f"{'  clift_sample_slots alone':<28}{t_s[0]:>10.3f}{t_s[1]:>10.3f}{t_s[2]:>10.3f}")
        lines.append(f"{'  clift_ray_layers alone':<28}{t_l[0]:>10.3f}{t_l[1]:>10.3f}{t_l[2]:>10.3f}")
        n_listed, n_render = sum(c.M for c in ctxs), sum(c.M_render for c in ctxs)
        again = inf.render_rays_layers(model, renderer, rays, a.chunk, table=table)
        assigned = sum(int((c.slots >= 0).sum()) for c in ctxs if c.M > 0)
        lines.append(f"-- K = {K} slots; the alpha-list holds {n_listed} samples, the render's list {n_render}: n_listed / M = {n_listed / max(n_render, 1):.2f}; "
                     f"{assigned} of them got a slot; the two kernels are {100.0 * (t_s[0] + t_l[0]) / t_lay[0]:.1f} % of the layer pass, the pass is "
                     f"{t_lay[0] / t_plain[0]:.2f} x the plain render; a second run is bit-identical: {all(torch.equal(x, y) for x, y in zip(again, lay))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
