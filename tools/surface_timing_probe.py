#!/usr/bin/env python3
"""Time of the surface outputs of the ray route on one frame of the bench's synthetic scene (synthetic.make_scene: grid G,
opaque blob; the first camera's image x image rays, rendered in chunks like inference.render_rays):

    python tools/surface_timing_probe.py [--grid 128] [--image 512] [--chunk 32768] [--repeats 5] [--out profiles/surface_timing.txt]

  render              inference.render_rays: the plain frame render
  render + surface    inference.render_rays_surface: the same passes plus engine.surface_from_ctx per chunk (two more launches)
  surface_forward     engine.surface_forward per chunk: march, active positions and the two launches, no head

Device events around each, after one untimed warm-up; the median and the spread of the repeats are printed.  Also reports how many rays
hit, checks that the first four outputs of the two renders are the same bits, that surface_forward gives the bits of surface_from_ctx, and
that a second run repeats them.  Recorded in profiles/surface_timing.txt, not gated.
"""
import argparse
import os
import sys

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
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.image)
    rays = pool[:a.image * a.image].contiguous()
    P = rays.shape[0]

    def geometry():
        outs = [engine.surface_forward(model, renderer, rays[i:i + a.chunk])[0] for i in range(0, P, a.chunk)]
        return {k: torch.cat([o[k] for o in outs], 0) for k in ("depth_median", "hit", "normals")}

    plain, *t_plain = timed(lambda: inf.render_rays(model, renderer, rays, a.chunk), a.repeats)
    both, *t_both = timed(lambda: inf.render_rays_surface(model, renderer, rays, a.chunk), a.repeats)
    geo, *t_geo = timed(geometry, a.repeats)
    lines = [f"grid {a.grid}, one frame of {a.image} x {a.image} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}; {a.repeats} repeats after "
             f"one warm-up; ms (device events)", f"{'stage':<20}{'median':>10}{'min':>10}{'max':>10}"]
    for name, t in (("render", t_plain), ("render + surface", t_both), ("surface_forward", t_geo)):
        lines.append(f"{name:<20}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}")
    again = inf.render_rays_surface(model, renderer, rays, a.chunk)
    hit = both[5] > 0.5
    lines.append(f"-- the surface pass adds {t_both[0] - t_plain[0]:.3f} ms ({100.0 * (t_both[0] - t_plain[0]) / t_plain[0]:.1f} % of the plain render); "
                 f"{int(hit.sum())} of {P} rays hit; render outputs bit-equal with and without it: "
                 f"{all(torch.equal(x, y) for x, y in zip(plain, both[:4]))}; surface_forward gives the bits of surface_from_ctx: "
                 f"{torch.equal(geo['depth_median'], both[4]) and torch.equal(geo['hit'], hit) and torch.equal(geo['normals'], both[6])}; "
                 f"a second run is bit-identical: {all(torch.equal(x, y) for x, y in zip(again, both))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
