#!/usr/bin/env python3
"""Time of the surface outputs of an EDITED scene on one frame of the bench's synthetic scene (synthetic.make_scene: grid G,
opaque blob; the first camera's image x image rays, rendered in chunks like inference.render_rays_edit), under a program of three edits
-- the blob's box moved with a 30 degree yaw, the moved blob copied, a small box deleted:

    python tools/edit_surface_timing_probe.py [--grid 128] [--image 512] [--chunk 32768] [--repeats 5] [--only_edit]
                                              [--out profiles/edit_surface_timing.txt]

  edit render             inference.render_rays_edit: the edited frame render
  edit render + surface   inference.render_rays_edit_surface: the same passes plus engine.edit_surface_from_ctx per chunk (two more launches,
                          the first of which walks the program a third time per active sample)
  edit_surface_forward    engine.edit_surface_forward per chunk: the edit's density forward, the march and the two launches, no head

Device events around each, after one untimed warm-up; the median and the spread of the repeats are printed.  Also reports how many rays
hit, checks that the first four outputs of the two renders are the same bits, that edit_surface_forward gives the bits of
edit_surface_from_ctx, and that a second run repeats them.  ``--only_edit`` times the first row alone (it then runs on a commit that has
no surface outputs of an edited scene).  Recorded in profiles/edit_surface_timing.txt, not gated.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import edit as ed            # noqa: E402
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


def three_edits():
    """In the unit cube of synthetic.make_scene, whose blob sits at the origin."""
    box = ed.EditBox(np.eye(3), np.zeros(3), -np.full(3, 0.35), np.full(3, 0.35))
    move = ed.move(box, np.array([0.45, 0.2, 0.0]), ed.rotation_from_euler_deg(0.0, 0.0, 30.0))
    copy = ed.copy(move.dst, np.array([-0.9, 0.1, 0.1]), ed.rotation_from_euler_deg(20.0, 0.0, 0.0))
    return ed.EditProgram([move, copy, ed.delete(ed.EditBox(np.eye(3), np.array([0.45, 0.2, 0.3]), -np.full(3, 0.12), np.full(3, 0.12)))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only_edit", action="store_true", help="time inference.render_rays_edit alone")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.image)
    rays = pool[:a.image * a.image].contiguous()
    P = rays.shape[0]
    prog = three_edits()
    lines = [f"grid {a.grid}, one frame of {a.image} x {a.image} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}, a program of "
             f"{len(prog)} edits; {a.repeats} repeats after one warm-up; ms (device events)", f"{'stage':<24}{'median':>10}{'min':>10}{'max':>10}"]
    plain, *t_plain = timed(lambda: inf.render_rays_edit(model, renderer, rays, a.chunk, edit=prog), a.repeats)
    rows = [("edit render", t_plain)]
    if not a.only_edit:
        def geometry():
            outs = [engine.edit_surface_forward(model, renderer, rays[i:i + a.chunk], prog)[0] for i in range(0, P, a.chunk)]
            return {k: torch.cat([o[k] for o in outs], 0) for k in ("depth_median", "hit", "normals")}

        both, *t_both = timed(lambda: inf.render_rays_edit_surface(model, renderer, rays, a.chunk, edit=prog), a.repeats)
        geo, *t_geo = timed(geometry, a.repeats)
        rows += [("edit render + surface", t_both), ("edit_surface_forward", t_geo)]
    for name, t in rows:
        lines.append(f"{name:<24}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}")
    if not a.only_edit:
        again = inf.render_rays_edit_surface(model, renderer, rays, a.chunk, edit=prog)
        hit = both[5] > 0.5
        lines.append(f"-- the surface pass adds {t_both[0] - t_plain[0]:.3f} ms ({100.0 * (t_both[0] - t_plain[0]) / t_both[0]:.1f} % of the edited frame "
                     f"with it, {100.0 * (t_both[0] - t_plain[0]) / t_plain[0]:.1f} % of the one without); {int(hit.sum())} of {P} rays hit; render outputs "
                     f"bit-equal with and without it: {all(torch.equal(x, y) for x, y in zip(plain, both[:4]))}; edit_surface_forward gives the bits "
                     f"of edit_surface_from_ctx: "
                     f"{torch.equal(geo['depth_median'], both[4]) and torch.equal(geo['hit'], hit) and torch.equal(geo['normals'], both[6])}; "
                     f"a second run is bit-identical: {all(torch.equal(x, y) for x, y in zip(again, both))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
