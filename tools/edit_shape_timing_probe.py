#!/usr/bin/env python3
"""Time of shaped edits on one frame of the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob; rows x cols rays
of the first camera, rendered in chunks like inference.render_rays), under the program of tools/edit_layers_timing_probe.py -- the middle
of the scene copied to one side, then the copy moved on and turned:

    python tools/edit_shape_timing_probe.py [--grid 128] [--rows 256] [--cols 384] [--chunk 32768] [--repeats 7]
                                            [--tree DIR --label NAME] [--out profiles/edit_shape_timing.txt]

  box render        inference.render_rays_edit under the plain program (weight_thres 0, as the tool renders): clift_edit_list_*
  shaped render     the same program, every edit following a shape read from the field (EditShape.from_field at G^3, grow 1; the copy's
                    move reuses the copy's shape object), G = 32 and 64: clift_edit_shaped_*
  from_field        EditShape.from_field itself at 32^3 and 64^3: the density and the two heads at the cell centres, the slots, the pack

``--tree DIR`` imports the package from another checkout (with its own built library) and times the box render alone: the parent commit's
tree gives the "before" row of the unshaped A/B, whose kernels have the same listing.  Device events around each call, after one untimed
warm-up; the median and the spread of the repeats are printed.  Recorded in profiles/edit_shape_timing.txt, not gated.
"""
import argparse
import os
import sys

import numpy as np
import torch


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
    ap.add_argument("--tree", type=str, default=None, help="import the package from this checkout and time the box render alone")
    ap.add_argument("--label", type=str, default="this tree")
    ap.add_argument("--sigma_min", type=float, default=15.0,
                    help="from_field: a cell is occupied at this density (15: a ball of radius ~0.3 of the synthetic blob, which the box of half-width 0.25 clips)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats: at least 7")
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from contrastive_lift_amd import synthetic
    from contrastive_lift_amd import edit as ed
    from contrastive_lift_amd import inference as inf

    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.cols)
    P = a.rows * a.cols
    rays = pool[:P].contiguous()
    box = ed.EditBox(np.eye(3), np.zeros(3), -np.full(3, 0.25), np.full(3, 0.25))
    t1, R1 = np.array([0.55, 0.1, 0.0]), ed.rotation_from_euler_deg(0.0, 0.0, 30.0)
    t2, R2 = np.array([0.0, -0.2, 0.15]), ed.rotation_from_euler_deg(20.0, 0.0, 0.0)
    copy = ed.copy(box, t1, R1)
    prog = ed.EditProgram([copy, ed.move(copy.dst, t2, R2)])
    lines = [f"[{a.label}] grid {a.grid}, one frame of {a.rows} x {a.cols} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}, a copy and a "
             f"move of the copy; {a.repeats} repeats after one warm-up; ms (device events)", f"{'stage':<40}{'median':>10}{'min':>10}{'max':>10}"]

    def row(label, t):
        lines.append(f"{label:<40}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}")

    plain, *t_box = timed(lambda: inf.render_rays_edit(model, renderer, rays, a.chunk, edit=prog), a.repeats)
    row("box render (clift_edit_list_*)", t_box)
    if a.tree is None:
        from contrastive_lift_amd.layers import SlotTable
        C_, E = model.num_semantic_classes, int(model.render_instance_mlp.output_channels)
        table = SlotTable.from_scores(range(C_), C_, E)
        for G in (32, 64):
            make = lambda: ed.EditShape.from_field(model, renderer, box, table, dims=(G, G, G), grow=1, sigma_min=a.sigma_min)
            sh, *t_ff = timed(make, a.repeats)
            row(f"from_field {G}^3", t_ff)
            cp = ed.copy(box, t1, R1, shape=sh)
            shaped = ed.EditProgram([cp, ed.move(cp.dst, t2, R2, shape=sh)])
            out, *t_sh = timed(lambda: inf.render_rays_edit(model, renderer, rays, a.chunk, edit=shaped), a.repeats)
            row(f"shaped render {G}^3 (clift_edit_shaped_*)", t_sh)
            again = inf.render_rays_edit(model, renderer, rays, a.chunk, edit=shaped)
            lines.append(f"-- {G}^3: slot {sh.slot}, {sh.n_set} of {sh.n_cells} cells set ({sh.n_occupied} occupied); the shaped render is "
                         f"{t_sh[0] / t_box[0]:.3f} x the box render; depth differs from the box render on "
                         f"{int((out[3] != plain[3]).sum())} of {P} rays; a second run is bit-identical: "
                         f"{all(torch.equal(x, y) for x, y in zip(again, out))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
