#!/usr/bin/env python3
"""Time of the amodal instance layers of an edited scene on one frame of the bench's synthetic scene (synthetic.make_scene:
grid G, opaque blob; rows x cols rays of the first camera, rendered in chunks like inference.render_rays), under a program that copies the
blob's middle and then moves the copy:

    python tools/edit_layers_timing_probe.py [--grid 128] [--rows 256] [--cols 384] [--chunk 32768] [--repeats 7] [--slots 24]
                                             [--out profiles/edit_layers_timing.txt]

  layers           inference.render_rays_layers: the plain layer pass of the same frame
  edit render      inference.render_rays_edit under the program (weight_thres 0, as the tool renders)
  edit layers      inference.render_rays_edit_layers: the edit march, alpha-list, origin walk, semantic head and fast instance net over it,
                   slots, retargeting, per-ray composite with K + c columns
  the new kernel   clift_edit_list_active_origin alone, launched again over every chunk's kept context

Device events around each, all in this one call, after one untimed warm-up; the median and the spread of the repeats are printed.  Recorded
in profiles/edit_layers_timing.txt, not gated.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import _lib, engine, synthetic    # noqa: E402
from contrastive_lift_amd import edit as ed                  # noqa: E402
from contrastive_lift_amd import inference as inf            # noqa: E402
from contrastive_lift_amd.layers import SlotTable            # noqa: E402


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


def program():
    """The middle of the scene copied to one side, then the copy moved on and turned."""
    box = ed.EditBox(np.eye(3), np.zeros(3), -np.full(3, 0.25), np.full(3, 0.25))
    copy = ed.copy(box, np.array([0.55, 0.1, 0.0]), ed.rotation_from_euler_deg(0.0, 0.0, 30.0))
    return ed.EditProgram([copy, ed.move(copy.dst, np.array([0.0, -0.2, 0.15]), ed.rotation_from_euler_deg(20.0, 0.0, 0.0))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=384)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slots", type=int, default=24)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats: at least 7")
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.cols)
    P = a.rows * a.cols
    rays = pool[:P].contiguous()
    prog = program()
    C_, E = model.num_semantic_classes, model.render_instance_mlp.output_channels
    rng = np.random.default_rng(0)
    per = max(a.slots // max(C_ - 1, 1), 1)
    cents = {c: (0.5 * rng.standard_normal((per, E))).astype(np.float32) for c in range(1, C_)}
    cents = {c: v for i, (c, v) in enumerate(cents.items()) if i * per < a.slots}
    table = SlotTable.from_centroids(cents, list(cents), C_)
    lines = [f"grid {a.grid}, one frame of {a.rows} x {a.cols} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}, a copy and a move of "
             f"the copy; {a.repeats} repeats after one warm-up; ms (device events)", f"{'stage':<40}{'median':>10}{'min':>10}{'max':>10}"]

    def row(label, t):
        lines.append(f"{label:<40}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}")

    _, *t_lay = timed(lambda: inf.render_rays_layers(model, renderer, rays, a.chunk, table=table), a.repeats)
    row("layers (unedited)", t_lay)
    _, *t_edit = timed(lambda: inf.render_rays_edit(model, renderer, rays, a.chunk, edit=prog), a.repeats)
    row("edit render", t_edit)
    lay, *t_el = timed(lambda: inf.render_rays_edit_layers(model, renderer, rays, a.chunk, table=table, edit=prog), a.repeats)
    row("edit layers", t_el)
    ctxs = [engine.edit_layers_forward(model, renderer, rays[i:i + a.chunk], prog, table)[1] for i in range(0, P, a.chunk)]
    recs = prog.records()

    def origin_again():
        for c in ctxs:
            if c.M > 0:
                _lib.call("clift_edit_list_active_origin", ctypes.byref(c.ms), recs, len(prog), _lib.ptr(c.rays), _lib.ptr(c.act_idx), c.M,
                          _lib.ptr(c.xa), _lib.ptr(c.origin), _lib.ptr(c.state), _lib.stream())
    _, *t_o = timed(origin_again, a.repeats)
    row("  clift_edit_list_active_origin alone", t_o)
    n_listed = sum(c.M for c in ctxs)
    copied = sum(int((c.origin > 0).sum()) for c in ctxs if c.M > 0)
    in_column = sum(int((c.slots >= table.K).sum()) for c in ctxs if c.M > 0)
    again = inf.render_rays_edit_layers(model, renderer, rays, a.chunk, table=table, edit=prog)
    lines.append(f"-- K = {table.K} slots + {len(prog.copies())} copy column(s); the alpha-list holds {n_listed} samples, {copied} of them came through a copy, {in_column} "
                 f"of those have a slot and sit in a copy column; the new kernel is {100.0 * t_o[0] / t_el[0]:.1f} % of the pass, the pass is "
                 f"{t_el[0] / t_lay[0]:.2f} x the plain layer pass and {t_el[0] / t_edit[0]:.2f} x the edit render; a second run is bit-identical: "
                 f"{all(torch.equal(x, y) for x, y in zip(again, lay))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
