#!/usr/bin/env python3
"""Time of the amodal colour layers on the frame of 6i's table (tools/layers_timing_probe.py): one frame of the bench's
synthetic scene (synthetic.make_scene: grid G, opaque blob; rows x cols rays of the first camera, in chunks like inference.render_rays),
a table of ``--slots`` made-up centroids spread over the first thing classes.

    python tools/layers_colour_timing_probe.py [--grid 128] [--rows 256] [--cols 384] [--chunk 32768] [--repeats 7] [--slots 24]
                                               [--only plain] [--label layers] [--root DIR] [--out profiles/layers_colour_timing.txt]

  layers                    inference.render_rays_layers without colour: what the pass was before the option existed
  layers + colour           ... with colour=True: the appearance chain over the listed rows that have a slot, then clift_ray_layer_colour
  layers + colour + rest    ... with colour_rest=True: every listed row
  the two kernels           clift_ray_layers and clift_ray_layer_colour alone, launched again over every chunk's kept context

Device events around each, after one untimed warm-up; the median and the spread of the repeats are printed, with Mc / M, the share of the
listed rows that is coloured.  ``--only plain`` times the first row alone and uses nothing the option added: with ``--root DIR`` (a
checkout whose package is imported in place of this one's) it gives the row of the commit before, in a process of its own -- the two are
alternated by whoever calls.  Recorded in profiles/layers_colour_timing.txt, not gated.
"""
import argparse
import ctypes
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


def row(label, t):
    return f"{label:<34}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=384)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slots", type=int, default=24)
    ap.add_argument("--only", choices=("plain",), default=None)
    ap.add_argument("--label", type=str, default="layers")
    ap.add_argument("--root", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose contrastive_lift_amd is imported (default: this one)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from contrastive_lift_amd import _lib, engine, synthetic
    from contrastive_lift_amd import inference as inf
    from contrastive_lift_amd.layers import SlotTable
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda", image=a.cols)
    P = a.rows * a.cols
    rays = pool[:P].contiguous()
    C_, E = model.num_semantic_classes, model.render_instance_mlp.output_channels
    rng = np.random.default_rng(0)
    per = max(a.slots // max(C_ - 1, 1), 1)
    cents = {c: (0.5 * rng.standard_normal((per, E))).astype(np.float32) for c in range(1, C_)}
    cents = {c: v for i, (c, v) in enumerate(cents.items()) if i * per < a.slots}
    table = SlotTable.from_centroids(cents, list(cents), C_)
    K = table.K
    lines = [f"grid {a.grid}, one frame of {a.rows} x {a.cols} = {P} rays in chunks of {a.chunk}, S = {renderer.n_samples}, K = {K} slots; "
             f"{a.repeats} repeats after one warm-up; ms (device events)", f"{'stage':<34}{'median':>10}{'min':>10}{'max':>10}"]
    lay, *t_plain = timed(lambda: inf.render_rays_layers(model, renderer, rays, a.chunk, table=table), a.repeats)
    lines.append(row(a.label, t_plain))
    if a.only is None:
        col, *t_col = timed(lambda: inf.render_rays_layers(model, renderer, rays, a.chunk, table=table, colour=True), a.repeats)
        lines.append(row("layers + colour", t_col))
        _, *t_rest = timed(lambda: inf.render_rays_layers(model, renderer, rays, a.chunk, table=table, colour=True, colour_rest=True), a.repeats)
        lines.append(row("layers + colour + rest", t_rest))
        ctxs = [engine.layers_forward(model, renderer, rays[i:i + a.chunk], table, colour=True)[1] for i in range(0, P, a.chunk)]
        dev = rays.device

        def layers_again():
            for c in ctxs:
                out = torch.empty((c.N, K + 1, 4), dtype=torch.float32, device=dev)
                _lib.call("clift_ray_layers", ctypes.byref(c.ms), _lib.ptr(c.rays), None, c.N, _lib.ptr(c.alpha), _lib.ptr(c.w), _lib.ptr(c.ray_start),
                          _lib.ptr(c.act_idx) if c.M > 0 else None, c.M, _lib.ptr(c.slots), K, _lib.ptr(out), _lib.stream())

        def colour_again():
            for c in ctxs:
                out = torch.empty((c.N, K + 1, 4), dtype=torch.float32, device=dev)
                n_rgb = 0 if c.layer_rgb is None else c.layer_rgb.shape[0]
                _lib.call("clift_ray_layer_colour", ctypes.byref(c.ms), c.N, _lib.ptr(c.alpha), _lib.ptr(c.ray_start),
                          _lib.ptr(c.act_idx) if c.M > 0 else None, c.M, _lib.ptr(c.slots), K, _lib.ptr(c.layer_rgb), 3, n_rgb,
                          _lib.ptr(c.layer_rgb_row), _lib.ptr(out), _lib.stream())
        _, *t_l = timed(layers_again, a.repeats)
        _, *t_c = timed(colour_again, a.repeats)
        lines.append(row("  clift_ray_layers alone", t_l))
        lines.append(row("  clift_ray_layer_colour alone", t_c))
        M = sum(c.M for c in ctxs)
        Mc = sum(0 if c.layer_rgb is None else int(c.layer_rgb.shape[0]) for c in ctxs)
        again = inf.render_rays_layers(model, renderer, rays, a.chunk, table=table, colour=True)
        same_plain = all(torch.equal(x, y) for x, y in zip(col[:3], lay))
        lines.append(f"-- the alpha-list holds M = {M} samples, Mc = {Mc} of them are coloured: Mc / M = {Mc / max(M, 1):.2f}; colour adds "
                     f"{t_col[0] - t_plain[0]:.3f} ms to the pass ({t_col[0] / t_plain[0]:.2f} x), of which clift_ray_layer_colour is {t_c[0]:.3f} ms: the rest "
                     f"is the appearance chain over the Mc rows and the row selection, {1e6 * (t_col[0] - t_plain[0] - t_c[0]) / max(Mc, 1):.2f} ns per row; "
                     f"layers, opacity, depth with colour have the bits of the pass without: {same_plain}; a second run is bit-identical: "
                     f"{all(torch.equal(x, y) for x, y in zip(again, col))}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
