#!/usr/bin/env python3
"""Time of the clearance sweep at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), on the labelled inside set of the
default level, at upsample 1 and 2:

    python tools/clearance_timing_probe.py [--grid 128] [--alpha_level 0.5] [--repeats 7] [--out profiles/clearance_timing.txt]

  clearance          clift_lattice_clearance alone (both launches), into buffers allocated once (the call fills them itself)
  relations          clift_lattice_relations alone at gap 2 on the SAME key lattice: the existing kernel, as the yardstick
  floor              both passes read the lattice once per axis: 6 x 4 B x points over the achievable HBM rate (6.29 TB/s, the measured
                     float4 copy rate) -- the share of it that the sweep reaches
  settle             clearance.settle_offset of a box copy of the blob's core set 0.8 above it (the edited density lattice, the point walk
                     of the last edit, the keys, the sweep, two reads of the result) beside ONE frame of inference/edit_scene.py's render
                     of that edit (256 x 384 rays of the bench's first camera): the share --settle adds to a frame

Twice per lattice: on the scene's own labels (a handful of nodes: the tables in LDS) and on a lattice of 1000 keys (connected components of
the inside set plus 2 % of the lattice points at random, numbered modulo 1000: the tables in memory).  Device events around every stage,
after one untimed warm-up; the median and the spread of the repeats are printed.  Also checks that two device runs give the same bits and
that the device tables are those of the host backend on the scene's labels.  Recorded in profiles/clearance_timing.txt, not gated.
"""
import argparse
import importlib.util
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from contrastive_lift_amd import _lib, clearance, components, edit, inference, relations, synthetic   # noqa: E402

HBM_RATE = 6.29e12                                               # B/s, the measured streaming rate of the MI355X


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


def clearance_kernel(key, n_keys, slack, out):
    _lib.call("clift_lattice_clearance", _lib.ptr(key), *key.shape, n_keys, slack, _lib.ptr(out["pair"]), _lib.ptr(out["travel"]),
              _lib.ptr(out["landing"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


def relations_kernel(key, n_keys, gap, out):
    _lib.call("clift_lattice_relations", _lib.ptr(key), *key.shape, n_keys, gap, _lib.ptr(out["count"]), _lib.ptr(out["isum"]), _lib.ptr(out["ibox"]),
              _lib.ptr(out["faces"]), _lib.ptr(out["near"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--alpha_level", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_probe", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    model, renderer, pool = synthetic.make_scene(grid=a.grid, device="cuda")
    level = -math.log(1.0 - a.alpha_level) / (renderer.step_size_host * float(renderer.distance_scale))      # as tools/relations_timing_probe.py
    things = list(range(1, 22))
    dev = "cuda"
    lines = [f"grid {a.grid}, level {level:.5g}, {a.repeats} repeats after one warm-up; ms (device events), median min max"]
    for upsample in (1, 2):
        sigma = renderer.get_dense_sigma(model, upsample)
        sem, ids = cli.lattice_nodes(model, renderer, sigma, level, things, None, False)
        scene_key, nodes = relations.node_keys(sem, ids)
        g = torch.Generator(device="cuda").manual_seed(0)
        noisy = (sigma >= level) | (torch.rand(sigma.shape, device="cuda", generator=g) < 0.02)
        many_key = torch.where(noisy, (components.label_components(noisy)[0] - 1) % 999 + 1, 0).int()
        floor_ms = 6 * 4 * sigma.numel() / HBM_RATE * 1e3
        lines.append(f"== upsample {upsample}: lattice {tuple(sigma.shape)}, {sigma.numel()} points; traffic floor 6 x 4 B x points = {floor_ms:.4f} ms at 6.29 TB/s")
        for title, key, n_keys in ((f"the scene's labels: {len(nodes)} nodes", scene_key, len(nodes) + 1), ("1000 keys", many_key, 1000)):
            out = dict(pair=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), travel=torch.empty((n_keys, 6), dtype=torch.int32, device=dev),
                       landing=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), rejected=torch.empty(1, dtype=torch.int32, device=dev))
            _, *t_clr = timed(lambda: clearance_kernel(key, n_keys, 1, out), a.repeats)
            first = {k: v.clone() for k, v in out.items()}
            clearance_kernel(key, n_keys, 1, out)
            same_bits = all(torch.equal(v, out[k]) for k, v in first.items())
            rel = dict(count=torch.empty(n_keys, dtype=torch.int64, device=dev), isum=torch.empty((n_keys, 3), dtype=torch.int64, device=dev),
                       ibox=torch.empty((n_keys, 6), dtype=torch.int32, device=dev), faces=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev),
                       near=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev), rejected=torch.empty(1, dtype=torch.int32, device=dev))
            _, *t_rel = timed(lambda: relations_kernel(key, n_keys, 2, rel), a.repeats)
            events = int((out["pair"] != clearance.NONE).sum())
            row = (f"-- {title}: {int((key > 0).sum())} keyed points; clearance {t_clr[0]:9.3f} {t_clr[1]:9.3f} {t_clr[2]:9.3f}   relations(gap 2) "
                   f"{t_rel[0]:9.3f} {t_rel[1]:9.3f} {t_rel[2]:9.3f}   floor / clearance = {100.0 * floor_ms / t_clr[0]:.1f} %   pairs with an event: {events}   "
                   f"a second run is bit-identical: {same_bits}")
            if n_keys < 100:
                host = clearance.clearance_tables(key.cpu(), n_keys, 1, backend="host")
                row += f"   equals the host backend: {all(torch.equal(host[k], out[k].cpu()) for k in host)}"
            lines.append(row)
        # the share of --settle in a frame: a box copy of the blob's core, 0.8 above it
        e = edit.copy(edit.EditBox(np.eye(3), [0.0, 0.0, 0.0], [-0.25] * 3, [0.25] * 3), [0.0, 0.0, 0.8])
        found, *t_settle = timed(lambda: clearance.settle_offset(model, renderer, e, "-z", upsample=upsample), a.repeats)
        rays = pool[:256 * 384].contiguous()
        _, *t_frame = timed(lambda: inference.render_rays_edit(model, renderer, rays, 32768, False, edit=e), a.repeats)
        lines.append(f"-- settle_offset (steps {found['steps']}, faces {found['faces']}, {found['n_moved']} points moved) {t_settle[0]:9.3f} {t_settle[1]:9.3f} "
                     f"{t_settle[2]:9.3f}   one 256 x 384 frame of the edit render {t_frame[0]:9.3f} {t_frame[1]:9.3f} {t_frame[2]:9.3f}   "
                     f"settle / frame = {100.0 * t_settle[0] / t_frame[0]:.1f} %")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
