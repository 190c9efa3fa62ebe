#!/usr/bin/env python3
"""Time of the placement map at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), on the labelled inside set of the
default level, at upsample 1 and 2:

    python tools/placement_timing_probe.py [--grid 128] [--alpha_level 0.5] [--repeats 7] [--out profiles/placement_timing.txt]

  node               clift_lattice_placement alone (three launches) for the scene's largest node as the object (placement.object_of), every
                     other key solid, the target its own origin, into buffers allocated once
  box                the same for a dense 24 x 24 x 32 box as the object over every key >= 1: no empty mask row to skip, the worst case
  conv3d             the yardstick, what the same device could do before: torch.nn.functional.conv3d of the solid lattice as fp32 with the
                     shape as the filter, which yields ``overlap`` only; whether its rounded result equals ``overlap`` is reported.  Where
                     the library refuses the filter the row says so.  A filter of more than --yardstick_max_macs multiply-adds in all is
                     not run and the row says so (at 256^3 the box, 2.2e11, did not return within minutes).
  host               the wall time of the numpy host backend for the box at upsample 1, for orientation

Device events around every stage, after one untimed warm-up; the median and the spread of the repeats are printed.  Also checks that two
device runs give the same bits and, at upsample 1 for the box, that the device tables are those of the host backend.  Recorded in
profiles/placement_timing.txt, not gated.
"""
import argparse
import importlib.util
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from contrastive_lift_amd import _lib, lattice, placement, relations, synthetic   # noqa: E402


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


def placement_kernel(key, n_keys, site, shape, target, out, work, d=5, min_support=1):
    _lib.call("clift_lattice_placement", _lib.ptr(key), *key.shape, n_keys, _lib.ptr(site), _lib.ptr(shape), *shape.shape, d, min_support, *target,
              _lib.ptr(out["overlap"]), _lib.ptr(out["support"]), _lib.ptr(out["count"]), _lib.ptr(out["best"]), _lib.ptr(out["rejected"]),
              _lib.ptr(work), _lib.stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--alpha_level", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--yardstick_max_macs", type=float, default=1e11)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_probe", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    model, renderer, _ = synthetic.make_scene(grid=a.grid, device="cuda")
    level = -math.log(1.0 - a.alpha_level) / (renderer.step_size_host * float(renderer.distance_scale))      # as tools/relations_timing_probe.py
    things = list(range(1, 22))
    dev = "cuda"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say(f"grid {a.grid}, level {level:.5g}, {a.repeats} repeats after one warm-up; ms (device events), median min max")
    for upsample in (1, 2):
        sigma = renderer.get_dense_sigma(model, upsample)
        sem, ids = cli.lattice_nodes(model, renderer, sigma, level, things, None, False)
        key, nodes = relations.node_keys(sem, ids)
        n_keys = len(nodes) + 1
        n = tuple(int(x) for x in key.shape)
        sizes = torch.bincount(key.reshape(-1).long(), minlength=n_keys)
        u = 1 + int(sizes[1:].argmax())
        node_shape, origin = placement.object_of(key, u)
        others = lattice.key_table(None, n_keys)
        others[u] = False
        box = torch.ones((24, 24, 32), dtype=torch.uint8, device=dev)
        say(f"== upsample {upsample}: lattice {n}, {key.numel()} points, {len(nodes)} nodes, {int((key > 0).sum())} keyed points")
        for title, shape, table, target in ((f"node {u} ({int(node_shape.sum())} cells in {tuple(node_shape.shape)}), every other key solid", node_shape, others, origin),
                                            ("dense 24 x 24 x 32 box, every key >= 1 solid", box, lattice.key_table(None, n_keys), (0, 0, 0))):
            m = tuple(int(x) for x in shape.shape)
            T = tuple(n[i] - m[i] + 1 for i in range(3))
            site = torch.from_numpy(table.astype(np.uint8)).to(dev)
            out = dict(overlap=torch.empty(T, dtype=torch.int32, device=dev), support=torch.empty(T, dtype=torch.int32, device=dev),
                       count=torch.empty(2, dtype=torch.int32, device=dev), best=torch.empty(2, dtype=torch.int64, device=dev),
                       rejected=torch.empty(1, dtype=torch.int32, device=dev))
            work = torch.empty(placement.work_words(n, m), dtype=torch.int64, device=dev)
            _, *t = timed(lambda: placement_kernel(key, n_keys, site, shape, target, out, work), a.repeats)
            first = {name: v.clone() for name, v in out.items()}
            placement_kernel(key, n_keys, site, shape, target, out, work)
            row = (f"-- {title}: {t[0]:9.3f} {t[1]:9.3f} {t[2]:9.3f}   translations {int(np.prod(T))}, free {int(out['count'][0])}, supported {int(out['count'][1])}   "
                   f"a second run is bit-identical: {all(torch.equal(v, out[name]) for name, v in first.items())}")
            if upsample == 1 and shape is box:
                wall = time.perf_counter()
                host = placement.placement_tables(key.cpu(), shape.cpu(), n_keys, table, "-z", target, backend="host")
                wall = 1e3 * (time.perf_counter() - wall)
                row += f"   equals the host backend: {all(torch.equal(host[name], out[name].cpu()) for name in host)} (numpy host backend {wall:9.1f} ms wall)"
            say(row)
            macs = float(np.prod(T)) * float(np.prod(m))
            if macs > a.yardstick_max_macs:
                say(f"   conv3d yardstick: not run ({macs:.3g} multiply-adds, above --yardstick_max_macs {a.yardstick_max_macs:.3g})")
                continue
            solid = site[key.long()].float()[None, None]
            weight = shape.float()[None, None]
            try:
                ref, *c = timed(lambda: torch.nn.functional.conv3d(solid, weight), min(a.repeats, 3))
                equal = bool(torch.equal(ref[0, 0].round().int(), out["overlap"]))
                say(f"   conv3d yardstick (overlap only, fp32, {min(a.repeats, 3)} repeats): {c[0]:9.3f} {c[1]:9.3f} {c[2]:9.3f}   its rounded result equals overlap: "
                    f"{equal}   the kernel's slowest repeat beats its fastest: {t[2] < c[1]}")
            except RuntimeError as err:
                say(f"   conv3d yardstick: refused by the library ({str(err).splitlines()[0][:160]})")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
