#!/usr/bin/env python3
"""Time of the lattice distance transform at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), on the labelled inside
set of the default level, at upsample 1 and 2:

    python tools/distance_timing_probe.py [--grid 128] [--alpha_level 0.5] [--repeats 7] [--no_scipy] [--out profiles/distance_timing.txt]

  transform          clift_lattice_distance alone (three passes, with key_min), every node a site, into buffers allocated once
  complement         the same with key 0 as the only site: the distance of every inside point to the nearest empty one
  separation         distance.separation of the labelled lattice: one transform per node, and the torch code that reads the minima
  corner             a single site in the corner of an otherwise empty lattice: the longest distances, every column with one word at its end
  two corners        a site in each of two opposite corners: along x every column holds two words, one at each end and far away in the
                     plane, and every point walks past the nearer one to the other -- the worst case of the expanding search
  scipy              scipy.ndimage.distance_transform_edt of the same site masks on the host's CPUs, one run each, for orientation only

Device events around every stage, after one untimed warm-up; the median and the spread of the repeats are printed.  Also checks that two
device runs give the same bits and, at upsample 1, that the device words are those of the host backend.  Recorded in
profiles/distance_timing.txt, not gated.
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

from contrastive_lift_amd import _lib, distance, lattice, relations, synthetic   # noqa: E402


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


def transform_kernel(key, n_keys, site, out, work):
    _lib.call("clift_lattice_distance", _lib.ptr(key), *key.shape, n_keys, _lib.ptr(site), _lib.ptr(out["packed"]), _lib.ptr(work),
              _lib.ptr(out["key_min"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


def scipy_ms(mask):
    from scipy import ndimage
    t = time.perf_counter()
    ndimage.distance_transform_edt(~mask)
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--alpha_level", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no_scipy", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_probe", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    model, renderer, _ = synthetic.make_scene(grid=a.grid, device="cuda")
    level = -math.log(1.0 - a.alpha_level) / (renderer.step_size_host * float(renderer.distance_scale))      # as tools/relations_timing_probe.py
    things = list(range(1, 22))
    dev = "cuda"
    lines = [f"grid {a.grid}, level {level:.5g}, {a.repeats} repeats after one warm-up; ms (device events), median min max"]
    for upsample in (1, 2):
        sigma = renderer.get_dense_sigma(model, upsample)
        sem, ids = cli.lattice_nodes(model, renderer, sigma, level, things, None, False)
        key, nodes = relations.node_keys(sem, ids)
        n_keys = len(nodes) + 1
        corner, corners = torch.zeros_like(key), torch.zeros_like(key)
        corner[0, 0, 0] = corners[0, 0, 0] = corners[-1, -1, -1] = 1
        out = dict(packed=torch.empty(key.shape, dtype=torch.int64, device=dev), key_min=torch.empty(n_keys, dtype=torch.int64, device=dev),
                   rejected=torch.empty(1, dtype=torch.int32, device=dev))
        work = torch.empty(key.numel(), dtype=torch.int64, device=dev)
        lines.append(f"== upsample {upsample}: lattice {tuple(key.shape)}, {key.numel()} points, {len(nodes)} nodes, {int((key > 0).sum())} keyed points")
        for title, k, table in (("transform, every node a site", key, lattice.key_table(None, n_keys)), ("complement, key 0 the site", key, lattice.key_table(0, n_keys)),
                                ("corner, a single site", corner, lattice.key_table(None, n_keys)),
                                ("two opposite corners", corners, lattice.key_table(None, n_keys))):
            site = torch.from_numpy(table.astype(np.uint8)).to(dev)
            _, *t = timed(lambda: transform_kernel(k, n_keys, site, out, work), a.repeats)
            first = {name: v.clone() for name, v in out.items()}
            transform_kernel(k, n_keys, site, out, work)
            row = (f"-- {title}: {t[0]:9.3f} {t[1]:9.3f} {t[2]:9.3f}   largest dist2 {int(distance.split(out['packed'])[0].max())}   "
                   f"a second run is bit-identical: {all(torch.equal(v, out[name]) for name, v in first.items())}")
            if upsample == 1 and k is key:                         # (the corner walks every offset of every axis on the host: left to the tests)
                host = distance.distance_tables(k.cpu(), n_keys, table, key_min=True, backend="host")
                row += f"   equals the host backend: {all(torch.equal(host[name], out[name].cpu()) for name in host)}"
            if not a.no_scipy:
                mask = table[k.cpu().numpy()]
                row += f"   scipy on the host {scipy_ms(mask):9.1f}"
            lines.append(row)
        sep, *t = timed(lambda: distance.separation(key, n_keys), a.repeats)
        again = distance.separation(key, n_keys)
        lines.append(f"-- separation of the {len(nodes)} nodes: {t[0]:9.3f} {t[1]:9.3f} {t[2]:9.3f}   pairs found: {int((sep['gap2'] != distance.NONE).sum()) // 2}   "
                     f"a second run is bit-identical: {all(torch.equal(sep[name], again[name]) for name in sep)}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
