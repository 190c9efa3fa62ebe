#!/usr/bin/env python3
"""Time of the relations stage of the surface export at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), upsample U,
on the labelled inside set of the default level:

    python tools/relations_timing_probe.py [--grid 128] [--upsample 2] [--alpha_level 0.5] [--repeats 7] [--out profiles/relations_timing.txt]

  kernel             clift_lattice_relations alone, into buffers allocated once (the call clears them itself)
  lattice_relations  relations.lattice_relations: the buffers, the call and the one read of ``rejected``
  torch_gap0         the same gap-0 integers composed from torch ops -- bincount of the keys, index sums by index_add_, the index box by
                     scatter_reduce, and per axis two shifted views of the lattice, a joint code and a bincount -- the comparator: there is
                     no earlier device stage, and a look through a gap cannot be composed this way at all
  export stages      inference/extract_mesh.py's surface_stages with --relations, for the share of the stage in a whole export

Twice: on the scene's own labels (class and id of every inside point, a handful of nodes: the table in LDS) and on a lattice of 1000 keys
(connected components of the inside set plus 2 % of the lattice points at random, numbered modulo 1000: the table in memory), each at gap 0
and gap 2.  Device events around every stage, after one untimed warm-up; the median and the spread of the repeats are printed.  Also checks
that kernel and composition give the same integers and that two device runs give the same bits.  Recorded in profiles/relations_timing.txt,
not gated.
"""
import argparse
import importlib.util
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from contrastive_lift_amd import _lib, components, relations, synthetic   # noqa: E402


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


def buffers(n_keys, gap, dev):
    return dict(count=torch.empty(n_keys, dtype=torch.int64, device=dev), isum=torch.empty((n_keys, 3), dtype=torch.int64, device=dev),
                ibox=torch.empty((n_keys, 6), dtype=torch.int32, device=dev), faces=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev),
                near=torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev) if gap > 0 else None,
                rejected=torch.empty(1, dtype=torch.int32, device=dev))


def kernel(key, n_keys, gap, out):
    _lib.call("clift_lattice_relations", _lib.ptr(key), *key.shape, n_keys, gap, _lib.ptr(out["count"]), _lib.ptr(out["isum"]), _lib.ptr(out["ibox"]),
              _lib.ptr(out["faces"]), _lib.ptr(out["near"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


def torch_gap0(key, n_keys):
    """count, isum, ibox and faces of gap 0 from torch ops (keys known to lie inside [0, n_keys))."""
    dev, flat = key.device, key.reshape(-1).long()
    count = torch.bincount(flat, minlength=n_keys)
    isum = torch.zeros((n_keys, 3), dtype=torch.int64, device=dev)
    ibox = torch.empty((n_keys, 6), dtype=torch.int32, device=dev)
    faces = torch.empty((n_keys, n_keys, 3), dtype=torch.int32, device=dev)
    for a in range(3):
        view = [1, 1, 1]
        view[a] = key.shape[a]
        idx = torch.arange(key.shape[a], device=dev).view(view).expand(key.shape).reshape(-1)
        isum[:, a].index_add_(0, flat, idx)
        lo = torch.full((n_keys,), key.shape[a], dtype=torch.int64, device=dev).scatter_reduce(0, flat, idx, "amin")
        hi = torch.full((n_keys,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, flat, idx, "amax")
        ibox[:, a], ibox[:, 3 + a] = lo.int(), hi.int()
        u, v = key.narrow(a, 0, key.shape[a] - 1).long(), key.narrow(a, 1, key.shape[a] - 1).long()
        code = (u * n_keys + v)[u != v]
        faces[:, :, a] = torch.bincount(code, minlength=n_keys * n_keys).view(n_keys, n_keys).int()
    return dict(count=count, isum=isum, ibox=ibox, faces=faces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--upsample", type=int, default=2)
    ap.add_argument("--alpha_level", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("clift_extract_mesh_cli_probe", os.path.join(REPO, "inference", "extract_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    model, renderer, _ = synthetic.make_scene(grid=a.grid, device="cuda")
    level = -math.log(1.0 - a.alpha_level) / (renderer.step_size_host * float(renderer.distance_scale))      # as tools/mesh_timing_probe.py
    things = list(range(1, 22))                                  # as tools/mesh_timing_probe.py: make_scene has 22 classes, 0 is stuff
    sigma = renderer.get_dense_sigma(model, a.upsample)
    lines = [f"grid {a.grid}, upsample {a.upsample}: sigma lattice {tuple(sigma.shape)}, level {level:.5g}, {a.repeats} repeats after one warm-up; "
             f"ms (device events), median min max"]

    sem, ids = cli.lattice_nodes(model, renderer, sigma, level, things, None, False)
    scene_key, nodes = relations.node_keys(sem, ids)
    g = torch.Generator(device="cuda").manual_seed(0)
    noisy = (sigma >= level) | (torch.rand(sigma.shape, device="cuda", generator=g) < 0.02)
    many_key = torch.where(noisy, (components.label_components(noisy)[0] - 1) % 999 + 1, 0).int()
    for title, key, n_keys in ((f"the scene's labels: {len(nodes)} nodes", scene_key, len(nodes) + 1), ("1000 keys", many_key, 1000)):
        largest = int(torch.bincount(key.reshape(-1).long())[1:].max())
        lines.append(f"-- {title}: {int((key > 0).sum())} keyed points of {key.numel()}, the largest key owns {largest}")
        for gap in (0, 2):
            out = buffers(n_keys, gap, key.device)
            _, *t_kernel = timed(lambda: kernel(key, n_keys, gap, out), a.repeats)
            first = {k: None if v is None else v.clone() for k, v in out.items()}
            kernel(key, n_keys, gap, out)
            same_bits = all(v is None or torch.equal(v, out[k]) for k, v in first.items())
            rel, *t_call = timed(lambda: relations.lattice_relations(key, n_keys, gap), a.repeats)
            row = f"gap {gap}: kernel {t_kernel[0]:9.3f} {t_kernel[1]:9.3f} {t_kernel[2]:9.3f}   lattice_relations {t_call[0]:9.3f} {t_call[1]:9.3f} {t_call[2]:9.3f}"
            if gap == 0:
                ref, *t_torch = timed(lambda: torch_gap0(key, n_keys), a.repeats)
                equal = all(torch.equal(ref[k], rel[k]) for k in ref)
                row += f"   torch_gap0 {t_torch[0]:9.3f} {t_torch[1]:9.3f} {t_torch[2]:9.3f}   equal integers: {equal}"
            else:
                row += f"   near contacts: {int(rel['near'].sum())}"
            lines.append(row + f"   a second run is bit-identical: {same_bits}")

    timer = cli.StageTimer()
    dense = renderer.get_dense_sigma(model, a.upsample)
    timer.done("dense_sigma")
    m = cli.surface_stages(model, renderer, dense, level, things, None, False, timer, relations=dict(gap=2, up="+z", min_faces=4))
    times = timer.report()
    total = sum(times.values())
    lines.append("-- export stages with --relations --relations_gap 2 (one run, after the warm-ups above): " + ", ".join(f"{k} {v:.3f}" for k, v in times.items()) +
                 f"; relations is {100.0 * times['relations'] / total:.1f} % of {total:.3f} ms ({len(m['relations']['graph'].nodes)} nodes, "
                 f"{m['verts'].shape[0]} vertices)")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
