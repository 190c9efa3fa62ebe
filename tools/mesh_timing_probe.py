#!/usr/bin/env python3
"""Stage times of the surface export at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), upsample U:

    python tools/mesh_timing_probe.py [--grid 128] [--upsample 2] [--alpha_level 0.5] [--repeats 5]

  dense_sigma      TensoRFRenderer.get_dense_sigma (clift_dense_sigma, one launch)
  sigma_meshgrid   the same lattice the way the code before clift_dense_sigma could get it: a materialised (n, 3) meshgrid, normalised, through
                   clift_density_points (TensorVMSplit.compute_density) -- the comparator
  isosurface       mesh.extract_isosurface (classify, two cumsums, one host read, vertices + normals, faces)
  label_vertices   mesh.label_vertices (three heads on every vertex)

Device events around each stage, after one untimed warm-up of every stage; the median and the spread of the repeats are printed.  Also
checks that both sigma lattices agree and that two extractions give the same bits.  Recorded in profiles/mesh_timing.txt, not gated.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import mesh, synthetic               # noqa: E402


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
    ap.add_argument("--upsample", type=int, default=2)
    ap.add_argument("--alpha_level", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    model, renderer, _ = synthetic.make_scene(grid=a.grid, device="cuda")
    # make_scene's renderer keeps the TRAINING step ratio (extract_mesh.py doubles its renderer's step because load_for_inference halved it)
    level = -math.log(1.0 - a.alpha_level) / (renderer.step_size_host * float(renderer.distance_scale))
    n = [a.grid * a.upsample] * 3

    def meshgrid_way():
        s = torch.stack(torch.meshgrid(*[torch.linspace(0, 1, k) for k in n], indexing="ij"), -1).to("cuda")
        xyz = renderer.bbox_aabb[0] * (1 - s) + renderer.bbox_aabb[1] * s
        return model.compute_density(renderer.normalize_coordinates(xyz).reshape(-1, 3)).view(*n)

    rows = []
    sigma, *t = timed(lambda: renderer.get_dense_sigma(model, a.upsample), a.repeats)
    rows.append(("dense_sigma", t))
    ref, *t = timed(meshgrid_way, a.repeats)
    rows.append(("sigma_meshgrid", t))
    print(f"sigma lattice {tuple(sigma.shape)}: largest difference between the two ways {float((sigma - ref).abs().max()):.3g} (max sigma {float(ref.max()):.4g})")
    del ref
    ticks = renderer.lattice_ticks(sigma.shape)
    (verts, faces, normals), *t = timed(lambda: mesh.extract_isosurface(sigma, level, ticks), a.repeats)
    rows.append(("isosurface", t))
    v2, f2, n2 = mesh.extract_isosurface(sigma, level, ticks)
    print(f"level {level:.5g}: {verts.shape[0]} vertices, {faces.shape[0]} faces; a second extraction is bit-identical: "
          f"{bool(torch.equal(verts, v2) and torch.equal(faces, f2) and torch.equal(normals, n2))}")
    _, *t = timed(lambda: mesh.label_vertices(model, renderer, verts, normals, thing_classes=range(1, 22)), a.repeats)
    rows.append(("label_vertices", t))
    print(f"grid {a.grid}, upsample {a.upsample}, {a.repeats} repeats after one warm-up; device-event ms")
    print(f"{'stage':<16}{'median':>10}{'min':>10}{'max':>10}")
    for name, (med, lo, hi) in rows:
        print(f"{name:<16}{med:>10.3f}{lo:>10.3f}{hi:>10.3f}")


if __name__ == "__main__":
    main()
