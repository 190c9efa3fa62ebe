#!/usr/bin/env python3
"""Time of the density lattice of an EDITED scene at the bench's synthetic scene (synthetic.make_scene: grid G, opaque blob), upsample U
(128 x 2: the 16.8 M points of a 256^3 export):

    python tools/edit_mesh_timing_probe.py [--grid 128] [--upsample 2] [--repeats 5] [--out profiles/edit_mesh_timing.txt]

  dense_sigma         TensoRFRenderer.get_dense_sigma without an edit (clift_dense_sigma, one launch)
  fused n             get_dense_sigma(edit=program of n edits, return_state=True): clift_edit_list_dense_sigma, one launch
  composed n          the same lattice from the entry points that exist beside it: the lattice points materialised ((N, 3) meshgrid of the
                      ticks), clift_edit_list_points over them, normalised, TensorVMSplit.compute_density (clift_density_points), the
                      killed points zeroed -- the comparator
  walk n              clift_edit_list_points alone over the materialised points (part of ``composed``)

for programs of 1, 3 and 8 edits: moves, copies and deletes of boxes of side ~0.5 around the blob (a move first, so that every program
remaps and kills).  Device events around each, after one untimed warm-up; the median and the spread of the repeats are printed.  Also
checks that fused and composed agree -- state equal, sigma within rel 1e-3 / abs 1e-6 (what the unedited kernel is held to), the points no
edit touches bit-equal to the unedited lattice, in both -- and that two fused runs give the same bits.  Recorded in
profiles/edit_mesh_timing.txt, not gated.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastive_lift_amd import edit, synthetic   # noqa: E402


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


def programs():
    """Eight boxes on a ring around the blob, turned differently; edit i: 0, 3, 6 move, 1, 4, 7 copy, 2, 5 delete.  -> {1, 3, 8: EditProgram}."""
    edits = []
    for i in range(8):
        ang = 0.8 * i
        c = [0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.25 * np.cos(1.7 * i + 0.4)]
        R = edit.rotation_from_euler_deg(6.0 * i, -4.0 * i, 13.0 * i)
        box = edit.EditBox(R, c, [-0.26, -0.24, -0.25], [0.24, 0.26, 0.25])
        t = [0.35 * np.cos(ang + 0.5), 0.35 * np.sin(ang + 0.5), 0.1 * (-1) ** i]
        turn = edit.rotation_from_euler_deg(10.0, 5.0 * i, -20.0)
        edits.append(edit.move(box, t, turn) if i % 3 == 0 else edit.copy(box, t, turn) if i % 3 == 1 else edit.delete(box))
    return {n: edit.EditProgram(edits[:n]) for n in (1, 3, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--upsample", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args()
    model, renderer, _ = synthetic.make_scene(grid=a.grid, device="cuda")
    plain, *t_plain = timed(lambda: renderer.get_dense_sigma(model, a.upsample), a.repeats)
    shape = tuple(plain.shape)
    N = plain.numel()
    ticks = renderer.lattice_ticks(shape)
    lines = [f"grid {a.grid}, upsample {a.upsample}: sigma lattice {shape} = {N} points, {a.repeats} repeats after one warm-up; ms (device events)",
             f"{'stage':<16}{'median':>10}{'min':>10}{'max':>10}", f"{'dense_sigma':<16}{t_plain[0]:>10.3f}{t_plain[1]:>10.3f}{t_plain[2]:>10.3f}"]
    checks = []

    def walk(prog):
        pts = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1).reshape(-1, 3)
        return prog.apply_to_points(pts)

    def composed(prog):
        src, _, state = walk(prog)
        sigma = model.compute_density(renderer.normalize_coordinates(src).contiguous())
        sigma[(state & edit.STATE_KILLED) != 0] = 0.0
        return sigma.view(shape), state.view(shape)

    for n, prog in programs().items():
        (f_sigma, f_state), *tf = timed(lambda: renderer.get_dense_sigma(model, a.upsample, edit=prog, return_state=True), a.repeats)
        (c_sigma, c_state), *tc = timed(lambda: composed(prog), a.repeats)
        _, *tw = timed(lambda: walk(prog), a.repeats)
        for name, t in ((f"fused {n}", tf), (f"composed {n}", tc), (f"walk {n}", tw)):
            lines.append(f"{name:<16}{t[0]:>10.3f}{t[1]:>10.3f}{t[2]:>10.3f}")
        again = renderer.get_dense_sigma(model, a.upsample, edit=prog)
        free = f_state == 0
        err = (f_sigma - c_sigma).abs()
        close = bool((err <= 1e-3 * c_sigma.abs() + 1e-6).all())
        checks.append(f"-- {n} edits: {int(((f_state & edit.STATE_REMAPS) > 0).sum())} points remapped, {int(((f_state & edit.STATE_KILLED) != 0).sum())} killed; "
                      f"state equal: {bool(torch.equal(f_state, c_state))}; sigma within rel 1e-3 + 1e-6: {close} (worst abs {float(err.max()):.3g}); "
                      f"untouched points bit-equal to the unedited lattice: fused {bool(torch.equal(f_sigma[free], plain[free]))}, "
                      f"composed {bool(torch.equal(c_sigma[free], plain[free]))}; a second fused run is bit-identical: {bool(torch.equal(again, f_sigma))}")
        del f_sigma, f_state, c_sigma, c_state, again
    lines += checks
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
