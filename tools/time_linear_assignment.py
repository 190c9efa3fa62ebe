#!/usr/bin/env python3
"""Time one ``linear_assignment_loss(..., return_grad=True)`` call -- one image of instance_loss_mode "linear_assignment" -- on both backends:
"host" (torch.unique + one-hot product + scipy on the CPU + table upload + the "any label off its slot" read, three synchronisations) and
"device" (one clift_assign_loss call, seven launches, nothing read back).

    python tools/time_linear_assignment.py [--calls 100] [--warmup 10] [--out profiles/linear_assignment_timing.txt]

Wall clock between two ``torch.cuda.synchronize()`` calls: the host path's cost IS its synchronisations, which device events would not see.
Median of ``--calls`` (at least 50) calls after ``--warmup``, inputs resident on the device; the quartiles are printed beside it.  Four inputs,
all n = 1024 rays: (E = 25, 12 ids) and (E = 500, 80 ids), each with peaked scores (randn + 8 on a per-id slot: short augmenting paths) and
with plain 3 * randn scores (near-uniform costs: long augmenting paths).  Asserts nothing but equal virtual labels where both backends must
agree; the numbers are recorded, not gated."""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from contrastive_lift_amd.loss import create_virtual_gt_with_linear_assignment, linear_assignment_loss      # noqa: E402

INPUTS = [(25, 12, "peaked"), (25, 12, "plain"), (500, 80, "peaked"), (500, 80, "plain")]


def make_input(E, ids, kind, n=1024, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, ids + 1, (n,), generator=g)
    if kind == "peaked":
        slot = torch.randperm(E, generator=g)
        f = torch.randn(n, E, generator=g)
        f[torch.arange(n), slot[y]] += 8
    else:
        f = 3 * torch.randn(n, E, generator=g)
    conf = torch.rand(n, generator=g) * 0.8 + 0.2
    return f.cuda(), y.cuda(), conf.cuda()


def wall_us(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), q[0], q[2]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    lines = [f"linear_assignment_loss(return_grad=True), n = 1024, {torch.cuda.get_device_name(0)}; wall clock between synchronisations, "
             f"median [quartiles] of {args.calls} calls after {args.warmup} warm-up calls, microseconds",
             "| E | ids | scores | host | device | host / device |", "|---|---|---|---|---|---|"]
    for E, ids, kind in INPUTS:
        f, y, conf = make_input(E, ids, kind)
        same = bool(torch.equal(create_virtual_gt_with_linear_assignment(y, f), create_virtual_gt_with_linear_assignment(y, f, backend="device")))
        res = {}
        for backend in ("host", "device"):
            res[backend] = wall_us(lambda: linear_assignment_loss(f, y, conf, return_grad=True, backend=backend), args.calls, args.warmup)
        h, d = res["host"], res["device"]
        lines.append(f"| {E} | {ids} | {kind} | {h[0]:.0f} [{h[1]:.0f}, {h[2]:.0f}] | {d[0]:.0f} [{d[1]:.0f}, {d[2]:.0f}] | {h[0] / d[0]:.2f} |"
                     + ("" if same else "  (virtual labels differ: a near-tie in the cost matrix)"))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
