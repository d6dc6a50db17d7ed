#!/usr/bin/env python3
"""Timing of the attribute calls beside two things from the SAME trace: the two stage kernels of
ws_read_cohesion on the same state -- the model of the diffusion stage: the same two sweeps, with a gradient in pass A and
one more 16-byte gather per candidate in pass B -- and the kernels of the ws_step that follows.

C3 (4 M particles, lattice) in the sparse state (step 15) and settled (step 450).  Per state, each after one unmeasured
warm-up call: R x ws_diffuse_attributes with iterations = 1 and R x with iterations = 8 (k_attr_density once per call,
k_attr_diffuse once per iteration, around them the binning, the gather into cell order and the scatter back), R x
ws_read_cohesion (k_cohesion_normals, k_cohesion_stage), R x ws_paint_attributes with 16 brushes and their counts
(k_attr_paint), R x ws_sample_attribute_grid on 96 x 64 x 64 nodes of spacing h / 2 around the fluid's median (the brick
form) and R x ws_sample_attribute_points at the same nodes (the points form: the same work per node, the other kernel),
then one step.  Kernel times come from `rocprofv3 --kernel-trace`, with no counters collected in that run; a case reports
the median of its launches and their range (min .. max), and for a whole call the sum of every kernel it launched.

    python3 tools/attributes_timing.py [--out DIR] [--repeats R] [--states 15,450]   # runs itself under rocprofv3
    python3 tools/attributes_timing.py child OUT.json R STATES                        # the measured program
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_KERNELS = ("k_scan", "k_place", "k_reorder", "k_density", "k_force")
FIRST = "k_gather_positions"  # what every measured call launches first
# (call, the kernel that ends it, the kernels reported on their own)
PHASES = (("diffuse x1", "k_attr_scatter", ("k_attr_density", "k_attr_diffuse")),
          ("diffuse x8", "k_attr_scatter", ("k_attr_density", "k_attr_diffuse")),
          ("read_cohesion", "k_cohesion_unpack", ("k_cohesion_normals", "k_cohesion_stage")),
          ("paint x16", "k_attr_paint", ("k_attr_paint",)),
          ("field grid", "k_field_bricks", ("k_field_bricks",)),
          ("field points", "k_field_points", ("k_field_points",)))
GRID = (96, 64, 64)


def child(out_path, repeats, states):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    n = len(pos)
    dt = float(params.delta_time)
    h = np.float32(params.smoothing_radius)
    w.write_attributes(np.random.default_rng(1).random((n, 4)).astype(np.float32))
    one = ws.fluid.diffuse_params(rate=(20.0, 10.0, 5.0, 1.0), iterations=1)
    eight = ws.fluid.diffuse_params(rate=(20.0, 10.0, 5.0, 1.0), iterations=8)
    cohesion = ws.fluid.cohesion_params()
    cases = []
    done = 0
    for at in states:
        w.run(at - done)
        done = at + 1
        cur = w.read_positions()
        centre = np.median(cur[::64].astype(np.float64), 0)
        rng = np.random.default_rng(at)
        brushes = [ws.fluid.brush(("mix", "add")[e % 2], cur[rng.integers(n)], 4.0 * float(h), rng.random(4), strength=0.5,
                                  falloff=(0.0, 0.5, 1.0)[e % 3], channels=1 + e % 15) for e in range(16)]
        spacing = np.full(3, h / np.float32(2), np.float32)
        origin = (centre - spacing.astype(np.float64) * np.asarray(GRID) / 2).astype(np.float32)
        ax = [(origin[a] + (np.arange(GRID[a]).astype(np.float32) * spacing[a])).astype(np.float32) for a in range(3)]
        zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        nodes = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float32)
        affected = painted = wet = 0
        for _ in range(repeats + 1):  # (the first of each is the warm-up)
            affected = w.diffuse_attributes(one, dt)
        for _ in range(repeats + 1):
            w.diffuse_attributes(eight, dt)
        for _ in range(repeats + 1):
            w.read_cohesion(cohesion, dt)
        for _ in range(repeats + 1):
            painted = int(w.paint_attributes(brushes).sum())
        for _ in range(repeats + 1):
            gval, grho = w.sample_attribute_grid(origin, spacing, GRID, density=True)
        for _ in range(repeats + 1):
            pval, prho = w.sample_attribute_points(nodes, density=True)
        same = bool(np.array_equal(gval.reshape(-1, 4).view(np.uint32), pval.view(np.uint32)))
        wet = int(np.count_nonzero(grho))
        cases.append(dict(step=at, repeats=repeats, n=n, affected=affected, painted=painted, wet_nodes=wet, nodes=len(nodes),
                          grid_equals_points=same))
        w.run(1)  # the step the shares are taken of
        w.sync()
    w.close()
    json.dump(cases, open(out_path, "w"))


def summary(times):
    return {"us": float(np.median(times)), "min_us": float(min(times)), "max_us": float(max(times)), "launches": len(times)}


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="attributes_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    states = sys.argv[sys.argv.index("--states") + 1] if "--states" in sys.argv else "15,450"
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(min(int(env.get(var, "16") or 16), 16))
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats), states]
    subprocess.check_call(cmd, timeout=1100, env=env)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows]
    cases = json.load(open(cases_path))
    pos = [0]

    def call(end):
        """The kernels of the next measured call: from its k_gather_positions to the kernel that ends it."""
        while FIRST not in disp[pos[0]][0]:
            pos[0] += 1
        first = pos[0]
        while end not in disp[pos[0]][0]:
            pos[0] += 1
            if FIRST in disp[pos[0]][0]:  # (a read of the positions came before the call)
                first = pos[0]
        pos[0] += 1
        return disp[first:pos[0]]

    result = []
    for c in cases:
        times = {}
        for what, end, kernels in PHASES:
            for rep in range(c["repeats"] + 1):
                mine = call(end)
                if not rep:  # (rep 0 is the warm-up)
                    continue
                times.setdefault((what, "whole call"), []).append(sum(us for _, us in mine))
                for name in kernels:
                    hits = [us for k, us in mine if name in k]
                    assert hits, (what, name)
                    times.setdefault((what, name), []).append(sum(hits))
        step = {}
        while True:  # the step that follows: everything up to and including its force kernel
            name, us = disp[pos[0]]
            pos[0] += 1
            key = next((k for k in STEP_KERNELS if k in name), None)
            if key is None:
                continue
            step[key] = step.get(key, 0.0) + us
            if key == "k_force":
                break
        total = sum(step.values())
        for (what, name), t in times.items():
            result.append(dict(step=c["step"], call=what, kernel=name, share_of_step=float(np.median(t)) / total, step_us=total,
                               step_kernels_us=step, case=c, **summary(t)))
    print("%-6s %-14s %-20s %10s %22s %10s" % ("step", "call", "kernel", "median us", "min .. max us", "of step"))
    for r in result:
        print("%-6d %-14s %-20s %10.1f %10.1f .. %-9.1f %9.1f%%" % (r["step"], r["call"], r["kernel"], r["us"], r["min_us"],
                                                                  r["max_us"], 100.0 * r["share_of_step"]))
    for at in sorted({r["step"] for r in result}):
        mine = {(r["call"], r["kernel"]): r["us"] for r in result if r["step"] == at}
        step = next(r for r in result if r["step"] == at)
        print("step %d: pass A / k_cohesion_normals %.2f, pass B / k_cohesion_stage %.2f, the eight-iteration call / eight "
              "one-iteration calls %.2f, field grid (bricks) / points form %.2f; grid == points: %s; the step that follows %.1f us (%s)" % (
                  at, mine[("diffuse x1", "k_attr_density")] / mine[("read_cohesion", "k_cohesion_normals")],
                  mine[("diffuse x1", "k_attr_diffuse")] / mine[("read_cohesion", "k_cohesion_stage")],
                  mine[("diffuse x8", "whole call")] / (8.0 * mine[("diffuse x1", "whole call")]),
                  mine[("field grid", "k_field_bricks")] / mine[("field points", "k_field_points")],
                  step["case"]["grid_equals_points"], step["step_us"],
                  ", ".join("%s %.1f" % (k, step["step_kernels_us"].get(k, 0.0)) for k in STEP_KERNELS)))
    json.dump(result, open(os.path.join(out, "attributes_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]), [int(s) for s in sys.argv[4].split(",")])
    else:
        main()
