#!/usr/bin/env python3
"""Timing of k_edit_current<EditSolids<..>> (ws_collide_solids) beside three things from the SAME trace: the floor for the
bytes it must move -- both record halves read and written (64 B) and cell id and rank (8 B) per particle -- at the float4
copy rate bench.py's roofline uses (HBM_COPY_GBS); the five kernels of the step that follows, for the share; and
k_edit_current<EditForces<..>> with 16 emitters with and without counts, whose counted / uncounted ratio is the price of per-wave
atomics that the workgroup reduction of the reaction is there to avoid.

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400): k = 1 and k = 16 solids, with and
without the reaction.  The solids stand in the lower half of the container, where the fluid is once it has settled; every
launch of a case shifts them by a fraction of the smoothing radius, so that each launch finds fresh contacts (a launch
leaves the particles it touched at the margin).  Kernel times come from `rocprofv3 --kernel-trace`, median of the
launches of a case.

    python3 tools/solids_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/solids_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
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
BYTES_PER_PARTICLE = 32 + 32 + 8
HBM_COPY_GBS = 6290.0  # bench.py


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    lo = np.asarray(params.ext_min[:3], np.float64)
    hi = np.asarray(params.ext_max[:3], np.float64)
    h = float(params.smoothing_radius)
    rng = np.random.default_rng(1)
    kinds = ("sphere", "box", "capsule")
    size = float(hi[1] - lo[1]) / 12.0
    centres = [lo + rng.random(3) * (hi - lo) * (1.0, 0.5, 1.0) for _ in range(16)]

    def solids(k, shift):
        out = []
        for e in range(k):
            kind = kinds[e % 3]
            dims = {"sphere": size, "box": (size, 0.5 * size, 0.75 * size), "capsule": (0.5 * size, size)}[kind]
            out.append(ws.fluid.solid(kind, centres[e] + np.array([shift, 0.0, 0.0]), dims, restitution=0.3, friction=0.2, margin=0.5 * h,
                                      rot=(0.8, 0.6, 0.0, -0.6, 0.8, 0.0, 0.0, 0.0, 1.0)))
        return out

    many = [ws.fluid.force(("radial", "jet", "vortex")[e % 3], centres[e], 2.0 * size, 0.0, axis=(0.0, 1.0, 0.0)) for e in range(16)]
    dt = float(params.delta_time)
    cases = []
    done = 0
    launch = 0
    for at in (10, 400):
        w.run(at - done)
        done = at + 1
        for counts in (False, True):
            for _ in range(repeats):
                affected = w.apply_forces(many, dt, counts=counts)
            cases.append(dict(step=at, kernel="EditForces", k=16, react=counts, repeats=repeats, n=len(pos),
                              contacts=None if affected is None else [int(a) for a in affected]))
        for k in (1, 16):
            for react in (False, True):
                got = None
                for _ in range(repeats):
                    launch += 1
                    got = w.collide_solids(solids(k, 0.25 * h * launch), reaction=react)
                cases.append(dict(step=at, kernel="EditSolids", k=k, react=react, repeats=repeats, n=len(pos),
                                  contacts=None if got is None else [int(c) for c in got[0]]))
        w.run(1)  # the step the shares are taken of
        w.sync()
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="solids_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(min(int(env.get(var, "16") or 16), 16))
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats)]
    subprocess.check_call(cmd, timeout=1100, env=env)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    edits = ("k_edit_current",)
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if any(k in r["Kernel_Name"] for k in edits + STEP_KERNELS)]
    cases = json.load(open(cases_path))
    result = []
    i = 0
    for at in sorted({c["step"] for c in cases}):
        mine = [c for c in cases if c["step"] == at]
        while not any(k in disp[i][0] for k in edits):  # the steps before this state
            i += 1
        for c in mine:
            times = []
            for _ in range(c["repeats"]):
                name, us = disp[i]
                assert "k_edit_current<%s<%s>" % (c["kernel"], "true" if c["react"] else "false") in name, (c, name)
                times.append(us)
                i += 1
            c["us"] = float(np.median(times))
        step = {}
        while True:  # the step that follows: everything up to and including its force kernel
            name, us = disp[i]
            key = next(k for k in STEP_KERNELS if k in name)
            step[key] = step.get(key, 0.0) + us
            i += 1
            if key == "k_force":
                break
        total = sum(step.values())
        for c in mine:
            floor_us = c["n"] * BYTES_PER_PARTICLE / (HBM_COPY_GBS * 1e9) * 1e6 if c["kernel"] == "EditSolids" else None
            result.append({"step": at, "kernel": c["kernel"], "k": c["k"], "react": c["react"], "us": c["us"], "floor_us": floor_us,
                           "floor_frac": None if floor_us is None else floor_us / c["us"], "share_of_step": c["us"] / total,
                           "step_us": total, "contacts": c["contacts"]})
    print("%-6s %-18s %-4s %-9s %10s %10s %12s %10s %10s" % ("step", "k_edit_current", "k", "sums", "us", "floor us", "floor / us", "step us", "share"))
    for r in result:
        print("%-6d %-18s %-4d %-9s %10.1f %10s %12s %10.1f %9.1f%%" % (
            r["step"], r["kernel"], r["k"], "yes" if r["react"] else "no", r["us"],
            "-" if r["floor_us"] is None else "%.1f" % r["floor_us"], "-" if r["floor_frac"] is None else "%.2f" % r["floor_frac"],
            r["step_us"], 100.0 * r["share_of_step"]))
    for at in sorted({r["step"] for r in result}):
        def us(kernel, k, react):
            return next(r["us"] for r in result if (r["step"], r["kernel"], r["k"], r["react"]) == (at, kernel, k, react))
        print("step %d, k = 16: reaction on / off %.2f (EditSolids), counts on / off %.2f (EditForces)" % (
            at, us("EditSolids", 16, True) / us("EditSolids", 16, False), us("EditForces", 16, True) / us("EditForces", 16, False)))
    json.dump(result, open(os.path.join(out, "solids_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
