#!/usr/bin/env python3
"""Timing of ws_read_cohesion / ws_apply_cohesion beside two things from the SAME trace: the two stage
kernels of ws_read_whitewater on the same state -- the closest existing work: the same two sweeps, with one 16-byte gather
fewer per candidate in pass B -- and the five kernels of the ws_step that follows.

C3 (4 M particles, lattice) in the sparse state (step 15) and settled (step 450).  Per state, each after one unmeasured
warm-up call: R x ws_read_cohesion (k_cohesion_normals, k_cohesion_stage), R x ws_read_whitewater (k_whitewater_normals,
k_whitewater_stage), R x ws_apply_cohesion with the count (the two stage kernels again, then the edit pass
k_edit_current<EditCohesion<true>>), then one step.  The apply runs with all strengths 0: nothing in the kernels looks at a
strength, and the step that follows starts from the state the run had reached.  Kernel times come from
`rocprofv3 --kernel-trace`; a case reports the median of its launches and their range (min .. max).

    python3 tools/cohesion_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/cohesion_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
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
COHESION = ("k_cohesion_normals", "k_cohesion_stage")
WHITEWATER = ("k_whitewater_normals", "k_whitewater_stage")
EDIT = "k_edit_current<EditCohesion<true>"
STATES = (15, 450)


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    dt = float(params.delta_time)
    timed = ws.fluid.cohesion_params()
    still = ws.fluid.cohesion_params(cohesion=0.0, curvature=0.0, xsph=0.0)
    cases = []
    done = 0
    for at in STATES:
        w.run(at - done)
        done = at + 1
        affected = 0
        for _ in range(repeats + 1):  # (the first of each is the warm-up)
            w.read_cohesion(timed, dt)
        for _ in range(repeats + 1):
            w.read_whitewater()
        for _ in range(repeats + 1):
            affected = w.apply_cohesion(still, dt)
        cases.append(dict(step=at, repeats=repeats, n=len(pos), affected=affected))
        w.run(1)  # the step the shares are taken of
        w.sync()
    w.close()
    json.dump(cases, open(out_path, "w"))


def summary(times):
    return {"us": float(np.median(times)), "min_us": float(min(times)), "max_us": float(max(times)), "launches": len(times)}


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="cohesion_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
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
    wanted = COHESION + WHITEWATER + ("k_edit_current",) + STEP_KERNELS
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if any(k in r["Kernel_Name"] for k in wanted)]
    cases = json.load(open(cases_path))
    pos = [0]

    def take(name):
        """The next dispatch of `name`; only the binning's k_scan may come before it."""
        while name not in disp[pos[0]][0]:
            assert "k_scan" in disp[pos[0]][0], (name, disp[pos[0]][0])
            pos[0] += 1
        pos[0] += 1
        return disp[pos[0] - 1][1]

    result = []
    for c in cases:
        while COHESION[0] not in disp[pos[0]][0]:  # the steps before this state
            pos[0] += 1
        times = {}
        for what, kernels in (("read_cohesion", COHESION), ("read_whitewater", WHITEWATER), ("apply_cohesion", COHESION + (EDIT,))):
            for rep in range(c["repeats"] + 1):
                for name in kernels:
                    us = take(name)
                    if rep:  # (rep 0 is the warm-up)
                        times.setdefault((what, name), []).append(us)
        step = {}
        while True:  # the step that follows: everything up to and including its force kernel
            name, us = disp[pos[0]]
            key = next(k for k in STEP_KERNELS if k in name)
            step[key] = step.get(key, 0.0) + us
            pos[0] += 1
            if key == "k_force":
                break
        total = sum(step.values())
        for (what, name), t in times.items():
            result.append(dict(step=c["step"], call=what, kernel=name, share_of_step=float(np.median(t)) / total, step_us=total,
                               step_kernels_us=step, affected=c["affected"], **summary(t)))
    print("%-6s %-16s %-36s %10s %22s %10s" % ("step", "call", "kernel", "median us", "min .. max us", "of step"))
    for r in result:
        print("%-6d %-16s %-36s %10.1f %10.1f .. %-9.1f %9.1f%%" % (r["step"], r["call"], r["kernel"], r["us"], r["min_us"],
                                                                  r["max_us"], 100.0 * r["share_of_step"]))
    for at in sorted({r["step"] for r in result}):
        mine = {(r["call"], r["kernel"]): r["us"] for r in result if r["step"] == at}
        step = next(r for r in result if r["step"] == at)
        print("step %d: pass A / whitewater pass A %.2f, pass B / whitewater pass B %.2f; the step that follows %.1f us (%s)" % (
            at, mine[("read_cohesion", COHESION[0])] / mine[("read_whitewater", WHITEWATER[0])],
            mine[("read_cohesion", COHESION[1])] / mine[("read_whitewater", WHITEWATER[1])], step["step_us"],
            ", ".join("%s %.1f" % (k, step["step_kernels_us"].get(k, 0.0)) for k in STEP_KERNELS)))
    json.dump(result, open(os.path.join(out, "cohesion_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
