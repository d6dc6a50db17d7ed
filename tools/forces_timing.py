#!/usr/bin/env python3
"""Timing of k_edit_current<EditForces<..>> (ws_apply_forces) beside three things from the SAME trace: the five kernels
of the step that follows it, the kernel as a share of that step, and the floor for the bytes it must move -- the record
read (32 B), the velocity record written (16 B) and cell id, rank and count (about 12 B) per particle -- at the float4
copy rate bench.py's roofline uses (HBM_COPY_GBS).

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400): k = 1 and k = 16 emitters, with and
without counts.  The emitters have strength 0 and no brake: the kernel does all its work (nothing in it looks at the
strength) and the state the following step starts from is the one the run had reached.  Kernel times come from
`rocprofv3 --kernel-trace`, median of the launches of a case.

    python3 tools/forces_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/forces_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
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
BYTES_PER_PARTICLE = 32 + 16 + 12
HBM_COPY_GBS = 6290.0  # bench.py


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    lo = np.asarray(params.ext_min[:3], np.float64)
    hi = np.asarray(params.ext_max[:3], np.float64)
    rng = np.random.default_rng(1)
    kinds = ("radial", "jet", "vortex")
    # reach: a sixth of the container's height, centres in the lower half (where the fluid is once it has settled)
    many = [ws.fluid.force(kinds[e % 3], lo + rng.random(3) * (hi - lo) * (1.0, 0.5, 1.0), float(hi[1] - lo[1]) / 6.0, 0.0,
                           axis=(0.0, 1.0, 0.0)) for e in range(16)]
    dt = float(params.delta_time)
    cases = []
    done = 0
    for at in (10, 400):
        w.run(at - done)
        done = at + 1
        for k in (1, 16):
            for counts in (False, True):
                affected = None
                for _ in range(repeats):
                    affected = w.apply_forces(many[:k], dt, counts=counts)
                cases.append(dict(step=at, k=k, counts=counts, repeats=repeats, n=len(pos),
                                  affected=None if affected is None else [int(a) for a in affected]))
        w.run(1)  # the step the shares are taken of
        w.sync()
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="forces_timing_")
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
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if "k_edit_current" in r["Kernel_Name"] or any(k in r["Kernel_Name"] for k in STEP_KERNELS)]
    cases = json.load(open(cases_path))
    result = []
    i = 0
    for at in sorted({c["step"] for c in cases}):
        mine = [c for c in cases if c["step"] == at]
        while "k_edit_current" not in disp[i][0]:  # the steps before this state
            i += 1
        for c in mine:
            times = []
            for _ in range(c["repeats"]):
                name, us = disp[i]
                assert "k_edit_current<EditForces<%s>" % ("true" if c["counts"] else "false") in name, (c, name)
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
            floor_us = c["n"] * BYTES_PER_PARTICLE / (HBM_COPY_GBS * 1e9) * 1e6
            result.append({"step": at, "k": c["k"], "counts": c["counts"], "us": c["us"], "floor_us": floor_us,
                           "floor_frac": floor_us / c["us"], "share_of_step": c["us"] / total, "step_us": total,
                           "step_kernels_us": step, "affected": c["affected"]})
    print("%-6s %-4s %-7s %10s %10s %12s %10s %10s" % ("step", "k", "counts", "us", "floor us", "floor / us", "step us", "share"))
    for r in result:
        print("%-6d %-4d %-7s %10.1f %10.1f %12.2f %10.1f %9.1f%%" % (r["step"], r["k"], "yes" if r["counts"] else "no", r["us"],
                                                                     r["floor_us"], r["floor_frac"], r["step_us"],
                                                                     100.0 * r["share_of_step"]))
    for at in sorted({r["step"] for r in result}):
        step = next(r for r in result if r["step"] == at)["step_kernels_us"]
        print("step %d: " % at + ", ".join("%s %.1f us" % (k, step.get(k, 0.0)) for k in STEP_KERNELS))
    json.dump(result, open(os.path.join(out, "forces_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
