#!/usr/bin/env python3
"""Timing of the whitewater kernels (ws_read_whitewater / ws_emit_whitewater / ws_step_whitewater) beside
two yardsticks measured in the same process: the density sampler's points kernel at the particles' own positions with
the gradient (one sweep per particle, what pass A does), and k_advect with one substep on the same diffuse points (two
sweeps per point that is in the fluid, against the step's one).

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400): the two stage kernels, the emission
kernels at the default parameters (the count, then the spawns into a buffer that holds them), and k_whitewater_step on
1 M uniform points.  Kernel times come from `rocprofv3 --kernel-trace`, median of the launches of a case.

    python3 tools/whitewater_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/whitewater_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_whitewater_normals", "k_whitewater_stage", "k_whitewater_count", "k_whitewater_spawn", "k_whitewater_step",
           "k_field_points", "k_advect")


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    n = len(pos)
    origin = np.asarray(params.ext_min[:3], np.float32)
    top = np.asarray(params.ext_max[:3], np.float32)
    rng = np.random.default_rng(1)
    pts = (origin + rng.random((1 << 20, 3), np.float32) * (top - origin)).astype(np.float32)
    vel = rng.normal(0.0, 1.0, pts.shape).astype(np.float32)
    life = np.full(len(pts), 3.0, np.float32)
    emit = ws.fluid.whitewater_emit_params()
    step = ws.fluid.whitewater_step_params()
    march = ws.fluid.advect_params(step.dt, 1)
    cases = []

    def case(at, what, kernels, items, call, **extra):
        for _ in range(repeats):
            call()
        cases.append(dict(step=at, what=what, kernels=kernels, items=items, repeats=repeats, **extra))

    done = 0
    for at in (10, 400):
        w.run(at - done)
        done = at
        cur = w.read_positions()
        stage = ["k_whitewater_normals", "k_whitewater_stage"]
        case(at, "stage (read_whitewater)", stage, n, w.read_whitewater)
        case(at, "yardstick: density + gradient at the particles", ["k_field_points"], n,
             lambda: w.sample_density_points(cur, gradient=True))
        count = w.emit_whitewater(emit, cap=0)["count"]  # (not a measured case: its kernels are skipped below)
        cases.append(dict(step=at, what="(count)", kernels=stage + ["k_whitewater_count"], items=n, repeats=1, skip=True))
        spawn = ["k_whitewater_spawn"] if count else []
        case(at, "emit, default parameters", stage + ["k_whitewater_count"] + spawn, n,
             lambda: w.emit_whitewater(emit, cap=count), emitted=count)
        case(at, "diffuse step, 1 M uniform points", ["k_whitewater_step"], len(pts), lambda: w.step_whitewater(step, pts, vel, life))
        case(at, "yardstick: advect 1 M points x 1 substep", ["k_advect"], len(pts), lambda: w.advect_points(march, pts))
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="whitewater_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats)]
    subprocess.check_call(cmd, timeout=1100)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if any(k in r["Kernel_Name"] for k in KERNELS) and not re.search(r"\bk_field_\w+<.*\bFieldVel\b", r["Kernel_Name"].split("(")[0])]
    cases = json.load(open(cases_path))
    result = []
    k = 0
    for c in cases:
        times = {name: [] for name in c["kernels"]}
        for _ in range(c["repeats"]):
            for name in c["kernels"]:
                got, us = disp[k]
                assert name in got, (c, got)
                times[name].append(us)
                k += 1
        if c.get("skip"):
            continue
        for name in c["kernels"]:
            us = float(np.median(times[name]))
            result.append({"step": c["step"], "what": c["what"], "kernel": name, "us": us,
                           "items_per_s": c["items"] / (us * 1e-6), "emitted": c.get("emitted")})
    assert k == len(disp), (k, len(disp))
    print("%-6s %-48s %-22s %10s %10s" % ("step", "case", "kernel", "us", "G items/s"))
    for r in result:
        print("%-6d %-48s %-22s %10.1f %10.3f" % (r["step"], r["what"], r["kernel"], r["us"], r["items_per_s"] * 1e-9))
    json.dump(result, open(os.path.join(out, "whitewater_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
