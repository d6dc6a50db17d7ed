#!/usr/bin/env python3
"""Timing of the velocity field's kernels (ws_sample_velocity_grid / _points, ws_advect_points) beside
the density sampler's own, re-measured in the same process as the yardstick.

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400).  Grids of 256 x 144 x 144 (spacing h)
and 512 x 288 x 288 (spacing h / 2) over the container, each sampled by the grid call (brick kernel) and by the points
call on the same nodes (points kernel), velocity + density against the density sampler's density alone; then 1 M uniform
points through the points call, and the same 1 M points as tracers through ws_advect_points with one substep (two sweeps
per tracer that is in the fluid).  Kernel times come from `rocprofv3 --kernel-trace`, median of the launches of a case.

    python3 tools/velocity_timing.py [--out DIR] [--repeats R]      # runs itself under rocprofv3, prints a table + JSON
    python3 tools/velocity_timing.py child OUT.json R                 # the measured program (what rocprofv3 runs)
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

# The two field kernels serve both fields: an instantiation is told by the kernel's name together with the candidate
# source among its template arguments (whole word: FieldVel is a prefix of FieldVelCount).
KERNELS = {"velocity bricks": ("k_field_bricks", "FieldVel"), "velocity points": ("k_field_points", "FieldVel"),
           "k_advect": ("k_advect", None), "density bricks": ("k_field_bricks", "FieldIso"),
           "density points": ("k_field_points", "FieldIso")}


def is_kernel(name, key):
    kernel, source = KERNELS[key]
    head = name.split("(")[0]
    return re.search(r"\b%s\b" % kernel, head) is not None and (source is None or re.search(r"\b%s\b" % source, head) is not None)


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    h = np.float32(params.smoothing_radius)
    origin = np.asarray(params.ext_min[:3], np.float32)
    top = np.asarray(params.ext_max[:3], np.float32)
    pts = (origin + np.random.default_rng(1).random((1 << 20, 3), np.float32) * (top - origin)).astype(np.float32)
    march = ws.fluid.advect_params(4.0 * params.delta_time, 1)
    cases = []

    def case(step, what, kernel, items, call):
        for _ in range(repeats):
            call()
        cases.append({"step": step, "what": what, "kernel": kernel, "items": items, "repeats": repeats})

    done = 0
    for step in (10, 400):
        w.run(step - done)
        done = step
        for name, dims, spacing in (("256x144x144 @ h", (256, 144, 144), h), ("512x288x288 @ h/2", (512, 288, 288), h / np.float32(2))):
            sp = np.full(3, spacing, np.float32)
            nodes = dims[0] * dims[1] * dims[2]
            case(step, "velocity grid " + name, "velocity bricks", nodes, lambda: w.sample_velocity_grid(origin, sp, dims, density=True))
            case(step, "density grid " + name, "density bricks", nodes, lambda: w.sample_density_grid(origin, sp, dims))
            ax = [origin[a] + np.arange(dims[a], dtype=np.float32) * sp[a] for a in range(3)]
            z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
            q = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
            del x, y, z
            case(step, "velocity points " + name, "velocity points", nodes, lambda: w.sample_velocity_points(q, density=True))
            case(step, "density points " + name, "density points", nodes, lambda: w.sample_density_points(q))
            del q
        case(step, "velocity points 1 M uniform", "velocity points", len(pts), lambda: w.sample_velocity_points(pts, density=True))
        case(step, "density points 1 M uniform", "density points", len(pts), lambda: w.sample_density_points(pts))
        case(step, "advect 1 M tracers x 1 substep", "k_advect", len(pts), lambda: w.advect_points(march, pts))
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="velocity_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats)]
    subprocess.check_call(cmd, timeout=1100)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if any(is_kernel(r["Kernel_Name"], k) for k in KERNELS)]
    cases = json.load(open(cases_path))
    result = []
    k = 0
    for c in cases:
        ds = disp[k:k + c["repeats"]]
        k += c["repeats"]
        assert len(ds) == c["repeats"] and all(is_kernel(n, c["kernel"]) for n, _ in ds), (c, [n for n, _ in ds])
        us = float(np.median([t for _, t in ds]))
        result.append({"step": c["step"], "what": c["what"], "kernel": c["kernel"], "us": us, "items_per_s": c["items"] / (us * 1e-6)})
    assert k == len(disp), (k, len(disp))
    by = {(r["step"], r["what"]): r for r in result}
    print("%-6s %-36s %-18s %10s %10s %14s" % ("step", "case", "kernel", "us", "G items/s", "x density row"))
    for r in result:
        yard = by.get((r["step"], r["what"].replace("velocity", "density")))
        r["vs_density"] = r["us"] / yard["us"] if yard and yard is not r else None
        print("%-6d %-36s %-18s %10.1f %10.2f %14s" % (r["step"], r["what"], r["kernel"], r["us"], r["items_per_s"] * 1e-9,
                                                        "%.2f" % r["vs_density"] if r["vs_density"] else "-"))
    json.dump(result, open(os.path.join(out, "velocity_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
