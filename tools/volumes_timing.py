#!/usr/bin/env python3
"""Timing of k_edit_current<EditVolumes<..>> (ws_collide_volumes) beside its yardstick from the SAME trace:
k_edit_current<EditSolids<..>> with the analytic box whose distance field the volume holds, at the same places -- the same
contacts, so the difference is what the grid costs: eight gathers per lane and pose, the interpolation, and a reach that is
the volume's padded domain instead of the box.

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400): k = 1 and k = 16 poses of one 64^3
volume (1 MiB: the exact distance to a box, padded with four cells of positive distance), with and without the reaction.
The boxes stand in the lower half of the container, where the fluid is once it has settled; every launch of a case shifts
them by a fraction of the smoothing radius, so that each launch finds fresh contacts.  Kernel times come from one run
under `rocprofv3 --kernel-trace`: the median of a case's launches, with the smallest and the largest beside it -- a single
run cannot resolve anything inside the spread of the yardstick rows.

    python3 tools/volumes_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/volumes_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
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

N = 64    # nodes per axis
PAD = 4   # cells of positive distance round the box


def box_distance(xyz, b):
    """The exact signed distance to the axis-aligned box of half extents b, float64."""
    a = np.abs(xyz) - b
    return np.sqrt((np.maximum(a, 0.0) ** 2).sum(axis=-1)) + np.minimum(a.max(axis=-1), 0.0)


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    lo = np.asarray(params.ext_min[:3], np.float64)
    hi = np.asarray(params.ext_max[:3], np.float64)
    h = float(params.smoothing_radius)
    rng = np.random.default_rng(1)
    size = float(hi[1] - lo[1]) / 12.0
    b = np.array([size, 0.5 * size, 0.75 * size])            # the box's half extents
    spacing = 2.0 * b / (N - 1 - 2 * PAD)                     # the box spans N - 1 - 2 PAD cells
    origin = -b - PAD * spacing
    axes = [origin[a] + np.arange(N) * spacing[a] for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    w.upload_volume(0, origin, spacing, box_distance(np.stack([x, y, z], axis=-1), b).astype(np.float32))
    centres = [lo + rng.random(3) * (hi - lo) * (1.0, 0.5, 1.0) for _ in range(16)]
    rot = (0.8, 0.6, 0.0, -0.6, 0.8, 0.0, 0.0, 0.0, 1.0)
    common = dict(restitution=0.3, friction=0.2, margin=0.5 * h, rot=rot)

    def boxes(k, shift):
        return [ws.fluid.solid("box", centres[e] + np.array([shift, 0.0, 0.0]), b, **common) for e in range(k)]

    def poses(k, shift):
        return [ws.fluid.volume_pose(0, centres[e] + np.array([shift, 0.0, 0.0]), **common) for e in range(k)]

    cases = []
    done = 0
    launch = 0
    for at in (10, 400):
        w.run(at - done)
        done = at + 1
        for kernel, call, objects in (("EditSolids", w.collide_solids, boxes), ("EditVolumes", w.collide_volumes, poses)):
            for k in (1, 16):
                for react in (False, True):
                    got = None
                    for _ in range(repeats):
                        launch += 1
                        got = call(objects(k, 0.25 * h * launch), reaction=react)
                    cases.append(dict(step=at, kernel=kernel, k=k, react=react, repeats=repeats, n=len(pos),
                                      contacts=None if got is None else [int(c) for c in got[0]]))
        w.run(1)
        w.sync()
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="volumes_timing_")
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
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if "k_edit_current" in r["Kernel_Name"]]
    cases = json.load(open(cases_path))
    i = 0
    for c in cases:  # the edits of the trace, in the order the child made them
        times = []
        for _ in range(c["repeats"]):
            name, us = disp[i]
            assert "k_edit_current<%s<%s>" % (c["kernel"], "true" if c["react"] else "false") in name, (c, name)
            times.append(us)
            i += 1
        c["us"], c["us_min"], c["us_max"] = float(np.median(times)), float(min(times)), float(max(times))
    assert i == len(disp), (i, len(disp))
    print("%-6s %-16s %-4s %-6s %10s %10s %10s %12s  %s" % ("step", "k_edit_current", "k", "sums", "median us", "min us", "max us", "/ yardstick", "contacts"))
    for c in cases:
        yard = next(y for y in cases if (y["step"], y["kernel"], y["k"], y["react"]) == (c["step"], "EditSolids", c["k"], c["react"]))
        c["over_yardstick"] = c["us"] / yard["us"]
        print("%-6d %-16s %-4d %-6s %10.1f %10.1f %10.1f %12.2f  %s" % (
            c["step"], c["kernel"], c["k"], "yes" if c["react"] else "no", c["us"], c["us_min"], c["us_max"], c["over_yardstick"],
            "-" if c["contacts"] is None else sum(c["contacts"])))
    spread = max((y["us_max"] - y["us_min"]) / y["us"] for y in cases if y["kernel"] == "EditSolids")
    print("spread of the yardstick rows (max - min over median, worst row): %.1f%%" % (100.0 * spread))
    json.dump(cases, open(os.path.join(out, "volumes_timing.json"), "w"), indent=1)
    print(json.dumps(cases))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
