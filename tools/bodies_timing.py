#!/usr/bin/env python3
"""Timing of k_body_forces + k_body_finish (ws_body_forces) beside the yardstick from the SAME trace: the
points kernel of the velocity field, k_field_points over FieldVel, on the same samples (ws_sample_velocity_points with
both outputs) -- the sweep the fused kernel makes too -- plus the floor for the bytes the reduction adds to it: a sample's
velocity and volume read (16 B), a chunk's table entry read, its partial written and read again (16 + 32 + 32 B), a
body's first chunk, centre and results (4 + 12 + 32 B), at the float4 copy rate bench.py's roofline uses (HBM_COPY_GBS).

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400): 64 bodies of 4 096 samples and 4 096
bodies of 64 samples, boxes of jittered samples scattered over the fluid's bounding box, so that some float, some are
under water and some hang in the air.  Kernel times come from `rocprofv3 --kernel-trace`, median of the launches of a case.

    python3 tools/bodies_timing.py [--out DIR] [--repeats R]    # runs itself under rocprofv3, prints a table + JSON
    python3 tools/bodies_timing.py child OUT.json R               # the measured program (what rocprofv3 runs)
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

CHUNK = 256  # samples per workgroup of k_body_forces
HBM_COPY_GBS = 6290.0  # bench.py
SHAPES = ((64, 4096), (4096, 64))  # (bodies, samples per body)


def bodies(rng, lo, hi, nb, per, half):
    """nb boxes of `per` jittered samples, centres uniform over [lo, hi]."""
    c = lo + rng.random((nb, 3)) * (hi - lo)
    xyz = (c[:, None, :] + rng.uniform(-half, half, (nb, per, 3))).reshape(-1, 3).astype(np.float32)
    vel = rng.normal(0.0, 0.5, xyz.shape).astype(np.float32)
    vol = np.full(len(xyz), (2.0 * half) ** 3 / per, np.float32)
    start = (np.arange(nb + 1) * per).astype(np.uint32)
    return xyz, vel, vol, start, c.astype(np.float32)


def added_bytes(nb, per):
    chunks = nb * ((per + CHUNK - 1) // CHUNK)
    return 16 * nb * per + (16 + 32 + 32) * chunks + (4 + 12 + 32) * nb


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    bp = ws.fluid.body_params()
    rng = np.random.default_rng(1)
    h = float(params.smoothing_radius)
    cases = []
    done = 0
    for at in (10, 400):
        w.run(at - done)
        done = at
        cur = w.read_positions()
        lo, hi = cur.min(0).astype(np.float64), cur.max(0).astype(np.float64)
        hi[1] += 4.0 * h  # up into the air above the fluid
        for nb, per in SHAPES:
            xyz, vel, vol, start, centres = bodies(rng, lo, hi, nb, per, 4.0 * h if per > 1000 else h)
            wet = None
            for _ in range(repeats):
                wet = w.body_forces(bp, xyz, vel, vol, start, centres).wet
            for _ in range(repeats):
                w.sample_velocity_points(xyz, density=True)
            cases.append(dict(step=at, bodies=nb, per_body=per, repeats=repeats, n=len(pos), wet_samples=int(wet.sum()),
                              floating=int(np.count_nonzero((wet > 0) & (wet < per)))))
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="bodies_timing_")
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
            if "k_body_forces" in r["Kernel_Name"] or "k_body_finish" in r["Kernel_Name"]
            or ("k_field_points" in r["Kernel_Name"] and "FieldVel" in r["Kernel_Name"])]
    cases = json.load(open(cases_path))
    assert len(disp) == sum(3 * c["repeats"] for c in cases), (len(disp), len(cases))
    result = []
    i = 0
    for c in cases:
        sweep, finish, points = [], [], []
        for _ in range(c["repeats"]):
            assert "k_body_forces" in disp[i][0] and "k_body_finish" in disp[i + 1][0], disp[i:i + 2]
            sweep.append(disp[i][1])
            finish.append(disp[i + 1][1])
            i += 2
        for _ in range(c["repeats"]):
            assert "k_field_points" in disp[i][0], disp[i]
            points.append(disp[i][1])
            i += 1
        fused = float(np.median(np.add(sweep, finish)))
        floor_us = added_bytes(c["bodies"], c["per_body"]) / (HBM_COPY_GBS * 1e9) * 1e6
        result.append(dict(c, sweep_us=float(np.median(sweep)), finish_us=float(np.median(finish)), fused_us=fused,
                           points_us=float(np.median(points)), ratio=fused / float(np.median(points)), floor_us=floor_us,
                           within_points_plus_two_floors=bool(fused <= float(np.median(points)) + 2.0 * floor_us)))
    print("%-6s %-7s %-9s %10s %10s %10s %10s %8s %10s %8s" % ("step", "bodies", "per body", "sweep us", "finish us", "fused us",
                                                                "points us", "ratio", "floor us", "wet"))
    for r in result:
        print("%-6d %-7d %-9d %10.1f %10.1f %10.1f %10.1f %8.3f %10.2f %8d" % (
            r["step"], r["bodies"], r["per_body"], r["sweep_us"], r["finish_us"], r["fused_us"], r["points_us"], r["ratio"],
            r["floor_us"], r["wet_samples"]))
    json.dump(result, open(os.path.join(out, "bodies_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
