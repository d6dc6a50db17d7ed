#!/usr/bin/env python3
"""Timing of the density field sampler's two kernels (ws_sample_density_grid / _points, DESIGN.md "The fluid as a field").

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400); grids of 256 x 144 x 144 (spacing h)
and 512 x 288 x 288 (spacing h / 2) over the container, each sampled by the grid call (brick kernel) and by the points
call on the same nodes (points kernel).  Kernel times come from `rocprofv3 --kernel-trace`; the pair counts from the
positions on the host: tested = candidates the kernel's loops visit (points: the node's 27 cells; bricks: 64 lanes x
the brick's support cells), accepted = particle-node pairs within h.

    python3 tools/field_timing.py [--out DIR] [--repeats R]      # runs itself under rocprofv3, prints a table + JSON
    python3 tools/field_timing.py child OUT.json R                 # the measured program (what rocprofv3 runs)
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


def box_sums(counts, lo, hi):
    """Sum of counts over the cell boxes [lo, hi] (inclusive, per row), via a 3-D prefix sum."""
    P = np.zeros(tuple(s + 1 for s in counts.shape), np.int64)
    P[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)
    a, b = lo, hi + 1
    s = np.zeros(len(lo), np.int64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                x = b[:, 0] if cx else a[:, 0]
                y = b[:, 1] if cy else a[:, 1]
                z = b[:, 2] if cz else a[:, 2]
                s += (-1) ** (3 - cx - cy - cz) * P[x, y, z]
    return s


def pair_counts(pos, params, origin, spacing, dims):
    h = np.float32(params.smoothing_radius)
    org = np.floor(np.asarray(params.ext_min[:3], np.float32) / h).astype(np.int64) - 2
    top = np.floor(np.asarray(params.ext_max[:3], np.float32) / h).astype(np.int64) + 2
    gdim = top - org + 1

    def cell(x):
        return np.clip(np.floor(x / h).astype(np.int64) - org, 0, gdim - 1)

    counts = np.zeros(gdim, np.int64)
    np.add.at(counts, tuple(cell(pos).T), 1)
    ax = [np.float32(origin[a]) + np.arange(dims[a], dtype=np.float32) * np.float32(spacing[a]) for a in range(3)]
    axc = [np.clip(np.floor(ax[a] / h).astype(np.int64) - org[a], 0, gdim[a] - 1) for a in range(3)]
    # points kernel: every node tests its 27 cells
    cx, cy, cz = np.meshgrid(axc[0], axc[1], axc[2], indexing="ij")
    c = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 1)
    tested_points = int(box_sums(counts, np.maximum(c - 1, 0), np.minimum(c + 1, gdim - 1)).sum())
    del cx, cy, cz, c
    # brick kernel: 64 lanes test every candidate of the brick's support box
    first = [axc[a][0::4] for a in range(3)]
    last = [axc[a][np.minimum(np.arange(0, dims[a], 4) + 3, dims[a] - 1)] for a in range(3)]
    fx, fy, fz = np.meshgrid(*first, indexing="ij")
    lx, ly, lz = np.meshgrid(*last, indexing="ij")
    lo = np.maximum(np.stack([fx.ravel(), fy.ravel(), fz.ravel()], 1) - 1, 0)
    hi = np.minimum(np.stack([lx.ravel(), ly.ravel(), lz.ravel()], 1) + 1, gdim - 1)
    tested_bricks = int(64 * box_sums(counts, lo, hi).sum())
    # accepted: per particle, the nodes within h
    sp = np.asarray(spacing, np.float32)
    o = np.asarray(origin, np.float32)
    r = [int(np.ceil(h / sp[a])) + 1 for a in range(3)]
    accepted = 0
    for b in range(0, len(pos), 1 << 17):
        p = pos[b:b + (1 << 17)]
        base = np.floor((p - o) / sp).astype(np.int64)
        for dx in range(-r[0] + 1, r[0] + 1):
            for dy in range(-r[1] + 1, r[1] + 1):
                for dz in range(-r[2] + 1, r[2] + 1):
                    idx = base + np.array([dx, dy, dz])
                    ok = np.all((idx >= 0) & (idx < np.asarray(dims)), 1)
                    node = o + idx.astype(np.float32) * sp
                    e = p - node
                    d2 = (e * e).sum(1)
                    accepted += int(np.count_nonzero(ok & (d2 <= h * h)))
    return tested_points, tested_bricks, accepted


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    h = np.float32(params.smoothing_radius)
    origin = np.asarray(params.ext_min[:3], np.float32)
    cases = []
    done = 0
    for step in (10, 400):
        w.run(step - done)
        done = step
        cur = w.read_positions()
        for name, dims, spacing in (("256x144x144 @ h", (256, 144, 144), h), ("512x288x288 @ h/2", (512, 288, 288), h / np.float32(2))):
            sp = np.full(3, spacing, np.float32)
            tp, tb, acc = pair_counts(cur, params, origin, sp, dims)
            nodes = dims[0] * dims[1] * dims[2]
            for _ in range(repeats):
                w.sample_density_grid(origin, sp, dims)
            ax = [origin[a] + np.arange(dims[a], dtype=np.float32) * sp[a] for a in range(3)]
            z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
            q = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
            del x, y, z
            for _ in range(repeats):
                w.sample_density_points(q)
            del q
            cases.append({"step": step, "grid": name, "nodes": nodes, "repeats": repeats, "tested_points": tp,
                          "tested_bricks": tb, "accepted": acc})
    w.close()
    json.dump(cases, open(out_path, "w"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="field_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats)]
    subprocess.check_call(cmd, timeout=1500)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows
            if re.search(r"\bk_field_(bricks|points)<.*\bFieldIso\b", r["Kernel_Name"].split("(")[0])]  # (the density field's)
    cases = json.load(open(cases_path))
    result = []
    k = 0
    for c in cases:
        for kind, tested in (("bricks", c["tested_bricks"]), ("points", c["tested_points"])):
            ds = disp[k:k + c["repeats"]]
            k += c["repeats"]
            assert all(("k_field_" + kind) in n for n, _ in ds), (kind, [n for n, _ in ds])
            us = float(np.median([t for _, t in ds]))
            result.append({"step": c["step"], "grid": c["grid"], "kernel": kind, "us": us,
                           "nodes_per_s": c["nodes"] / (us * 1e-6), "tested_pairs_per_s": tested / (us * 1e-6),
                           "accepted_pairs_per_s": c["accepted"] / (us * 1e-6), "tested": tested, "accepted": c["accepted"]})
    print("%-6s %-20s %-7s %10s %12s %14s %14s" % ("step", "grid", "kernel", "us", "Gnodes/s", "Gtested/s", "Gaccepted/s"))
    for r in result:
        print("%-6d %-20s %-7s %10.1f %12.2f %14.2f %14.2f" % (r["step"], r["grid"], r["kernel"], r["us"], r["nodes_per_s"] * 1e-9,
                                                              r["tested_pairs_per_s"] * 1e-9, r["accepted_pairs_per_s"] * 1e-9))
    json.dump(result, open(os.path.join(out, "field_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
