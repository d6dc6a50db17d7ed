#!/usr/bin/env python3
"""Timing of the anisotropic kernels, modelled on tools/surface_timing.py.

C3 (4 M particles, lattice) at step 10 (sparse) and step 400 (settled); grids of 256 x 144 x 144 (spacing h) and
512 x 288 x 288 (spacing h / 2) over the container from ext_min, iso = target_density / 2, default ws_aniso_params.
Each (step, grid) case runs in its own program under `rocprofv3 --kernel-trace`: R density-only calls of
ws_sample_aniso_grid and of ws_sample_aniso_points on every node of the same grid (both the points form,
k_field_points over FieldAniso) and of ws_sample_density_grid (the isotropic brick kernel), then R calls of
ws_extract_aniso_surface at exact capacity with normals, and one ws_read_anisotropy for the neighbour-count histogram and the lone fraction.  Per kernel: the median
launch.  The stage's tested pairs are the particles' 27-cell candidates (what k_aniso's distance test sees).

    python3 tools/aniso_timing.py [--out DIR] [--repeats R]      # runs the cases under rocprofv3, prints a table + JSON
    python3 tools/aniso_timing.py child OUT.json STEP GRID R      # one measured case (what rocprofv3 runs)
"""
import csv
import ctypes as C
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

GRIDS = {"h": (256, 144, 144), "h/2": (512, 288, 288)}
BIN = ("k_field_keys", "k_view_count", "k_scan", "k_scatter", "k_view_fix")


def _tested_pairs(pos, params):
    """Sum over particles of the particles in the 27 cells around its cell (the handle's grid, no merged cells)."""
    h = np.float32(params.smoothing_radius)
    mn = np.asarray(params.ext_min[:3], np.float32)
    mx = np.asarray(params.ext_max[:3], np.float32)
    org = np.floor(mn / h).astype(np.int64) - 2
    dim = np.floor(mx / h).astype(np.int64) + 2 - org + 1
    c = np.clip(np.floor(pos / h).astype(np.int64) - org, 0, dim - 1)
    cnt = np.zeros(tuple(dim), np.int64)
    np.add.at(cnt, (c[:, 0], c[:, 1], c[:, 2]), 1)
    box = np.zeros_like(cnt)
    pad = np.pad(cnt, 1)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                box += pad[dx:dx + dim[0], dy:dy + dim[1], dz:dz + dim[2]]
    return int(box[c[:, 0], c[:, 1], c[:, 2]].sum())


def child(out_path, step, grid, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(step)
    h = np.float32(params.smoothing_radius)
    iso = np.float32(0.5 * params.target_density)
    origin = np.asarray(params.ext_min[:3], np.float32)
    dims = GRIDS[grid]
    sp = np.full(3, h if grid == "h" else h / np.float32(2), np.float32)
    a = ws.fluid.aniso_params()
    for _ in range(repeats):
        w.sample_aniso_grid(origin, sp, dims, aniso=a)
    ax = [origin[k] + np.arange(dims[k], dtype=np.float32) * sp[k] for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    nodes = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.float32)
    del x, y, z
    for _ in range(repeats):
        w.sample_aniso_points(nodes, aniso=a)
    del nodes
    for _ in range(repeats):
        w.sample_density_grid(origin, sp, dims)
    d = np.asarray(dims, np.uint32)
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    call = w._L.ws_extract_aniso_surface
    w._check(call(w._h, C.byref(a), origin.ctypes.data, sp.ctypes.data, d.ctypes.data, C.c_float(iso), 0, 0, None, None,
                  None, C.byref(nv), C.byref(nt)))
    V, T = nv.value, nt.value
    xyz = np.empty((max(V, 1), 3), np.float32)
    nrm = np.empty((max(V, 1), 3), np.float32)
    tri = np.empty((max(T, 1), 3), np.uint32)
    for _ in range(repeats):
        w._check(call(w._h, C.byref(a), origin.ctypes.data, sp.ctypes.data, d.ctypes.data, C.c_float(iso), V, T,
                      xyz.ctypes.data, nrm.ctypes.data, tri.ctypes.data, C.byref(nv), C.byref(nt)))
    c, m, f, n = w.anisotropy(a)
    x = w.read_positions()
    w.close()
    lone = (m[:, 3] == 0) & (m[:, 4] == 0) & (m[:, 5] == 0) & (m[:, 0] == m[:, 1]) & (m[:, 1] == m[:, 2]) & (f == 8)
    hist = np.bincount(n.astype(np.int64))
    json.dump({"step": step, "grid": grid, "nodes": int(np.prod(dims)), "vertices": V, "triangles": T,
               "particles": int(len(n)), "tested_pairs": _tested_pairs(x, params), "accepted_pairs": int(n.sum()),
               "lone_fraction": float(lone.mean()), "below_min_neighbours": float((n < a.min_neighbours).mean()),
               "neighbour_histogram": hist.tolist(), "neighbour_median": float(np.median(n))}, open(out_path, "w"))


def kernel_medians(trace_dir):
    kt = glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True)[0]
    by = {}
    for r in csv.DictReader(open(kt)):
        name = r["Kernel_Name"]
        key = name.split("(")[0].split("<")[0].replace("void ", "").strip()
        if key in ("k_field_bricks", "k_field_points"):
            key += {"FieldAniso": "_aniso", "FieldIso": "_iso", "FieldVel": "_vel"}[  # (the candidate source, a whole word)
                re.search(r"\b(FieldAniso|FieldIso|FieldVel)\b", name.split("(")[0]).group(1)]
        by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {k: float(np.median(v)) for k, v in by.items()}, {k: len(v) for k, v in by.items()}


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="aniso_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    os.makedirs(out, exist_ok=True)
    result = []
    for step in (10, 400):
        for grid in ("h", "h/2"):
            tag = "s%d_%s" % (step, grid.replace("/", ""))
            case_path = os.path.join(out, tag + ".json")
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, tag), "--",
                   sys.executable, os.path.abspath(__file__), "child", case_path, str(step), grid, str(repeats)]
            subprocess.check_call(cmd, timeout=900)
            case = json.load(open(case_path))
            us, launches = kernel_medians(os.path.join(out, tag))
            case["us"] = us
            case["launches"] = launches
            case["stage_G_tested_pairs_per_s"] = case["tested_pairs"] / (us["k_aniso"] * 1e-6) * 1e-9
            case["stage_G_accepted_pairs_per_s"] = case["accepted_pairs"] / (us["k_aniso"] * 1e-6) * 1e-9
            result.append(case)
    print("| state | grid | M nodes | stage µs | G tested pairs/s | rebin µs | aniso points µs | "
          "iso bricks µs | mesh passes µs | M vertices | M triangles | lone fraction |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in result:
        u = r["us"]
        rebin = sum(u.get(k, 0.0) for k in BIN) + u.get("k_aniso_gather", 0.0)
        mesh = sum(u.get(k, 0.0) for k in ("k_iso_count", "k_iso_totals", "k_iso_vertices", "k_iso_triangles"))
        print("| step %d | %s | %.2f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.3f | %.3f | %.4f |" % (
            r["step"], r["grid"], r["nodes"] * 1e-6, u["k_aniso"], r["stage_G_tested_pairs_per_s"], rebin,
            u.get("k_field_points_aniso", float("nan")),
            u.get("k_field_bricks_iso", float("nan")), mesh, r["vertices"] * 1e-6, r["triangles"] * 1e-6,
            r["lone_fraction"]))
    for r in result:
        if r["grid"] == "h":
            hist = r["neighbour_histogram"]
            print("step %d: neighbours median %.0f, below N_eps %.4f, histogram (count: particles) %s" % (
                r["step"], r["neighbour_median"], r["below_min_neighbours"],
                ", ".join("%d: %d" % (k, v) for k, v in enumerate(hist) if v)))
    json.dump(result, open(os.path.join(out, "aniso_timing.json"), "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    else:
        main()
