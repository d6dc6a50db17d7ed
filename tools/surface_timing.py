#!/usr/bin/env python3
"""Timing of ws_extract_surface's passes ("The surface as a mesh").

C3 (4 M particles, lattice) in the sparse window (step 10) and settled (step 400); grids of 256 x 144 x 144 (spacing h)
and 512 x 288 x 288 (spacing h / 2) over the container, iso = target_density / 2, with normals.  Per case: one counts-only
call, then R calls at exact capacity.  Kernel times come from `rocprofv3 --kernel-trace`: the sample kernel
(k_field_bricks), k_iso_count, the two scans of the per-workgroup totals, k_iso_totals, k_iso_vertices and
k_iso_triangles.
"B/node" is the compulsory traffic of the passes after sampling: 4 B of density read and 1 B of code written per node
(count), 1 B of code read per node by each later pass, plus the mesh written (24 B per vertex with its normal, 12 B per
triangle); "mesh MB" against "volume MB" (density + gradient, what a host-side extractor would have to read back).

    python3 tools/surface_timing.py [--out DIR] [--repeats R]      # runs itself under rocprofv3, prints a table + JSON
    python3 tools/surface_timing.py child OUT.json R                 # the measured program (what rocprofv3 runs)
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

PASSES = ("k_field_bricks", "k_iso_count", "scan_v", "scan_t", "k_iso_totals", "k_iso_vertices", "k_iso_triangles")


def child(out_path, repeats):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    h = np.float32(params.smoothing_radius)
    iso = np.float32(0.5 * params.target_density)
    origin = np.asarray(params.ext_min[:3], np.float32)
    cases = []
    done = 0
    for step in (10, 400):
        w.run(step - done)
        done = step
        for name, dims, spacing in (("256x144x144 @ h", (256, 144, 144), h), ("512x288x288 @ h/2", (512, 288, 288), h / np.float32(2))):
            sp = np.full(3, spacing, np.float32)
            d = np.asarray(dims, np.uint32)
            nv, nt = C.c_uint32(0), C.c_uint32(0)
            call = w._L.ws_extract_surface
            w._check(call(w._h, origin.ctypes.data, sp.ctypes.data, d.ctypes.data, C.c_float(iso), 0, 0, None, None, None,
                          C.byref(nv), C.byref(nt)))
            V, T = nv.value, nt.value
            xyz = np.empty((max(V, 1), 3), np.float32)
            nrm = np.empty((max(V, 1), 3), np.float32)
            tri = np.empty((max(T, 1), 3), np.uint32)
            for _ in range(repeats):
                w._check(call(w._h, origin.ctypes.data, sp.ctypes.data, d.ctypes.data, C.c_float(iso), V, T, xyz.ctypes.data,
                              nrm.ctypes.data, tri.ctypes.data, C.byref(nv), C.byref(nt)))
            nodes = int(dims[0]) * int(dims[1]) * int(dims[2])
            cases.append({"step": step, "grid": name, "nodes": nodes, "repeats": repeats, "vertices": V, "triangles": T})
    w.close()
    json.dump(cases, open(out_path, "w"))


def groups(rows):
    """Per ws_extract_surface call: the kernels from its k_iso_count to the next one, and the last sample kernel before."""
    names = [r[0] for r in rows]
    starts = [i for i, n in enumerate(names) if "k_iso_count" in n]
    out = []
    for g, i in enumerate(starts):
        end = starts[g + 1] if g + 1 < len(starts) else len(rows)
        body = rows[i:end]
        if not any("k_iso_triangles" in n for n, _ in body):
            continue  # a counts-only call
        brick = [t for n, t in rows[:i] if "k_field_bricks" in n and re.search(r"\bFieldIso\b", n.split("(")[0])][-1]
        scans = [t for n, t in body if "k_scan" in n]
        pick = {"k_field_bricks": brick, "k_iso_count": body[0][1], "scan_v": scans[0], "scan_t": scans[1],
                "k_iso_totals": [t for n, t in body if "k_iso_totals" in n][0],
                "k_iso_vertices": [t for n, t in body if "k_iso_vertices" in n][0],
                "k_iso_triangles": [t for n, t in body if "k_iso_triangles" in n][0]}
        out.append(pick)
    return out


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="surface_timing_")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    os.makedirs(out, exist_ok=True)
    cases_path = os.path.join(out, "cases.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "child", cases_path, str(repeats)]
    subprocess.check_call(cmd, timeout=1500)
    kt = glob.glob(os.path.join(out, "trace", "**", "*_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows]
    full = groups(rows)
    cases = json.load(open(cases_path))
    assert len(full) == sum(c["repeats"] for c in cases), (len(full), [c["repeats"] for c in cases])
    result = []
    k = 0
    for c in cases:
        calls = full[k:k + c["repeats"]]
        k += c["repeats"]
        us = {p: float(np.median([g[p] for g in calls])) for p in PASSES}
        after = sum(us[p] for p in PASSES[1:])
        nodes, V, T = c["nodes"], c["vertices"], c["triangles"]
        mesh_b = V * 24 + T * 12
        moved = nodes * (4 + 1 + 1 + 1) + mesh_b
        result.append({"step": c["step"], "grid": c["grid"], "nodes": nodes, "vertices": V, "triangles": T,
                       "us": us, "us_after_sampling": after, "bytes_per_node": moved / nodes,
                       "GB_per_s_after_sampling": moved / (after * 1e-6) * 1e-9,
                       "mesh_MB": mesh_b / 1e6, "volume_MB": nodes * 16 / 1e6})
    print("%-5s %-18s %9s %9s %9s | %8s %8s %7s %7s %7s %8s %8s | %7s %6s %8s %9s" % (
        "step", "grid", "Mnodes", "Mverts", "Mtris", "sample", "count", "scan_v", "scan_t", "totals", "verts", "tris", "after",
        "B/node", "mesh MB", "volume MB"))
    for r in result:
        u = r["us"]
        print("%-5d %-18s %9.2f %9.3f %9.3f | %8.1f %8.1f %7.1f %7.1f %7.1f %8.1f %8.1f | %7.1f %6.2f %8.1f %9.1f" % (
            r["step"], r["grid"], r["nodes"] * 1e-6, r["vertices"] * 1e-6, r["triangles"] * 1e-6, u["k_field_bricks"],
            u["k_iso_count"], u["scan_v"], u["scan_t"], u["k_iso_totals"], u["k_iso_vertices"], u["k_iso_triangles"],
            r["us_after_sampling"],
            r["bytes_per_node"], r["mesh_MB"], r["volume_MB"]))
    json.dump(result, open(os.path.join(out, "surface_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
