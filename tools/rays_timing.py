#!/usr/bin/env python3
"""Timing of ws_cast_camera, modelled on tools/surface_timing.py.

C3 (4 M particles, lattice) at step 10 (sparse) and step 400 (settled).  A camera 45 units from the container's centre
looks down at it at 45 degrees over the whole container, at 640 x 360 and 1280 x 720; dt = h / 2, t_start = 15 (the
container begins at depth 19.5), steps = what crosses the container's diagonal, refine = 6, iso = target_density / 2,
with normals, density field; one more row for the anisotropic field (settled, 640 x 360, default ws_aniso_params).
Every case is cast R times by the product library (the plain per-lane loop) and R times by a build of the occupancy-bit
and wave-vote patch (tools/ab_build.sh rays_vote "" rays_occupancy_vote), in the same process from the same state; the
two must agree bit for bit.  Each state runs in a program of its own under `rocprofv3 --kernel-trace`.  Per case, the median over the calls of:
the occupancy pass (k_ray_occupancy), the cast kernel (k_ray_cast), the rebin (every other kernel of the call: the
sampler's counting sort, with the anisotropic field also the stage and the centres' sort).  The product launches no
occupancy pass, so its occupancy time is always 0; the patched build's cast kernel PLUS its occupancy pass is what has to
beat the product's cast kernel.

    python3 tools/rays_timing.py [--out DIR] [--repeats R] [--variant tools/ab/librays_vote.so]
    python3 tools/rays_timing.py child OUT.json STEP R VARIANT     # one measured state (what rocprofv3 runs)
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

SIZES = ((640, 360), (1280, 720))
# what a ray call launches before its cast kernel, first to last: the positions by id, the counting sort (its memset may
# show as a fill kernel of the runtime), with the anisotropic field the stage and the centres' sort, the occupancy pass
CALL_KERNELS = ("k_gather_positions", "k_field_", "k_view_", "k_scan", "k_scatter", "k_aniso", "k_ray_occupancy", "fillBuffer")


def child(out_path, step, repeats, variant_path):
    import water_sandbox_amd as ws

    pos, params = ws.workloads.make_workload("c3", "lattice")
    libs = [("product", ws.load_library())]
    if variant_path:
        libs.append(("vote", ws.fluid.bind_library(variant_path)))
    h = np.float32(params.smoothing_radius)
    mn = np.asarray(params.ext_min[:3], np.float64)
    mx = np.asarray(params.ext_max[:3], np.float64)
    dt = float(h / np.float32(2))
    steps = int(np.ceil(np.linalg.norm(mx - mn) / dt))
    march = ws.fluid.ray_params(15.0, dt, steps, 6, 0.5 * params.target_density)
    s = np.sqrt(0.5)
    centre = 0.5 * (mn + mx)
    forward = np.array([0.0, -s, -s])
    cases = [("density", size) for size in SIZES] + ([("aniso", SIZES[0])] if step >= 400 else [])
    calls, results = [], {}
    for lib_name, lib in libs:
        w = ws.FluidWorker(pos, params, library=lib)
        w.run(step)
        for field, size in cases:
            up = np.array([0.0, s, -s]) * 0.75 * size[1] / size[0]
            cam = ws.fluid.camera(centre - 45.0 * forward, forward, (0.75, 0.0, 0.0), up)
            aniso = ws.fluid.aniso_params() if field == "aniso" else None
            for _ in range(repeats):
                t, n = w.cast_camera(march, cam, size, aniso=aniso)
                calls.append({"lib": lib_name, "field": field, "size": list(size)})
            key = "%s %dx%d" % (field, size[0], size[1])
            if key in results:
                same = bool(np.array_equal(t.view(np.uint32), results[key][0].view(np.uint32))
                            and np.array_equal(n.view(np.uint32), results[key][1].view(np.uint32)))
                results[key] = results[key] + (same,)
            else:
                results[key] = (t, n)
        w.close()
    out = {"step": step, "steps_per_ray": steps, "calls": calls, "cases": {
        k: {"hit_fraction": float(np.isfinite(v[0]).mean()), "vote_bit_identical": (v[2] if len(v) > 2 else None)}
        for k, v in results.items()}}
    json.dump(out, open(out_path, "w"))


def per_call(rows):
    """One record per k_ray_cast launch, in launch order: its time, the occupancy pass before it and the other kernels of
    the same call (walking back to the call's first kernel, k_gather_positions; at the latest to the previous cast or to
    a kernel no ray call launches: a step's)."""
    out = []
    for i, (name, us) in enumerate(rows):
        if "k_ray_cast" not in name:
            continue
        rec = {"cast": us, "occupancy": 0.0, "rebin": 0.0}
        j = i - 1
        while j >= 0 and "k_ray_cast" not in rows[j][0] and any(k in rows[j][0] for k in CALL_KERNELS):
            rec["occupancy" if "k_ray_occupancy" in rows[j][0] else "rebin"] += rows[j][1]
            if "k_gather_positions" in rows[j][0]:
                break
            j -= 1
        out.append(rec)
    return out


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    out = arg("--out", None) or tempfile.mkdtemp(prefix="rays_timing_")
    repeats = int(arg("--repeats", 5))
    variant = arg("--variant", os.path.join(ROOT, "tools", "ab", "librays_vote.so"))
    if not os.path.exists(variant):
        print("no %s: timing the product library alone (build it: tools/ab_build.sh rays_vote \"\" rays_occupancy_vote)" % variant)
        variant = ""
    os.makedirs(out, exist_ok=True)
    result = []
    for step in (10, 400):
        state_path = os.path.join(out, "state_%d.json" % step)
        trace = os.path.join(out, "trace_%d" % step)
        # the measured program runs under a limit of its own (ending rocprofv3 alone would leave it on the GPU); a failed
        # or overdue state ends the run: nothing more is started
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace, "--", "timeout", "-k", "10", "540",
               sys.executable, os.path.abspath(__file__), "child", state_path, str(step), str(repeats), variant]
        subprocess.check_call(cmd, timeout=600)
        kt = glob.glob(os.path.join(trace, "**", "*_kernel_trace.csv"), recursive=True)[0]
        rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
        rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows]
        state = json.load(open(state_path))
        recs = per_call(rows)
        assert len(recs) == len(state["calls"]), (len(recs), len(state["calls"]))
        table = {}
        for call, rec in zip(state["calls"], recs):
            key = "%s %dx%d" % (call["field"], call["size"][0], call["size"][1])
            table.setdefault(key, {}).setdefault(call["lib"], []).append(rec)
        for key, libs in table.items():
            med = {lib: {k: float(np.median([r[k] for r in rs])) for k in ("occupancy", "cast", "rebin")} for lib, rs in libs.items()}
            w, hgt = (int(x) for x in key.split()[1].split("x"))
            p = med["product"]
            row = {"step": step, "case": key, "rays": w * hgt, "steps_per_ray": state["steps_per_ray"], "repeats": repeats,
                   "us": p, "Mrays_per_s_cast_kernel": w * hgt / p["cast"],
                   "Mrays_per_s_call": w * hgt / (p["cast"] + p["occupancy"] + p["rebin"]), **state["cases"][key]}
            if "vote" in med:
                row["vote_us"] = med["vote"]
                row["product_over_vote"] = p["cast"] / (med["vote"]["cast"] + med["vote"]["occupancy"])
            result.append(row)
    print("%-5s %-18s %8s | %9s %10s %9s | %9s %9s | %6s | %10s %6s %5s" % (
        "step", "case", "rays", "occup us", "cast us", "rebin us", "Mray/s k", "Mray/s c", "hit", "vote us", "ratio", "same"))
    for r in result:
        pl = r.get("vote_us", {}).get("cast", float("nan")) + r.get("vote_us", {}).get("occupancy", float("nan"))
        print("%-5d %-18s %8d | %9.1f %10.1f %9.1f | %9.1f %9.1f | %6.3f | %10.1f %6.2f %5s" % (
            r["step"], r["case"], r["rays"], r["us"]["occupancy"], r["us"]["cast"], r["us"]["rebin"],
            r["Mrays_per_s_cast_kernel"], r["Mrays_per_s_call"], r["hit_fraction"], pl,
            r.get("product_over_vote", float("nan")), r["vote_bit_identical"]))
    json.dump(result, open(os.path.join(out, "rays_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else "")
    else:
        main()
