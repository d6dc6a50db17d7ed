#!/usr/bin/env python3
"""Timing of the gauges (ws_measure / ws_select_particles) beside three things from the SAME job:
  (a) what a host could do before these calls existed: ws_read_particles (80 bytes per particle over PCIe) and the numpy
      restatement of the definition (tests/gauges_ref.py) -- whose gauges must be the device's, bit for bit;
  (b) ws_apply_forces with 16 emitters and counts: a pass over the same 32-byte records that also writes them;
  (c) the floor: n x 32 bytes at the float4 copy rate bench.py's roofline uses (HBM_COPY_GBS).

C3 (4 M particles, cloud) in the sparse window (step 10) and settled (step 400).  ws_measure with 1 region that holds
everything and with 16 mixed regions, with and without WS_GAUGE_ATTRIBUTES; ws_select_particles at about 1 % selected.
Every call timed here is synchronous, so the host clock around it is the time a frame loop would lose: the median of R
repeats after one untimed call (the first call allocates its scratch).

    python3 tools/gauges_timing.py [--out DIR] [--repeats R] [--no-host]    # prints a table + one JSON line
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_COPY_GBS = 6290.0  # bench.py


def mixed_regions(G, params, seed=5):
    """16 regions over the container: everything, nothing, a thin slab, a small ball, six spheres and six boxes."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    mid, ext = (lo + hi) / 2, hi - lo
    rng = np.random.default_rng(seed)
    out = [G.region(G.BOX, mid, (1e15, 1e15, 1e15)), G.region(G.SPHERE, hi + 50.0, 1.0),
           G.region(G.BOX, (mid[0], lo[1] + 0.05 * ext[1], mid[2]), (ext[0], 0.05 * ext[1], ext[2])),
           G.region(G.SPHERE, mid, 0.04 * ext.min())]
    while len(out) < 16:
        c = lo + rng.random(3) * ext
        out.append(G.region(G.SPHERE, c, rng.uniform(0.15, 0.45) * ext.min()) if len(out) % 2 else
                   G.region(G.BOX, c, rng.uniform(0.1, 0.4, 3) * ext))
    return out


def lasso(G, params, frac=0.01, k=16):
    """k boxes side by side over the low `frac` of the container along x: about that share of a uniform cloud."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    width = (hi[0] - lo[0]) * frac / k
    mid, half = (lo + hi) / 2, (hi - lo) / 2 + 1.0
    return [G.region(G.BOX, (lo[0] + (e + 0.5) * width, mid[1], mid[2]), (width / 2, half[1], half[2])) for e in range(k)]


def median_ms(f, repeats):
    f()  # untimed: scratch, staging
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter_ns()
        out = f()
        times.append((time.perf_counter_ns() - t0) * 1e-6)
    return float(np.median(times)), out


def main():
    import gauges_ref as G
    import water_sandbox_amd as ws

    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    host = "--no-host" not in sys.argv
    pos, params = ws.workloads.make_workload("c3", "cloud")
    n = len(pos)
    w = ws.FluidWorker(pos, params)
    w.write_attributes(np.random.default_rng(3).uniform(0.0, 1.0, (n, 4)).astype(np.float32))
    everything, mixed, few = mixed_regions(G, params)[:1], mixed_regions(G, params), lasso(G, params)
    arr = {"everything": G.to_ws(ws, everything), "mixed": G.to_ws(ws, mixed), "lasso": G.to_ws(ws, few)}
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    rng = np.random.default_rng(1)
    emitters = [ws.fluid.force(("radial", "jet", "vortex")[e % 3], lo + rng.random(3) * (hi - lo) * (1.0, 0.5, 1.0),
                               float(hi[1] - lo[1]) / 6.0, 0.0, axis=(0.0, 1.0, 0.0)) for e in range(16)]
    floor_ms = n * 32 / (HBM_COPY_GBS * 1e9) * 1e3
    rows, done = [], 0
    for state, at in (("sparse", 10), ("settled", 400)):
        w.run(at - done)
        done = at
        w.sync()
        for name, k in (("everything", 1), ("mixed", 16)):
            for attributes in (False, True):
                t, g = median_ms(lambda: w.measure(arr[name], attributes=attributes), repeats)
                rows.append(dict(state=state, call="ws_measure", regions=k, attributes=attributes, ms=t, floor_ms=floor_ms,
                                 floor_frac=floor_ms / t, counts=[int(c) for c in g["count"]]))
        t, (ids, total) = median_ms(lambda: w.select_particles(arr["lasso"]), repeats)
        rows.append(dict(state=state, call="ws_select_particles", regions=16, ms=t, selected=total, share=total / n))
        t, _ = median_ms(lambda: w.select_particles(arr["lasso"], cap=0), repeats)
        rows.append(dict(state=state, call="ws_select_particles (count only)", regions=16, ms=t, selected=total))
        t, affected = median_ms(lambda: w.apply_forces(emitters, float(params.delta_time), counts=True), repeats)
        rows.append(dict(state=state, call="ws_apply_forces, counts (b)", regions=16, ms=t, floor_ms=floor_ms))
        if host:  # (a), once per state: its gauges are the device's
            t0 = time.perf_counter_ns()
            rec = w.read_vec("particles")
            t_read = (time.perf_counter_ns() - t0) * 1e-6
            x, v = np.ascontiguousarray(rec["position"][:, :3]), np.ascontiguousarray(rec["velocity"][:, :3])
            for name, regions in (("everything", everything), ("mixed", mixed)):
                t0 = time.perf_counter_ns()
                want = G.measure(x, v, regions)
                t_numpy = (time.perf_counter_ns() - t0) * 1e-6
                bad = G.same(w.measure(arr[name]), want)
                assert not bad, (state, name, bad)
                rows.append(dict(state=state, call="ws_read_particles + numpy (a)", regions=len(regions), ms=t_read + t_numpy,
                                 read_ms=t_read, numpy_ms=t_numpy))
            t0 = time.perf_counter_ns()
            want = G.select(x, few)
            t_numpy = (time.perf_counter_ns() - t0) * 1e-6
            assert np.array_equal(w.select_particles(arr["lasso"])[0], want), state
            rows.append(dict(state=state, call="ws_read_particles + numpy select (a)", regions=16, ms=t_read + t_numpy,
                             read_ms=t_read, numpy_ms=t_numpy))
    w.close()
    print("%-8s %-38s %4s %5s %11s %10s" % ("state", "call", "k", "attr", "ms", "floor / ms"))
    for r in rows:
        print("%-8s %-38s %4d %5s %11.3f %10s" % (r["state"], r["call"], r["regions"], {True: "yes", False: "no"}.get(r.get("attributes"), "-"),
                                                  r["ms"], "%.2f" % r["floor_frac"] if "floor_frac" in r else "-"))
    print("floor (c): %d x 32 B at %.0f GB/s = %.4f ms" % (n, HBM_COPY_GBS, floor_ms))
    result = {"config": "c3 cloud", "n": n, "repeats": repeats, "floor_ms": floor_ms, "rows": rows}
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        json.dump(result, open(os.path.join(out_dir, "gauges_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
