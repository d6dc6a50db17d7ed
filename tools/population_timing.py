#!/usr/bin/env python3
"""Timing of a count change on the device (ws_remove_particles / ws_add_particles) beside the only way a
host could change the count before these calls existed: ws_read_particles, a numpy filter, ws_destroy, ws_create at the
new count, ws_write_particles.

C3 (4 M particles, cloud) after a few steps.  16 sinks drain about 1 % of the fluid; the drained particles are then poured
back.  The round trip makes the same two changes (filter the records, then append the drained ones again).  Every call
timed here ends in a device synchronise of its own -- the count-changing calls are synchronous, ws_create and
ws_write_particles wait for their uploads -- so the host clock around them is the time a frame loop would lose.  The
median of R repeats of each; one untimed round first (the first removal allocates its scratch, the first read its
staging buffer).

    python3 tools/population_timing.py [--out DIR] [--repeats R]    # prints a table + one JSON line
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sinks_for(ws, params, frac=0.01, k=16):
    """k boxes side by side over the low `frac` of the container along x: about that share of a uniform cloud."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    width = (hi[0] - lo[0]) * frac / k
    mid, half = (lo + hi) / 2, (hi - lo) / 2 + 1.0
    return [ws.fluid.sink("box", (lo[0] + (e + 0.5) * width, mid[1], mid[2]), (width / 2, half[1], half[2])) for e in range(k)]


def ms(f):
    t0 = time.perf_counter_ns()
    out = f()
    return (time.perf_counter_ns() - t0) * 1e-6, out


def main():
    import population_ref as P
    import water_sandbox_amd as ws

    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    pos, params = ws.workloads.make_workload("c3", "cloud")
    n = len(pos)
    sinks = sinks_for(ws, params)
    ref_sinks = [P.sink(s.kind, tuple(s.centre), tuple(s.half)) for s in sinks]
    w = ws.FluidWorker(pos, params)
    w.run(5)
    w.sync()
    t = dict(remove=[], add=[], trip_remove=[], trip_add=[])
    drained = 0
    for r in range(repeats + 1):
        # ---- on the device: drain, pour back ----
        rec = w.read_vec("particles")
        t_remove, (counts, new) = ms(lambda: w.remove_particles(sinks))
        gone = new == ws.fluid.REMOVED
        drained = int(gone.sum())
        assert drained == int(counts.sum()) and w.n == n - drained
        back_pos = np.ascontiguousarray(rec["position"][gone, :3])
        back_vel = np.ascontiguousarray(rec["velocity"][gone, :3])
        t_add, _ = ms(lambda: w.add_particles(back_pos, back_vel))
        assert w.n == n
        # ---- the round trip: read, filter, destroy, create, write ----
        def trip(change):
            records = w.read_vec("particles")
            records = change(records)
            w.close()
            fresh = ws.FluidWorker(np.ascontiguousarray(records["position"][:, :3]), params)
            fresh.write_slice("particles", records)
            return fresh, records

        def drain(records):
            owner, _ = P.claims(np.ascontiguousarray(records["position"][:, :3]), ref_sinks)
            drain.lost = records[owner >= 0]
            return records[owner < 0]

        t_trip_remove, (w, _) = ms(lambda: trip(drain))
        assert w.n == n - len(drain.lost)
        t_trip_add, (w, _) = ms(lambda: trip(lambda records: np.concatenate([records, drain.lost])))
        assert w.n == n
        if r:  # (round 0 warms up)
            for key, value in (("remove", t_remove), ("add", t_add), ("trip_remove", t_trip_remove), ("trip_add", t_trip_add)):
                t[key].append(value)
        w.run(2)
        w.sync()
    w.close()
    med = {key: float(np.median(v)) for key, v in t.items()}
    result = {"config": "c3 cloud", "n": n, "sinks": len(sinks), "drained": drained, "repeats": repeats,
              "device_remove_ms": med["remove"], "device_add_ms": med["add"], "device_ms": med["remove"] + med["add"],
              "round_trip_remove_ms": med["trip_remove"], "round_trip_add_ms": med["trip_add"],
              "round_trip_ms": med["trip_remove"] + med["trip_add"], "all_ms": t}
    print("%-28s %12s %12s" % ("%d of %d particles" % (drained, n), "remove ms", "add ms"))
    print("%-28s %12.3f %12.3f" % ("on the device", med["remove"], med["add"]))
    print("%-28s %12.3f %12.3f" % ("read/filter/create/write", med["trip_remove"], med["trip_add"]))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        json.dump(result, open(os.path.join(out_dir, "population_timing.json"), "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
