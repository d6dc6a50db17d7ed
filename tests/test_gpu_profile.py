"""Handles created with WS_FLAG_PROFILE: the instrument bench.py and every A/B tool measure with.

A profiled handle does not take the path the rest of the suite steps (csrc/ws_api.cpp "profiling", csrc/ws_kernels.hip
WS_LAUNCH): scan, place / scatter, reorder and the stand-alone binning sit between two recorded events (struct Prof),
K4 and K5 -- in every form: simple, listed, early / late, scheduled, 64- and 128-particle tiles -- are launched by
hipExtLaunchKernelGGL with a start / stop event pair (struct ProfLaunch), a split slab step times them as early + late and
counts them once, ws_step drains the pending pairs behind a stream synchronise once there are 4096 of them, and the
field calls drain them too.  Three things are held here:

  A  the profiled step is the same step: ws_read_particles records equal an unprofiled twin's as uint32;
  B  launch counts are exact.  The rule, as the code has it: every ws_step adds ONE launch to each of cell_scan,
     cell_scatter, reorder, density and force_integrate_bin whose bit is set in the ws_profile_select mask AT THE MOMENT
     THE STEP IS ENQUEUED, also when the step is split; `bin` counts the stand-alone binning of ws_create, ws_reset,
     ws_write_particles and a re-gridding ws_set_params (single handles: a slab handle bins inside its first step,
     unbracketed); nothing else counts anything; a WS_FLAG_GRAPH handle records nothing.  Every expected count below is
     computed from what the test asked the handle to do;
  C  times that need no measured number: all timed intervals lie on one in-order stream between a host clock read taken
     after ws_sync and one taken after the closing ws_sync, so they are disjoint and inside that window: their sum, and
     each of them, is at most the window's wall time, every counted kernel has time, and totals accumulate.

The only slack of C is the granularity of a timestamp: a pair's elapsed time is the difference of two readings of the
device's constant-rate clock, each quantised to one tick, so a pair over-reads by less than ONE tick.  The tick is
read from the device (hipDeviceAttributeWallClockRate, in kHz): 100 MHz on an MI355X, 10 ns -- written here, asserted
below, and nothing is added to it."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from test_gpu_launch_shapes import DENSITIES, SCHED_MIN, SMALL_BELOW, _cloud, _same

pytestmark = pytest.mark.gpu

BOTH_ARITHMETICS = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
STEP_KERNELS = ("cell_scan", "cell_scatter", "reorder", "density", "force_integrate_bin")
SCAN, SCATTER, REORDER, K4, K5, BIN = (1 << k for k in range(6))  # ws_profile_select bits = 1 << WS_K_*
ALL = 0xFFFFFFFF
WALL_CLOCK_KHZ = 100000  # the MI355X's constant-rate clock: one tick = 10 ns
HIP_DEVICE_ATTRIBUTE_WALL_CLOCK_RATE = 10017  # hip_runtime_api.h: hipDeviceAttributeAmdSpecificBegin + 17
PENDING_DRAIN = 4096  # bound_pending (csrc/ws_api.cpp): pairs pending before ws_step synchronises and reads them


@pytest.fixture(scope="module")
def tick_ms(ws):
    """One tick of the clock the event timestamps are readings of, in milliseconds, from the device."""
    ws.load_library()  # (the HIP runtime is in the process from here on: the very copy the library calls)
    with open("/proc/self/maps") as maps:
        loaded = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    khz = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(khz), HIP_DEVICE_ATTRIBUTE_WALL_CLOCK_RATE, 0) == 0
    assert khz.value == WALL_CLOCK_KHZ, khz.value
    return 1.0 / khz.value


def _counts(profile):
    return {k: n for k, (_, n) in profile.items()}


def _stepped(k, mask=ALL):
    """What k steps under `mask` must have counted."""
    bits = dict(zip(STEP_KERNELS, (SCAN, SCATTER, REORDER, K4, K5)))
    return dict({name: k if mask & bit else 0 for name, bit in bits.items()}, bin=0)


def _window(w, steps):
    """`steps` steps in one run() between two host clock reads, each taken after a ws_sync (ws_profile_reset waits like
    ws_sync): (profile of the window, its wall time in ms)."""
    w.profile_reset()
    w.sync()
    t0 = time.perf_counter_ns()
    w.run(steps)
    w.sync()
    t1 = time.perf_counter_ns()
    return w.profile(), (t1 - t0) * 1e-6


def _assert_times(profile, wall_ms, tick_ms, what, split=False):
    """C: each counted kernel has time and at most the window's; the sum of all is at most the window's.  Slack: one
    tick per pair, and a counted launch is one pair -- but for K4 and K5 of a split slab step, which are two."""
    pairs = 0
    for name, (ms, n) in profile.items():
        print("PROFILE %s %s: %.6f ms in %d launches, window %.6f ms" % (what, name, ms, n, wall_ms))
        if n == 0:
            assert ms == 0.0, (what, name, ms)
            continue
        own = n * (2 if split and name in ("density", "force_integrate_bin") else 1)
        pairs += own
        assert 0.0 < ms <= wall_ms + own * tick_ms, "%s: %s %.6f ms in a window of %.6f ms" % (what, name, ms, wall_ms)
    total = sum(ms for ms, _ in profile.values())
    assert total <= wall_ms + pairs * tick_ms, "%s: the kernels sum to %.6f ms in a window of %.6f ms" % (what, total, wall_ms)


def _twins(ws, pos, params, steps, tick_ms, what, mask=ALL, library=None, env=None, **kw):
    """A: `steps` steps on an unprofiled handle and on a profiled twin, each in one run() with no host synchronisation in
    between; records equal as uint32.  B and C of the profiled window on the way.  Returns the profiled handle's stats."""
    def make(profile):
        os.environ.update(env or {})
        try:
            return ws.FluidWorker(pos, params, profile=profile, library=library, **kw)
        finally:
            for k in env or {}:
                os.environ.pop(k, None)

    plain, prof = make(False), make(True)
    try:
        plain.run(steps)
        want = plain.read_vec("particles")
        assert _counts(plain.profile()) == dict(_stepped(0)), what  # (an unprofiled handle records nothing)
        prof.profile_select(mask)
        profile, wall = _window(prof, steps)
        _same(prof.read_vec("particles"), want, what)
        assert _counts(profile) == _stepped(steps, mask), what
        assert profile == prof.profile(), what  # (the unprofiled force pass of ws_read_particles counted nothing)
        _assert_times(profile, wall, tick_ms, what)
        return prof.stats(), plain.stats()
    finally:
        plain.close()
        prof.close()


# ---- A. the profiled step is the same step ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    assert pos.shape[0] == 4096
    return pos, params


@BOTH_ARITHMETICS
def test_small_cloud_long_run(ws, c1, tick_ms, ieee):
    """1000 steps in one run(): five pairs a step, so ws_step drains behind a synchronise once (after step 820) and the
    pooled events are used again and again.  No pair may be lost at the drain: 1000 launches of each."""
    assert 5 * 819 < PENDING_DRAIN <= 5 * 820 < 5 * 1000 < 2 * PENDING_DRAIN
    _twins(ws, *c1, 1000, tick_ms, "c1 1000 steps", ieee_division=ieee)


@BOTH_ARITHMETICS
@pytest.mark.parametrize("mask", [K4 | K5, 0], ids=["mask-k4-k5", "mask-0"])
def test_small_cloud_under_the_benchmarks_mask_and_under_none(ws, c1, tick_ms, ieee, mask):
    """K4 | K5 is what bench.py's timed windows select: the brackets are off, the two event-carrying launches on."""
    _twins(ws, *c1, 20, tick_ms, "c1 20 steps mask %#x" % mask, mask=mask, ieee_division=ieee)


@pytest.mark.parametrize("n,ieee", [(SMALL_BELOW - 1, False), (SMALL_BELOW - 1, True), (SMALL_BELOW, False)],
                         ids=["2^19-1-hw", "2^19-1-ieee", "2^19-hw"])
def test_k5_tile_sizes_under_the_event_carrying_launch(ws, tick_ms, n, ieee):
    """K5 in tiles of 64 below NF_SMALL_BELOW and of 128 from there (and the walk limits that go with them), both inside
    the tile schedule's window: the scheduled listed kernels through the event-carrying launch."""
    pos, params = _cloud(ws, n, DENSITIES["9w"][1], 0x5A0 + n % 997)
    stats, _ = _twins(ws, pos, params, 5, tick_ms, "n=%d 9w" % n, ieee_division=ieee)
    assert stats["tile_schedule"]


def test_the_tile_schedule_on_the_product_library(ws, tick_ms):
    """2^18 particles: the first size on the schedule.  k_schedule runs on a stream of its own between K4 and K5, and its
    two events sit beside the launch's own."""
    pos, params = _cloud(ws, SCHED_MIN, DENSITIES["9w"][1], 0x5A0 + SCHED_MIN % 997)
    stats, plain = _twins(ws, pos, params, 12, tick_ms, "n=2^18 scheduled")
    assert stats["tile_schedule"] and plain["tile_schedule"]


def test_the_tile_schedule_forced_on_at_a_small_size(ws, devlib, tick_ms):
    """The developer library's WS_TILE_SCHEDULE=1 at 16 384 particles (one K5 tile count far below the window's)."""
    params = ws.make_params(container_size=(6.0, 4.0, 3.0))
    pos = ws.workloads.uniform_cloud(16384, 21, list(params.ext_min), list(params.ext_max))
    stats, plain = _twins(ws, pos, params, 12, tick_ms, "n=16384 forced schedule", library=devlib, env={"WS_TILE_SCHEDULE": "1"})
    assert stats["tile_schedule"] and plain["tile_schedule"]


def test_the_one_thread_per_particle_kernels(ws, devlib, c1, tick_ms):
    """k_density_simple / k_force_simple<false>: the developer library's WS_VARIANT=simple."""
    _twins(ws, *c1, 20, tick_ms, "c1 simple", library=devlib, env={"WS_VARIANT": "simple"})


def test_the_hash_aliasing_kernels(ws, tick_ms):
    """n = 8 (tests/test_gpu_edge.py test_tiny_n_hash_aliasing): cells of one stencil share a bucket of the reference's
    table, and the handle runs k_density_simple / k_force_simple<true>."""
    _twins(ws, ws.cube_fluid(2, 2, 2), ws.make_params(container_size=(4.0, 4.0, 4.0)), 20, tick_ms, "n=8 aliasing")


def test_a_captured_handle_records_nothing(ws, c1):
    """graph=True, profile=True: WS_FLAG_GRAPH clears the flag (event brackets are not part of a captured step).  Same
    bits, the steps are replays, and the profile is all zeros -- also for the stand-alone binning of its creation."""
    pos, params = c1
    plain, g = ws.FluidWorker(pos, params), ws.FluidWorker(pos, params, graph=True, profile=True)
    try:
        plain.run(30)
        g.run(30)
        _same(g.read_vec("particles"), plain.read_vec("particles"), "c1 captured and profiled")
        assert g.stats()["graph_steps"] > 0
        assert g.profile() == {name: (0.0, 0) for name in ws.fluid.KERNEL_IDS}
    finally:
        plain.close()
        g.close()


# ---- slabs -------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 40
SLAB_MODES = {"exact": {}, "lagged": dict(lagged_messages=True), "no-overlap": dict(overlap=False)}


@pytest.fixture(scope="module")
def slab_scene(ws):
    """tests/test_gpu_slab_exact.py's: 65 536 particles, gravity with an x component, so particles change owner; and what
    the single unprofiled handle holds after SLAB_STEPS steps."""
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    w = ws.FluidWorker(pos, params)
    w.run(SLAB_STEPS)
    want = w.read_vec("particles")
    w.close()
    return pos, params, want


def _slab_program(steps):
    def program(w, rank):
        loaded = w.profile()
        w.sync()
        t0 = time.perf_counter_ns()
        w.run(steps)
        w.sync()
        t1 = time.perf_counter_ns()
        profile = w.profile()
        rec, ids = w.read()
        return rec, ids, loaded, profile, w.profile(), (t1 - t0) * 1e-6, w.counters()["left"]
    return program


@pytest.mark.parametrize("mode", sorted(SLAB_MODES))
@pytest.mark.parametrize("world", [2, 3])
def test_profiled_slabs_equal_the_single_handle(ws, slab_scene, tick_ms, world, mode):
    """Profiled on every rank.  With exact message sizes (the default) the early range of K4 is launched BEFORE the host
    waits for the sizes, so the pair made for it afterwards is taken by no launch and must go back to the pool unread;
    lagged sizes launch it after; without overlap nothing is split.

    What makes a step split (csrc/ws_slab.inc): world >= 2, overlap on, and every rank at least three owned cell layers
    thick -- 16 / 0.25 = 64 layers over two or three ranks here.  A split step runs K4 and K5 as an early and a late
    launch each, and must count ONE density and ONE force_integrate_bin: SLAB_STEPS of each, not twice that."""
    pos, params, want = slab_scene
    res = ws.slab.run_loopback_program(pos, params, world, _slab_program(SLAB_STEPS), profile=True, **SLAB_MODES[mode])
    got = np.zeros_like(want)
    for rank, (rec, ids, loaded, profile, again, wall, left) in enumerate(res):
        what = "%d slabs %s rank %d" % (world, mode, rank)
        got[ids] = rec
        assert _counts(loaded) == _stepped(0), what  # (a slab handle bins inside its first step, unbracketed)
        assert _counts(profile) == _stepped(SLAB_STEPS), what
        assert again == profile, what  # (ws_slab_read_particles in between counted nothing)
        _assert_times(profile, wall, tick_ms, what, split=mode != "no-overlap")
    assert sum(len(r[1]) for r in res) == len(want) and sum(r[6] for r in res) > 0  # (particles did change owner)
    _same(got, want, "%d slabs %s" % (world, mode))


@pytest.mark.parametrize("world,kw", [(1, {}), (2, {}), (2, dict(overlap=False)), (3, dict(lagged_messages=True))],
                         ids=["world-1", "world-2-split", "world-2-no-overlap", "world-3-split-lagged"])
def test_slab_launch_counts_step_by_step(ws, slab_scene, tick_ms, world, kw):
    """The first step after a load fills cell cursors with k_scatter in place of k_place and counts ONE cell_scatter like
    any other; then k steps count k of everything, whether the step is split (world >= 2, overlap on, every rank >= 3
    layers: "split" in the ids), not split with overlap off, or a world of one."""
    pos, params, _ = slab_scene

    def program(w, rank):
        out = []
        for k in (1, 6):
            w.profile_reset()
            w.sync()
            t0 = time.perf_counter_ns()
            w.run(k)
            w.sync()
            out.append((k, w.profile(), (time.perf_counter_ns() - t0) * 1e-6))
        w.run(3)  # no reset: totals accumulate
        out.append((9, w.profile(), None))
        return out

    for rank, out in enumerate(ws.slab.run_loopback_program(pos, params, world, program, profile=True, **kw)):
        for k, profile, wall in out:
            what = "%d slabs %r rank %d, %d steps" % (world, kw, rank, k)
            assert _counts(profile) == _stepped(k), what
            if wall is not None:
                _assert_times(profile, wall, tick_ms, what, split=world > 1 and kw.get("overlap", True))
        for name in STEP_KERNELS:
            assert out[2][1][name][0] > out[1][1][name][0] > 0.0, (rank, name)


# ---- B. launch counts ------------------------------------------------------------------------------------------------------
def test_bin_counts_the_stand_alone_binnings(ws, c1):
    pos, params = c1
    w = ws.FluidWorker(pos, params, profile=True)
    try:
        want = dict(_stepped(0), bin=1)  # ws_create
        assert _counts(w.profile()) == want and w.profile()["bin"][0] > 0.0
        w.reset(pos)
        want["bin"] += 1
        assert _counts(w.profile()) == want
        w.run(2)
        rec = w.read_vec("particles")
        w.write_slice("particles", rec)
        want = dict(_stepped(2), bin=3)
        assert _counts(w.profile()) == want
        w.set_params(ws.make_params(container_size=(16.0, 18.0, 0.2), gravity=(3.0, -9.8, 0.0, 0.0)))  # no re-grid
        assert _counts(w.profile()) == want
        w.set_params(ws.make_params(container_size=(16.0, 18.0, 0.2), gravity=(3.0, -9.8, 0.0, 0.0), smoothing_radius=0.2))
        want["bin"] += 1
        assert _counts(w.profile()) == want
        w.set_params(w.params)  # the same again: nothing
        w.run(3)
        assert _counts(w.profile()) == dict(_stepped(5), bin=4)
        first = w.profile()
        assert first == w.profile()  # reading twice without stepping
        w.profile_reset()
        assert w.profile() == {name: (0.0, 0) for name in ws.fluid.KERNEL_IDS}
    finally:
        w.close()


def test_reads_and_field_calls_between_steps_count_nothing(ws, c1, tick_ms):
    """ws_read_particles runs the force kernel once more, unprofiled (refresh_accel); ws_sample_density_points and
    ws_extract_surface drain the pending pairs (drain_profile) behind their own synchronise.  k steps stay k launches,
    and the totals of the first steps stay what they were."""
    pos, params = c1
    w = ws.FluidWorker(pos, params, profile=True)
    try:
        w.profile_reset()
        w.run(4)
        w.read_vec("particles")
        assert _counts(w.profile()) == _stepped(4)
        w.run(3)
        rho = w.sample_density_points(pos[:65])
        assert rho.shape == (65,) and _counts(w.profile()) == _stepped(7)
        before = w.profile()
        h = params.smoothing_radius
        origin = np.asarray(params.ext_min[:3], np.float32) - np.float32(1.25 * h)
        dims = tuple(int(x) for x in np.ceil((np.asarray(params.ext_max[:3]) - origin + 1.25 * h) / (h / 2)) + 1)
        mesh = w.extract_surface(origin, np.full(3, h / 2, np.float32), dims, np.float32(0.1 * rho.max()))
        assert len(mesh[2]) > 0 and w.profile() == before
        w.run(2)
        w.read_positions()
        w.run(1)
        after = w.profile()
        assert _counts(after) == _stepped(10)
        assert all(after[name][0] > before[name][0] > 0.0 for name in STEP_KERNELS)
    finally:
        w.close()


def test_the_mask_of_the_moment_a_step_is_enqueued(ws, c1):
    """Under a mask, kernels whose bit is clear stay at (0.0, 0).  Changing the mask while steps are in flight -- no
    synchronise between the run() calls -- attributes every pair to the kernel it was recorded for."""
    pos, params = c1
    w = ws.FluidWorker(pos, params, profile=True)
    try:
        w.profile_select(K4 | K5)
        w.profile_reset()
        w.run(5)
        p = w.profile()
        assert _counts(p) == _stepped(5, K4 | K5)
        assert all(p[name] == (0.0, 0) for name in ("cell_scan", "cell_scatter", "reorder", "bin"))
        w.profile_reset()
        plan = [(ALL, 3), (K4, 4), (0, 2), (SCAN | K5, 5)]
        want = _stepped(0)
        for mask, k in plan:
            w.profile_select(mask)
            w.run(k)
            want = {name: want[name] + n for name, n in _stepped(k, mask).items()}
        assert want == dict(cell_scan=8, cell_scatter=3, reorder=3, density=7, force_integrate_bin=8, bin=0)
        p = w.profile()
        assert _counts(p) == want and all((ms > 0.0) == (n > 0) for ms, n in p.values())
        w.profile_select(BIN)  # `bin` has a bit like the others
        w.profile_reset()
        w.reset(pos)
        w.run(2)
        assert _counts(w.profile()) == dict(_stepped(0), bin=1)
    finally:
        w.close()


def test_profile_read_arguments(ws, c1):
    pos, params = c1
    lib, invalid = ws.load_library(), 1  # WS_ERR_INVALID_ARG
    w = ws.FluidWorker(pos, params, profile=True)
    try:
        w.run(2)
        ms, cnt = C.c_double(-1.0), C.c_uint64(77)
        for k in (6, 7, 0xFFFFFFFF):  # WS_K_COUNT and beyond
            assert lib.ws_profile_read(w._h, k, C.byref(ms), C.byref(cnt)) == invalid
        assert lib.ws_profile_read(None, 0, C.byref(ms), C.byref(cnt)) == invalid
        assert (ms.value, cnt.value) == (-1.0, 77)  # a refused call writes nothing
        for k in range(6):
            assert lib.ws_profile_read(w._h, k, None, None) == 0
            assert lib.ws_profile_read(w._h, k, C.byref(ms), None) == 0
            assert lib.ws_profile_read(w._h, k, None, C.byref(cnt)) == 0
            assert (ms.value, cnt.value) == w.profile()[lib.ws_kernel_name(k).decode()]
    finally:
        w.close()


# ---- C. times ----------------------------------------------------------------------------------------------------------------
def test_totals_accumulate_and_stay_inside_the_window(ws, c1, tick_ms):
    """run(10), read, run(10) without a reset: every counted kernel's total strictly increases; the totals of both stay
    inside the host's window around them."""
    pos, params = c1
    w = ws.FluidWorker(pos, params, profile=True)
    try:
        w.run(5)
        first, wall = _window(w, 10)
        t0 = time.perf_counter_ns()
        w.run(10)
        w.sync()
        wall += (time.perf_counter_ns() - t0) * 1e-6
        second = w.profile()
        assert _counts(first) == _stepped(10) and _counts(second) == _stepped(20)
        for name in STEP_KERNELS:
            assert second[name][0] > first[name][0] > 0.0, name
        assert second["bin"] == (0.0, 0)
        _assert_times(first, wall, tick_ms, "c1 first 10 of 20")
        _assert_times(second, wall, tick_ms, "c1 20 steps in two windows")
    finally:
        w.close()
