"""The listed density / force kernels equal the one-thread-per-particle kernels bit for bit at the particle counts where
the launch shape switches: the walk limit of K5's in-step mask walk (4 / 6 / 12 words by tile count), K5's tile size
(64 / 128 particles), the tile schedule's window, a one-particle or partial last tile and a tile count that is not a
multiple of 8.  Every switch is selected silently from n, so each size sits on one side of one of them.

`simple` comes from the developer build's WS_VARIANT hook (the product library has no such switch), `listed` is the
product library as it ships.  Uniform clouds at three densities make both walk forms run under every limit."""
import os

import numpy as np
import pytest

import f64_step as F
from test_gpu_f64_step import gpu_step_check

pytestmark = pytest.mark.gpu

BOTH_ARITHMETICS = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])

# the library's launch constants (csrc/ws_kernels.hip, csrc/ws_api.cpp), restated to name what each size selects
SCHED_MIN, SCHED_END = 1 << 18, 1 << 20  # WS_SCHED_MIN_PARTICLES, WS_SCHED_END_PARTICLES
SMALL_BELOW = 1 << 19  # NF_SMALL_BELOW: K5 tiles of 64 below, 128 from here
TINY_TILES, BIG_TILES = 2048, 16384  # NF_WORDSYNC_TINY_TILES, NF_WORDSYNC_BIG_TILES

SIZES = [131008, 131009, SCHED_MIN - 1, SCHED_MIN, SMALL_BELOW - 1, SMALL_BELOW, SCHED_END - 1, SCHED_END, 2097024, 2097025]

# (mean candidates per particle band, particles per cell): about 3, 9 and 17 accept-mask words of 32 candidates
DENSITIES = {"3w": ((64, 128), 3.5), "9w": ((224, 352), 10.7), "17w": ((480, 640), 22.0)}
FREE_STEPS = 30


def shape(n, ieee, graph=False):
    """(K5 tile, K5 tiles, in-step walk limit in words, tile schedule on) of a single-GPU handle of n particles.  A graph
    handle never takes the schedule (ws_api.cpp: its captured step has no cross-stream schedule launch)."""
    tile = 64 if n < SMALL_BELOW else 128
    tiles = (n + tile - 1) // tile
    sched = SCHED_MIN <= n < SCHED_END and not graph
    if ieee:
        limit = 4
    elif sched:
        limit = 6  # scheduled launches take NF_WORDSYNC_MAX
    else:
        limit = 12 if tiles >= BIG_TILES else 6 if tiles >= TINY_TILES else 4
    return tile, tiles, limit, sched


def test_the_sizes_sit_where_the_table_says():
    """The table of the issue, restated: each pair of sizes straddles one switch; none of them aliases."""
    assert [shape(n, False)[2] for n in (131008, 131009)] == [4, 6]
    assert shape(131009, False)[1] * 64 - 131009 == 63  # a one-particle last tile
    assert [shape(n, False)[3] for n in (SCHED_MIN - 1, SCHED_MIN, SCHED_END - 1, SCHED_END)] == [False, True, True, False]
    assert [shape(n, False)[0] for n in (SMALL_BELOW - 1, SMALL_BELOW)] == [64, 128]
    assert [shape(n, False)[2] for n in (2097024, 2097025)] == [6, 12]
    assert 2097025 % 128 != 0 and shape(2097024, False)[1] % 8 != 0
    assert not any(F.stencil_aliases(n) for n in SIZES)
    assert F.stencil_aliases(15823) and F.stencil_aliases(8)


def _cloud(ws, n, ppc, seed):
    """n particles uniform in a 2:1:1 container whose interior holds `ppc` particles per cell on average."""
    h = 0.25
    vol = n * h ** 3 / ppc
    lo, hi = 0.5, 200.0
    for _ in range(100):
        L = (lo + hi) / 2
        lo, hi = (L, hi) if (2 * L - 0.2) * (L - 0.2) ** 2 < vol else (lo, L)
    params = ws.make_params(container_size=(2 * L, L, L))
    return ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max)), params


def _worker(ws, variant, pos, params, ieee, devlib, graph=False):
    if variant == "listed":
        return ws.FluidWorker(pos, params, ieee_division=ieee, graph=graph)
    os.environ["WS_VARIANT"] = variant
    try:
        return ws.FluidWorker(pos, params, ieee_division=ieee, library=devlib)
    finally:
        os.environ.pop("WS_VARIANT", None)


def _same(a, b, what):
    for f in a.dtype.names:
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), "%s: field %s differs" % (what, f)


def _listed_equals_simple(ws, devlib, n, density, ieee, graph=False):
    band, ppc = DENSITIES[density]
    pos, params = _cloud(ws, n, ppc, 0x5A0 + n % 997)
    cand = F.CellList(pos, params.smoothing_radius).candidates(np.arange(n))
    assert band[0] < cand.mean() <= band[1], (n, density, cand.mean())
    tile, tiles, limit, sched = shape(n, ieee, graph)
    what = "n=%d %s %s tile %d x %d limit %d sched %d%s" % (n, density, "ieee" if ieee else "hw", tile, tiles, limit, sched,
                                                           " graph" if graph else "")
    simple = _worker(ws, "simple", pos, params, ieee, devlib)
    listed = _worker(ws, "listed", pos, params, ieee, devlib, graph)
    try:
        assert listed.stats()["tile_schedule"] == sched, what
        state = listed.read_vec("particles")
        for w in (simple, listed):  # one teacher-forced step from the same records
            w.write_slice("particles", state)
            w.run()
        _same(simple.read_vec("particles"), listed.read_vec("particles"), what + " step 1")
        simple.run(FREE_STEPS)
        listed.run(FREE_STEPS)
        _same(simple.read_vec("particles"), listed.read_vec("particles"), what + " free step %d" % (1 + FREE_STEPS))
        if graph:
            assert listed.stats()["graph_steps"] >= FREE_STEPS - 2
    finally:
        simple.close()
        listed.close()


@BOTH_ARITHMETICS
@pytest.mark.parametrize("density", sorted(DENSITIES))
@pytest.mark.parametrize("n", SIZES)
def test_listed_equals_simple_at_the_switches(ws, devlib, n, density, ieee):
    _listed_equals_simple(ws, devlib, n, density, ieee)


def test_listed_graph_equals_simple_inside_the_schedule_window(ws, devlib):
    """Inside the window a graph handle runs the unscheduled launches (walk limit by tile count) from its capture."""
    _listed_equals_simple(ws, devlib, SCHED_MIN, "9w", False, graph=True)


@BOTH_ARITHMETICS
@pytest.mark.parametrize("n", [131009, 2097025])
def test_per_particle_check_at_the_odd_shapes(ws, n, ieee):
    """Part of the float64 net at the two odd shapes (one-particle last tile; partial last tile): 131 009 every particle,
    2 097 025 the last K5 tile of the sorted order plus a uniform sample of 2^18."""
    pos, params = _cloud(ws, n, DENSITIES["9w"][1], 0x5A0 + n % 997)
    queries = None
    if n > 1 << 20:
        def queries(st):
            keys = F.hash_keys(F.cells_of(st["predicted_position"], params.smoothing_radius), n)
            tail = np.argsort(keys, kind="stable")[-(n % 128):]  # the particles of the partial last tile
            rng = np.random.default_rng(5)
            return np.union1d(tail, rng.choice(n, 1 << 18, replace=False))
    gpu_step_check(ws, pos, params, ieee, "f64 launch shape n=%d 9w" % n, queries=queries)
