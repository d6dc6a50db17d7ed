"""K4's phase 1 keeps each lane's list position as a running LDS address, walks a run in trip loops of their own, votes on
the scalar unit and finds a mask-word crossing in the carry of one add.  (Two more parts -- pushing and marking under the
accept mask, and trips without validity tests while every lane has four candidates left -- live as patches: HISTORY.md
round 7.  The cases below are chosen for them too.)  None of that may change a bit: the product library equals the
developer build's one-thread-per-particle kernels (WS_VARIANT=simple) in the densities and near densities of a
teacher-forced step, in the records after 3 steps and in the overflow counter, in both arithmetics, on the smallest
inputs at which the code can go wrong:

 lattice   1 000 particles (16 waves, 24 shadow lanes in the last) on a lattice of spacing h / 4: accepted candidates come in
           rows, so lists stand at 13, 14, 15 and 16 entries when a trip brings four more (slots up to 18), and the
           lists are emptied in the middle of runs;
 sparse    4 096 particles at the reference's density: runs of 0 to 5 candidates, every trip ends a run, and few waves
           take the wave-uniform walk at all;
 column    4 096 particles in a column two cells wide: runs of 40 to 70 candidates, many trips of four in a row, and the
           mask-word crossings (position 28 to 31 in the word) fall inside them;
 one cell  2 112 particles in one cell: more candidates than the 2 048 a mask holds, row 63 fills and the walk goes on;
 slabs     two slabs (loopback transport) of a cloud: the instantiation that cuts its runs at the slab's range;
 schedule  262 144 particles, 2 steps: the instantiation that takes its tiles from the schedule.

`simple` comes from the developer build's WS_VARIANT hook, `listed` is the product library as it ships."""
import os

import numpy as np
import pytest

import f64_step as F
from test_gpu_launch_shapes import _cloud, _same, _worker

BOTH_ARITHMETICS = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])

H = np.float32(0.25)  # the smoothing radius of every case (make_params' default)
MASK_CANDIDATES = 2048  # 32 * ND_MASK_WORDS
LIST_FLUSH = 16  # ND_K
REFERENCE_PER_CELL = 65536 * 0.25 ** 3 / (16.0 * 9.0 * 9.0)  # the reference's 65 536 particles in its 16 x 9 x 9 container
SCHED_N = 1 << 18


def lattice(ws):
    """10 x 10 x 10 points h / 4 apart, none on a cell face, in the middle of a small container."""
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    k = (np.arange(10, dtype=np.float32) + np.float32(0.5)) * (H / 4)
    pos = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    return pos[np.random.default_rng(0x1A7).permutation(len(pos))], params


def sparse(ws):
    return _cloud(ws, 4096, REFERENCE_PER_CELL, 0x4B4)


def column(ws):
    """Uniform in 2 x 2 x 57 cells: 18 particles per cell, 54 per run of three cells."""
    params = ws.make_params(container_size=(4.0, 4.0, 16.0))
    rng = np.random.default_rng(0xC01)
    pos = rng.uniform((0.0, 0.0, -28 * 0.25), (0.5, 0.5, 29 * 0.25), (4096, 3)).astype(np.float32)
    return pos, params


def one_cell(ws):
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(0x0CE)
    return (rng.uniform(0.2, 0.8, (2112, 3)) * H).astype(np.float32), params


def slabs(ws):
    return _cloud(ws, 4096, 14.0, 0x51B)


def schedule(ws):
    return _cloud(ws, SCHED_N, 10.7, 0x5C4)


CASES = {"lattice": lattice, "sparse": sparse, "column": column, "one_cell": one_cell}


def runs(pos):
    """Per particle, the candidates of its nine runs (one per (dx, dy): three cells along z), shape (n, 9)."""
    cell = F.cells_of(pos, H)
    c = cell - cell.min(axis=0) + 2
    dims = c.max(axis=0) + 3
    count = np.zeros(dims, np.int64)
    np.add.at(count, (c[:, 0], c[:, 1], c[:, 2]), 1)
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            out.append(sum(count[c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz] for dz in (-1, 0, 1)))
    return np.stack(out, axis=1)


def test_the_inputs_are_what_the_cases_say(ws):
    """Host side only."""
    for make in list(CASES.values()) + [slabs]:
        pos, params = make(ws)
        assert np.float32(params.smoothing_radius) == H and not F.stencil_aliases(len(pos))
        lo, hi = np.array(list(params.ext_min)[:3]), np.array(list(params.ext_max)[:3])
        assert np.all(pos > lo) and np.all(pos < hi)
    pos, _ = lattice(ws)
    assert len(pos) == 1000 and len(pos) % 64 == 40
    d2 = ((pos[:, None, :].astype(np.float64) - pos[None, :, :]) ** 2).sum(axis=2)
    accepted = (d2 <= float(F.accept(H))).sum(axis=1)
    assert accepted.min() > 3 * LIST_FLUSH  # every list is emptied several times, in the middle of runs
    # along z (the order inside a run) the accepted candidates of an inner particle come 4 to 9 in a row: a list that
    # stands at 13, 14, 15 or 16 entries takes four more in its next trip
    assert runs(pos).max() >= 120 and accepted.max() >= 250
    r = runs(sparse(ws)[0])
    assert r.min() == 0 and np.percentile(r, 90) <= 5 and r.max() < 16
    r = runs(column(ws)[0])
    assert np.all((r > 0).sum(axis=1) == 4)  # two cells wide: four runs per particle
    assert 40 <= np.percentile(r[r > 0], 10) and np.percentile(r[r > 0], 95) <= 70
    pos, _ = one_cell(ws)
    assert len(np.unique(F.cells_of(pos, H), axis=0)) == 1 and len(pos) > MASK_CANDIDATES + 63
    assert F.CellList(pos, H).candidates(np.arange(len(pos))).min() == 2112


def step_and_compare(ws, devlib, pos, params, ieee, what, free_steps):
    simple = _worker(ws, "simple", pos, params, ieee, devlib)
    listed = _worker(ws, "listed", pos, params, ieee, devlib)
    try:
        state = listed.read_vec("particles")
        for w in (simple, listed):  # one teacher-forced step from the same records: densities and near densities
            w.write_slice("particles", state)
            w.run()
        got = listed.read_vec("particles")
        overflow = listed.stats()["mask_overflow"]
        sched = listed.stats()["tile_schedule"]
        _same(simple.read_vec("particles"), got, what + " step 1")
        simple.run(free_steps)
        listed.run(free_steps)
        _same(simple.read_vec("particles"), listed.read_vec("particles"), what + " free step %d" % (1 + free_steps))
        return overflow, sched
    finally:
        simple.close()
        listed.close()


@pytest.mark.gpu
@BOTH_ARITHMETICS
@pytest.mark.parametrize("name", sorted(CASES))
def test_listed_equals_simple(ws, devlib, name, ieee):
    pos, params = CASES[name](ws)
    overflow, sched = step_and_compare(ws, devlib, pos, params, ieee, "%s %s" % (name, "ieee" if ieee else "hw"), 2)
    cand = F.CellList(pos, H).candidates(np.arange(len(pos)))
    assert overflow == int((cand > MASK_CANDIDATES).sum()) and not sched
    assert (overflow > 0) == (name == "one_cell")


@pytest.mark.gpu
@BOTH_ARITHMETICS
def test_listed_equals_simple_on_two_slabs(ws, devlib, ieee):
    pos, params = slabs(ws)
    got, owned = ws.slab.run_loopback(pos, params, 2, 3, ieee_division=ieee)
    assert sum(owned) == len(pos) and min(owned) > 64
    os.environ["WS_VARIANT"] = "simple"
    try:
        want, _ = ws.slab.run_loopback(pos, params, 2, 3, ieee_division=ieee, library=devlib)
    finally:
        os.environ.pop("WS_VARIANT", None)
    _same(want, got, "two slabs %s" % ("ieee" if ieee else "hw"))


@pytest.mark.gpu
@BOTH_ARITHMETICS
def test_listed_equals_simple_under_the_tile_schedule(ws, devlib, ieee):
    pos, params = schedule(ws)
    overflow, sched = step_and_compare(ws, devlib, pos, params, ieee, "schedule %s" % ("ieee" if ieee else "hw"), 1)
    assert sched and overflow == 0
