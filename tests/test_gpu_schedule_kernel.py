"""k_schedule on tile costs the TEST chooses (csrc/ws_kernels.hip "tile schedule"; the developer build's ws_dev_* hooks,
tests/schedule_dev.py).  In a step the kernel sees whatever the clock measured -- smooth costs, cuts near the equal
shares -- so its clamps, its equal-share branch, its fill of unmeasured tiles, ranges that are empty and groups that
straddle a cut are reached here: the kernel against tests/schedule_ref.py word for word, and the scheduled K4 / K5
under planted schedules against an unscheduled handle, with every tile shown to have run."""
import os

import numpy as np
import pytest

import schedule_dev as D
import schedule_ref as R

pytestmark = pytest.mark.gpu

UNWRITTEN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def handle(ws, devlib):
    """A C1-sized handle to run k_schedule on: the tile counts of ws_dev_schedule have nothing to do with its n."""
    D.bind(devlib)
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    yield w
    w.close()


@pytest.fixture(scope="module")
def expected():
    """(shape, T, G, nclasses) -> (cost, split, perm) of the restatement; each computed once."""
    cut_of, full = {}, {}

    def get(name, T, G, k):
        if (name, T) not in cut_of:
            cost = R.SHAPES[name](T)
            cut_of[name, T] = (cost, R.cuts(cost))
        if (name, T, G, k) not in full:
            cost, c = cut_of[name, T]
            full[name, T, G, k] = (cost, c.split, R.order(c, k, G))
        return full[name, T, G, k]

    return get


def assert_same(what, T, split, perm, want_split, want_perm):
    R.check_schedule(split, perm, T)  # names the fault, and does not depend on the restatement
    assert split.tolist() == want_split, (what, split.tolist(), want_split)
    if not np.array_equal(perm, want_perm):
        at = int(np.flatnonzero(perm != want_perm)[0])
        raise AssertionError("%s: perm differs first at %d: kernel %s, restatement %s" % (what, at, perm[at:at + 8], want_perm[at:at + 8]))


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_kernel_equals_the_restatement_word_for_word(handle, expected, shape):
    """Every tile count with every grouping and class count.  One launch schedules two kernels: its K4 half gets one tile
    count and its K5 half the next one of the list, so every case runs in both halves, beside a half of another size."""
    small = list(R.TILE_COUNTS)
    runs = [(T, small[(i + 1) % len(small)], G, k) for G, k in R.groupings(small[0]) for i, T in enumerate(small)]
    big = list(R.BIG_TILE_COUNTS)
    runs += [(T, big[(i + 1) % len(big)], 1, 8) for i, T in enumerate(big)]
    for T4, T5, G, k in runs:
        cost4, want_split4, want_perm4 = expected(shape, T4, G, k)
        cost5, want_split5, want_perm5 = expected(shape, T5, G, k)
        split4, perm4, split5, perm5 = D.run_schedule(handle, cost4, cost5, k, G)
        assert_same("%s T=%d G=%d classes=%d (K4 half, beside T=%d)" % (shape, T4, G, k, T5), T4, split4, perm4, want_split4, want_perm4)
        assert_same("%s T=%d G=%d classes=%d (K5 half, beside T=%d)" % (shape, T5, G, k, T4), T5, split5, perm5, want_split5, want_perm5)


def test_a_half_without_tiles_returns_at_once_and_the_class_count_is_clamped(handle, expected):
    cost, want_split, want_perm = expected("lognormal", 313, 3, 8)
    none = np.zeros(0, np.uint32)
    split4, perm4, split5, perm5 = D.run_schedule(handle, cost, none, 8, 3)
    assert_same("K4 half alone", 313, split4, perm4, want_split, want_perm)
    assert (split5 == UNWRITTEN).all()
    split4, perm4, split5, perm5 = D.run_schedule(handle, none, cost, 99, 3)  # (more classes than the kernel has: 8)
    assert_same("K5 half alone", 313, split5, perm5, want_split, want_perm)
    assert (split4 == UNWRITTEN).all()
    split4, perm4, split5, perm5 = D.run_schedule(handle, cost, cost, 0, 3)  # (no class: one)
    assert_same("one class", 313, split4, perm4, want_split, np.arange(313, dtype=np.uint32))
    assert np.array_equal(perm5, perm4) and np.array_equal(split5, split4)


def scheduled(ws, devlib, pos, params, on, ieee):
    os.environ["WS_TILE_SCHEDULE"] = "1" if on else "0"
    try:
        return ws.FluidWorker(pos, params, ieee_division=ieee, library=devlib)
    finally:
        os.environ.pop("WS_TILE_SCHEDULE", None)


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
@pytest.mark.parametrize("n", [500, 1000, 4096, 20011])
def test_the_consumers_run_every_tile_of_a_planted_schedule(ws, devlib, n, ieee):
    """8, 16, 64 and 313 K4 tiles (empty ranges; nmin = 1; a partial last tile).  Before each of five steps a cost array
    is planted (K5 gets it reversed, so the two kernels are cut differently); after each, every tile of both kernels
    has written a cost -- it ran -- and every field equals an unscheduled handle's, bit for bit."""
    D.bind(devlib)
    mn, mx = ws.get_ext((0, 0, 0), (6.0, 4.0, 4.0), 0.1)
    pos = ws.workloads.uniform_cloud(n, 99, mn, mx)
    params = ws.make_params(container_size=(6.0, 4.0, 4.0))
    on, off = scheduled(ws, devlib, pos, params, True, ieee), scheduled(ws, devlib, pos, params, False, ieee)
    try:
        t4, t5 = D.tile_counts(on)
        assert t4 == (n + 63) // 64
        # reach: the arrays about to be planted put a range on either clamp, for K4 and for K5
        for T, flip in ((t4, False), (t5, True)):
            nmin, nmax = R.limits(T)
            seen = set()
            for kind in R.PLANTED:
                split = R.cuts(R.planted(kind, T)[::-1] if flip else R.planted(kind, T)).split
                seen |= {split[x + 1] - split[x] for x in range(8)}
            assert nmin in seen and nmax in seen, (T, flip, sorted(seen))
        on.run(3)
        off.run(3)
        for kind in R.PLANTED:
            D.plant(on, R.planted(kind, t4), R.planted(kind, t5)[::-1])
            on.run(1)
            off.run(1)
            cost4, cost5 = D.read_tile_costs(on)
            assert cost4.min() >= 1, (kind, "K4 never ran tiles", np.flatnonzero(cost4 == 0)[:8])
            assert cost5.min() >= 1, (kind, "K5 never ran tiles", np.flatnonzero(cost5 == 0)[:8])
            assert max(cost4.max(), cost5.max()) <= R.COST_CLAMP
            assert on.stats()["tile_schedule"] and not off.stats()["tile_schedule"]
            a, b = on.read_vec("particles"), off.read_vec("particles")
            for f in a.dtype.names:
                assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (kind, f)
    finally:
        on.close()
        off.close()
