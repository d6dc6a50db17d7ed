"""tests/schedule_ref.py -- the plain restatement of k_schedule the GPU test compares the kernel with -- checked on its
own: its invariants over the whole input matrix, known answers worked by hand from the kernel's text, that the matrix
reaches the clamps and branches it was chosen for, and that the invariant checker can fail."""
import numpy as np
import pytest

import schedule_ref as R


@pytest.fixture(scope="module")
def cases():
    """[(T, shape, cost, Cuts)] over the matrix: computed once, read by every test."""
    return [(T, name, cost, R.cuts(cost)) for T, name, cost in R.matrix()]


def lengths(split):
    return [split[x + 1] - split[x] for x in range(8)]


def test_invariants_hold_over_the_matrix(cases):
    for T, name, cost, c in cases:
        for G, k in R.groupings(T):
            R.check_schedule(c.split, R.order(c, k, G), T)


def test_invariants_hold_on_seeded_random_costs():
    rng = np.random.default_rng(7)
    for _ in range(300):
        T = int(rng.integers(1, 3000))
        cost = rng.integers(0, R.COST_CLAMP + 1, T, dtype=np.uint32) >> rng.integers(0, 25, T, dtype=np.uint32)
        split, perm = R.schedule(cost, int(rng.integers(1, 9)), int(rng.integers(1, 20)))
        R.check_schedule(split, perm, T)


# ---- known answers, each worked by hand from the text of k_schedule (not read off the restatement)
def test_sixteen_equal_small_costs_take_the_equal_shares():
    """Costs below 2^10 scale to 0, total_s = 0 < 8: cuts T k / 8; one class value per range, so perm is the identity."""
    split, perm = R.schedule([1] * 16)
    assert split == [0, 2, 4, 6, 8, 10, 12, 14, 16]
    assert perm.tolist() == list(range(16))


def test_sixteen_equal_measurable_costs():
    """Every tile 2^10: mine_s = 1 per thread, total_s = 16, target k = 2 k is owned by thread 2 k (before_s = 2 k), whose
    one tile takes `run` from 2 k << 10 to past it: t = 2 k, cut = 2 k + 1.  (Tile 2 k - 1 ends exactly ON the target,
    and the search wants `run > want`.)  nmin = 1, nmax = 4: no clamp moves anything."""
    split, perm = R.schedule([1024] * 16)
    assert split == [0, 3, 5, 7, 9, 11, 13, 15, 16]
    assert perm.tolist() == list(range(16))


def test_one_hot_tile_of_313():
    """Tile 0 at 2^24: total_s = 2^14, every target lies in thread 0's tile, all seven raw cuts are 1.  nmin = 19,
    nmax = 59: the first three cuts are lifted to prev + nmin; from the fourth on `T - left * nmax` (77, 136, 195, 254)
    is the larger bound."""
    cost = [1 << 24] + [1] * 312
    split, _ = R.schedule(cost)
    assert lengths(split) == [19, 19, 19, 20, 59, 59, 59, 59]


def test_one_hot_tile_of_4096():
    """per = 4; thread 0 sums 2^24 + 3, scaled 2^14; raw cuts all 1.  nmin = 256, nmax = 769: cuts 256, 512, 768, then
    max(1024, 4096 - 4 * 769 = 1020) = 1024, then 4096 - 3 * 769 = 1789, 2558, 3327."""
    cost = [1 << 24] + [1] * 4095
    split, _ = R.schedule(cost)
    assert lengths(split) == [256, 256, 256, 256, 765, 769, 769, 769]


def test_five_tiles_leave_three_ranges_empty():
    """nmin = 0, nmax = 1; equal shares 5 k / 8 = 0, 1, 1, 2, 3, 3, 4 already satisfy both bounds."""
    split, perm = R.schedule([1] * 5)
    assert R.limits(5) == (0, 1)
    assert split == [0, 0, 1, 1, 2, 3, 3, 4, 5]
    assert lengths(split).count(0) == 3
    assert perm.tolist() == [0, 1, 2, 3, 4]


def test_groups_of_three_in_two_classes():
    """T = 64, every cost below 2^10: equal shares of 8 tiles.  Range 1 = tiles 8 .. 15 with G = 3 is the groups
    {8} (of 6, 7, 8), {9, 10, 11}, {12, 13, 14}, {15} (of 15, 16, 17) with mean costs 10, 200, 501, 1000; cmax = 1001;
    classes ((1000 - v) * 2) / 1001 = 1, 1, 0, 0: the two heavy groups first, each class in tile order.  Every other
    range holds one cost value only: class 0 throughout, identity."""
    cost = [1] * 64
    cost[8:16] = [10, 100, 200, 300, 500, 500, 503, 1000]
    split, perm = R.schedule(cost, nclasses=2, G=3)
    assert split == [0, 8, 16, 24, 32, 40, 48, 56, 64]
    assert perm[8:16].tolist() == [12, 13, 14, 15, 8, 9, 10, 11]
    assert perm[:8].tolist() == list(range(8)) and perm[16:].tolist() == list(range(16, 64))


def test_an_unmeasured_tile_counts_as_the_average_of_the_measured():
    """T = 4: costs 4096, 0, 0, 12288.  Scaled per-thread sums 4 + 12 = 16 over 2 known tiles: fill = (16 << 10) / 2 = 8192.
    Filled and scaled: 4, 8, 8, 12 (threads start at 0, 4, 12, 20); total_s = 32; targets 4 k.  Targets 4 and 8 fall to
    thread 1, whose tile passes both: cut 2, 2; 12 and 16 to thread 2: cut 3, 3; 20, 24, 28 to thread 3: cut 4, 4, 4.
    nmin = 0, nmax = 1: `hi` = prev + 1 pulls the first three cuts down to 1, 2, 3; the fourth (3) and the rest (4, no
    more than prev + 1) stand."""
    c = R.cuts([4096, 0, 0, 12288])
    assert c.fill == 8192 and c.total_s == 32
    assert c.split == [0, 1, 2, 3, 3, 4, 4, 4, 4]


def test_the_two_total_s_arrays_sit_on_either_side_of_the_branch(cases):
    for T, name, cost, c in cases:
        if name in ("total-7", "total-8"):
            assert c.total_s == int(name[-1]), (T, name)


# ---- the matrix reaches what it was chosen to reach
def test_coverage_of_the_inputs(cases):
    """How many (T, shape) cases put a range exactly on nmax or on nmin (counted at T >= 64 only: below, the two bounds are
    so close that nearly every schedule touches them), take the equal-share branch, fill an unmeasured tile from measured
    ones, and leave a range empty.  DESIGN.md 3 records the counts."""
    count = dict.fromkeys(("cases", "cases of T >= 64", "on nmax", "on nmin", "equal-share branch", "fill used", "empty range"), 0)
    for T, name, cost, c in cases:
        nmin, nmax = R.limits(T)
        n = lengths(c.split)
        count["cases"] += 1
        count["cases of T >= 64"] += T >= 64
        count["on nmax"] += T >= 64 and nmax in n
        count["on nmin"] += T >= 64 and nmin in n
        count["equal-share branch"] += c.total_s < 8
        count["fill used"] += bool(np.any(cost == 0) and np.any(cost != 0))
        count["empty range"] += 0 in n
    print("\nschedule matrix coverage:", count)
    assert count["cases"] == len(R.SHAPES) * (len(R.TILE_COUNTS) + len(R.BIG_TILE_COUNTS))
    for what, k in count.items():
        assert k > 0, what
    # the hot-tile shapes are the ones that must reach BOTH clamps wherever the bounds differ from "everything"
    for T, name, cost, c in cases:
        if T >= 64 and name in ("hot-first", "hot-last", "first-eighth-hot", "last-eighth-hot"):
            nmin, nmax = R.limits(T)
            assert nmin in lengths(c.split) and nmax in lengths(c.split), (T, name, c.split)


@pytest.mark.parametrize("T", [8, 16, 64, 313])
def test_the_planted_arrays_reach_both_clamps(T):
    """The arrays tests/test_gpu_schedule_kernel.py plants under the scheduled K4 / K5 (500, 1000, 4096 and 20 011
    particles): for every tile count at least one of them puts a range on nmax and one on nmin, in either direction."""
    nmin, nmax = R.limits(T)
    for flip in (False, True):
        seen = set()
        for kind in R.PLANTED:
            cost = R.planted(kind, T)
            seen |= set(lengths(R.cuts(cost[::-1] if flip else cost).split))
        assert nmin in seen and nmax in seen, (T, flip, sorted(seen))


# ---- the checker can fail
@pytest.fixture(scope="module")
def valid():
    T = 313
    split, perm = R.schedule(R.SHAPES["hot-first"](T))
    R.check_schedule(split, perm, T)
    assert lengths(split)[4] == R.limits(T)[1]  # range 4 sits on nmax
    return T, split, perm


def fault_of(split, perm, T):
    with pytest.raises(R.ScheduleFault) as e:
        R.check_schedule(split, perm, T)
    assert e.value.fault in R.FAULTS
    return e.value.fault


def test_checker_names_a_dropped_last_tile(valid):
    T, split, perm = valid
    assert fault_of(split[:8] + [T - 1], perm[:-1], T) == "last cut is not T"
    assert fault_of(split, perm[:-1], T) == "perm has the wrong length"


def test_checker_names_a_duplicated_tile(valid):
    T, split, perm = valid
    bad = perm.copy()
    bad[split[2] + 1] = bad[split[2]]
    assert fault_of(split, bad, T) == "tile duplicated"


def test_checker_names_a_cut_one_past_nmax(valid):
    T, split, perm = valid
    bad = list(split)
    bad[5] += 1  # range 4: nmax + 1 tiles, still fewer than the launch has rows -- the bound is checked before it bites
    assert fault_of(bad, np.arange(T), T) == "range longer than nmax"


def test_checker_names_swapped_cuts(valid):
    T, split, perm = valid
    bad = list(split)
    bad[2], bad[3] = bad[3], bad[2]
    assert fault_of(bad, perm, T) == "split is not monotone"


def test_checker_names_a_tile_in_the_neighbouring_range(valid):
    T, split, perm = valid
    bad = perm.copy()
    at = split[3]
    bad[at - 1], bad[at] = bad[at], bad[at - 1]  # still a permutation of 0 .. T - 1 as a whole
    assert sorted(bad.tolist()) == list(range(T))
    assert fault_of(split, bad, T) == "tile outside its range"


def test_checker_names_a_short_range_and_a_bad_first_cut(valid):
    T, split, perm = valid
    bad = list(split)
    bad[1] -= 1  # range 0 sat on nmin
    assert fault_of(bad, np.arange(T), T) == "range shorter than nmin"
    assert fault_of([1] + split[1:], perm, T) == "first cut is not 0"
