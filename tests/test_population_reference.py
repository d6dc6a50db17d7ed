"""The restatement of the count-changing calls (tests/population_ref.py) against a brute-force Python loop over float32
scalars, on planted cases: overlapping sinks and the order of the claims, a particle exactly on a box face (inside), a
particle at d == R of a sphere (outside), a NaN coordinate (stays), duplicate ids."""
import numpy as np

import population_ref as P

F32 = np.float32


def _inside(x, s):
    """One particle, one sink, scalar by scalar in the header's order."""
    q = [F32(x[a]) - F32(s["centre"][a]) for a in range(3)]
    if s["kind"] == P.SPHERE:
        d = np.sqrt(F32(F32(F32(q[0] * q[0]) + F32(q[1] * q[1])) + F32(q[2] * q[2])))
        return bool(d < F32(s["half"][0]))
    return all(bool(abs(q[a]) <= F32(s["half"][a])) for a in range(3))


def _brute(pos, sinks):
    owner, counts = [], [0] * len(sinks)
    for x in pos:
        who = -1
        for e, s in enumerate(sinks):
            if _inside(x, s):
                who = e
                break
        owner.append(who)
        if who >= 0:
            counts[who] += 1
    new, rank = [], 0
    for who in owner:
        if who < 0:
            new.append(rank)
            rank += 1
        else:
            new.append(0xFFFFFFFF)
    return np.array(owner, np.int32), np.array(counts, np.uint32), np.array(new, np.uint32)


def _state(pos, seed=0):
    rng = np.random.default_rng(seed)
    n = len(pos)
    return np.asarray(pos, F32), rng.normal(0, 1, (n, 3)).astype(F32), rng.uniform(0, 1, (n, 4)).astype(F32)


def _check(pos, sinks):
    pos = np.asarray(pos, F32)
    with np.errstate(invalid="ignore"):
        owner, counts, new = _brute(pos, sinks)
    got_owner, got_counts = P.claims(pos, sinks)
    assert np.array_equal(got_owner, owner) and np.array_equal(got_counts, counts)
    state = _state(pos)
    after, c2, got_new = P.remove_by_sinks(state, sinks)
    assert np.array_equal(c2, counts) and np.array_equal(got_new, new)
    keep = owner < 0
    for before, now in zip(state, after):
        assert now.shape[0] == keep.sum()
        assert np.array_equal(now.view(np.uint32), before[keep].view(np.uint32))
    # the survivor with old id i sits at new[i]
    for i in np.flatnonzero(keep):
        assert np.array_equal(after[0][new[i]].view(np.uint32), pos[i].view(np.uint32))
    return owner, counts, new


def test_random_clouds_and_random_sinks():
    rng = np.random.default_rng(5)
    for n, k in ((1, 1), (65, 3), (500, 16)):
        pos = rng.uniform(-1, 1, (n, 3)).astype(F32)
        sinks = [P.sink(e % 2, rng.uniform(-0.8, 0.8, 3), rng.uniform(0.2, 0.7) if e % 2 == 0 else rng.uniform(0.1, 0.6, 3))
                 for e in range(k)]
        owner, counts, _ = _check(pos, sinks)
        assert counts.sum() == np.count_nonzero(owner >= 0)
    assert counts.sum() > 100 and (counts > 0).sum() >= 8


def test_overlapping_sinks_the_first_claims():
    pos = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.9, 0.0, 0.0), (5.0, 5.0, 5.0)]
    big, small = P.sink(P.BOX, (0, 0, 0), (1, 1, 1)), P.sink(P.SPHERE, (0, 0, 0), 0.5)
    owner, counts, new = _check(pos, [small, big])
    assert list(owner) == [0, 0, 1, -1] and list(counts) == [2, 1] and list(new) == [P.REMOVED] * 3 + [0]
    owner, counts, _ = _check(pos, [big, small])  # the other order: the box takes all three, the sphere nothing
    assert list(owner) == [0, 0, 0, -1] and list(counts) == [3, 0]


def test_a_particle_on_a_box_face_is_inside_and_one_at_the_radius_is_outside():
    box = P.sink(P.BOX, (1.0, 2.0, 3.0), (0.5, 0.25, 0.125))
    on_face = [(1.5, 2.0, 3.0), (1.0, 1.75, 3.0), (1.0, 2.0, 3.125), (1.5, 2.25, 2.875)]
    off = [(np.nextafter(F32(1.5), F32(2)), 2.0, 3.0), (1.0, 2.0, np.nextafter(F32(2.875), F32(0)))]
    owner, _, _ = _check(on_face + off, [box])
    assert list(owner) == [0, 0, 0, 0, -1, -1]
    ball = P.sink(P.SPHERE, (0, 0, 0), 0.5)
    pts = [(0.5, 0.0, 0.0), (0.0, -0.5, 0.0), (np.nextafter(F32(0.5), F32(0)), 0.0, 0.0), (0.3, 0.4, 0.0), (0.0, 0.0, 0.0)]
    owner, _, _ = _check(pts, [ball])
    # (0.3, 0.4, 0): fl(0.09) + fl(0.16) rounds to d = 0.5 exactly or next to it; the loop decides, the restatement agrees
    assert list(owner[:3]) == [-1, -1, 0] and owner[4] == 0


def test_a_nan_coordinate_is_contained_by_nothing():
    nan = F32(np.nan)
    pos = [(nan, 0.0, 0.0), (0.0, nan, 0.0), (0.0, 0.0, nan), (0.0, 0.0, 0.0)]
    for s in (P.sink(P.BOX, (0, 0, 0), (9, 9, 9)), P.sink(P.SPHERE, (0, 0, 0), 9.0)):
        owner, counts, new = _check(pos, [s])
        assert list(owner) == [-1, -1, -1, 0] and list(counts) == [1] and list(new) == [0, 1, 2, P.REMOVED]


def test_duplicate_ids_count_once_and_the_add_appends_in_order():
    state = _state(np.arange(30, dtype=F32).reshape(10, 3), seed=3)
    keep = P.keep_of_ids(10, [7, 2, 7, 2, 9])
    assert list(np.flatnonzero(~keep)) == [2, 7, 9]
    after, new = P.remove(state, keep)
    assert list(new) == [0, 1, P.REMOVED, 2, 3, 4, 5, P.REMOVED, 6, P.REMOVED]
    assert np.array_equal(after[0][:, 0], [0, 3, 9, 12, 15, 18, 24])
    assert np.array_equal(P.renumber(np.ones(4, bool)), np.arange(4))  # nothing removed: the identity
    more = P.add(after, [(1, 2, 3), (4, 5, 6)], attr=[(1, 0, 0, 0), (0, 1, 0, 0)])
    assert more[0].shape == (9, 3) and np.array_equal(more[0][7:], [(1, 2, 3), (4, 5, 6)])
    assert not more[1][7:].any() and not np.signbit(more[1][7:]).any()  # at rest: +0
    assert np.array_equal(more[2][7:], [(1, 0, 0, 0), (0, 1, 0, 0)])
    again = P.add(more, [(7, 8, 9)], vel=[(1, 1, 1)])
    assert not again[2][9].any() and np.array_equal(again[1][9], (1, 1, 1))
    pred = P.predicted(again)
    assert np.array_equal(pred[9], (F32(7) + F32(1) * F32(0.02), F32(8) + F32(0.02), F32(9) + F32(0.02)))
