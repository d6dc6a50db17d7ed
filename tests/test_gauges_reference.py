"""The numpy restatement of the gauges (tests/gauges_ref.py) against its own brute-force loop over particles, on planted
cases: what the definition says about faces, radii, NaN, signed zeros, the clamp, empty regions and overlap.  No device."""
import numpy as np

import gauges_ref as G

F32 = np.float32


def _agree(pos, vel, regions, attr=None):
    got, want = G.measure(pos, vel, regions, attr), G.measure_loop(pos, vel, regions, attr)
    assert G.same(got, want) == [], G.same(got, want)
    assert np.array_equal(G.select(pos, regions), G.select_loop(pos, regions))
    return got


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (n, 3)).astype(F32), rng.normal(0.0, 1.5, (n, 3)).astype(F32), rng.uniform(0.0, 1.0, (n, 4)).astype(F32)


def test_overlapping_regions_each_count_and_the_sums_are_the_definitions():
    pos, vel, attr = _cloud(300, 1)
    regions = [G.region(G.SPHERE, (0.0, 0.0, 0.0), 1.5), G.region(G.BOX, (0.5, 0.0, 0.0), (1.0, 1.0, 1.0)),
               G.region(G.SPHERE, (0.25, 0.25, 0.0), 1.0)]
    got = _agree(pos, vel, regions, attr)
    inside = [G.contains(pos, s) for s in regions]
    assert (inside[0] & inside[1] & inside[2]).sum() > 10  # they overlap, and every region counts its own
    assert [int(c) for c in got["count"]] == [int(m.sum()) for m in inside]
    # the fixed point is the float sum to 2^-24 per term
    for e, m in enumerate(inside):
        assert np.allclose(got["sum_pos"][e] / 2.0 ** 24, pos[m].astype(np.float64).sum(axis=0), atol=len(pos) * 2.0 ** -24)
        ang = np.cross(pos[m].astype(np.float64) - regions[e]["centre"], vel[m].astype(np.float64)).sum(axis=0)
        assert np.allclose(got["sum_ang"][e] / 2.0 ** 24, ang, atol=1e-3)
        assert np.allclose(got["sum_attr"][e] / 2.0 ** 24, attr[m].astype(np.float64).sum(axis=0), atol=1e-4)
        assert np.array_equal(got["min_pos"][e], pos[m].min(axis=0)) and np.array_equal(got["max_pos"][e], pos[m].max(axis=0))
        assert got["max_speed2"][e] == G.dot(vel, vel)[m].max()
    without = _agree(pos, vel, regions)
    assert not without["sum_attr"].any() and G.same(dict(got, sum_attr=without["sum_attr"]), without) == []


def test_a_box_face_is_inside_and_a_sphere_radius_is_outside():
    pos = np.array([(1.0, 0.25, -0.5), (1.0000001, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 1.9999999, 0.0)], F32)
    vel = np.ones((4, 3), F32)
    box, ball = G.region(G.BOX, (0.0, 0.0, 0.0), (1.0, 0.25, 0.5)), G.region(G.SPHERE, (0.0, 0.0, 0.0), 2.0)
    got = _agree(pos, vel, [box, ball])
    assert list(G.contains(pos, box)) == [True, False, False, False]  # on three faces at once: in; one ulp beyond: out
    assert list(G.contains(pos, ball)) == [True, True, False, True]   # d == R: out
    assert [int(c) for c in got["count"]] == [1, 3]
    assert np.array_equal(G.select(pos, [box]), [0]) and np.array_equal(G.select(pos, [box, ball]), [0, 1, 3])


def test_a_nan_coordinate_is_contained_by_nothing_and_a_nan_velocity_is_skipped_by_the_maximum():
    pos = np.array([(0.0, np.nan, 0.0), (0.1, 0.1, 0.1), (0.2, 0.0, 0.0)], F32)
    vel = np.array([(1.0, 1.0, 1.0), (np.nan, 0.0, 0.0), (0.0, 3.0, 0.0)], F32)
    everything = G.region(G.BOX, (0.0, 0.0, 0.0), (1e15, 1e15, 1e15))
    got = _agree(pos, vel, [everything, G.region(G.SPHERE, (0.0, 0.0, 0.0), 5.0)])
    assert [int(c) for c in got["count"]] == [2, 2]
    assert got["max_speed2"][0] == F32(9.0)  # the NaN speed is skipped, as fmaxf skips it
    assert got["sum_vel"][0, 0] == -(1 << 55) + 0  # ... but enters its sum as fmaxf leaves it: -2^31
    assert got["sum_speed2"][0] == -(1 << 55) + 9 * (1 << 24)
    assert np.array_equal(G.select(pos, [everything]), [1, 2])


def test_signed_zeros_order_the_same_way_in_either_input_order():
    for order in ([0, 1], [1, 0]):
        pos = np.array([(-0.0, 0.0, -0.0), (0.0, -0.0, -0.0)], F32)[order]
        got = _agree(pos, np.zeros((2, 3), F32), [G.region(G.SPHERE, (0.0, 0.0, 0.0), 1.0)])
        assert np.signbit(got["min_pos"][0]).tolist() == [True, True, True]     # min = -0 wherever there is one
        assert np.signbit(got["max_pos"][0]).tolist() == [False, False, True]   # max = +0 wherever there is one
        assert not got["min_pos"][0].any() and not got["max_pos"][0].any()
        assert not np.signbit(got["max_speed2"][0]) and got["max_speed2"][0] == 0


def test_a_value_beyond_the_clamp_enters_as_two_to_the_31():
    pos = np.array([(0.5, 0.0, 0.0), (-0.5, 0.0, 0.0)], F32)
    vel = np.array([(3e9, 0.0, 0.0), (-3e9, 1.0, 0.0)], F32)
    got = _agree(pos, vel, [G.region(G.SPHERE, (0.0, 0.0, 0.0), 1.0)])
    assert got["sum_vel"][0].tolist() == [0, 1 << 24, 0]            # +2^31 and -2^31 cancel
    assert got["sum_speed2"][0] == 2 * (1 << 55)                     # 9e18 twice, each clamped to 2^31
    assert got["max_speed2"][0] == F32(F32(3e9) * F32(3e9)) + 0     # the extremes are not clamped
    one = _agree(pos[:1], vel[:1], [G.region(G.SPHERE, (0.0, 0.0, 0.0), 1.0)])
    assert one["sum_vel"][0, 0] == 1 << 55
    # 2^39 of magnitude in all is what a sum holds without wrapping: 256 terms of 2^31 reach 2^63 and wrap to -2^63
    many = _agree(np.zeros((256, 3), F32), np.tile(F32([3e9, 0, 0]), (256, 1)), [G.region(G.BOX, (0, 0, 0), (1, 1, 1))])
    assert many["sum_vel"][0, 0] == -(1 << 63) and many["count"][0] == 256


def test_an_empty_region_and_a_huge_box_as_everything():
    pos, vel, attr = _cloud(200, 2)
    regions = [G.region(G.SPHERE, (50.0, 50.0, 50.0), 1.0), G.region(G.BOX, (0.0, 0.0, 0.0), (1e15, 1e15, 1e15))]
    got = _agree(pos, vel, regions, attr)
    assert got["count"].tolist() == [0, 200]
    for name in ("sum_pos", "sum_vel", "sum_ang", "sum_speed2", "sum_attr"):
        assert not np.any(got[name][0]), name
    assert np.all(got["min_pos"][0] == np.inf) and np.all(got["max_pos"][0] == -np.inf)
    assert got["max_speed2"][0] == 0 and not np.signbit(got["max_speed2"][0])
    assert np.array_equal(got["min_pos"][1], pos.min(axis=0)) and np.array_equal(got["max_pos"][1], pos.max(axis=0))
    assert np.array_equal(G.select(pos, regions), np.arange(200)) and G.select(pos, regions[:1]).size == 0


def test_rounding_to_nearest_even_and_the_key_order():
    assert list(G.quantise(F32([2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 0.5 + 2.0 ** -24]))) == [0, 2, 0, 1, (1 << 23) + 1]
    assert [G._fixed(t) for t in F32([2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25])] == [0, 2, 0]
    xs = F32([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf])
    keys = G.key(xs)
    assert np.all(np.diff(keys.astype(np.int64)) > 0) and np.array_equal(G.unkey(keys).view(np.uint32), xs.view(np.uint32))
    assert [G._order(x) for x in xs] == keys.tolist()
    assert G.wrap((1 << 63) + 5) == -(1 << 63) + 5 and G.wrap(-(1 << 63) - 1) == (1 << 63) - 1
