"""The attribute restatement (tests/attributes_ref.py) checked on its own, without a device: float32 diffusion against a
float64 brute force over all pairs within the bound of a recursive sum, the properties the header states (the channel
totals are conserved to rounding, a step with r = 0.5 stays inside the neighbourhood's range, iterating lowers the
variance monotonically), and the corners of paint, diffusion and the field."""
import numpy as np

import aniso_ref as A
import attributes_ref as At
from test_cohesion_reference import _blob, _scene

F32 = np.float32
U = 2.0 ** -23
DT = 1.0 / 60.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _random_attr(n, seed=9):
    return np.random.default_rng(seed).random((n, 4)).astype(F32)


def _bound(ref):
    """(c_i + 16) 2^-23 (the particle's sum of absolute terms), per channel: test_cohesion_reference's bound."""
    return (ref["neighbours"][:, None] + 16.0) * U * ref["S_abs"]


def _fed_pair(ws, rate, dt=DT, seed=9):
    """The 2 048-particle scene with random A in [0, 1]: the float64 densities, rounded once, fed to both."""
    pos, _, params = _scene(ws)
    attr = _random_attr(len(pos), seed)
    own = At.diffuse64(ws, params, pos, attr, rate, dt)
    fed = own["density"].astype(F32)
    new, cnt, S = At.diffuse(params, pos, attr, rate, dt, fed=fed, sums=True)
    ref = At.diffuse64(ws, params, pos, attr, rate, dt, fed=fed)
    return pos, params, attr, new, cnt, S, ref


# ---- (a) float32 against float64 ---------------------------------------------------------------------------------------
def test_diffusion_agrees_with_a_float64_brute_force_over_all_pairs(ws):
    rate = (30.0, 20.0, 10.0, 5.0)
    pos, params, attr, new, cnt, S, ref = _fed_pair(ws, rate)
    safe = ~ref["near"]
    print("measured: restriction keeps %.4f of the particles" % safe.mean())
    assert safe.mean() >= 0.8
    assert np.array_equal(cnt[safe], ref["neighbours"][safe])
    assert np.mean(ref["neighbours"] >= 8) > 0.2
    err = np.abs(S.astype(np.float64) - ref["S"])[safe]
    bound = _bound(ref)[safe]
    worst = (err / np.maximum(bound, 1e-300))[bound > 0]
    print("measured: S worst |f32 - f64| / bound = %.3g" % worst.max())
    assert np.all(err <= bound)
    # A' = A + r S: the sum's bound scaled by r, and the two roundings of the update itself
    r = ref["r"]
    err = np.abs(new.astype(np.float64) - ref["A"])[safe]
    bound = (r * _bound(ref) + U * (np.abs(r * ref["S"]) + np.abs(ref["A"])))[safe]
    print("measured: A' worst |f32 - f64| / bound = %.3g" % (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    # pass A on its own is the cohesion pass A: the density against float64 with its own terms
    mine = At.densities(params, pos)
    own = At.diffuse64(ws, params, pos, attr, rate, DT)
    c = own["neighbours"] + 1.0  # (the density has i's own term)
    assert np.all(np.abs(mine - own["density"])[safe] <= ((c + 16.0) * U * own["density"])[safe])


# ---- (b) the properties the header states -------------------------------------------------------------------------------
def test_the_total_of_every_channel_is_conserved_to_rounding(ws):
    rate = (30.0, 20.0, 10.0, 5.0)
    pos, params, attr, new, cnt, S, ref = _fed_pair(ws, rate)
    r = ref["r"]
    # g_ij and g_ji are the same bits and the differences exact negatives: the pair terms cancel exactly, and the total
    # moves by the roundings of the particles' own sums (and of the update) alone
    drift = np.abs(new.astype(np.float64).sum(0) - attr.astype(np.float64).sum(0))
    bound = (r * _bound(ref) + U * (np.abs(r * ref["S"]) + np.abs(ref["A"]))).sum(0)
    moved = np.abs(new.astype(np.float64) - attr.astype(np.float64)).sum(0)
    print("measured: |sum A' - sum A| =", drift, "bound", bound, "sum |A' - A| =", moved)
    assert np.all(drift <= bound) and np.all(moved >= 1e3 * bound)
    # the same with the restatement's own pass A
    own, cnt2 = At.diffuse(params, pos, attr, rate, DT)
    assert np.array_equal(cnt2, cnt)
    assert np.all(np.abs(own.astype(np.float64).sum(0) - attr.astype(np.float64).sum(0)) <= bound)


def test_a_step_of_half_stays_inside_the_neighbourhoods_range(ws):
    rate = (30.0, 30.0, 30.0, 30.0)  # r = 30 / 60 = 0.5
    pos, params, attr, new, cnt, S, ref = _fed_pair(ws, rate)
    assert np.all((F32(30.0) * F32(DT)).astype(F32) == F32(0.5))
    qi, pj, g = ref["pairs"]
    lo, hi = attr.astype(np.float64).copy(), attr.astype(np.float64).copy()
    np.minimum.at(lo, qi, attr[pj].astype(np.float64))
    np.maximum.at(hi, qi, attr[pj].astype(np.float64))
    assert np.bincount(qi, g, minlength=len(pos)).max() < 2.0  # sum_j g_ij < 2
    safe = ~ref["near"]
    slack = 0.5 * _bound(ref) + U * (np.abs(0.5 * ref["S"]) + np.abs(ref["A"]))
    a = new.astype(np.float64)
    assert np.all((a >= lo - slack)[safe]) and np.all((a <= hi + slack)[safe])
    assert np.any(cnt > 0) and not np.array_equal(new, attr)


def test_sixteen_iterations_lower_every_channels_variance_monotonically(ws):
    params, x, centre, outer = _blob(ws)
    a = _random_attr(len(x), 3)
    var = lambda v: ((v.astype(np.float64) - v.astype(np.float64).mean(0)) ** 2).sum(0)  # noqa: E731
    rate = (20.0, 10.0, 30.0, 5.0)
    trace = [var(a)]
    cur = a
    for _ in range(16):
        cur, cnt = At.diffuse(params, x, cur, rate, DT)
        trace.append(var(cur))
    trace = np.asarray(trace)
    print("measured: variance", trace[0], "->", trace[-1])
    assert np.all(cnt > 0) and np.all(trace[1:] < trace[:-1])
    # ... and the sixteen as one call are the same bits
    once, _ = At.diffuse(params, x, a, rate, DT, iterations=16)
    assert np.array_equal(bits(once), bits(cur))


# ---- (c) corners ---------------------------------------------------------------------------------------------------------
def _params(ws):
    return ws.make_params(container_size=(3.0, 2.0, 2.0))


def test_a_lone_particle_and_a_coincident_pair_keep_their_bits(ws):
    params = _params(ws)
    for pts in ([[0.5, 0.5, 0.5]], [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]):
        x = np.asarray(pts, F32)
        a = np.array([[-0.0, 1.0, -2.5, 0.0]] * len(pts), F32)
        a[-1, 1] = 7.0  # (a coincident pair with different values: d == 0 contributes nothing)
        new, cnt = At.diffuse(params, x, a, (30.0,) * 4, DT, iterations=3)
        assert not cnt.any() and np.array_equal(bits(new), bits(a))
    assert At.densities(params, np.asarray([[0.5, 0.5, 0.5]] * 2, F32))[0] == 2 * At.densities(params, np.asarray([[0.5, 0.5, 0.5]], F32))[0]


def test_a_zero_rate_and_an_unpainted_particle_keep_a_negative_zero(ws):
    params = _params(ws)
    x = np.asarray([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [1.5, 1.0, 1.0]], F32)
    a = np.full((3, 4), -0.0, F32)
    new, cnt = At.diffuse(params, x, a, (30.0, 0.0, 30.0, 0.0), DT)
    assert list(cnt) == [1, 1, 0]
    assert np.array_equal(bits(new[:, [1, 3]]), bits(a[:, [1, 3]]))  # rate 0: the bits
    assert np.array_equal(bits(new[2]), bits(a[2]))                   # unaffected: the bits
    assert np.array_equal(bits(new[:2, [0, 2]]), np.zeros((2, 2), np.uint32))  # -0 + fl(r * +0) = +0: it took part
    b = At.brush("add", (0.5, 0.5, 0.5), 0.2, (1.0, 1.0, 1.0, 1.0), channels=0b0101)
    painted, counts = At.paint(x, a, [b])
    assert list(counts) == [2]
    assert np.array_equal(bits(painted[2]), bits(a[2]))                       # out of reach
    assert np.array_equal(bits(painted[:2, [1, 3]]), bits(a[:2, [1, 3]]))     # outside the mask
    assert np.all(painted[:2, [0, 2]] == 1.0)
    # the rim is outside: d < R is strict
    rim = At.brush("add", (0.5, 0.5, 0.5), float(F32(0.6) - F32(0.5)), (1.0,) * 4)
    assert list(At.paint(x, a, [rim])[1]) == [1]


def test_mix_at_full_strength_gives_the_value_exactly_and_brush_order_matters(ws):
    x = np.asarray([[0.5, 0.5, 0.5], [0.55, 0.5, 0.5], [0.69, 0.5, 0.5]], F32)
    a = np.asarray([[0.1, -3.0, 1e10, -0.0]] * 3, F32)
    val = (0.3, -0.7, 123.456, 1e-20)
    full = At.brush("mix", (0.5, 0.5, 0.5), 0.2, val, strength=1.0, falloff=0.0)
    painted, counts = At.paint(x, a, [full])
    assert list(counts) == [3]
    assert np.array_equal(bits(painted), bits(np.tile(np.asarray(val, F32), (3, 1))))
    # a linear falloff: w = 1 - d / R by hand
    soft = At.brush("mix", (0.5, 0.5, 0.5), 0.2, val, strength=0.5, falloff=1.0, channels=1)
    got, _ = At.paint(x, a, [soft])
    d = (x[:, 0] - F32(0.5)).astype(np.float64)
    s = 0.5 * (1.0 - d / float(F32(0.2)))
    want = (1.0 - s) * float(F32(0.1)) + s * float(F32(0.3))
    assert np.all(np.abs(got[:, 0] - want) <= 8 * U * np.abs(want)) and np.array_equal(bits(got[:, 1:]), bits(a[:, 1:]))
    # order: MIX then ADD differs from ADD then MIX
    add = At.brush("add", (0.5, 0.5, 0.5), 0.2, (1.0, 1.0, 1.0, 1.0), strength=2.0)
    half = At.brush("mix", (0.5, 0.5, 0.5), 0.2, val, strength=0.5)
    ab, _ = At.paint(x, a, [add, half])
    ba, _ = At.paint(x, a, [half, add])
    assert not np.array_equal(ab[:, 0], ba[:, 0])
    step, _ = At.paint(x, At.paint(x, a, [add])[0], [half])
    assert np.array_equal(bits(ab), bits(step))  # the running value


def test_the_field_of_a_constant_is_that_constant(ws):
    pos, _, params = _scene(ws, 1024)
    const = np.asarray([0.75, -2.0, 1e-3, 300.0], F32)
    attr = np.tile(const, (len(pos), 1))
    q = np.concatenate([pos[:64], pos[:64] + F32(0.05), np.asarray([[-5.0, -5.0, -5.0]], F32)])
    val, rho, mom, cnt = At.field(params, pos, attr, q)
    wet = rho > 0
    assert wet[:64].all() and not wet[-1] and np.array_equal(bits(val[~wet]), np.zeros(((~wet).sum(), 4), np.uint32))
    err = np.abs(val[wet].astype(np.float64) - const.astype(np.float64))
    assert np.all(err <= (cnt[wet][:, None] + 16.0) * U * np.abs(const.astype(np.float64)))
    # the density is the density sampler's, and a merged grid offers the same pairs
    import velocity_ref as V

    assert np.array_equal(bits(rho), bits(V.field32(params, pos, np.zeros_like(pos), q)[1]))
    other = At.field(params, pos, attr, q, merged=(1, 1, 3))
    assert A.Grid(params, (1, 1, 3)).dim.prod() < A.Grid(params).dim.prod()
    assert np.array_equal(other[3], cnt) and np.max(np.abs(other[0] - val)) <= 256 * U * 300.0
    # the grid's nodes: x fastest
    nodes = At.grid_nodes((0.0, 0.5, 1.0), (0.25, 0.5, 0.125), (3, 2, 2))
    assert nodes.shape == (12, 3) and list(nodes[1]) == [0.25, 0.5, 1.0] and list(nodes[3]) == [0.0, 1.0, 1.0]
    assert list(nodes[6]) == [0.0, 0.5, 1.125]
