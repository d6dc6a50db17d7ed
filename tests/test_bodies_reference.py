"""tests/bodies_ref.py, the float32 restatement of ws_body_forces the GPU tests compare bits with: the canonical sum against
its own further padding and against the exact sum, a sample's terms against a float64 evaluation of the same formulas, and
the properties the definition promises (include/wsfluid.h).

The tolerances are derived, not tuned; u = 2^-24 is the unit roundoff of float32, and every bound below is first order in
u with a factor (1 + 2^-20) for the higher orders (the longest chain has 8 roundings: (1 + u)^8 - 1 < 8 u (1 + 2^-20)).

The tree: a level rounds every partial sum once, and the partial sums of one level add up to at most sum|t| in magnitude,
so a level adds at most u * sum|t| of error and ceil(log2 P) levels at most ceil(log2 P) * u * sum|t|.

A wet sample, with the field (u, rho) given in float32 to both evaluations, so that only the call's own roundings count:
    f = rho / rho_0 (1 rounding; fminf is exact)                                       relative error   u
    vol = V * f (+1)                                                                                  2 u
    lift = fluid_density * vol, kd = drag * vol (+1)                                                  3 u
    kd * (u_a - w_a): the difference (1) and the product (1) on top of kd's 3                         5 u
    lift * g_a (+1)                                                                                   4 u
    F_a = the difference, rounded at |F_a| <= |kd (u_a - w_a)| + |lift g_a|:
        |F_a - F_a64| <= 6 u |kd (u_a - w_a)| + 5 u |lift g_a|                                        = eF_a
    r_a = p_a - c_a (1 rounding); a product r_y * F_z carries r's rounding, its own and F_z's error; the difference one more:
        |T_x - T_x64| <= |r_y| eF_z + |r_z| eF_y + 3 u (|r_y F_z| + |r_z F_y|), and cyclically."""
import math

import numpy as np

import bodies_ref as B

F32 = np.float32
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
LENGTHS = (0, 1, 2, 3, 255, 256, 257, 4097)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _pow2_above(c):
    P = 1
    while P <= c:
        P *= 2
    return P


def test_the_tree_ignores_further_padding_and_is_within_its_bound_of_the_exact_sum():
    rng = np.random.default_rng(3)
    for c in LENGTHS:
        P = _pow2_above(c)
        t = (rng.normal(0.0, 1.0, c) * 10.0 ** rng.uniform(-3, 3, c)).astype(F32)
        got = B.tree_sum(t)
        assert got.dtype == F32 and got.shape == ()
        for leaves in (2 * P, 8 * P):
            assert bits(B.tree_sum(t, leaves)) == bits(got), (c, leaves)
        exact = math.fsum(float(x) for x in t)
        tol = math.ceil(math.log2(P)) * U * math.fsum(abs(float(x)) for x in t)
        err = abs(float(got) - exact)
        print("c %d: error / bound %.3f" % (c, err / tol if tol else 0.0))
        assert err <= tol, (c, err, tol)
        # the columns of a 2-D array are summed independently
        two = np.stack([t, t[::-1]], axis=1)
        assert bits(B.tree_sum(two)[0]) == bits(got)


def test_the_tree_never_gives_minus_zero():
    minus = F32(-0.0)
    for c in LENGTHS:
        P = _pow2_above(c)
        all_minus = np.full(c, minus, F32)
        for leaves in (None, 2 * P, 8 * P):
            assert bits(B.tree_sum(all_minus, leaves)) == 0, (c, leaves)  # +0: at least one +0 leaf always enters
        if c:
            lone = np.zeros(c, F32)
            lone[c // 2] = minus
            for leaves in (None, 2 * P, 8 * P):
                assert bits(B.tree_sum(lone, leaves)) == 0, (c, leaves)
    assert bits(B.tree_sum(np.zeros(0, F32))) == 0 and bits(B.tree_sum(np.zeros((0, 3), F32))).tolist() == [0, 0, 0]


def test_the_order_of_the_samples_is_part_of_the_contract():
    rng = np.random.default_rng(5)
    t = (rng.normal(0.0, 1.0, 4097) * 10.0 ** rng.uniform(-3, 3, 4097)).astype(F32)
    a, b = B.tree_sum(t), B.tree_sum(t[::-1])
    assert bits(a) != bits(b) and abs(float(a) - float(b)) <= 2 * 13 * U * float(np.abs(t.astype(np.float64)).sum())
    # a sequential sum is another function
    seq = F32(0.0)
    for x in t:
        seq = F32(seq + x)
    assert bits(seq) != bits(a)


def scene(seed, m=3000):
    rng = np.random.default_rng(seed)
    g = np.array([rng.normal(0, 2.0), -9.8, rng.normal(0, 2.0)], F32)
    params = dict(fluid_density=F32(rng.uniform(200.0, 1500.0)), drag=F32(rng.uniform(0.0, 900.0)), rest_density=F32(0.0))
    rho0 = F32(10.0)
    u = rng.normal(0.0, 2.0, (m, 3)).astype(F32)
    rho = (rng.uniform(0.0, 25.0, m) * (rng.random(m) > 0.3)).astype(F32)  # dry, partly submerged and saturated samples
    u[rho == 0] = 0
    p = rng.uniform(-2.0, 2.0, (m, 3)).astype(F32)
    w = rng.normal(0.0, 1.0, (m, 3)).astype(F32)
    V = rng.uniform(0.0, 1e-3, m).astype(F32)
    c = rng.uniform(-1.0, 1.0, 3).astype(F32)
    return params, g, rho0, u, rho, p, w, V, c


def test_a_samples_terms_are_within_the_derived_bound_of_float64():
    for seed in range(5):
        params, g, rho0, u, rho, p, w, V, c = scene(seed)
        F, T, vol, f, wet = B.sample_terms(params, g, rho0, u, rho, p, w, V, c)
        F64, T64, vol64, f64, wet64 = B.sample_terms64(params, g, rho0, u, rho, p, w, V, c)
        assert np.array_equal(wet, wet64) and 0 < wet.sum() < len(wet)
        assert np.any((f > 0) & (f < 1)) and np.any(f == 1)
        for a in (F, T, vol, f):
            assert a.dtype == F32
        kd = float(params["drag"]) * vol64
        lift = float(params["fluid_density"]) * vol64
        drag_term = np.abs(kd[:, None] * (u.astype(np.float64) - w.astype(np.float64)))
        lift_term = np.abs(lift[:, None] * g.astype(np.float64)[None, :])
        eF = (6 * drag_term + 5 * lift_term) * U * SLACK
        r = np.abs(p.astype(np.float64) - c.astype(np.float64))
        aF = np.abs(F64)
        eT = np.stack([r[:, (a + 1) % 3] * eF[:, (a + 2) % 3] + r[:, (a + 2) % 3] * eF[:, (a + 1) % 3]
                       + 3 * U * SLACK * (r[:, (a + 1) % 3] * aF[:, (a + 2) % 3] + r[:, (a + 2) % 3] * aF[:, (a + 1) % 3])
                       for a in range(3)], axis=1)
        worst = {}
        for name, got, want, tol in (("f", f, f64, U * SLACK * f64), ("vol", vol, vol64, 2 * U * SLACK * vol64), ("F", F, F64, eF),
                                     ("T", T, T64, eT)):
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= tol), (seed, name, float((err - tol).max()))
            worst[name] = float((err[tol > 0] / tol[tol > 0]).max())
        print("seed %d: worst error / bound %s" % (seed, worst))


def test_the_per_body_sums_are_within_the_trees_bound_of_float64_sums_of_the_same_terms():
    params, g, rho0, u, rho, p, w, V, c = scene(9, m=5000)
    body_start = np.array([0, 0, 1, 3, 258, 514, 4611, 5000], np.uint32)
    F, T, vol, f, wet = B.sample_terms(params, g, rho0, u, rho, p, w, V, c)
    force, torque, volume, count = B.reduce(body_start, F, T, vol, wet)
    f64 = B.reduce64(body_start, F, T, vol, wet)  # float64 sums of the float32 terms: the tree's own error alone
    assert count.dtype == np.uint32 and np.array_equal(count, f64[3]) and count.sum() == wet.sum()
    for b in range(len(body_start) - 1):
        s = slice(int(body_start[b]), int(body_start[b + 1]))
        levels = math.ceil(math.log2(_pow2_above(s.stop - s.start)))
        for got, want, terms in ((force[b], f64[0][b], F[s]), (torque[b], f64[1][b], T[s]), (volume[b:b + 1], f64[2][b:b + 1], vol[s, None])):
            tol = levels * U * np.abs(terms.astype(np.float64)).sum(axis=0)
            assert np.all(np.abs(got.astype(np.float64) - want) <= tol), b
    assert not np.any(np.signbit(force)) or np.all(force[np.signbit(force)] != 0)
    assert bits(force[0]).tolist() == [0, 0, 0] and bits(volume[0]) == 0 and count[0] == 0  # the empty body


def test_dry_samples_give_plus_zero_everywhere():
    params, g, rho0, u, rho, p, w, V, c = scene(2)
    rho[::2] = 0
    rho[1::4] = F32(-0.0)
    F, T, vol, f, wet = B.sample_terms(params, g, rho0, u, rho, p, w, V, c)
    dry = ~wet
    assert dry.sum() >= len(rho) // 2 and np.array_equal(dry, ~(rho > 0))
    for a in (F[dry], T[dry], vol[dry], f[dry]):
        assert not bits(a).any()  # +0, whatever the sample's position, velocity and volume
    out = B.forces(params, g, rho0, u, np.zeros_like(rho), p, w, V, [0, 10, len(rho)], np.zeros((2, 3), F32))
    for k in ("force", "torque", "volume", "sample_force", "sample_fraction"):
        assert not bits(out[k]).any(), k
    assert not out["wet"].any()


def test_without_drag_the_force_is_the_lift_alone_and_points_up():
    params, g, rho0, u, rho, p, w, V, c = scene(4)
    params["drag"] = F32(0.0)
    g = np.array([0.0, -9.8, 0.0], F32)
    V = np.maximum(V, F32(1e-6))
    F, T, vol, f, wet = B.sample_terms(params, g, rho0, u, rho, p, w, V, c)
    assert wet.sum() > 100
    assert np.all(F[wet][:, 0] == 0) and np.all(F[wet][:, 2] == 0) and np.all(F[wet][:, 1] > 0)
    # Archimedes: the lift is fluid_density * submerged volume * |g|, three roundings
    want = float(params["fluid_density"]) * (V.astype(np.float64) * f.astype(np.float64)) * 9.8
    assert np.all(np.abs(F[wet][:, 1].astype(np.float64) - want[wet]) <= 4 * U * SLACK * want[wet])


def test_a_tiny_rest_density_saturates_the_fraction():
    params, g, rho0, u, rho, p, w, V, c = scene(6)
    params["rest_density"] = F32(1e-30)
    rho0 = B.rest_density_of(params, 10.0)
    assert rho0 == F32(1e-30) and B.rest_density_of(B.defaults(), 10.0) == F32(10.0)
    F, T, vol, f, wet = B.sample_terms(params, g, rho0, u, rho, p, w, V, c)
    assert np.all(f[wet] == 1) and np.all(bits(vol[wet]) == bits(V[wet])) and not bits(f[~wet]).any()
    # ... and rho_0 = 0 (a handle whose target_density is 0) divides to +inf: the same saturation, no NaN
    F0, _, _, f0, _ = B.sample_terms(params, g, F32(0.0), u, rho, p, w, V, c)
    assert np.all(f0[wet] == 1) and np.all(np.isfinite(F0))
