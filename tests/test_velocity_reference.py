"""The velocity field's numpy restatement (tests/velocity_ref.py) checked on its own, without a device: a constant
velocity comes back exactly, one midpoint substep in it moves a tracer by exactly dt * v, and the float32 field agrees with
the float64 brute force within the density test's tolerance construction."""
import numpy as np

import velocity_ref as V

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
CONST = np.array([2.0, -0.5, 0.0], F32)  # powers of two (and 0): w * v_a is exact, so M_a carries rho's own rounding


def _scene(ws, n=2048, seed=5):
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    pos = ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max))
    return np.ascontiguousarray(pos, F32), params


def _queries(pos, params, seed=6):
    """At particles, near particles, uniform in the container padded by 2 h, and far outside the grid."""
    rng = np.random.default_rng(seed)
    h = float(params.smoothing_radius)
    mn = np.asarray(params.ext_min[:3], np.float64) - 2 * h
    mx = np.asarray(params.ext_max[:3], np.float64) + 2 * h
    at = pos[rng.choice(len(pos), 64, replace=False)].astype(np.float64)
    near = pos[rng.choice(len(pos), 256, replace=False)] + rng.normal(0.0, 0.05, (256, 3))
    box = mn + rng.random((256, 3)) * (mx - mn)
    far = mx + 10 * h + rng.exponential(2.0, (32, 3))
    return np.concatenate([at, near, box, far]).astype(F32)


def test_a_constant_velocity_is_returned_exactly_and_zero_in_the_air(ws):
    pos, params = _scene(ws)
    vel = np.tile(CONST, (len(pos), 1))
    q = _queries(pos, params)
    u, rho, mom = V.field32(params, pos, vel, q)
    wet = rho > 0
    assert wet.sum() > 300 and (~wet).sum() >= 32 and not rho[-32:].any()
    assert np.array_equal(u[wet], np.tile(CONST, (int(wet.sum()), 1)))
    assert np.array_equal(mom[wet], (rho[wet, None] * CONST).astype(F32))
    assert np.array_equal(u[~wet].view(np.uint32), np.zeros((int((~wet).sum()), 3), np.uint32))  # +0, not -0
    assert np.array_equal(rho, V.A.iso_field32(params, pos, q))  # the density sampler's restatement, bit for bit


def test_one_midpoint_substep_in_a_constant_field_moves_a_tracer_by_exactly_dt_v(ws):
    pos, params = _scene(ws)
    vel = np.tile(CONST, (len(pos), 1))
    rng = np.random.default_rng(7)
    mn = np.asarray(params.ext_min[:3], np.float64)
    mx = np.asarray(params.ext_max[:3], np.float64)
    # tracers on multiples of 2^-6, so p + dt * v is a float32 for dt = 2^-4; some of them well outside the fluid
    inside = np.round((mn + rng.random((400, 3)) * (mx - mn)) * 64) / 64
    air = np.round((mx + 1.0 + rng.random((50, 3))) * 64) / 64
    p0 = np.concatenate([inside, air]).astype(F32)

    def field(p):
        u, rho, _ = V.field32(params, pos, vel, p)
        return u, rho

    dt = F32(0.0625)
    p1, took = V.advect(field, dt, 1, p0)
    moved = ~took["air"]
    assert moved[:400].sum() > 300 and took["air"][400:].all() and took["ordinary"].sum() > 300
    assert np.array_equal(p1[moved], p0[moved] + dt * CONST)
    assert np.array_equal(p1[~moved], p0[~moved])
    # backwards by the same step: the tracers that moved are still in the fluid's constant field
    p2, took2 = V.advect(field, -dt, 1, p1)
    back = moved & ~took2["air"]
    assert back.sum() > 300 and np.array_equal(p2[back], p0[back])


def test_the_restatement_agrees_with_float64(ws):
    pos, params = _scene(ws)
    vel = np.random.default_rng(8).normal(0.0, 2.0, pos.shape).astype(F32)
    q = _queries(pos, params)
    u, rho, mom = V.field32(params, pos, vel, q)
    want_rho, want_mom, noise, cnt = V.field64(ws, params, pos, vel, q)
    assert np.mean(cnt >= 8) > 0.25 and np.mean(cnt == 0) > 0.05
    for got, want, nz in ((rho, want_rho, noise[0]), (mom, want_mom, noise[1:].max())):
        tol = 4.0 * float(nz) + 4.0 * EPS32 * float(np.max(np.abs(want)))
        assert float(np.max(np.abs(got.astype(np.float64) - want))) <= tol
    assert not rho[cnt == 0].any() and not mom[cnt == 0].any() and not u[cnt == 0].any()
    # u is M / rho: the weighted mean lies inside the hull of the velocities
    wet = rho > 0
    assert np.all(np.abs(u[wet]) <= np.abs(vel).max(0) * (1 + 1e-5))
