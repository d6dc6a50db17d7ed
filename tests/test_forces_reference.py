"""tests/forces_ref.py, the float32 restatement of ws_apply_forces the GPU tests compare bits with, against a float64
evaluation of the same formulas, and the properties the definition promises (include/wsfluid.h).

The tolerance is derived, not tuned.  Every float32 operation on the path from the inputs to one axis of v' is rounded
once and contributes at most 2^-24 of the magnitude it runs at.  Per emitter the longest chain is
    q = x - c (1), dot(q, q) (3 products + 2 sums = 5), sqrt (1), d / R (1), 1 - . (1), strength * w (1)       = 10
    the kind's term: VORTEX, the longest: two products and a difference (3), t * s (1), A + . (1)              =  5
    the brake: damping * w (1), v * g (1), A - . (1)                                                           =  3
and after the loop dt * A (1) and v + . (1): ROUNDINGS(k) = 18 k + 2.  The magnitudes those roundings run at are bounded
per axis by  M = |v| + dt * sum_e (|strength_e| * max(1, |axis_e|, |axis_e| * R_e) + damping_e * |v|)  (w, the unit vector
q / d and (axis x q) / (|axis| R) are at most 1 in magnitude), so |v'_32 - v'_64| <= ROUNDINGS(k) * 2^-24 * M."""
import numpy as np

import forces_ref as F

F32 = np.float32


def roundings(k):
    return 18 * k + 2


def scene(seed, n=2000, k=6):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    forces = []
    for e in range(k):
        forces.append(F.emitter(e % 3, rng.uniform(-0.6, 0.6, 3), rng.uniform(0.3, 1.2), rng.normal(0.0, 30.0),
                                rng.normal(0.0, 1.5, 3), rng.uniform(0.0, 4.0) if e % 2 else 0.0))
    return pos, vel, forces, F32(rng.uniform(0.004, 0.02))


def bound(vel, forces, dt, k):
    vn = np.sqrt((vel.astype(np.float64) ** 2).sum(axis=1))
    m = vn.copy()
    for f in forces:
        an = float(np.sqrt((f["axis"].astype(np.float64) ** 2).sum()))
        m = m + float(dt) * (abs(float(f["strength"])) * max(1.0, an, an * float(f["radius"])) + float(f["damping"]) * vn)
    return roundings(k) * 2.0 ** -24 * m


def test_the_restatement_is_within_the_derived_bound_of_float64():
    for seed in range(6):
        k = (1, 3, 6, 16, 2, 5)[seed]
        pos, vel, forces, dt = scene(seed, k=k)
        v32, pred, counts = F.apply(pos, vel, forces, dt)
        v64, hit = F.apply64(pos, vel, forces, dt)
        assert hit.any() and not hit.all(), seed
        err = np.abs(v32.astype(np.float64) - v64)
        tol = bound(vel, forces, dt, k)
        print("seed %d k %d: worst error / bound %.3f" % (seed, k, float((err / tol[:, None]).max())))
        assert np.all(err <= tol[:, None]), (seed, float((err / tol[:, None]).max()))
        assert counts.dtype == np.uint32 and counts.shape == (k,)
        # pred' is the library's rule on the new velocity, two roundings
        assert np.array_equal(pred, (pos + (v32 * F32(0.02)).astype(F32)).astype(F32))


def test_unaffected_particles_keep_their_bits_minus_zero_included():
    pos, vel, forces, dt = scene(11, k=3)
    vel[::7] = F32(-0.0)
    vel[3::7, 1] = F32(-0.0)
    for f in forces:
        f["radius"] = F32(0.4)
    v32, _, counts = F.apply(pos, vel, forces, dt)
    _, hit, _ = F.accelerate(pos, vel, forces)
    assert 0 < np.count_nonzero(hit) < len(pos) and counts.sum() >= np.count_nonzero(hit)
    assert np.array_equal(v32[~hit].view(np.uint32), vel[~hit].view(np.uint32))
    assert np.any(np.signbit(v32[~hit]) & (v32[~hit] == 0))  # some -0 survived: v + dt * 0 would have made them +0
    assert np.any(v32[hit].view(np.uint32) != vel[hit].view(np.uint32))


def test_the_edge_of_reach_is_out_and_the_centre_is_in():
    pos = np.array([[0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [np.nextafter(F32(0.5), F32(0)), 0.0, 0.0]], F32)
    vel = np.array([[1.0, 2.0, 3.0]] * 3, F32)
    for kind in (F.RADIAL, F.JET, F.VORTEX):
        f = F.emitter(kind, (0, 0, 0), 0.5, 8.0, axis=(0.0, 1.0, 0.0), damping=2.0)
        v32, _, counts = F.apply(pos, vel, [f], F32(0.01))
        assert counts[0] == 2, kind                            # d == R is out, d == 0 and d just below R are in
        assert np.array_equal(v32[0].view(np.uint32), vel[0].view(np.uint32)), kind
        A, hit, _ = F.accelerate(pos, vel, [f])
        assert list(hit) == [False, True, True]
        brake = -(vel[1] * F32(2.0)).astype(F32)                 # w == 1 at the centre: g = damping
        want = {F.RADIAL: brake, F.JET: (np.array([0, 8, 0], F32) + brake).astype(F32), F.VORTEX: brake}[kind]
        assert np.array_equal(A[1], want), (kind, A[1], want)  # no RADIAL term at d == 0 (and axis x 0 = 0); JET and brake act
        assert np.all(np.isfinite(v32))


def test_a_radial_puller_brings_particles_closer_in_float64():
    pos, vel, _, _ = scene(5)
    vel[:] = 0
    dt = F32(0.01)
    f = F.emitter(F.RADIAL, (0.1, -0.2, 0.05), 0.9, 25.0)
    v32, _, counts = F.apply(pos, vel, [f], dt)
    _, hit, _ = F.accelerate(pos, vel, [f])
    c = f["centre"].astype(np.float64)
    x = pos.astype(np.float64)
    before = np.sqrt(((x - c) ** 2).sum(axis=1))
    after = np.sqrt(((x + v32.astype(np.float64) * float(dt) - c) ** 2).sum(axis=1))
    moved = hit & (before > 0)
    assert counts[0] > 100 and np.all(after[moved] < before[moved])
    pusher = F.emitter(F.RADIAL, (0.1, -0.2, 0.05), 0.9, -25.0)
    vp, _, _ = F.apply(pos, vel, [pusher], dt)
    after = np.sqrt(((x + vp.astype(np.float64) * float(dt) - c) ** 2).sum(axis=1))
    assert np.all(after[moved] > before[moved])


def test_a_vortex_term_is_perpendicular_to_axis_and_radius_in_float64():
    pos, vel, _, _ = scene(6)
    vel[:] = 0
    f = F.emitter(F.VORTEX, (0.0, 0.1, 0.0), 1.0, 12.0, axis=(0.3, 1.0, -0.2))
    A, hit, _ = F.accelerate(pos, vel, [f])
    q = pos.astype(np.float64) - f["centre"].astype(np.float64)
    a = f["axis"].astype(np.float64)
    A = A.astype(np.float64)[hit]
    q = q[hit]
    qn, an = np.sqrt((q * q).sum(axis=1)), np.sqrt(a @ a)
    assert hit.sum() > 100 and np.sqrt((A * A).sum(axis=1)).max() > 1.0
    # the products of the cross product are rounded at the magnitude |axis| |q| (not at |t|: they may cancel), then one
    # difference and the product with s, and q = x - c before them: at most 5 roundings of 2^-24 per component, at the
    # magnitude |strength| |axis| |q|
    scale = 5 * 2.0 ** -24 * 12.0 * an * qn * np.sqrt(3.0)
    assert np.all(np.abs(A @ a) <= scale * an)
    assert np.all(np.abs((A * q).sum(axis=1)) <= scale * qn)


def test_the_order_of_the_emitters_is_part_of_the_contract():
    pos, vel, forces, dt = scene(7, k=6)
    for f in forces:
        f["radius"] = F32(1.5)  # everything overlaps
    a, _, ca = F.apply(pos, vel, forces, dt)
    b, _, cb = F.apply(pos, vel, forces[::-1], dt)
    assert np.array_equal(ca, cb[::-1])
    differ = np.any(a.view(np.uint32) != b.view(np.uint32), axis=1)
    assert differ.any()                                        # float addition is not associative: the order shows
    assert np.allclose(a, b, rtol=1e-4, atol=1e-4)             # ... in the last bits only
