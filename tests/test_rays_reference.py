"""The ray restatement (tests/rays_ref.py) on the analytic field of one particle: the header's kernel and accept test
restated in numpy, so the hit radius, the normal, misses, rays that start inside and the camera's rays have closed forms."""
import numpy as np
import pytest

import rays_ref as R

F32 = np.float32
H = F32(0.25)
POW2 = F32(F32(15.0) / F32(F32(F32(2.0) * F32(np.pi)) * F32(H ** 5)))
POW2_DER = F32(F32(15.0) / F32(F32(np.pi) * F32(H ** 5)))
ISO = F32(5.0)
CENTRE = np.array([0.3, -0.2, 0.1], F32)
RADIUS = float(H) - np.sqrt(float(ISO) / float(POW2))  # (h - d)^2 * pow2 = iso


def _accept(h):
    """Largest f32 T with sqrtf(T) <= h (the library's d2_accept)."""
    t = F32(h * h)
    while np.sqrt(t) > h:
        t = np.nextafter(t, F32(0))
    while np.sqrt(np.nextafter(t, F32(np.inf))) <= h:
        t = np.nextafter(t, F32(np.inf))
    return t


def one_particle(p):
    """ws_sample_density_points for the single particle at CENTRE: e = x_p - o, the accept test, (h - d)^2 * pow2 and
    ((o - x_p) / d) * ((d - h) * pow2_der), every operation in float32."""
    e = (CENTRE[None, :] - p).astype(F32)
    d2 = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(F32) + e[:, 2] * e[:, 2]).astype(F32)
    ok = ~(d2 > _accept(H))
    d = np.sqrt(d2, dtype=F32)
    v = (H - d).astype(F32)
    rho = np.where(ok, ((v * v).astype(F32) * POW2).astype(F32), F32(0)).astype(F32)
    slope = ((d - H).astype(F32) * POW2_DER).astype(F32)
    apart = ok & (d > 0)
    g = np.zeros_like(p)
    g[apart] = ((-e[apart] / d[apart, None]).astype(F32) * slope[apart, None]).astype(F32)
    return rho, g


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


DIRS = _unit([[1, 0, 0], [0, -1, 0], [1, 2, 3], [-3, 1, 2], [0.2, -0.9, 0.4], [-1, -1, -1]])
MARCH = R.March(t_start=0.0, dt=float(H) / 2, steps=40, refine=6, iso=float(ISO))


def test_a_ray_through_the_centre_hits_at_the_analytic_radius_with_the_radial_normal():
    dist = 2.0
    o = (CENTRE.astype(np.float64) - dist * DIRS).astype(F32)
    v = DIRS.astype(F32)
    t, n, K = R.cast(one_particle, MARCH, o, v)
    assert np.all(K >= 1) and t.dtype == F32 and n.dtype == F32
    # |v| and the origin are rounded to float32: the exact crossing of THIS ray, in float64
    oc = o.astype(np.float64) - CENTRE.astype(np.float64)
    vv = v.astype(np.float64)
    b = (oc * vv).sum(1)
    a = (vv * vv).sum(1)
    c = (oc * oc).sum(1) - RADIUS ** 2
    want = (-b - np.sqrt(b * b - a * c)) / a
    assert np.all(np.abs(t.astype(np.float64) - want) <= MARCH.dt / 2 ** MARCH.refine)
    hit = o.astype(np.float64) + t.astype(np.float64)[:, None] * vv
    assert np.max(np.abs(n.astype(np.float64) - _unit(hit - CENTRE.astype(np.float64)))) <= 1e-5
    # the field at the reported point is >= iso
    assert np.all(one_particle(R.points(o, v, t))[0] >= ISO)


def test_a_ray_that_passes_farther_than_h_misses():
    side = _unit(np.cross(DIRS, [0.3, 0.5, -0.8]))
    o = (CENTRE.astype(np.float64) - 2.0 * DIRS + 1.01 * float(H) * side).astype(F32)
    t, n, K = R.cast(one_particle, MARCH, o, DIRS.astype(F32))
    assert np.all(K == -1) and np.all(np.isposinf(t)) and not n.any()


def test_a_ray_that_starts_at_the_centre_returns_t_start():
    march = MARCH._replace(t_start=0.375)
    v = DIRS.astype(F32)
    o = (CENTRE[None, :] - (F32(march.t_start) * v).astype(F32)).astype(F32)  # p(t_start) is the centre, up to rounding
    t, n, K = R.cast(one_particle, march, o, v)
    assert np.all(K == 0) and np.all(t == F32(march.t_start))


def test_refine_zero_returns_the_first_sample_inside():
    march = MARCH._replace(refine=0, dt=0.03)
    o = (CENTRE.astype(np.float64) - 1.0 * DIRS).astype(F32)
    v = DIRS.astype(F32)
    t, _, K = R.cast(one_particle, march, o, v, normals=False)
    for r in range(len(o)):
        ks = np.arange(march.steps + 1)
        rho, _ = one_particle(R.points(np.repeat(o[r:r + 1], len(ks), 0), np.repeat(v[r:r + 1], len(ks), 0), R.sample_t(march, ks)))
        first = int(np.flatnonzero(rho >= ISO)[0])
        assert first >= 1 and K[r] == first and t[r] == R.sample_t(march, first)


def test_bisection_keeps_the_upper_end():
    """t = hi: a coarser refinement brackets a finer one from above, and every result lies in (t_{K-1}, t_K]."""
    o = (CENTRE.astype(np.float64) - 2.0 * DIRS).astype(F32)
    v = DIRS.astype(F32)
    prev = None
    for refine in (0, 1, 3, 6, 12):
        t, _, K = R.cast(one_particle, MARCH._replace(refine=refine), o, v, normals=False)
        assert np.all(t > R.sample_t(MARCH, K - 1)) and np.all(t <= R.sample_t(MARCH, K))
        if prev is not None:
            assert np.all(t <= prev)
        prev = t


@pytest.mark.parametrize("size", [(1, 1), (3, 1), (7, 5), (71, 51), (641, 361)])
def test_the_camera_looks_along_forward_at_the_centre_of_an_odd_image(size):
    eye = np.array([1.0, 2.0, 3.0], F32)
    f = np.array([0.0, -0.6, 0.8], F32)
    r = np.array([1.5, 0.0, 0.0], F32)
    up = np.array([0.0, 0.8, 0.6], F32)
    o, v = R.camera_rays(eye, f, r, up, size)
    W, Hh = size
    assert o.shape == v.shape == (W * Hh, 3) and o.dtype == v.dtype == F32 and np.all(o == eye)
    mid = v[(Hh // 2) * W + W // 2]
    # u and w at the centre are fl((k + 0.5) * fl(2 / (2 k + 1))) - 1: 0 up to one rounding of 1.0
    assert np.all(np.abs(mid - f) <= 2.0 ** -23 * (np.abs(r) + np.abs(up)))
    if size == (1, 1):
        assert np.array_equal(mid, f)
    # corners: u = -1 + 1/W, w = 1 - 1/H (x fastest, j downwards)
    want = f.astype(np.float64) + (-1 + 1 / W) * r.astype(np.float64) + (1 - 1 / Hh) * up.astype(np.float64)
    assert np.max(np.abs(v[0] - want)) <= 1e-6
    want = f.astype(np.float64) + (1 - 1 / W) * r.astype(np.float64) + (-1 + 1 / Hh) * up.astype(np.float64)
    assert np.max(np.abs(v[-1] - want)) <= 1e-6
