"""The cohesion restatement (tests/cohesion_ref.py) checked on its own, without a device: the float32 stage against a
float64 brute force over all pairs within the bound of a recursive sum, the properties of the definition on a jittered
lattice blob (cohesion pulls the outer layer inward, momentum is conserved to rounding, XSPH lowers the velocity
variance), the corners (a lone particle, a coincident pair, both branches of the spline, the default rest density), and
a merged grid."""
import numpy as np

import aniso_ref as A
import cohesion_ref as Co

F32 = np.float32
U = 2.0 ** -23
DT = 1.0 / 60.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _scene(ws, n=2048, seed=5):
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    pos = ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max))
    vel = np.random.default_rng(seed + 1).normal(0.0, 2.0, (n, 3)).astype(F32)
    return np.ascontiguousarray(pos, F32), vel, params


def _bound(ref, key):
    """(c_i + 16) 2^-23 (the particle's sum of absolute terms): the standard bound of a recursive float32 sum of c_i terms,
    each of which carries a handful of roundings of its own."""
    return (ref["neighbours"][:, None] + 16.0) * U * ref[key + "_abs"]


# ---- (a) float32 against float64 ---------------------------------------------------------------------------------------
def test_the_stage_agrees_with_a_float64_brute_force_over_all_pairs(ws):
    pos, vel, params = _scene(ws)
    cp = dict(Co.defaults(), xsph=0.3)
    # the terms carry n_i, n_j and rho, sums themselves: the float64 stage's normals and densities, rounded once to
    # float32, are fed to both, so that the bound is applied per quantity
    own = Co.stage64(ws, params, pos, vel, cp, DT)
    fed = (own["normal"].astype(F32), own["density"].astype(F32))
    st = Co.stage(params, pos, vel, cp, DT, fed=fed)
    ref = Co.stage64(ws, params, pos, vel, cp, DT, fed=fed)
    safe = ~ref["near"]
    print("measured: restriction keeps %.4f of the particles" % safe.mean())
    assert safe.mean() >= 0.8
    assert np.array_equal(st["neighbours"][safe], ref["neighbours"][safe])
    assert np.mean(ref["neighbours"] >= 8) > 0.2
    for key in ("A", "X", "dv"):
        err = np.abs(st[key].astype(np.float64) - ref[key])[safe]
        bound = _bound(ref, key)[safe]
        worst = (err / np.maximum(bound, 1e-300))[bound > 0]
        print("measured: %s worst |f32 - f64| / bound = %.3g" % (key, worst.max()))
        assert np.all(err <= bound), key
    # pass A on its own: the density and the normal against float64, same bound with their own absolute terms
    mine = Co.stage(params, pos, vel, cp, DT)
    c = own["neighbours"] + 1.0  # (the density has i's own term)
    assert np.all(np.abs(mine["density"] - own["density"])[safe] <= ((c + 16.0) * U * own["density"])[safe])


# ---- (b) properties of the definition on a jittered lattice blob --------------------------------------------------------
def _blob(ws):
    """8^3 points at spacing 0.12 around the container's centre, normal jitter sigma = 0.004: the outer layer is the 296
    particles with max_a |x_a - centre_a| > 0.4."""
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    assert float(params.smoothing_radius) == 0.25
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    centre = 0.5 * (lo + hi)
    ax = (np.arange(8) - 3.5) * 0.12
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + centre
    x = (lattice + np.random.default_rng(1).normal(0.0, 0.004, lattice.shape)).astype(F32)
    outer = np.abs(x.astype(np.float64) - centre).max(1) > 0.4
    assert len(x) == 512 and outer.sum() == 296
    return params, x, centre, outer


def _momentum_is_conserved(ws, params, x, v, cp, st):
    """The pair terms are antisymmetric, so sum_i dv_i is zero up to the roundings of the particles' own sums."""
    ref = Co.stage64(ws, params, x, v, cp, DT)
    assert np.array_equal(st["neighbours"], ref["neighbours"])
    total = np.abs(st["dv"].astype(np.float64).sum(0))
    bound = _bound(ref, "dv").sum(0)
    print("measured: |sum dv| =", total, "bound", bound, "sum |dv| =", np.abs(st["dv"]).sum(0))
    assert np.all(total <= bound) and np.all(np.abs(st["dv"]).sum(0) > 1e3 * bound)


def test_cohesion_pulls_the_outer_layer_inward_and_conserves_momentum(ws):
    params, x, centre, outer = _blob(ws)
    v = np.zeros_like(x)
    for cp in (dict(Co.defaults(), curvature=0.0, xsph=0.0), dict(Co.defaults(), xsph=0.0)):
        st = Co.stage(params, x, v, cp, DT)
        ref = Co.stage64(ws, params, x, v, cp, DT)
        inward = centre - x.astype(np.float64)
        for dv in (st["dv"].astype(np.float64), ref["dv"]):
            pull = (dv * inward).sum(1)
            assert np.all(pull[outer] > 0), cp
        assert np.all(st["neighbours"] > 0)
        _momentum_is_conserved(ws, params, x, v, cp, st)
    # the normal points into the fluid, and is longer on the outer layer (neighbours on one side only) than anywhere in
    # the 4^3 core, whose particles are 0.24 and more from the faces and see all but a sliver of their kernel's support
    nrm = st["normal"].astype(np.float64)
    inner = np.abs(x.astype(np.float64) - centre).max(1) < 0.2
    assert inner.sum() == 64 and np.all((nrm * inward).sum(1)[outer] > 0)
    assert np.linalg.norm(nrm[outer], axis=1).min() > np.linalg.norm(nrm[inner], axis=1).max()


def test_xsph_lowers_the_velocity_variance_and_conserves_momentum(ws):
    params, x, centre, outer = _blob(ws)
    v = np.random.default_rng(2).normal(0.0, 1.0, x.shape).astype(F32)
    cp = dict(cohesion=0.0, curvature=0.0, xsph=0.5, rest_density=0.0)
    st = Co.stage(params, x, v, cp, DT)
    after = Co.apply(v, st).astype(np.float64)
    before = v.astype(np.float64)
    var = lambda a: ((a - a.mean(0)) ** 2).sum()  # noqa: E731
    print("measured: variance %.6g -> %.6g" % (var(before), var(after)))
    assert var(after) < var(before)
    _momentum_is_conserved(ws, params, x, v, cp, st)
    # with the strengths at 0, A stays +0 and dv is xsph * X alone
    assert not st["A"].any() and np.array_equal(bits(st["dv"]), bits((F32(0.5) * st["X"]).astype(F32) + F32(0)))


# ---- (c) corners ---------------------------------------------------------------------------------------------------------
def _few(ws, pts, vel=None, **cp):
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    x = np.asarray(pts, F32).reshape(-1, 3)
    v = np.zeros_like(x) if vel is None else np.asarray(vel, F32).reshape(-1, 3)
    return params, x, v, Co.stage(params, x, v, dict(Co.defaults(), **cp), DT)


def test_a_lone_particle_and_a_coincident_pair_are_unaffected(ws):
    for pts in ([[0.5, 0.5, 0.5]], [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]):
        vel = np.full((len(pts), 3), -0.0, F32)
        params, x, v, st = _few(ws, pts, vel)
        assert not st["neighbours"].any()
        assert np.array_equal(bits(st["dv"]), np.zeros((len(pts), 3), np.uint32))  # +0
        assert np.all(st["density"] > 0) and not st["normal"].any()
        assert np.array_equal(bits(Co.apply(v, st)), bits(vel))  # the -0 stays
    # the pair's densities count both particles, the lone one's only itself
    assert _few(ws, [[0.5, 0.5, 0.5]] * 2)[3]["density"][0] == 2 * _few(ws, [[0.5, 0.5, 0.5]])[3]["density"][0]


def _by_hand(ws, params, d, n_i, n_j, rho_i, rho_j, gc=1.0, gn=1.0):
    """A of particle i along the axis from i to j for a neighbour at distance d on that axis, in float64."""
    h = 0.25
    pp = (h - d) ** 3 * d ** 3
    s = pp if 2 * d > h else 2 * pp - h ** 6 / 64
    C = 32.0 / (float(F32(3.14159274)) * h ** 9) * s
    K = float(params.target_density) * 2.0 / (rho_i + rho_j)
    return -K * (gc * C * -1.0 + gn * (n_i - n_j))


def test_both_branches_of_the_spline(ws):
    h = F32(0.25)
    beyond = np.nextafter(F32(0.625), F32(1))
    cases = {"at h/2": F32(0.625), "just beyond": beyond, "repulsive h/4": F32(0.5625), "attractive 3h/4": F32(0.6875)}
    got = {}
    for name, xj in cases.items():
        params, x, v, st = _few(ws, [[0.5, 0.5, 0.5], [xj, 0.5, 0.5]], xsph=0.0)
        assert float(params.smoothing_radius) == 0.25 and np.array_equal(st["neighbours"], [1, 1])
        d = float(xj) - 0.5
        assert (2 * F32(d) > h) == (name in ("just beyond", "attractive 3h/4")), name
        want = _by_hand(ws, params, d, float(st["normal"][0, 0]), float(st["normal"][1, 0]), float(st["density"][0]),
                        float(st["density"][1]))
        a = st["A"].astype(np.float64)
        assert abs(a[0, 0] - want) <= 32 * U * abs(want) + 1e-30, (name, a[0, 0], want)
        assert a[0, 0] == -a[1, 0] and not a[:, 1:].any(), name  # antisymmetric, on the axis
        assert np.array_equal(bits(st["dv"]), bits((F32(DT) * st["A"]).astype(F32) + F32(0))), name
        got[name] = a[0, 0]
    # the spline is continuous across its branch; cohesion alone is repulsive close and attractive far
    assert abs(got["at h/2"] - got["just beyond"]) <= 1e-5 * abs(got["at h/2"])
    params, x, v, st = _few(ws, [[0.5, 0.5, 0.5], [0.5625, 0.5, 0.5]], curvature=0.0, xsph=0.0)
    assert st["A"][0, 0] < 0 < st["A"][1, 0]  # pushed apart
    params, x, v, st = _few(ws, [[0.5, 0.5, 0.5], [0.6875, 0.5, 0.5]], curvature=0.0, xsph=0.0)
    assert st["A"][0, 0] > 0 > st["A"][1, 0]  # pulled together


def test_rest_density_zero_is_the_handles_target_density(ws):
    pos, vel, params = _scene(ws, 512)
    a = Co.stage(params, pos, vel, Co.defaults(), DT)
    b = Co.stage(params, pos, vel, dict(Co.defaults(), rest_density=float(params.target_density)), DT)
    c = Co.stage(params, pos, vel, dict(Co.defaults(), rest_density=2.0 * float(params.target_density)), DT)
    assert a["dv"].any()
    for k in Co.OUTPUTS:
        assert np.array_equal(bits(a[k]) if a[k].dtype == F32 else a[k], bits(b[k]) if b[k].dtype == F32 else b[k]), k
    assert not np.array_equal(a["dv"], c["dv"])


def test_a_merged_grid_offers_the_same_pairs(ws):
    pos, vel, params = _scene(ws, 1024)
    cp = Co.defaults()
    one = Co.stage(params, pos, vel, cp, DT)
    for merged in ((1, 1, 3), (2, 3, 1)):
        assert A.Grid(params, merged).dim.prod() < A.Grid(params).dim.prod()
        other = Co.stage(params, pos, vel, cp, DT, merged)
        # the cells differ, so the canonical order and with it the sums' roundings may; the pairs may not
        assert np.array_equal(one["neighbours"], other["neighbours"])
        scale = np.maximum(np.abs(one["dv"]), 1.0)
        assert np.max(np.abs(one["dv"] - other["dv"]) / scale) < 256 * U
        ids = np.array([5, 0, 1023, 77])
        part = Co.stage(params, pos, vel, cp, DT, merged, ids)
        for k in other:
            assert np.array_equal(part[k], other[k][ids]), k
