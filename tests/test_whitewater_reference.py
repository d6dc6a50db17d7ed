"""The whitewater restatement (tests/whitewater_ref.py) checked on its own, without a device: the integer mixer against
hand-computed words, U in [0, 1), the disc rejection and the spawn cylinder, T == 0 for equal velocities, the normals and
crest values of a flat slab, the stage against a float64 brute force over all pairs, and a merged grid."""
import numpy as np

import aniso_ref as A
import whitewater_ref as W

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def _scene(ws, n=2048, seed=5):
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    pos = ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max))
    vel = np.random.default_rng(seed + 1).normal(0.0, 2.0, (n, 3)).astype(F32)
    return np.ascontiguousarray(pos, F32), vel, params


def _mix_by_hand(x):
    """The header's five lines in Python integers."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_the_mixer_matches_hand_computed_words():
    # mix(0) = 0 (every line maps 0 to 0); mix(1): 1 -> 1 -> 0x7feb352d -> ^ (>> 15 = 0xffd6) = 0x7febcafb -> * 0x846ca68b
    assert int(W.mix(0)) == 0
    assert int(W.mix(1)) == ((0x7FEBCAFB * 0x846CA68B) & 0xFFFFFFFF) ^ (((0x7FEBCAFB * 0x846CA68B) & 0xFFFFFFFF) >> 16)
    for x in (1, 2, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert int(W.mix(x)) == _mix_by_hand(x), hex(x)
    # word(i, c) = mix(mix(seed + i * 0x9E3779B9) + c), wrapping
    for seed, i, c in ((0, 0, 0), (7, 3, 19), (0xFFFFFFFF, 4095, 1 + 18 * 63 + 17), (12345, 1 << 22, 5)):
        want = _mix_by_hand(_mix_by_hand(seed + i * 0x9E3779B9) + c)
        assert int(W.word(seed, i, c)) == want, (seed, i, c)
    # arrays behave as scalars do
    ids = np.arange(1000)
    assert np.array_equal(W.word(7, ids, 3), np.array([int(W.word(7, int(i), 3)) for i in ids], np.uint32))


def test_u_lies_in_the_half_open_unit_interval():
    ids = np.arange(1 << 16)
    for c in (0, 1, 2, 1151):
        u = W.uniform(99, ids, c)
        assert u.dtype == F32 and u.min() >= 0 and u.max() < 1
        assert abs(float(u.mean()) - 0.5) < 0.01 and u.max() > 0.999 and u.min() < 0.001
    # the largest word maps below 1: (2^24 - 1) * 2^-24
    assert F32(0xFFFFFFFF >> 8) * F32(2.0 ** -24) == F32(1) - F32(2.0 ** -24)


def test_the_disc_rejection_never_leaves_the_unit_disc():
    ids = np.repeat(np.arange(4096), 4)
    k = np.tile(np.arange(4), 4096)
    a, b = W.disc(3, ids, k)
    r2 = (a * a + b * b).astype(F32)
    assert np.all(r2 <= 1)
    assert np.mean((a == 0) & (b == 0)) < 1e-3  # eight rejections in a row: (1 - pi / 4)^8 ~ 5e-6
    assert 0.45 < float(np.mean(r2)) < 0.55  # uniform on the disc: E r^2 = 1 / 2
    for q in (a, b):
        assert q.min() < -0.95 and q.max() > 0.95


def test_every_spawn_lies_inside_its_cylinder(ws):
    pos, vel, params = _scene(ws, 1024)
    vel[:8] = np.eye(3, dtype=F32)[[0, 1, 2, 0, 1, 2, 0, 1]] * F32(3)  # axis-aligned: ties for the smallest component
    vel[8] = (1.0, 1.0, 1.0)
    e = dict(W.emit_defaults(), radius=0.15, dt=0.02, seed=11)
    m = np.full(len(pos), 5)
    s = W.spawn(pos, vel, m, e)
    assert s["count"] == 5 * len(pos) and np.array_equal(s["source"], np.repeat(np.arange(len(pos)), 5))
    src = s["source"]
    x, v = pos[src].astype(np.float64), vel[src].astype(np.float64)
    sv = np.linalg.norm(v, axis=1)
    vh = v / sv[:, None]
    off = s["xyz"].astype(np.float64) - x
    axial = (off * vh).sum(1)
    radial = np.linalg.norm(off - axial[:, None] * vh, axis=1)
    slack = 16 * EPS32 * (np.abs(x).max() + 1.0)
    assert np.all(radial <= 0.15 * (1 + 8 * EPS32) + slack)
    assert np.all(axial >= -slack) and np.all(axial <= 0.02 * sv * (1 + 8 * EPS32) + slack)
    # the velocity offset is the radial offset itself, and the lifetimes lie in [2, 5)
    dv = s["velocity"].astype(np.float64) - v
    assert np.all(np.abs((dv * vh).sum(1)) <= 16 * EPS32 * (1 + np.abs(v).max()))
    assert np.all(np.linalg.norm(dv, axis=1) <= 0.15 * (1 + 8 * EPS32) + 16 * EPS32 * np.abs(v).max())
    assert s["life"].min() >= 2 and s["life"].max() < 5 and s["life"].max() > 4.9
    # the frame is orthonormal to rounding
    e1, e2 = W.frame(vh.astype(F32))
    for a, b, want in ((e1, e1, 1), (e2, e2, 1), (e1, e2, 0), (e1, vh, 0), (e2, vh, 0)):
        assert np.max(np.abs((a.astype(np.float64) * b).sum(1) - want)) < 8 * EPS32


def test_trapped_air_is_zero_exactly_when_all_velocities_are_equal(ws):
    pos, vel, params = _scene(ws, 1024)
    same = np.tile(np.array([1.5, -0.3, 0.7], F32), (len(pos), 1))
    st = W.stage(params, pos, same)
    assert np.array_equal(st["trapped"].view(np.uint32), np.zeros(len(pos), np.uint32))  # +0
    assert st["neighbours"].max() > 8
    st = W.stage(params, pos, vel)
    assert np.all(st["trapped"][st["neighbours"] > 0] > 0) and not st["trapped"][st["neighbours"] == 0].any()


def test_a_flat_slab_has_upward_normals_on_top_and_flatter_crests_inside(ws):
    """A lattice slab of spacing 0.06 under h = 0.25, nine layers thick.  A layer at depth k below the top sees k layers
    above and four below (4 * 0.06 < h < 5 * 0.06), so the layers at depth 0 .. 3 have a well-defined gradient along -y and
    the normal +y, while the layer at depth 4 is symmetric: its gradient cancels to rounding noise and its normal is
    arbitrary.  A top particle away from the rim reaches that layer through five neighbours only (straight below at 0.24,
    four at 0.06 * sqrt(17)), of total weight W = 0.04 + 4 * 0.0104 = 0.082, so its K is at most 2 W = 0.17 whatever those
    normals are; a particle on the rim has neighbours whose normals lean outwards and K in the units.
    Measured: the normals of the inner top layer are +y to float32 resolution (cos == 1, angle < 3.5e-4 rad); K <= 0.123
    there and >= 2.62 on the rim."""
    params = ws.make_params(container_size=(6.0, 4.0, 6.0))
    assert float(params.smoothing_radius) == 0.25
    pos = ws.cube_fluid(18, 9, 18, 0.03)
    st = W.stage(params, pos, np.zeros_like(pos))
    y = pos[:, 1]
    top = y == y.max()
    xz = pos[:, [0, 2]]
    lo, hi = xz.min(0), xz.max(0)
    inner = np.all((xz > lo + 0.3) & (xz < hi - 0.3), 1)
    edge = np.any((xz == lo) | (xz == hi), 1)
    assert (top & inner).sum() >= 36 and (top & edge).sum() >= 64
    cosang = st["normal"][top & inner, 1]
    print("measured: angle %.3g rad, K inner max %.4g, K rim min %.4g" % (
        np.arccos(np.clip(cosang, -1, 1)).max(), st["crest"][top & inner].max(), st["crest"][top & edge].min()))
    assert np.all(np.arccos(np.clip(cosang, -1, 1)) < 1e-3)
    assert st["crest"][top & inner].max() < 0.17 < 1.0 < st["crest"][top & edge].min()
    assert not st["trapped"].any() and not st["energy"].any() and not st["align"].any()


def test_the_stage_agrees_with_a_float64_brute_force(ws):
    """Measured on this scene (2048 uniform particles, velocities N(0, 2)): worst |float32 - float64| over the sum of the
    |terms| is 1.98e-6 for T (its factor 1 - rh . xh cancels) and 9.56e-7 for K, over E 1.44e-7, worst normal error 9.95e-7
    (absolute, at cond >= 0.05), worst alignment error 7.3e-7 (absolute); the bounds are 8 x those: float32 sums over up
    to ~100 terms of mixed sign."""
    pos, vel, params = _scene(ws)
    st = W.stage(params, pos, vel)
    ref = W.stage64(ws, params, pos, vel)
    assert np.array_equal(st["neighbours"], ref["neighbours"])
    assert np.mean(ref["neighbours"] >= 8) > 0.2
    well = ref["cond"] >= 0.05  # the normal is a well-conditioned function of the positions
    assert np.mean(well) > 0.5
    qi, pj = ref["pairs"]
    around = np.ones(len(pos), bool)
    np.logical_and.at(around, qi, well[pj])  # ... and so are all its neighbours'
    safe = well & around & (ref["margin"] > 1e-3)  # no crest gate sits on its threshold
    assert safe.sum() > 200
    err_t = np.abs(st["trapped"] - ref["trapped"]) / np.maximum(ref["trapped_abs"], 1e-30)
    err_k = np.abs(st["crest"] - ref["crest"])[safe] / np.maximum(ref["crest_abs"][safe], 1e-30)
    err_e = np.abs(st["energy"] - ref["energy"]) / ref["energy"]
    err_n = np.abs(st["normal"] - ref["normal"])[well].max()
    err_a = np.abs(st["align"] - ref["align"])[well].max()
    has = ref["neighbours"] > 0
    print("measured: T %.3g K %.3g E %.3g normal %.3g align %.3g" % (err_t[has].max(), err_k.max(), err_e.max(), err_n, err_a))
    assert err_t[has].max() <= 8 * 1.98e-6
    assert err_k.max() <= 8 * 9.56e-7
    assert err_e.max() <= 8 * 1.44e-7
    assert err_n <= 8 * 9.95e-7
    assert err_a <= 8 * 7.3e-7


def test_a_merged_grid_offers_the_same_pairs(ws):
    pos, vel, params = _scene(ws, 1024)
    one = W.stage(params, pos, vel)
    for merged in ((1, 1, 3), (2, 3, 1)):
        assert A.Grid(params, merged).dim.prod() < A.Grid(params).dim.prod()
        other = W.stage(params, pos, vel, merged)
        # the cells differ, so the canonical order and with it the sums' roundings may; the pairs may not
        assert np.array_equal(one["neighbours"], other["neighbours"])
        assert np.array_equal(one["energy"], other["energy"])
        for k in ("trapped", "crest"):
            scale = np.maximum(np.abs(one[k]), 1.0)
            assert np.max(np.abs(one[k] - other[k]) / scale) < 64 * EPS32, k
        # a subset of rows is the same rows
        ids = np.array([5, 0, 1023, 77])
        part = W.stage(params, pos, vel, merged, ids)
        for k in other:
            assert np.array_equal(part[k], other[k][ids]), k
