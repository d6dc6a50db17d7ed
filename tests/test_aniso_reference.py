"""The anisotropic kernels' numpy restatement (tests/aniso_ref.py) checked on its own: the Jacobi, a planar
neighbourhood, the isotropic limit, a lone particle's ball, and the user-visible claim -- a flat sheet meshes flat."""
import numpy as np
import pytest

import aniso_ref as A
import surface_ref as S

F32 = np.float32
U = 2.0 ** -24


def _sym(a):
    """(m, 6) xx yy zz xy xz yz -> (m, 3, 3) float64"""
    a = np.asarray(a, np.float64)
    return np.stack([np.stack([a[:, 0], a[:, 3], a[:, 4]], 1), np.stack([a[:, 3], a[:, 1], a[:, 5]], 1),
                     np.stack([a[:, 4], a[:, 5], a[:, 2]], 1)], 1)


def _matrices(kind, m=2000):
    rng = np.random.default_rng(11)
    if kind == "random":
        b = rng.standard_normal((m, 3, 3)) * 0.05
        c = b @ b.transpose(0, 2, 1) - 0.001 * np.eye(3)  # (a few slightly negative eigenvalues too)
    elif kind == "diagonal":
        c = np.zeros((m, 3, 3))
        c[:, [0, 1, 2], [0, 1, 2]] = rng.uniform(0, 0.05, (m, 3))
    elif kind == "repeated":
        q, _ = np.linalg.qr(rng.standard_normal((m, 3, 3)))
        lam = np.repeat(rng.uniform(0.001, 0.05, (m, 1)), 3, 1)
        lam[:, 2] = rng.uniform(0.001, 0.05, m)
        c = q @ (lam[:, :, None] * q.transpose(0, 2, 1))
    else:
        c = np.zeros((m, 3, 3))
    return np.stack([c[:, 0, 0], c[:, 1, 1], c[:, 2, 2], c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]], 1).astype(F32)


@pytest.mark.parametrize("kind", ["random", "diagonal", "repeated", "zero"])
def test_jacobi_gives_an_orthonormal_basis_that_rebuilds_the_matrix(kind):
    a = _matrices(kind)
    sig, R = A.jacobi(a)
    R64 = R.astype(np.float64)
    eye = np.einsum("mki,mkj->mij", R64, R64)
    assert np.max(np.abs(eye - np.eye(3))) <= 64 * U
    back = np.einsum("mik,mk,mjk->mij", R64, sig.astype(np.float64), R64)
    c = _sym(a)
    scale = np.linalg.norm(c.reshape(len(c), -1), axis=1)
    err = np.max(np.abs(back - c).reshape(len(c), -1), axis=1)
    assert np.all(err <= 64 * U * scale), np.max(err / np.maximum(scale, 1e-30))
    if kind in ("diagonal", "zero"):  # nothing to rotate: every rotation is skipped
        assert np.array_equal(sig, a[:, :3]) and np.array_equal(R, np.broadcast_to(np.eye(3, dtype=F32), R.shape))


def _patch(n=2000, seed=3):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.5, 1.5, (n, 2))
    return np.concatenate([xy, np.zeros((n, 1))], 1).astype(F32)


def test_a_planar_neighbourhood_is_flattened_along_its_normal(ws):
    params = ws.make_params(container_size=(8.0, 8.0, 8.0))
    pos = _patch()
    c, m, f, n = A.stage(params, pos, A.defaults())
    kr = A.defaults()["max_ratio"]
    aniso = n >= 12
    assert aniso.sum() > len(pos) // 2
    # C_zz = C_xz = C_yz = 0 exactly: z is an eigenvector, its sigma 0 is floored to sigma_max / k_r, so M_zz = k_r
    assert np.all(m[aniso, 2] == F32(kr)) and np.all(m[aniso, 4] == 0) and np.all(m[aniso, 5] == 0)
    assert np.all(c[:, 2] == 0)
    # in the plane: 1 <= the eigenvalues of M <= k_r, the longest axis exactly 1 up to the rotation's rounding
    ev = np.linalg.eigvalsh(_sym(m[aniso])[:, :2, :2])
    assert np.all(ev >= 1 - 1e-5) and np.all(ev <= kr * (1 + 1e-5)) and np.all(np.abs(ev[:, 0] - 1) <= 1e-5)
    assert np.allclose(f[aniso], np.prod(ev, 1) * kr, rtol=1e-5)
    # with few neighbours: the lone ball
    lone = ~aniso
    assert np.all(m[lone] == np.array([2, 2, 2, 0, 0, 0], F32)) and np.all(f[lone] == F32(8))


def test_the_isotropic_limit_is_the_density_field_bit_for_bit(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    c, m, f, n = A.stage(params, pos, A.isotropic_limit())
    assert np.array_equal(c.view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(m, np.broadcast_to(np.array([1, 1, 1, 0, 0, 0], F32), m.shape)) and np.all(f == 1)
    assert np.all(m[:, 3:].view(np.uint32) == 0)  # +0 off the diagonal
    origin = np.array([-2.0, -2.0, -0.3], F32)
    spacing = np.full(3, F32(0.05), F32)
    q = A.grid_nodes(origin, spacing, (81, 81, 13))
    rho, _ = A.field32(params, c, m, f, q)
    want = A.iso_field32(params, pos, q)
    assert np.count_nonzero(want) > len(q) // 4
    assert np.array_equal(rho.view(np.uint32), want.view(np.uint32))


def test_a_lone_particle_meshes_as_the_predicted_ball(ws):
    params = ws.make_params(container_size=(8.0, 8.0, 8.0))
    k = ws.get_smoothing_kernel(params)
    h = F32(params.smoothing_radius)
    p = np.array([[0.3, -0.2, 0.1]], F32)
    a = A.defaults()
    c, m, f, n = A.stage(params, p, a)
    assert n[0] == 1 and np.array_equal(c, p) and f[0] == 8
    iso = F32(0.25 * float(k.pow2) * float(h) ** 2)
    r = A.lone_radius(float(h), float(k.pow2), float(iso), a["lone_scale"])
    sp = F32(h / F32(32))
    lo = p[0] - F32(0.7) * h
    dims = (46, 46, 46)
    xyz, nrm, tri = A.mesh(params, c, m, f, lo, np.full(3, sp, F32), dims, iso)
    dist = np.linalg.norm(xyz.astype(np.float64) - p[0], axis=1)
    L = np.sqrt(3.0) * float(sp)  # edge length: the linear interpolation's error along it (cf. tests/test_gpu_surface.py)
    assert np.max(np.abs(dist - r)) <= L * L / r, (np.max(np.abs(dist - r)), r)
    assert S.closed_and_oriented(tri, len(xyz)) and S.euler_characteristic(tri, len(xyz)) == 2
    assert np.all(np.einsum("ij,ij->i", nrm.astype(np.float64), xyz - p[0]) > 0)


def sheet_case(params, c, m, f, kr, field=None):
    """The C1-sheet comparison over the interior |x|, |y| <= 1.5 (more than 2 h from the sheet's edges at 6.3): the
    isotropic mesh at iso / k_r on a grid and the anisotropic one at iso on the same grid squashed k_r-fold in z.
    iso / k_r is half the isotropic field's minimum over the midplane, so both sheets cover the region without holes.
    field(grid) -> (rho, grad) of the anisotropic field (default: the restatement).  Returns the RMS in-plane normal
    component of (anisotropic, isotropic) mesh."""
    iso_m = np.array([1, 1, 1, 0, 0, 0], F32)
    ones = np.ones(len(c), F32)
    xs = A.grid_nodes(np.array([-1.5, -1.5, 0.0], F32), np.array([0.05, 0.05, 1.0], F32), (61, 61, 1))
    mid = A.iso_field32(params, c, xs)
    iso_lo = F32(0.5 * mid.min())
    dims = (61, 61, 41)
    o_iso, s_iso = np.array([-1.5, -1.5, -0.2], F32), np.array([0.05, 0.05, 0.01], F32)
    o_an, s_an = np.array([-1.5, -1.5, -0.2 / kr], F32), np.array([0.05, 0.05, 0.01 / kr], F32)
    iso_mesh = A.mesh(params, c, np.broadcast_to(iso_m, (len(c), 6)), ones, o_iso, s_iso, dims, iso_lo)
    if field is None:
        an_mesh = A.mesh(params, c, m, f, o_an, s_an, dims, F32(iso_lo * F32(kr)))
    else:
        an_mesh = field(o_an, s_an, dims, F32(iso_lo * F32(kr)))
    out = []
    for xyz, nrm, tri in (an_mesh, iso_mesh):
        assert len(tri) > 1000
        # the sheet covers the region: two layers, no hole (every column of the grid crosses the surface twice)
        assert S.euler_characteristic(tri, len(xyz)) is not None
        out.append(float(np.sqrt(np.mean(nrm[:, 0].astype(np.float64) ** 2 + nrm[:, 1].astype(np.float64) ** 2))))
    return out


def test_the_c1_sheet_meshes_flatter_than_the_isotropic_surface(ws):
    pos, params = ws.workloads.make_workload("c1", "lattice")
    a = dict(A.defaults(), min_neighbours=3)  # an interior particle has 5 neighbours (itself and 4 at 0.2)
    c, m, f, n = A.stage(params, pos, a)
    interior = (np.abs(pos[:, 0]) < 6.0) & (np.abs(pos[:, 1]) < 6.0)
    assert np.all(n[interior] == 5)
    kr = a["max_ratio"]
    assert np.all(m[interior, 2] == F32(kr))  # the normal axis is shortened k_r-fold
    rms_an, rms_iso = sheet_case(params, c, m, f, kr)
    assert rms_an <= 0.5 * rms_iso, (rms_an, rms_iso)


# ---- the restatement on merged and off-centre grids ---------------------------------------------------------------------
POSITIONS = {"centred": (0.0, 0.0, 0.0), "off-centre": (37.3, -21.7, 5.45)}


def _no_divisor(f, least):
    """The smallest factor >= least that does not divide f: the last merged cell is narrower than the others."""
    return next(m for m in range(least, int(f)) if f % m)


# merge factors per axis as functions of the reference-sized dims fdim (36 x 28 x 28 for the centred container)
MERGES = {"z": lambda f: (1, 1, 4), "zy": lambda f: (1, 5, 9), "zyx": lambda f: (3, 5, 9),
          "one-layer-x": lambda f: (int(f[0]), 9, 9),
          "ragged": lambda f: (_no_divisor(f[0], 5), _no_divisor(f[1], 3), _no_divisor(f[2], 2))}


def _grid_scene(ws, where, n=2000, seed=21):
    """About 2 000 points in an 8 x 6 x 6 container: three Gaussian clusters (sigma 0.3) and a uniform rest; and 600
    queries, half of them near points, the others uniform up to 1.5 beyond the container (clamped cells)."""
    params = ws.make_params(container_size=(8.0, 6.0, 6.0), container_position=POSITIONS[where])
    mn = np.asarray(params.ext_min[:3], np.float64)
    mx = np.asarray(params.ext_max[:3], np.float64)
    rng = np.random.default_rng(seed)
    centres = mn + rng.random((3, 3)) * (mx - mn)
    clustered = centres[rng.integers(0, 3, n * 3 // 5)] + rng.normal(0.0, 0.3, (n * 3 // 5, 3))
    uniform = mn + rng.random((n - len(clustered), 3)) * (mx - mn)
    x = np.clip(np.concatenate([clustered, uniform]), mn, mx).astype(F32)
    near = x[rng.choice(n, 300, replace=False)] + rng.normal(0.0, 0.05, (300, 3))
    wide = (mn - 1.5) + rng.random((300, 3)) * (mx - mn + 3.0)
    return params, x, np.concatenate([near, wide]).astype(F32)


def _candidates(bins, q, n):
    """(len(q), n) bool: particle j is in the candidate columns of query i."""
    cols = bins.columns(q)
    out = np.zeros((len(q), n), bool)
    rows = np.broadcast_to(np.arange(len(q))[:, None], cols.shape)
    out[rows[cols >= 0], bins.order[cols[cols >= 0]]] = True
    assert out.sum() == np.count_nonzero(cols >= 0)  # no particle twice in a query's columns
    return out


def _accepted(grid, x, q):
    """(len(q), n) bool: the float32 distance test of the kernels on every pair."""
    e = (x[None, :, :] - q[:, None, :]).astype(F32)
    d2 = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
    return ~(d2 > grid.d2_accept)


@pytest.mark.parametrize("where", list(POSITIONS))
def test_unit_merge_factors_bin_as_the_unmerged_restatement_did(ws, where):
    params, x, _ = _grid_scene(ws, where)
    g = A.Grid(params, merged=(1, 1, 1))
    b = A.Binned(g, x)
    # the restatement before it knew of merged cells, written out
    h = F32(params.smoothing_radius)
    org = np.floor(np.asarray(params.ext_min[:3], F32) / h).astype(np.int64) - A.GRID_PAD
    dim = np.floor(np.asarray(params.ext_max[:3], F32) / h).astype(np.int64) + A.GRID_PAD - org + 1
    c = np.clip(np.floor(x / h).astype(np.int64) - org, 0, dim - 1)
    key = (c[:, 0] * dim[1] + c[:, 1]) * dim[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(int(np.prod(dim)) + 1))
    assert np.array_equal(g.dim, dim) and np.array_equal(g.fdim, dim) and np.array_equal(g.org, org)
    assert np.array_equal(b.order, order) and np.array_equal(b.start, start)
    assert np.array_equal(A.Binned(A.Grid(params), x).start, start)  # the default is the un-merged grid
    if where == "off-centre":
        assert np.all(np.abs(org) >= 8) and len(set(np.sign(org))) == 2  # far from 0, mixed signs


@pytest.mark.parametrize("merge", list(MERGES))
@pytest.mark.parametrize("where", list(POSITIONS))
def test_merged_cells_hold_every_pair_within_h_and_accept_the_same_pairs(ws, where, merge):
    params, x, q = _grid_scene(ws, where)
    plain = A.Grid(params)
    merged = MERGES[merge](plain.fdim)
    g = A.Grid(params, merged)
    assert np.array_equal(g.dim, -(-plain.fdim // np.asarray(merged))) and np.array_equal(g.org, plain.org)
    if merge == "one-layer-x":
        assert g.dim[0] == 1
    if merge == "ragged":
        assert np.all(plain.fdim % np.asarray(merged) != 0)
    assert [m > 1 for m in merged] == {"z": [False, False, True], "zy": [False, True, True]}.get(merge, [True] * 3)
    b, b0 = A.Binned(g, x), A.Binned(plain, x)
    assert b.start[-1] == len(x) and len(b.start) == int(np.prod(g.dim)) + 1
    n = len(x)
    h = float(F32(params.smoothing_radius))
    for pts in (x, q):
        # the header's invariant: cell edges stay >= h, so every pair within h (float64, all pairs) is a candidate
        d = np.sqrt(((pts[:, None, :].astype(np.float64) - x[None, :, :].astype(np.float64)) ** 2).sum(2))
        cand = _candidates(b, pts, n)
        assert np.all(cand[d <= h])
        assert cand.sum() >= _candidates(b0, pts, n).sum()
        # ... and the distance test decides: the accepted pairs are the un-merged grid's
        acc = _accepted(g, x, pts)
        assert np.array_equal(cand & acc, _candidates(b0, pts, n) & acc)
        assert np.count_nonzero((cand & acc).sum(1) >= 8) >= len(pts) // 4
    # the same through the restated stage and fields: counts equal, float64 equal up to its own summation order, and
    # the float32 field of the merged order inside field64's bound
    a = A.defaults()
    s0 = A.stage(params, x, a)
    s1 = A.stage(params, x, a, merged=merged)
    assert np.array_equal(s1[3], s0[3]) and np.array_equal(s0[3], _accepted(g, x, x).sum(1))
    assert np.any(s0[3] >= a["min_neighbours"]) and np.any(s0[3] < a["min_neighbours"])
    # (the stage's float32 sums run in another order on the merged grid: the fields below take ONE stage as their input)
    r0, g0, tr0, tg0, n0 = A.field64(params, s0[0], s0[1], s0[2], q)
    r1, g1, tr1, tg1, n1 = A.field64(params, s0[0], s0[1], s0[2], q, merged=merged)
    assert np.array_equal(n1, n0) and np.count_nonzero(n0) > len(q) // 4 and np.count_nonzero(n0 == 0) > len(q) // 20
    # float64 sums of the same terms in two orders differ by at most n 2^-53 sum |t| <= 2^-29 of the float32 bound
    assert np.all(np.abs(r1 - r0) <= tr0 * 2.0 ** -24) and np.all(np.abs(g1 - g0) <= tg0 * 2.0 ** -24)
    assert np.allclose(tr1, tr0, rtol=1e-12, atol=0) and np.allclose(tg1, tg0, rtol=1e-12, atol=0)
    rho, grad = A.field32(params, s0[0], s0[1], s0[2], q, merged=merged)
    assert np.all(np.abs(rho - r0) <= tr0) and np.all(np.abs(grad - g0) <= tg0)
    assert np.all(rho[n0 == 0] == 0) and np.all(grad[n0 == 0] == 0)
    iso_m = A.iso_field32(params, x, q, merged=merged)
    iso_0 = A.iso_field32(params, x, q)
    assert np.array_equal(iso_m == 0, iso_0 == 0) and np.allclose(iso_m, iso_0, rtol=64 * 2.0 ** -24, atol=0)
