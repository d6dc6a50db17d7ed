"""The read-only calls (density field, anisotropic stage and field, both meshes, the ray caster) on every kind of cell
grid a handle can have: merged cells (z, z + y, z + y + x: the developer build's WS_CELL_BUDGET, and the product
library's own merge at a small radius), other smoothing radii and re-grids through ws_set_params, and containers far
from the origin.  include/wsfluid.h promises the same results on "the handle's grid" whatever it is; the other field
test files all run at h = 0.25 on un-merged cells around the origin.

The scenes are denser than the step tests': a query needs 8 particles within h for the float64 comparison to mean
something, and the fluid fills its container at a number density the container decides (the pressure solve pushes it
apart), so 16 384 particles sit in a 5.6 x 3.9 x 3.9 container at h = 0.25 and a 4.56 x 3.16 x 3.16 one at h = 0.2 (about 14
particles within h), and for the radii down to 0.15 in a 3 x 2 x 2 one.  Every share of "well-fed" and "empty" queries asserted here
comes from the float64 brute force or the host march, never from the library."""
import contextlib
import os

import numpy as np
import pytest

import aniso_ref as A
import rays_ref as R
import surface_ref as S
from test_gpu_aniso_surface import ISO_LIMIT, _check_f64, _check_stage, _slab_run, padded, params_of, same_bits
from test_gpu_density_field import brute_force, check_field, nodes
from test_gpu_rays import make_rays
from test_gpu_small_radius import _one_step_vs_oracle

pytestmark = pytest.mark.gpu
F32 = np.float32

N = 16384
SEED = 12
STEPS = 25
SIZES = {0.25: (5.6, 3.9, 3.9), 0.2: (4.56, 3.16, 3.16)}  # (26 x 20 x 20 reference-sized cells either way)
DENSE_SIZE = (3.0, 2.0, 2.0)
GRAVITY = (4.0, -9.8, 2.0, 0.0)
# developer-build cell budgets on SIZES[0.25] (26 x 20 x 20 reference-sized cells) -> the axes they merge
BUDGETS = {"4000": "z", "800": "zy", "100": "zyx"}
# container positions with large offsets of mixed signs; no wall is a whole number of cells from 0 at either radius
OFFSETS = {"east": (37.35, -21.7, 5.47), "west": (-64.23, 3.13, 18.93)}
# (kind, budget or container position, h)
GRIDS = ([("merged", b, 0.25) for b in BUDGETS]
         + [("offset", o, h) for o in OFFSETS for h in (0.25, 0.2)])
GRID_IDS = ["%s-%s-h%g" % g for g in GRIDS]
ARITH = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
ON_GRIDS = pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)


def scene(ws, h=0.25, position=(0.0, 0.0, 0.0), size=None):
    size = size or SIZES[h]
    params = ws.make_params(container_size=size, container_position=position, gravity=GRAVITY, smoothing_radius=F32(h))
    pos = ws.workloads.uniform_cloud(N, SEED, list(params.ext_min), list(params.ext_max))
    return pos, params


def probes(cur, params, seed=3, spread=0.05):
    """7 968 query points: 4 800 at particles + N(0, spread), 2 400 uniform in the container padded by h, 256 exactly at
    particles (d == 0: no gradient term), 512 at least 10 h outside the grid along one to three axes (clamped cells: the
    field there is exactly 0), eight of them 10^6 away."""
    rng = np.random.default_rng(seed)
    h = float(params.smoothing_radius)
    mn = np.asarray(params.ext_min[:3], np.float64) - h
    mx = np.asarray(params.ext_max[:3], np.float64) + h
    near = cur[rng.choice(len(cur), 4800, replace=False)] + rng.normal(0.0, spread, (4800, 3))
    inside = mn + rng.random((2400, 3)) * (mx - mn)
    at = cur[rng.choice(len(cur), 256, replace=False)].astype(np.float64)
    # the grid ends at most 3 h beyond the container (GRID_PAD cells and the one the wall is in)
    out = rng.random((512, 3)) < 0.5
    out[~out.any(1), 0] = True
    dist = 12.0 * h + rng.exponential(2.0, (512, 3))
    dist[:8] = 1e6
    up = rng.random((512, 3)) < 0.5
    far = np.where(out, np.where(up, mx + dist, mn - dist), mn + rng.random((512, 3)) * (mx - mn))
    q = np.concatenate([near, inside, at, far]).astype(F32)
    assert np.all((q[-768:-512, None, :] == cur[None, :, :]).all(2).any(1))
    return q


def well_fed(cnt, case, dense=0.25):
    """The float64 brute force's own counts: enough queries with 8 or more particles, and enough with none."""
    share = (float(np.mean(cnt >= 8)), float(np.mean(cnt == 0)))
    print("%s: %d queries, %.1f %% with 8 or more particles, %.1f %% with none" % (case, len(cnt), 100 * share[0], 100 * share[1]))
    assert share[0] >= dense and share[1] >= 0.05, (case, share)


def density_checks(ws, w, params, case, arith, spacings=(0.5, 1.5), dense=0.25):
    """Grids over the container padded by h at the given spacings (in h: the brick form and the points form) and the
    probe points against the float64 brute force; grid == points bit for bit."""
    cur = w.read_positions()
    h = F32(params.smoothing_radius)
    for per_h in spacings:
        origin, spacing, dims = padded(params, h * F32(per_h), h)
        assert all(d % 4 for d in dims), dims
        rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
        q = nodes(origin, spacing, dims)
        name = "%s grid %.1f h" % (case, per_h)
        well_fed(check_field(name, arith, q, rho, grad, cur, params, ws), name, dense)
        rp, gp = w.sample_density_points(q, gradient=True)
        assert same_bits(rp, rho.reshape(-1)) and same_bits(gp, grad.reshape(-1, 3)), name
        assert same_bits(w.sample_density_grid(origin, spacing, dims), rho), name
    q = probes(cur, params)
    rho, grad = w.sample_density_points(q, gradient=True)
    well_fed(check_field(case + " points", arith, q, rho, grad, cur, params, ws), case + " points", dense)
    assert not rho[-512:].any() and not grad[-512:].any()
    assert np.all(rho[-768:-512] > 0)  # (at a particle: d == 0, its own term has no gradient part)
    return cur


@contextlib.contextmanager
def cell_budget(cells):
    """WS_CELL_BUDGET of the developer build, which reads it when a handle derives its grid (at create): set for the
    creates inside the block, and put back."""
    before = os.environ.get("WS_CELL_BUDGET")
    os.environ["WS_CELL_BUDGET"] = cells
    try:
        yield
    finally:
        if before is None:
            del os.environ["WS_CELL_BUDGET"]
        else:
            os.environ["WS_CELL_BUDGET"] = before


class _Handles:
    """One handle per (grid, arithmetic) at step 25 with what describes its grid; made when first asked for, shared by
    the tests that follow on the same grid, and closed when another grid is asked for: at most two are open (a test
    function visits the grids in turn, both arithmetics of one next to each other; 25 steps of this scene are cheap)."""

    def __init__(self, ws, devlib):
        self.ws, self.devlib, self.made = ws, devlib, {}

    def get(self, grid, ieee):
        for key in [k for k in self.made if k[0] != grid]:
            self.made.pop(key)["w"].close()
        if (grid, ieee) not in self.made:
            kind, what, h = grid
            if kind == "merged":
                pos, params = scene(self.ws, h)
                with cell_budget(what):
                    w = self.ws.FluidWorker(pos, params, ieee_division=ieee, library=self.devlib)
            else:
                pos, params = scene(self.ws, h, OFFSETS[what])
                w = self.ws.FluidWorker(pos, params, ieee_division=ieee)
            w.run(STEPS)
            merged = w.stats()["cells_merged"]
            g = A.Grid(params, merged)
            assert tuple(int(v) for v in g.dim) == tuple(w.grid_dims()), (g.dim, w.grid_dims(), merged)
            if kind == "merged":
                axes = BUDGETS[what]
                assert [m > 1 for m in merged] == ["x" in axes, "y" in axes, "z" in axes], merged
                assert any(f % m for f, m in zip(g.fdim, merged)), "no ragged last cell"
            else:
                assert merged == (1, 1, 1)
                assert np.any(np.abs(g.org) > 90) and len(set(np.sign(g.org))) == 2  # far from 0, mixed signs
                e = np.asarray(list(params.ext_min[:3]) + list(params.ext_max[:3]), F32) / F32(h)
                assert np.all(e != np.floor(e))
            self.made[grid, ieee] = dict(w=w, pos=pos, params=params, merged=merged, case="%s-%s-h%g" % grid,
                                         arith="ieee-division" if ieee else "hw-rcp-sqrt")
        return self.made[grid, ieee]

    def close(self):
        for rec in self.made.values():
            rec["w"].close()


@pytest.fixture(scope="module")
def handles(ws, devlib):
    hs = _Handles(ws, devlib)
    yield hs
    hs.close()


# ---- (a) merged cells and (d) off-centre containers: the same checks on every grid ---------------------------------------
@ARITH
@ON_GRIDS
def test_the_density_field_against_float64_on_this_grid(ws, handles, grid, ieee):
    """WS_CELL_BUDGET 4000 / 800 / 100 merge (1, 1, 3), (1, 3, 6) and (5, 6, 6) reference-sized cells: 26 x 20 x 7,
    26 x 7 x 4 and 6 x 4 x 4 grid cells.  grid_dims()[0] == 1 is out of the hook's reach: the budget is floored at 64 and
    y and z keep at least three cells, at most 5 x 5 of them in a column layer, so x keeps 64 / 25 = 2 layers or more
    (tests/test_aniso_reference.py restates that shape on the CPU)."""
    rec = handles.get(grid, ieee)
    density_checks(ws, rec["w"], rec["params"], "grids " + rec["case"], rec["arith"])


@ARITH
@ON_GRIDS
def test_the_stage_and_the_anisotropic_field_on_this_grid(ws, handles, grid, ieee):
    rec = handles.get(grid, ieee)
    w, params, merged, case = rec["w"], rec["params"], rec["merged"], rec["case"]
    cur = w.read_positions()
    ids = np.sort(np.random.default_rng(2).choice(N, 768, replace=False))
    restated = {}
    _check_stage(ws, w, params, case, merged=merged, ids=ids, restated=restated)
    counts = restated["defaults"][3]  # (the restatement's own neighbour counts: both branches of the stage are taken)
    assert np.mean(counts >= 12) > 0.25 and np.any(counts < 12)
    a = params_of(ws, A.defaults())
    stage = w.anisotropy(a)
    h = F32(params.smoothing_radius)
    # the points form on a coarse grid, the brick form at h / 2, and probe points: about 1 000 queries of each against
    # float64 (the restatement walks every candidate of a merged cell: the queries are thinned, not the grids)
    origin, spacing, dims = padded(params, F32(1.5) * h, h)
    coarse = A.grid_nodes(origin, spacing, dims)
    rho_c, grad_c = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
    origin, spacing, dims = padded(params, h / F32(2), h)
    fine = A.grid_nodes(origin, spacing, dims)
    rho_f, grad_f = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
    pr, pg = w.sample_aniso_points(fine, gradient=True, aniso=a)
    assert same_bits(pr, rho_f.reshape(-1)) and same_bits(pg, grad_f.reshape(-1, 3)) and np.count_nonzero(pr) > len(pr) // 4
    pc, gc = w.sample_aniso_points(coarse, gradient=True, aniso=a)
    assert same_bits(pc, rho_c.reshape(-1)) and same_bits(gc, grad_c.reshape(-1, 3))
    q = probes(cur, params)[::8]
    rho_p, grad_p = w.sample_aniso_points(q, gradient=True, aniso=a)
    for name, pts, rho, grad in (("coarse grid", coarse[::3], rho_c.reshape(-1)[::3], grad_c.reshape(-1, 3)[::3]),
                                 ("fine grid", fine[::61], rho_f.reshape(-1)[::61], grad_f.reshape(-1, 3)[::61]),
                                 ("points", q, rho_p, grad_p)):
        _check_f64(params, stage, pts, rho, grad, "%s %s" % (case, name), merged=merged)
        if ieee:  # the IEEE form is the float32 restatement's, bit for bit
            r32, g32 = A.field32(params, stage[0], stage[1], stage[2], pts, merged=merged)
            assert same_bits(r32, rho) and same_bits(g32, grad), name
    # the isotropic limit is the density field
    limit = params_of(ws, ISO_LIMIT)
    for x, y in zip(w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=limit),
                    w.sample_density_grid(origin, spacing, dims, gradient=True)):
        assert same_bits(x, y)
    for x, y in zip(w.sample_aniso_points(q, gradient=True, aniso=limit), w.sample_density_points(q, gradient=True)):
        assert same_bits(x, y)


@ARITH
@ON_GRIDS
def test_both_meshes_equal_the_restated_mesh_of_the_sampled_field_on_this_grid(ws, handles, grid, ieee):
    rec = handles.get(grid, ieee)
    w, params = rec["w"], rec["params"]
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    a = params_of(ws, A.defaults())
    for name, sample, extract in (
            ("density", lambda: w.sample_density_grid(origin, spacing, dims, gradient=True),
             lambda iso: w.extract_surface(origin, spacing, dims, iso)),
            ("aniso", lambda: w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a),
             lambda iso: w.extract_aniso_surface(origin, spacing, dims, iso, aniso=a))):
        rho, grad = sample()
        iso = F32(np.median(rho[rho > 0]))
        want = S.extract(rho, grad, origin, spacing, dims, iso)
        assert len(want[2]) > 0, name
        for x, y in zip(extract(iso), want):
            assert same_bits(x, y), name


def _centre(params):
    return (np.asarray(params.ext_min[:3], np.float64) + np.asarray(params.ext_max[:3], np.float64)) / 2


def scene_rays(cur, params):
    """make_rays with its spheres about this container: radius 5 > the half diagonal 3.8 of the larger of SIZES; |v| >= 1.2 reaches
    24 > 5 + 3.8 in 160 steps of h / 2 = 0.125 (19 > 8.8 at h = 0.2), and 3.6 reaches 72 (58 at h = 0.2) from up to 54."""
    return make_rays(cur, params, radius=5.0, far=(50.0, 54.0), centre=_centre(params))


def scene_march(ws, params):
    h = F32(params.smoothing_radius)
    return ws.fluid.ray_params(0.0, float(h / F32(2)), 160, 6, float(F32(params.target_density) / F32(2)))


def _scale(params):
    """The container's size over that of SIZES[0.25]."""
    return (float(params.ext_max[0]) - float(params.ext_min[0])) / SIZES[0.25][0]


def scene_camera(ws, params, size=(40, 28)):
    """From above and in front of the container, 45 degrees down, at a distance in proportion to the container;
    40 x 28 is no multiple of the 8 x 8 tile."""
    s = np.sqrt(0.5)
    eye = (_centre(params) + _scale(params) * np.array([0.3, 3.6, 3.6])).astype(F32)
    vectors = (eye, np.array([0.0, -s, -s], F32), np.array([1.0, 0.0, 0.0], F32),
               (np.array([0.0, s, -s]) * (size[1] / size[0])).astype(F32))
    return ws.fluid.camera(*vectors), vectors, size


def camera_march(ws, params):
    """The rays of a camera share their origin, so at t = 0 they all start inside the fluid or all outside: the
    camera's march begins at a near distance that cuts through the fluid (the eye is 5.1 from the container's centre
    at h = 0.25), which leaves rays that start inside (K == 0), rays that enter later and rays that miss."""
    h = F32(params.smoothing_radius)
    return ws.fluid.ray_params(2.85 * _scale(params), float(h / F32(2)), 160, 6, float(F32(params.target_density) / F32(2)))


def ray_shares(K, what):
    m = len(K)
    shares = {"K>=1": np.count_nonzero(K >= 1) / m, "miss": np.count_nonzero(K < 0) / m, "K=0": np.count_nonzero(K == 0) / m}
    print("%s: %d rays, %s" % (what, m, shares))
    # the host march's own result, so the comparison cannot pass vacuously
    assert shares["K>=1"] >= 0.25 and shares["miss"] >= 0.05 and shares["K=0"] >= 0.05, (what, shares)


@ARITH
@ON_GRIDS
def test_rays_and_a_camera_against_a_host_march_on_this_grid(ws, handles, grid, ieee):
    rec = handles.get(grid, ieee)
    w, params = rec["w"], rec["params"]
    march = scene_march(ws, params)
    o, v, cls = scene_rays(w.read_positions(), params)
    cam, vectors, size = scene_camera(ws, params)
    near = camera_march(ws, params)
    co, cv = R.camera_rays(*vectors, size)
    for field in ("density", "aniso"):
        a = ws.fluid.aniso_params() if field == "aniso" else None
        if a is None:
            def host_field(p):
                return w.sample_density_points(p, gradient=True)
        else:
            def host_field(p):
                return w.sample_aniso_points(p, gradient=True, aniso=a)
        want_t, want_n, K = R.cast(host_field, march, o, v)
        ray_shares(K, "%s %s" % (rec["case"], field))
        assert np.all(K[cls == "c"] < 0)
        t, n = w.cast_rays(march, o, v, aniso=a)
        assert same_bits(t, want_t) and same_bits(n, want_n), field
        want_t, want_n, K = R.cast(host_field, near, co, cv)
        ray_shares(K, "%s %s camera" % (rec["case"], field))
        t, n = w.cast_camera(near, cam, size, aniso=a)
        assert t.shape == (size[1], size[0]) and same_bits(t.reshape(-1), want_t) and same_bits(n.reshape(-1, 3), want_n), field


def test_two_slabs_on_the_coarsest_grid_give_the_single_handles_bits(ws, devlib, handles):
    grid = ("merged", "100", 0.25)
    rec = handles.get(grid, False)
    w, params, pos = rec["w"], rec["params"], rec["pos"]
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    q = probes(w.read_positions(), params)
    a = params_of(ws, A.defaults())
    iso = F32(100.0)  # (the fluid's density is about 200, the field outside it 0)
    march = scene_march(ws, params)
    o, v, _ = scene_rays(w.read_positions(), params)

    def calls(s, r=None):
        kw = {} if r is None else {"want": r != 1}  # rank 1 only contributes
        return (s.sample_density_grid(origin, spacing, dims, gradient=True, **kw), s.sample_density_points(q, gradient=True, **kw),
                s.extract_aniso_surface(origin, spacing, dims, iso, aniso=a, **kw), s.cast_rays(march, o, v, **kw),
                s.cast_rays(march, o, v, aniso=a, **kw))

    want = calls(w)
    assert len(want[2][2]) > 0 and np.isfinite(want[3][0]).any()
    with cell_budget(grid[1]):  # (the ranks are created inside)
        got = _slab_run(ws, params, pos, 2, STEPS, calls, library=devlib)
    for g_part, w_part in zip(got[0], want):
        for x, y in zip(g_part, w_part):
            assert same_bits(x, y)
    assert all(x is None for part in got[1] for x in part)


# ---- (b) the product library merges on its own -----------------------------------------------------------------------------
def test_the_product_library_merges_at_a_small_radius_and_samples_the_same_field(ws):
    """16 x 9 x 9 at h = 0.04: 2.1e7 reference-sized cells, above the 2^24 budget of any handle this small.  The fluid is
    a jittered lattice of spacing h / 2 (32 x 32 x 16) in the container's lowest corner, sampled where it was put (at
    120 000 particles per unit volume a step would throw it across the container)."""
    h = F32(0.04)
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), smoothing_radius=h)
    rng = np.random.default_rng(8)
    block = (32, 32, 16)
    ijk = np.stack(np.meshgrid(*(np.arange(b) for b in block), indexing="ij"), -1).reshape(-1, 3)
    step = float(h) / 2
    pos = (np.asarray(params.ext_min[:3], np.float64) + (ijk + 0.5 * rng.random((N, 3))) * step).astype(F32)
    assert len(pos) == N and np.all(pos >= np.asarray(params.ext_min[:3], F32))
    w = ws.FluidWorker(pos, params)
    merged = w.stats()["cells_merged"]
    assert merged != (1, 1, 1), merged
    assert tuple(int(v) for v in A.Grid(params, merged).dim) == tuple(w.grid_dims())
    cur = w.read_positions()
    lo, hi = cur.min(0).astype(np.float64), cur.max(0).astype(np.float64)
    rng = np.random.default_rng(9)
    near = cur[rng.choice(N, 4800, replace=False)] + rng.normal(0.0, float(h) / 4, (4800, 3))
    box = (lo - 2 * float(h)) + rng.random((2400, 3)) * (hi - lo + 4 * float(h))
    at = cur[rng.choice(N, 256, replace=False)]
    # 256 outside the grid (it ends GRID_PAD cells and the wall's own beyond the container): clamped cells, nobody near
    side = rng.random((256, 3)) < 0.5
    side[~side.any(1), 1] = True
    gap = 10.0 * float(h) + rng.exponential(1.0, (256, 3))
    mn, mx = (np.asarray(e[:3], np.float64) for e in (params.ext_min, params.ext_max))
    far = np.where(side, np.where(rng.random((256, 3)) < 0.5, mx + 3 * float(h) + gap, mn - 3 * float(h) - gap), box[:256])
    q = np.concatenate([near, box, at, far]).astype(F32)
    rho, grad = w.sample_density_points(q, gradient=True)
    assert not rho[-256:].any() and not grad[-256:].any()
    case = "grids product merge %s" % (merged,)
    well_fed(check_field(case + " points", "hw-rcp-sqrt", q, rho, grad, cur, params, ws), case + " points", dense=0.5)
    spacing = np.full(3, h / F32(2), F32)
    origin = (lo - float(h)).astype(F32)
    dims = tuple(int(v) for v in np.ceil((hi - lo + 2 * float(h)) / spacing.astype(np.float64)).astype(np.int64) + 1)
    rg, gg = w.sample_density_grid(origin, spacing, dims, gradient=True)
    qn = nodes(origin, spacing, dims)
    well_fed(check_field(case + " grid", "hw-rcp-sqrt", qn, rg, gg, cur, params, ws), case + " grid", dense=0.5)
    rp, gp = w.sample_density_points(qn, gradient=True)
    assert same_bits(rp, rg.reshape(-1)) and same_bits(gp, gg.reshape(-1, 3))
    w.close()


# ---- (c) other radii, and what a re-grid leaves behind -------------------------------------------------------------------
def test_the_field_follows_the_smoothing_radius_through_regrids(ws):
    """h = 0.25 -> 0.2 -> 0.4 -> 0.15 on one handle (the cell count grows, shrinks, grows), ten steps between them; after
    each ws_set_params the field and the stage are those of the NEW radius, and at the end those of a fresh handle."""
    pos, params = scene(ws, 0.25, size=DENSE_SIZE)
    w = ws.FluidWorker(pos, params)
    ids = np.sort(np.random.default_rng(4).choice(N, 512, replace=False))
    cells = [int(np.prod(w.grid_dims()))]
    for h in (0.2, 0.4, 0.15):
        w.run(10)
        _, params = scene(ws, h, size=DENSE_SIZE)
        w.set_params(params)
        cells.append(int(np.prod(w.grid_dims())))
        assert w.stats()["cells_merged"] == (1, 1, 1) and tuple(A.Grid(params).dim) == tuple(w.grid_dims())
        case = "grids regrid h=%g" % h
        density_checks(ws, w, params, case, "hw-rcp-sqrt", spacings=(0.5,))
        _check_stage(ws, w, params, case, ids=ids)
    assert cells[1] > cells[0] and cells[2] < cells[1] and cells[3] > cells[2], cells
    # no stale table: a handle that never had another grid gives the same bits from the same state
    state = w.read_vec("particles")
    fresh = ws.FluidWorker(pos, params)
    fresh.write_slice("particles", state)
    hh = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, hh / F32(2), hh)
    q = probes(w.read_positions(), params)
    a = params_of(ws, A.defaults())
    rho = w.sample_density_grid(origin, spacing, dims)
    iso = F32(np.median(rho[rho > 0]))

    def calls(x):
        return (x.sample_density_grid(origin, spacing, dims, gradient=True) + x.sample_density_points(q, gradient=True)
                + x.anisotropy(a) + x.sample_aniso_points(q[::4], gradient=True, aniso=a)
                + x.extract_surface(origin, spacing, dims, iso))

    got, want = calls(w), calls(fresh)
    assert len(want[-1]) > 0
    for x, y in zip(got, want):
        assert same_bits(x, y)
    w.close()
    fresh.close()


# ---- (d) off-centre containers: the step, and translation ----------------------------------------------------------------
@ARITH
@pytest.mark.parametrize("h", [0.25, 0.2])
@pytest.mark.parametrize("where", list(OFFSETS))
def test_one_step_in_an_off_centre_container_against_the_oracle(oracle, ws, handles, where, h, ieee):
    rec = handles.get(("offset", where, h), ieee)
    state = rec["w"].read_vec("particles")
    assert np.isfinite(state["position"]).all()
    stats, _ = _one_step_vs_oracle(oracle, ws, rec["pos"], rec["params"], "grids step %s" % rec["case"], state=state, ieee=ieee)
    assert stats["cells_merged"] == (1, 1, 1)


def test_a_translation_by_whole_cells_keeps_every_neighbour_count(ws):
    """(64, -32, 16) is 256, -128 and 64 cells of h = 0.25, and exact in float32 on a cloud rounded to 2^-16: the
    translated cloud in the translated container has the same pairs, in the library and in the brute force."""
    shift = np.array([64.0, -32.0, 16.0], F32)
    pos, params = scene(ws, 0.25)
    pos = (np.round(pos.astype(np.float64) * 65536.0) / 65536.0).astype(F32)
    moved = pos + shift
    assert np.array_equal(moved.astype(np.float64), pos.astype(np.float64) + shift)
    _, params_m = scene(ws, 0.25, tuple(float(s) for s in shift))
    rng = np.random.default_rng(6)
    q = (pos[rng.choice(N, 4000, replace=False)] + (np.round(rng.normal(0, 0.1, (4000, 3)) * 65536.0) / 65536.0)).astype(F32)
    # ... and 400 in the padding cells beyond the walls, up to 2 h outside, where most have nobody within h
    wall = np.asarray(params.ext_max[:3], np.float64)
    out = np.round((wall + rng.uniform(0.5, 2.0, (400, 3)) * 0.25) * np.where(rng.random((400, 3)) < 0.5, -1.0, 1.0) * 65536.0) / 65536.0
    q = np.concatenate([q, out.astype(F32)])
    assert np.array_equal((q + shift).astype(np.float64), q.astype(np.float64) + shift)
    cnt = brute_force(q, pos, params, ws)[3]
    assert np.array_equal(brute_force(q + shift, moved, params_m, ws)[3], cnt)
    a = params_of(ws, A.defaults())
    counts = []
    for x, p, pts in ((pos, params, q), (moved, params_m, q + shift)):
        w = ws.FluidWorker(x, p)
        assert tuple(A.Grid(p).dim) == tuple(w.grid_dims())
        counts.append(w.anisotropy(a)[3])
        rho, grad = w.sample_density_points(pts, gradient=True)
        case = "grids translation %s" % (tuple(p.ext_min[:3]),)
        well_fed(check_field(case, "hw-rcp-sqrt", pts, rho, grad, x, p, ws), case)
        w.close()
    assert np.array_equal(counts[0], counts[1])
    restated = A.stage(params, pos, A.defaults(), ids=np.arange(0, N, 16))[3]
    assert np.array_equal(counts[0][::16], restated) and np.mean(restated >= 8) >= 0.25
