"""ws_read_velocities, ws_sample_velocity_grid / _points and ws_advect_points on the GPU: the density contract, a
constant velocity, bit for bit against the numpy restatement (tests/velocity_ref.py) on IEEE handles and against float64
in both arithmetics, grid == points, the readback, the march against a host march built on the points call, no effect on
the simulation, other cell grids, slabs, errors.

Default scene (as tests/test_gpu_rays.py): a 16 x 9 x 9 container, a 65 536-particle uniform cloud (seed 1234), 30 steps,
both arithmetics.  The bit-for-bit cases against numpy use 1 024 particles and at most 512 queries."""
import ctypes as C

import numpy as np
import pytest

import velocity_ref as V
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_field_grids import N as GRID_N
from test_gpu_field_grids import OFFSETS, STEPS as GRID_STEPS
from test_gpu_field_grids import scene as grid_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
STEPS = 30
CONST = np.array([2.0, -0.5, 0.0], F32)
ARITH = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])


def _arith(ieee):
    return "ieee-division" if ieee else "hw-rcp-sqrt"


def _box(params):
    return np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)


def probes(cur, box, h, seed=3, n=(1200, 600, 128, 128)):
    """Query points: at particles + N(0, h / 5), uniform in the box padded by h, exactly at particles, and 12 h and more
    outside the box (clamped cells: nobody near)."""
    rng = np.random.default_rng(seed)
    lo, hi = box[0] - h, box[1] + h
    near = cur[rng.choice(len(cur), n[0], replace=False)] + rng.normal(0.0, h / 5, (n[0], 3))
    inside = lo + rng.random((n[1], 3)) * (hi - lo)
    at = cur[rng.choice(len(cur), n[2], replace=False)].astype(np.float64)
    far = hi + 12.0 * h + rng.exponential(2.0, (n[3], 3))
    return np.concatenate([near, inside, at, far]).astype(F32)


def cover(box, spacing, pad):
    """A grid of the given spacing over the box padded by pad: (origin, spacing (3,), dims)."""
    mn, mx = (box[0] - pad).astype(F32), (box[1] + pad).astype(F32)
    sp = np.full(3, F32(spacing), F32)
    return mn, sp, tuple(int(v) for v in np.ceil((mx - mn) / sp).astype(np.int64) + 1)


class _Scene:
    """One worker per arithmetic at step 30 with its positions and velocities (read once, shared, never modified)."""

    def __init__(self, ws):
        self.ws = ws
        self.params = ws.make_params(container_size=(16.0, 9.0, 9.0))
        self.pos = ws.workloads.uniform_cloud(65536, 1234, list(self.params.ext_min), list(self.params.ext_max))
        self.made = {}

    def get(self, ieee):
        if ieee not in self.made:
            w = self.ws.FluidWorker(self.pos, self.params, ieee_division=ieee)
            w.run(STEPS)
            cur, vel = w.read_positions(), w.read_velocities()
            cur.setflags(write=False)
            vel.setflags(write=False)
            self.made[ieee] = (w, cur, vel)
        return self.made[ieee]

    def close(self):
        for w, _, _ in self.made.values():
            w.close()


@pytest.fixture(scope="module")
def scene(ws):
    s = _Scene(ws)
    yield s
    s.close()


# ---- shared checks (the default scene and the other grids) -------------------------------------------------------------------
def check_density_contract(w, cur, box, h, case):
    """out_density of the velocity calls == ws_sample_density_* bit for bit: at points, on grids at h / 2 (the density
    sampler's brick form), 1.5 h (its points form) and with dims that are no multiples of 4; with and without the
    velocity output."""
    q = probes(cur, box, h)
    u, rho = w.sample_velocity_points(q, density=True)
    want = w.sample_density_points(q)
    assert same_bits(rho, want), case
    assert np.count_nonzero(want) > len(q) // 4 and not want[-128:].any() and not u[-128:].any(), case
    only = np.empty(len(q), F32)
    assert w._L.ws_sample_velocity_points(w._h, q.ctypes.data, len(q), None, only.ctypes.data) == 0
    assert same_bits(only, want), case
    assert same_bits(w.sample_velocity_points(q), u), case  # (out_density NULL)
    grids = [cover(box, F32(h) / F32(2), h), cover(box, F32(1.5) * F32(h), h)]
    mid = (0.5 * (cur.min(0).astype(np.float64) + cur.max(0))).astype(F32)
    grids.append((mid - F32(h), np.full(3, F32(h) / F32(2), F32), (13, 7, 5)))
    for origin, spacing, dims in grids:
        ug, rg = w.sample_velocity_grid(origin, spacing, dims, density=True)
        wg = w.sample_density_grid(origin, spacing, dims)
        assert rg.shape == wg.shape == dims[::-1] and ug.shape == dims[::-1] + (3,), (case, dims)
        assert same_bits(rg, wg), (case, dims)
        assert np.count_nonzero(wg) > 0 and not ug[wg == 0].any(), (case, dims)
    return q, u, rho


def check_grid_equals_points(w, box, h, case):
    for per_h in (0.5, 1.0, 1.5):
        origin, spacing, dims = cover(box, F32(per_h) * F32(h), h)
        ug, rg = w.sample_velocity_grid(origin, spacing, dims, density=True)
        nodes = V.A.grid_nodes(origin, spacing, dims)
        up, rp = w.sample_velocity_points(nodes, density=True)
        assert same_bits(ug.reshape(-1, 3), up) and same_bits(rg.reshape(-1), rp), (case, per_h)
        assert np.count_nonzero(rp) > 0 and np.count_nonzero(rp == 0) > 0, (case, per_h)


def make_tracers(ws, w, cur, params, box, seed, each):
    """Four classes of `each` tracers (the class of each in cls): at particle positions, uniform in the box, in the air
    above every particle, and within h of the surface rho = target_density / 2 seen from above (found with ws_cast_rays)."""
    rng = np.random.default_rng(seed)
    h = float(params.smoothing_radius)
    lo, hi = box
    at = cur[rng.choice(len(cur), each, replace=False)].astype(np.float64)
    inside = lo + rng.random((each, 3)) * (hi - lo)
    air = lo + rng.random((each, 3)) * (hi - lo)
    air[:, 1] = float(cur[:, 1].max()) + 1.01 * h + rng.random(each)
    o = lo + rng.random((each, 3)) * (hi - lo)
    o[:, 1] = float(cur[:, 1].max()) + 1.0
    v = np.tile(np.array([0.0, -1.0, 0.0]), (each, 1))
    steps = int(np.ceil((o[0, 1] - lo[1]) / (h / 2))) + 4
    march = ws.fluid.ray_params(0.0, h / 2, steps, 6, float(F32(params.target_density) / F32(2)))
    t, _ = w.cast_rays(march, o, v, normals=False)
    hit = np.isfinite(t)
    assert hit.sum() >= each // 2, hit.sum()
    surf = o[hit] + t[hit, None].astype(np.float64) * v[hit]
    surf[:, 1] += rng.uniform(-h, h, int(hit.sum()))
    pts = np.concatenate([at, inside, air, surf]).astype(F32)
    cls = np.asarray(["particle"] * each + ["inside"] * each + ["air"] * each + ["surface"] * len(surf))
    return pts, cls


def check_march(ws, w, pts, cls, dt, substeps, case):
    """ws_advect_points == the host march over ws_sample_velocity_points, bit for bit; the host march itself takes every
    branch; the optional outputs are the field at out_xyz; a tracer's bits do not depend on its neighbours in the call."""
    def field(p):
        return w.sample_velocity_points(p, density=True)

    want, took = V.advect(field, dt, substeps, pts)
    counts = {k: int(v.sum()) for k, v in took.items()}
    print("%s dt %+.4f x %d: %d tracers, branches %s, per class %s" % (
        case, dt, substeps, len(pts), counts,
        {c: tuple(int(took[k][cls == c].sum()) for k in ("air", "euler", "ordinary")) for c in np.unique(cls)}))
    # a condition on the inputs: the host march's own result, so the comparison cannot pass vacuously
    assert counts["air"] > 0 and counts["euler"] > 0 and counts["ordinary"] > 0, counts
    assert took["air"][cls == "air"].all() and np.array_equal(want[cls == "air"], pts[cls == "air"])
    march = ws.fluid.advect_params(dt, substeps)
    out, u, rho = w.advect_points(march, pts, field=True)
    bad = np.flatnonzero((out.view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, (case, bad[:8], out[bad[:8]], want[bad[:8]], cls[bad[:8]])
    uf, rf = field(out)
    assert same_bits(u, uf) and same_bits(rho, rf), case
    assert same_bits(w.advect_points(march, pts), out), case  # (positions alone)
    return out


# ---- 1. the density contract --------------------------------------------------------------------------------------------------
@ARITH
def test_out_density_is_the_density_samplers_bits(scene, ieee):
    w, cur, _ = scene.get(ieee)
    check_density_contract(w, cur, _box(scene.params), float(scene.params.smoothing_radius), "default " + _arith(ieee))


# ---- 2. a constant velocity ---------------------------------------------------------------------------------------------------
@ARITH
def test_a_constant_velocity_comes_back_exactly(scene, ieee):
    ws = scene.ws
    _, cur, _ = scene.get(ieee)
    w = ws.FluidWorker(scene.pos, scene.params, ieee_division=ieee)
    rec = w.read_vec("particles")
    rec["position"][:, :3] = cur
    rec["velocity"][:, :3] = CONST
    w.write_slice("particles", rec)
    assert np.array_equal(w.read_velocities(), np.tile(CONST, (len(cur), 1))) and same_bits(w.read_positions(), cur)
    h = float(scene.params.smoothing_radius)
    q = probes(cur, _box(scene.params), h)
    u, rho = w.sample_velocity_points(q, density=True)
    wet = rho > 0
    assert wet.sum() > len(q) // 4 and (~wet).sum() >= 128
    assert np.array_equal(u[wet], np.tile(CONST, (int(wet.sum()), 1)))
    assert not u[~wet].view(np.uint32).any()  # (+0, +0, +0)
    assert same_bits(rho, w.sample_density_points(q))
    # one midpoint substep of dt = 2^-4 from multiples of 2^-6: exactly dt * v where the tracer is in the fluid
    rng = np.random.default_rng(5)
    lo, hi = _box(scene.params)
    p0 = (np.round((lo + rng.random((1500, 3)) * (hi - lo)) * 64) / 64).astype(F32)
    dt = F32(0.0625)
    rho0 = w.sample_density_points(p0)
    p1 = w.advect_points(ws.fluid.advect_params(dt, 1), p0)
    moved = rho0 > 0
    assert moved.sum() > 100 and (~moved).sum() > 100
    assert np.array_equal(p1[moved], p0[moved] + dt * CONST) and same_bits(p1[~moved], p0[~moved])
    w.close()


# ---- 3. IEEE handles against the numpy restatement ----------------------------------------------------------------------------
def test_an_ieee_handle_gives_the_restatements_bits(ws):
    params = ws.make_params(container_size=(2.0, 1.5, 1.5))
    pos = ws.workloads.uniform_cloud(1024, 77, list(params.ext_min), list(params.ext_max))
    w = ws.FluidWorker(pos, params, ieee_division=True)
    w.run(STEPS)
    cur, vel = w.read_positions(), w.read_velocities()
    assert np.abs(vel).max() > 0.1
    merged = w.stats()["cells_merged"]
    h = float(params.smoothing_radius)
    q = probes(cur, _box(params), h, n=(256, 160, 64, 32))
    assert len(q) == 512
    u, rho = w.sample_velocity_points(q, density=True)
    wu, wrho, _ = V.field32(params, cur, vel, q, merged)
    assert np.count_nonzero(wrho) > 256 and np.count_nonzero(wrho == 0) >= 32
    assert same_bits(rho, wrho) and same_bits(u, wu)
    # a grid of 9 x 7 x 8 = 504 nodes over the fluid, spacing 0.7 h
    lo = cur.min(0)
    origin, spacing, dims = (lo - F32(0.3 * h)).astype(F32), np.full(3, F32(0.7 * h), F32), (9, 7, 8)
    ug, rg = w.sample_velocity_grid(origin, spacing, dims, density=True)
    wu, wrho, _ = V.field32(params, cur, vel, V.A.grid_nodes(origin, spacing, dims), merged)
    assert np.count_nonzero(wrho) > 100
    assert same_bits(rg.reshape(-1), wrho) and same_bits(ug.reshape(-1, 3), wu)
    w.close()


# ---- 4. both arithmetics against float64 --------------------------------------------------------------------------------------
@ARITH
def test_the_momentum_sums_against_float64(scene, ieee):
    """M is not an output: u * rho (formed in float64 from the float32 outputs) is compared with the float64 sum of
    w * v, under the density test's tolerance -- 4 x the float32 summation noise of the terms + 4 eps x max|sum| --
    applied to the momentum sums; rho under the same construction."""
    ws = scene.ws
    w, cur, vel = scene.get(ieee)
    h = float(scene.params.smoothing_radius)
    q = probes(cur, _box(scene.params), h)
    u, rho = w.sample_velocity_points(q, density=True)
    want_rho, want_mom, noise, cnt = V.field64(ws, scene.params, cur, vel, q)
    print("float64 %s: %d queries, %.1f %% with 4 or more particles, %.1f %% with none, noise %s" % (
        _arith(ieee), len(q), 100 * np.mean(cnt >= 4), 100 * np.mean(cnt == 0), noise))
    assert np.mean(cnt >= 4) >= 0.1 and np.mean(cnt == 0) >= 0.05  # (the brute force's own counts)
    mom = u.astype(np.float64) * rho.astype(np.float64)[:, None]
    for name, got, want, nz in (("rho", rho.astype(np.float64), want_rho, noise[0]), ("M", mom, want_mom, noise[1:].max())):
        err = float(np.max(np.abs(got - want)))
        tol = 4.0 * float(nz) + 4.0 * EPS32 * float(np.max(np.abs(want)))
        print("  %s: L-inf error %.3e, tolerance %.3e" % (name, err, tol))
        assert err <= tol, (name, err, tol)
    assert not rho[cnt == 0].any() and not u[cnt == 0].any()


# ---- 5. grid == points ---------------------------------------------------------------------------------------------------------
@ARITH
def test_the_grid_call_gives_the_points_calls_bits(scene, ieee):
    w, _, _ = scene.get(ieee)
    check_grid_equals_points(w, _box(scene.params), float(scene.params.smoothing_radius), "default " + _arith(ieee))


# ---- 6. the readback -----------------------------------------------------------------------------------------------------------
def test_read_velocities_is_the_velocity_column_of_the_records(scene):
    ws = scene.ws
    w, _, vel = scene.get(False)
    rec = w.read_vec("particles")
    assert same_bits(vel, np.ascontiguousarray(rec["velocity"][:, :3])) and np.abs(vel).max() > 0.1
    fresh = ws.FluidWorker(scene.pos, scene.params)
    assert not fresh.read_velocities().view(np.uint32).any()
    fresh.run(3)
    assert fresh.read_velocities().any()
    fresh.reset(scene.pos)
    assert not fresh.read_velocities().view(np.uint32).any()
    fresh.close()


# ---- 7. advection --------------------------------------------------------------------------------------------------------------
@ARITH
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["forwards", "backwards"])
@pytest.mark.parametrize("substeps", [1, 8])
def test_advection_is_the_host_march_bit_for_bit(scene, ieee, sign, substeps):
    ws = scene.ws
    w, cur, _ = scene.get(ieee)
    pts, cls = make_tracers(ws, w, cur, scene.params, _box(scene.params), seed=21, each=500)
    dt = float(F32(sign) * F32(4) * F32(scene.params.delta_time))
    out = check_march(ws, w, pts, cls, dt, substeps, "default " + _arith(ieee))
    march = ws.fluid.advect_params(dt, substeps)
    # permuted, and split in two calls: every tracer keeps its bits
    order = np.random.default_rng(11).permutation(len(pts))
    assert same_bits(w.advect_points(march, pts[order]), out[order])
    cut = 777
    assert same_bits(np.concatenate([w.advect_points(march, pts[:cut]), w.advect_points(march, pts[cut:])]), out)
    # xyz and out_xyz the same buffer
    buf = pts.copy()
    assert w._L.ws_advect_points(w._h, C.byref(march), buf.ctypes.data, len(buf), buf.ctypes.data, None, None) == 0
    assert same_bits(buf, out)


# ---- 8. the simulation is untouched --------------------------------------------------------------------------------------------
def _trajectory(ws, pos, params, regrid, steps, calls, graph):
    w = ws.FluidWorker(pos, params, graph=graph)
    lo, hi = _box(params)
    q = (lo + np.random.default_rng(2).random((64, 3)) * (hi - lo)).astype(F32)
    march = ws.fluid.advect_params(0.05, 2)
    origin, spacing, dims = cover((lo, hi), 1.0, 0.0)
    seen = 0
    for t in range(steps):
        if t == steps // 2:
            w.set_params(regrid)
        w.run(1)
        if calls:
            seen += int(np.count_nonzero(w.read_velocities()))
            if t % 2:
                seen += int(np.count_nonzero(w.sample_velocity_grid(origin, spacing, dims)))
                seen += int(np.count_nonzero(w.advect_points(march, q) != q))
            else:
                seen += int(np.count_nonzero(w.sample_velocity_grid(origin, spacing, dims, density=True)[1]))
                seen += int(np.count_nonzero(w.advect_points(march, q, field=True)[2]))
            seen += int(np.count_nonzero(w.sample_velocity_points(q)))
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats, seen


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_the_calls_every_step_leave_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    regrid = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=F32(0.2))
    want, _, _ = _trajectory(ws, pos, params, regrid, 200, False, graph)
    got, stats, seen = _trajectory(ws, pos, params, regrid, 200, True, graph)
    assert seen > 0
    if graph:
        assert stats["graph_steps"] > 0
    assert got.dtype.itemsize == 80
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- 9. other cell grids -------------------------------------------------------------------------------------------------------
def _with_velocities(w, n, seed):
    """Random velocities loaded through ws_write_particles (positions kept): for a scene that is sampled where it was put."""
    rec = w.read_vec("particles")
    rec["velocity"][:, :3] = np.random.default_rng(seed).normal(0.0, 1.5, (n, 3)).astype(F32)
    w.write_slice("particles", rec)


def _other_grid_checks(ws, w, params, case, box=None):
    cur = w.read_positions()
    h = float(params.smoothing_radius)
    box = box or _box(params)
    check_density_contract(w, cur, box, h, case)
    check_grid_equals_points(w, box, h, case)
    pts, cls = make_tracers(ws, w, cur, params, box, seed=23, each=300)
    for dt in (0.05, -0.05):
        check_march(ws, w, pts, cls, dt, 2, case)


@ARITH
def test_the_product_librarys_merged_cells(ws, ieee):
    """16 x 9 x 9 at h = 0.04: the library merges cells on its own (tests/test_gpu_field_grids.py has the scene: a
    jittered lattice of spacing h / 2 in the container's lowest corner, sampled where it was put)."""
    h = F32(0.04)
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), smoothing_radius=h)
    rng = np.random.default_rng(8)
    ijk = np.stack(np.meshgrid(*(np.arange(b) for b in (32, 32, 16)), indexing="ij"), -1).reshape(-1, 3)
    pos = (np.asarray(params.ext_min[:3], np.float64) + (ijk + 0.5 * rng.random((GRID_N, 3))) * (float(h) / 2)).astype(F32)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    assert w.stats()["cells_merged"] != (1, 1, 1)
    _with_velocities(w, GRID_N, 31)
    cur = w.read_positions()
    box = (cur.min(0).astype(np.float64) - float(h), cur.max(0).astype(np.float64) + float(h))
    _other_grid_checks(ws, w, params, "product merge " + _arith(ieee), box)
    w.close()


@ARITH
def test_a_container_far_from_the_origin(ws, ieee):
    pos, params = grid_scene(ws, 0.2, OFFSETS["east"])
    assert OFFSETS["east"] == (37.35, -21.7, 5.47)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(GRID_STEPS)
    assert w.stats()["cells_merged"] == (1, 1, 1)
    _other_grid_checks(ws, w, params, "offset east h0.2 " + _arith(ieee))
    w.close()


# ---- 10. slabs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    h = float(params.smoothing_radius)
    w = ws.FluidWorker(pos, params)
    w.run(STEPS)
    cur = w.read_positions()
    q = probes(cur, _box(params), h)
    origin, spacing, dims = cover(_box(params), F32(1.5) * F32(h), h)
    march = ws.fluid.advect_params(0.05, 3)

    def calls(x, wanted=True):
        kw = {} if wanted is None else {"want": wanted}
        return [x.read_velocities(**kw), x.sample_velocity_points(q, density=True, **kw),
                x.sample_velocity_grid(origin, spacing, dims, density=True, **kw), x.advect_points(march, q, field=True, **kw)]

    want = calls(w, None)
    assert want[0].any() and want[1][1].any()
    w.close()
    got = _slab_run(ws, params, pos, world, STEPS, lambda s, r: calls(s, r != 1))
    assert got[1] == [None, (None, None), (None, None), (None, None, None)]  # rank 1 only contributed
    for r in [k for k in range(world) if k != 1]:
        assert same_bits(got[r][0], want[0]), r
        for a, b in zip(got[r][1:], want[1:]):
            assert all(same_bits(x, y) for x, y in zip(a, b)), r


# ---- 11. errors ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.05], [-3.0, 1.0, 0.0], [50.0, 0.0, 0.0]], F32)
    u, rho, out = np.empty((64, 3), F32), np.empty(64, F32), np.empty((64, 3), F32)
    origin, spacing = np.zeros(3, F32), np.full(3, 0.25, F32)
    dims = np.array([4, 4, 4], np.uint32)

    def ptr(x):
        return None if x is None else x.ctypes.data

    def points(xyz=pts, m=4, u=u, rho=rho):
        return L.ws_sample_velocity_points(h, ptr(xyz), m, ptr(u), ptr(rho))

    def grid(origin=origin, spacing=spacing, dims=dims, u=u, rho=rho):
        return L.ws_sample_velocity_grid(h, ptr(origin), ptr(spacing), ptr(dims), ptr(u), ptr(rho))

    def advect(a=True, dt=0.05, substeps=2, xyz=pts, m=4, out=out, u=u, rho=rho):
        march = ws.fluid.advect_params(dt, substeps)
        return L.ws_advect_points(h, C.byref(march) if a else None, ptr(xyz), m, ptr(out), ptr(u), ptr(rho))

    def bad(x, i, val):
        x = x.copy()
        x[i] = val
        return x

    def refused(call, what):
        assert call() == 1, what
        assert points() == 0 and grid() == 0 and advect() == 0, what  # ... and the next call succeeds

    by_id = np.empty((len(pos), 3), F32)
    assert points() == 0 and grid() == 0 and advect() == 0 and L.ws_read_velocities(h, ptr(by_id)) == 0
    refused(lambda: L.ws_read_velocities(h, None), "read NULL")
    refused(lambda: points(m=0), "m == 0")
    refused(lambda: points(xyz=None), "NULL points")
    refused(lambda: points(u=None, rho=None), "both outputs NULL")
    for val in (np.nan, np.inf, -np.inf):
        refused(lambda: points(xyz=bad(pts, (2, 1), val)), val)
        refused(lambda: grid(origin=bad(origin, 1, val)), val)
        refused(lambda: grid(spacing=bad(spacing, 2, val)), val)
        refused(lambda: advect(xyz=bad(pts, (1, 2), val)), val)
        refused(lambda: advect(dt=val), val)
    refused(lambda: grid(spacing=bad(spacing, 0, 0.0)), "spacing 0")
    refused(lambda: grid(spacing=bad(spacing, 0, -0.25)), "spacing < 0")
    refused(lambda: grid(dims=bad(dims, 1, 0)), "dims 0")
    refused(lambda: grid(dims=np.array([2048, 2048, 513], np.uint32)), "more than 2^31 nodes")
    refused(lambda: grid(origin=None), "NULL origin")
    refused(lambda: grid(spacing=None), "NULL spacing")
    refused(lambda: grid(dims=None), "NULL dims")
    refused(lambda: grid(u=None, rho=None), "both outputs NULL")
    refused(lambda: advect(a=False), "NULL params")
    refused(lambda: advect(substeps=0), "substeps 0")
    refused(lambda: advect(substeps=4097), "substeps 4097")
    refused(lambda: advect(dt=2e6), "dt 2e6")
    refused(lambda: advect(dt=-2e6), "dt -2e6")
    refused(lambda: advect(xyz=bad(pts, (0, 0), 2e15)), "coordinate 2e15")
    refused(lambda: advect(xyz=bad(pts, (3, 2), -2e15)), "coordinate -2e15")
    refused(lambda: advect(m=0), "m == 0")
    refused(lambda: advect(m=(1 << 28) + 1), "more than 2^28 points")  # refused before a point is read
    refused(lambda: advect(xyz=None), "NULL points")
    refused(lambda: advect(out=None), "NULL out_xyz with other outputs")
    refused(lambda: advect(out=None, u=None, rho=None), "every output NULL")
    # allowed: dt == 0 and < 0, the largest substeps, the largest dt and coordinates
    assert advect(dt=0.0) == 0 and np.array_equal(out[:4], pts)
    assert advect(dt=-0.05) == 0 and advect(substeps=4096) == 0 and advect(dt=1e6) == 0
    assert advect(xyz=bad(pts, (0, 0), 1e15)) == 0 and advect(u=None, rho=None) == 0
    # the handle steps on and samples what a handle that saw no refusal samples
    fresh = ws.FluidWorker(pos, params)
    for x in (w, fresh):
        x.run(20)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    q = probes(w.read_positions(), _box(params), float(params.smoothing_radius), n=(200, 100, 32, 32))
    a, b = w.sample_velocity_points(q, density=True), fresh.sample_velocity_points(q, density=True)
    assert a[0].any() and same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    march = ws.fluid.advect_params(0.05, 4)
    assert same_bits(w.advect_points(march, q), fresh.advect_points(march, q))
    w.close()
    fresh.close()


def _all_calls(ws, w):
    q = [[0.0, 0.0, 0.0]]
    return (lambda: w.read_velocities(), lambda: w.sample_velocity_points(q),
            lambda: w.sample_velocity_grid((0.0, 0.0, 0.0), (0.25, 0.25, 0.25), (2, 2, 2)),
            lambda: w.advect_points(ws.fluid.advect_params(0.05, 1), q))


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    for call in _all_calls(ws, w):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.close()


def test_a_dead_handle_refuses_every_call(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    assert w.read_velocities().any() and w.sample_velocity_points(w.read_positions()[:64]).any()
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in _all_calls(ws, w):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
