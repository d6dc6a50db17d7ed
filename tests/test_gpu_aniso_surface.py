"""The anisotropic kernels on the GPU (ws_read_anisotropy, ws_sample_aniso_*, ws_extract_aniso_surface): the isotropic
limit bit for bit against the density sampler and ws_extract_surface, the stage bit for bit against tests/aniso_ref.py,
the field against float64, grid == points, the mesh against the restatement and its shape, no effect on the
simulation, slabs and errors."""
import ctypes as C
import threading

import numpy as np
import pytest

import aniso_ref as A
import surface_ref as S
from test_aniso_reference import sheet_case

pytestmark = pytest.mark.gpu
F32 = np.float32


def padded(params, spacing, pad):
    mn = np.asarray(params.ext_min[:3], F32) - F32(pad)
    mx = np.asarray(params.ext_max[:3], F32) + F32(pad)
    sp = np.full(3, F32(spacing), F32)
    dims = tuple(int(v) for v in np.ceil((mx - mn) / sp).astype(np.int64) + 1)
    return mn, sp, dims


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def params_of(ws, d):
    return ws.fluid.aniso_params(**d)


ISO_LIMIT = A.isotropic_limit()
SHEET = dict(A.defaults(), min_neighbours=3)


# ---- 1. the isotropic limit -------------------------------------------------------------------------------------------
def _iso_limit_case(ws, w, params, origin, spacing, dims, case):
    a = params_of(ws, ISO_LIMIT)
    rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
    arho, agrad = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
    assert same_bits(arho, rho) and same_bits(agrad, grad), case
    q = A.grid_nodes(origin, spacing, dims)[::7]
    prho, pgrad = w.sample_density_points(q, gradient=True)
    parho, pagrad = w.sample_aniso_points(q, gradient=True, aniso=a)
    assert same_bits(parho, prho) and same_bits(pagrad, pgrad), case
    iso = F32(np.median(rho[rho > 0]))
    want = w.extract_surface(origin, spacing, dims, iso)
    got = w.extract_aniso_surface(origin, spacing, dims, iso, aniso=a)
    assert len(want[2]) > 0, case
    for x, y in zip(got, want):
        assert same_bits(x, y), case


@pytest.mark.parametrize("dist", ["cloud", "lattice"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_isotropic_limit_is_the_density_field_and_its_mesh_bit_for_bit(ws, dist, ieee):
    pos, params = ws.workloads.make_workload("c1", dist)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(3), 0.6)
    done = 0
    for steps in (0, 50, 400):
        w.run(steps - done)
        done = steps
        _iso_limit_case(ws, w, params, origin, spacing, dims, "c1 %s step %d" % (dist, steps))
        c, m, f, n = w.anisotropy(params_of(ws, ISO_LIMIT))
        assert same_bits(c, w.read_positions()) and np.all(f == 1) and np.all(m[:, :3] == 1)
    w.close()


def test_the_isotropic_limit_on_settled_c3_at_half_h(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(400)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    _iso_limit_case(ws, w, params, origin, spacing, dims, "c3 settled")
    w.close()


# ---- 2. the stage bit for bit -------------------------------------------------------------------------------------------
def _check_stage(ws, w, params, case, merged=(1, 1, 1), ids=None, restated=None):
    """The handle's stage against the restatement on its grid (of `merged` cells), at every particle or at `ids`; the
    restatement's own arrays go into the dict `restated` by parameter set."""
    x = w.read_positions()
    for name, d in (("defaults", A.defaults()), ("sheet", SHEET)):
        got = w.anisotropy(params_of(ws, d))
        want = A.stage(params, x, d, merged=merged, ids=ids)
        if restated is not None:
            restated[name] = want
        for label, a, b in zip(("centre", "matrix", "scale", "neighbours"), got, want):
            a = a if ids is None else a[ids]
            assert same_bits(a, b), "%s %s: %s differs in %d of %d" % (case, name, label,
                                                                       np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)), a.size)
    return got


def test_the_stage_equals_the_restatement_on_c1_and_ref(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    done = 0
    for steps in (0, 50, 400):
        w.run(steps - done)
        done = steps
        _check_stage(ws, w, params, "c1 step %d" % steps)
    w.close()
    pos, params = ws.workloads.make_workload("ref", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(20)
    c, m, f, n = _check_stage(ws, w, params, "ref")
    w.close()
    assert np.any(n >= 12) and np.any(n < 12)


def test_the_stage_on_coincident_pairs_and_an_overflow_clump(ws):
    params = ws.make_params(container_size=(8.0, 8.0, 8.0))
    # coincident pairs far apart: n = 2, C = 0, sigma_max = 0 -> the lone branch even with N_eps <= 2
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    pairs = (g * 0.9 - 3.2).astype(F32)
    pos = np.concatenate([pairs, pairs]).astype(F32)
    w = ws.FluidWorker(pos, params)
    for d in (dict(A.defaults(), min_neighbours=2), dict(A.defaults(), min_neighbours=0)):
        got = w.anisotropy(params_of(ws, d))
        want = A.stage(params, pos, d)
        for a, b in zip(got, want):
            assert same_bits(a, b)
        assert np.all(got[3] == 2) and np.all(got[2] == 8)  # lone: (1 / 0.5)^3
    w.close()
    # an overflow clump: 3000 particles in a ball of radius h / 2 next to a sparse cloud
    rng = np.random.default_rng(5)
    v = rng.standard_normal((3000, 3))
    clump = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0, 1, (3000, 1)) ** (1 / 3) * 0.12).astype(F32)
    rest = ws.workloads.uniform_cloud(1096, 9, [-3.9, -3.9, -3.9], [3.9, 3.9, 3.9])
    pos = np.concatenate([clump, np.asarray(rest, F32)]).astype(F32)
    w = ws.FluidWorker(pos, params)
    _check_stage(ws, w, params, "clump")
    w.close()


# ---- 3. the field against float64 -------------------------------------------------------------------------------------
def _check_f64(params, stage, q, rho, grad, case, merged=(1, 1, 1)):
    c, m, f, _ = stage
    r64, g64, tr, tg, _ = A.field64(params, c, m, f, q, merged=merged)
    er = np.abs(rho.astype(np.float64) - r64)
    eg = np.abs(grad.astype(np.float64) - g64)
    assert np.all(er <= tr), "%s: density err/tol %.3g" % (case, np.max(er / np.maximum(tr, 1e-300)))
    assert np.all(eg <= tg), "%s: gradient err/tol %.3g" % (case, np.max(eg / np.maximum(tg, 1e-300)))


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_c1_field_is_within_its_float64_bound_at_every_node(ws, ieee):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(50)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    a = params_of(ws, A.defaults())
    rho, grad = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
    stage = w.anisotropy(a)
    _check_f64(params, stage, A.grid_nodes(origin, spacing, dims), rho.reshape(-1), grad.reshape(-1, 3), "c1")
    if ieee:  # the IEEE form is the float32 restatement's, bit for bit
        q = A.grid_nodes(origin, spacing, dims)
        r32, g32 = A.field32(params, stage[0], stage[1], stage[2], q)
        assert same_bits(r32, rho.reshape(-1)) and same_bits(g32, grad.reshape(-1, 3))
    w.close()


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_settled_c3_field_is_within_its_float64_bound(ws, ieee):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(400)
    h = F32(params.smoothing_radius)
    origin = np.asarray(params.ext_min[:3], F32)
    spacing = np.full(3, h, F32)
    dims = (256, 144, 144)
    a = params_of(ws, A.defaults())
    rho = w.sample_aniso_grid(origin, spacing, dims, aniso=a).reshape(-1)
    iso = F32(0.5 * params.target_density)
    band = np.flatnonzero((rho >= iso / 4) & (rho <= iso * 4))
    rng = np.random.default_rng(1)
    rest = rng.permutation(np.setdiff1d(np.arange(rho.size), band))
    sel = np.union1d(band, rest[:max(0, (1 << 18) - band.size)])
    assert sel.size >= 1 << 18 and band.size > 0
    q = A.grid_nodes(origin, spacing, dims)[sel]
    prho, pgrad = w.sample_aniso_points(q, gradient=True, aniso=a)
    assert same_bits(prho, rho[sel])
    stage = w.anisotropy(a)
    w.close()
    _check_f64(params, stage, q, prho, pgrad, "c3 settled")


# ---- 4. grid == points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_grid_equals_points_bit_for_bit(ws, ieee):
    pos, params = ws.workloads.make_workload("ref", "cloud")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(30)
    h = F32(params.smoothing_radius)
    a = params_of(ws, A.defaults())
    for sp in (h / F32(4), h, F32(2) * h):  # (the isotropic sampler's brick and points ranges of spacing)
        origin, spacing, dims = padded(params, sp, sp)
        rho, grad = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
        q = A.grid_nodes(origin, spacing, dims)
        prho, pgrad = w.sample_aniso_points(q, gradient=True, aniso=a)
        assert same_bits(prho, rho.reshape(-1)) and same_bits(pgrad, grad.reshape(-1, 3)), float(sp)
        assert np.count_nonzero(prho) > 0
    w.close()


# ---- 5. the mesh --------------------------------------------------------------------------------------------------------
def test_the_mesh_equals_the_restatement_and_is_closed_on_a_padded_grid(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(50)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(3), h)
    for d in (A.defaults(), SHEET):
        a = params_of(ws, d)
        rho, grad = w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
        iso = F32(np.median(rho[rho > 0]))
        want = S.extract(rho, grad, origin, spacing, dims, iso)
        got = w.extract_aniso_surface(origin, spacing, dims, iso, aniso=a)
        assert len(want[2]) > 0
        for x, y in zip(got, want):
            assert same_bits(x, y)
        xyz, nrm, tri = got
        assert S.closed_and_oriented(tri, len(xyz))
        assert S.signed_volume(xyz, tri) > 0  # outward
    w.close()


def test_a_single_particle_gives_the_lone_ball(ws):
    params = ws.make_params(container_size=(8.0, 8.0, 8.0))
    k = ws.get_smoothing_kernel(params)
    h = F32(params.smoothing_radius)
    p = np.array([[0.3, -0.2, 0.1]], F32)
    rest = ws.workloads.uniform_cloud(4095, 7, [2.5, -3.9, -3.9], [3.9, 3.9, 3.9])
    w = ws.FluidWorker(np.concatenate([p, np.asarray(rest, F32)]).astype(F32), params)
    iso = F32(0.25 * float(k.pow2) * float(h) ** 2)
    kn = A.defaults()["lone_scale"]
    r = A.lone_radius(float(h), float(k.pow2), float(iso), kn)
    sp = F32(h / F32(32))
    lo = p[0] - F32(0.7) * h
    xyz, nrm, tri = w.extract_aniso_surface(lo, np.full(3, sp, F32), (46, 46, 46), iso)
    w.close()
    dist = np.linalg.norm(xyz.astype(np.float64) - p[0], axis=1)
    L = np.sqrt(3.0) * float(sp)
    assert np.max(np.abs(dist - r)) <= L * L / r, (np.max(np.abs(dist - r)), r)
    assert S.closed_and_oriented(tri, len(xyz)) and S.euler_characteristic(tri, len(xyz)) == 2
    assert np.all(np.einsum("ij,ij->i", nrm.astype(np.float64), xyz - p[0]) > 0)


def test_the_c1_sheet_meshes_flat_on_the_gpu(ws):
    pos, params = ws.workloads.make_workload("c1", "lattice")
    w = ws.FluidWorker(pos, params)
    a = params_of(ws, SHEET)
    c, m, f, n = w.anisotropy(a)

    def field(origin, spacing, dims, iso):
        return w.extract_aniso_surface(origin, spacing, dims, iso, aniso=a)

    rms_an, rms_iso = sheet_case(params, c, m, f, SHEET["max_ratio"], field)
    w.close()
    assert rms_an <= 0.5 * rms_iso, (rms_an, rms_iso)


# ---- 6. no effect on the simulation -------------------------------------------------------------------------------------
def _trajectory(ws, pos, params, steps, calls, graph=False, regrid_at=None, small=None):
    w = ws.FluidWorker(pos, params, graph=graph)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    a = params_of(ws, A.defaults())
    for t in range(steps):
        if regrid_at is not None and t == regrid_at:
            w.set_params(small)
        w.run(1)
        if calls:
            k = t % 4
            if k == 0:
                w.extract_aniso_surface(origin, spacing, dims, F32(2.0), aniso=a)
            elif k == 1:
                w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a)
            elif k == 2:
                w.sample_aniso_points(np.zeros((5, 3), F32), aniso=a)
            else:
                w.anisotropy(a)
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_anisotropic_calls_leave_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _ = _trajectory(ws, pos, params, 200, False, graph)
    got, stats = _trajectory(ws, pos, params, 200, True, graph)
    if graph:
        assert stats["graph_steps"] > 0
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


def test_anisotropic_calls_across_a_regrid_leave_the_trajectory_unchanged(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    small = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.2))
    want, _ = _trajectory(ws, pos, params, 80, False, regrid_at=40, small=small)
    got, _ = _trajectory(ws, pos, params, 80, True, regrid_at=40, small=small)
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


# ---- 7. slabs -----------------------------------------------------------------------------------------------------------
def _slab_run(ws, params, pos, world, steps, body_calls, **worker_args):
    owner = ws.slab.assign(params, pos, world, worker_args.get("library"))
    hub = ws.slab.LoopbackHub(world)
    got = [None] * world
    errors = []

    def body(r):
        try:
            sel = np.flatnonzero(owner == r).astype(np.uint32)
            s = ws.slab.SlabWorker(pos[sel], sel, pos.shape[0], params, r, world, hub.transport(r), **worker_args)
            s.run(steps)
            got[r] = body_calls(s, r)
            s.run(2)  # nobody was left waiting
            s.close()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not any(t.is_alive() for t in ts), "a rank is still waiting"
    assert not errors, errors
    return got


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    steps = 30
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    iso = F32(0.5 * params.target_density)
    a = params_of(ws, A.defaults())
    q = A.grid_nodes(origin, spacing, dims)[::97]
    w = ws.FluidWorker(pos, params)
    w.run(steps)
    want = (w.anisotropy(a), w.sample_aniso_grid(origin, spacing, dims, gradient=True, aniso=a),
            w.sample_aniso_points(q, gradient=True, aniso=a), w.extract_aniso_surface(origin, spacing, dims, iso, aniso=a))
    w.close()
    assert len(want[3][2]) > 0

    def calls(s, r):
        wanted = r != 1  # rank 1 only contributes
        return (s.anisotropy(a, want=wanted), s.sample_aniso_grid(origin, spacing, dims, True, wanted, aniso=a),
                s.sample_aniso_points(q, True, wanted, aniso=a), s.extract_aniso_surface(origin, spacing, dims, iso,
                                                                                         want=wanted, aniso=a))

    got = _slab_run(ws, params, pos, world, steps, calls)
    for r in range(world):
        if r == 1:
            continue
        for g_part, w_part in zip(got[r], want):
            for x, y in zip(g_part, w_part):
                assert same_bits(x, y), r


def test_a_slab_rank_with_refused_params_fails_after_the_gather(ws):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    iso = F32(0.5 * params.target_density)
    good = params_of(ws, A.defaults())
    bad = params_of(ws, dict(A.defaults(), max_ratio=0.5))
    w = ws.FluidWorker(pos, params)
    w.run(10)
    want_v, _, want_t = w.extract_aniso_surface(origin, spacing, dims, iso, aniso=good)
    want_c = w.anisotropy(good)[0]
    w.close()

    def calls(s, r):
        d = np.asarray(dims, np.uint32)
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        st = s._L.ws_extract_aniso_surface(s._h, C.byref(bad if r == 0 else good), origin.ctypes.data, spacing.ctypes.data,
                                           d.ctypes.data, C.c_float(iso), 0, 0, None, None, None, C.byref(nv), C.byref(nt))
        c = np.empty((s.n_global, 3), F32)
        st2 = s._L.ws_read_anisotropy(s._h, None if r == 0 else C.byref(good), c.ctypes.data, None, None, None)
        return st, nv.value, nt.value, st2, c

    got = _slab_run(ws, params, pos, 2, 10, calls)
    assert got[0][:4] == (1, 0, 0, 1)
    assert got[1][:4] == (0, len(want_v), len(want_t), 0)
    assert same_bits(got[1][4], want_c)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------
def test_invalid_parameters_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(2)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h, h)
    bad = [dict(smoothing=-0.1), dict(smoothing=1.5), dict(smoothing=float("nan")), dict(max_ratio=0.99),
           dict(max_ratio=float("inf")), dict(lone_scale=0.0), dict(lone_scale=1.01), dict(lone_scale=float("nan"))]
    for d in bad:
        a = params_of(ws, dict(A.defaults(), **d))
        for call in (lambda: w.anisotropy(a), lambda: w.sample_aniso_grid(origin, spacing, dims, aniso=a),
                     lambda: w.sample_aniso_points(np.zeros((3, 3), F32), aniso=a),
                     lambda: w.extract_aniso_surface(origin, spacing, dims, F32(2.0), aniso=a)):
            with pytest.raises(ws.WsError) as e:
                call()
            assert e.value.status == 1, d
    L = w._L
    d3 = np.asarray(dims, np.uint32)
    out = np.empty(int(np.prod(dims)), F32)
    assert L.ws_sample_aniso_grid(w._h, None, origin.ctypes.data, spacing.ctypes.data, d3.ctypes.data, out.ctypes.data, None) == 1
    assert L.ws_read_anisotropy(w._h, None, None, None, None, None) == 1
    w.run(2)
    w.sample_aniso_grid(origin, spacing, dims)
    w.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h, h)
    for call in (lambda: w.anisotropy(), lambda: w.sample_aniso_grid(origin, spacing, dims),
                 lambda: w.sample_aniso_points(np.zeros((3, 3), F32)),
                 lambda: w.extract_aniso_surface(origin, spacing, dims, F32(2.0))):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_the_anisotropic_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    w.extract_aniso_surface(origin, spacing, dims, 2.0)
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in (lambda: w.anisotropy(), lambda: w.sample_aniso_grid(origin, spacing, dims),
                 lambda: w.sample_aniso_points(np.zeros((3, 3), F32)),
                 lambda: w.extract_aniso_surface(origin, spacing, dims, 2.0)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()


def test_repeated_calls_then_destroy_then_a_new_handle(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    origin = np.asarray(params.ext_min[:3], F32)
    spacing = np.full(3, F32(params.smoothing_radius), F32)
    dims = (256, 144, 144)
    iso = F32(0.5 * params.target_density)
    first = None
    for _ in range(3):
        mesh = w.extract_aniso_surface(origin, spacing, dims, iso)
        w.anisotropy()
        if first is None:
            first = mesh
        w.run(2)
    assert len(first[2]) > 0 and len(mesh[2]) > 0
    w.close()
    w2 = ws.FluidWorker(pos, params)
    again = w2.extract_aniso_surface(origin, spacing, dims, iso)
    for a, b in zip(again, first):
        assert same_bits(a, b)
    w2.close()
