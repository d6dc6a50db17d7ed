"""ws_extract_surface on the GPU: bit for bit against the numpy restatement (tests/surface_ref.py) on the library's own
sampled field, closed outward meshes on grids padded around the container, a single particle's analytic sphere, no
effect on the simulation, slabs, the capacity protocol, errors and lifetime."""
import ctypes as C
import threading

import numpy as np
import pytest

import surface_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def padded(params, spacing, pad):
    """A grid reaching `pad` beyond the container on every side: (origin, spacing, dims)."""
    mn = np.asarray(params.ext_min[:3], F32) - F32(pad)
    mx = np.asarray(params.ext_max[:3], F32) + F32(pad)
    sp = np.full(3, F32(spacing), F32)
    dims = tuple(int(v) for v in np.ceil((mx - mn) / sp).astype(np.int64) + 1)
    return mn, sp, dims


def iso_of(rho):
    """An iso level inside the fluid's range (the median of the non-zero densities)."""
    return F32(np.median(rho[rho > 0]))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_against_restatement(w, origin, spacing, dims, iso, case):
    rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
    want = S.extract(rho, grad, origin, spacing, dims, iso)
    got = w.extract_surface(origin, spacing, dims, iso)
    assert len(want[2]) > 0, case
    for name, a, b in zip(("vertices", "normals", "triangles"), got, want):
        assert same_bits(a, b), "%s: %s differ (%s vs %s)" % (case, name, a.shape, b.shape)
    # without normals: the same vertices and triangles
    v, n, t = w.extract_surface(origin, spacing, dims, iso, normals=False)
    assert n is None and same_bits(v, want[0]) and same_bits(t, want[2]), case
    return want


@pytest.mark.parametrize("dist", ["cloud", "lattice"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_c1_mesh_equals_the_restatement_bit_for_bit(ws, dist, ieee):
    pos, params = ws.workloads.make_workload("c1", dist)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(3), 0.6)
    done = 0
    for steps in (0, 50, 400):
        w.run(steps - done)
        done = steps
        rho = w.sample_density_grid(origin, spacing, dims)
        check_against_restatement(w, origin, spacing, dims, iso_of(rho), "c1 %s step %d" % (dist, steps))
    w.close()


def test_c3_settled_mesh_equals_the_restatement_bit_for_bit(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(400)
    origin = np.asarray(params.ext_min[:3], F32)
    spacing = np.full(3, F32(params.smoothing_radius), F32)
    dims = (256, 144, 144)
    check_against_restatement(w, origin, spacing, dims, F32(0.5 * params.target_density), "c3 settled")
    w.close()


def _closed_outward(xyz, tri, case):
    assert len(tri) > 0, case
    assert S.closed_and_oriented(tri, len(xyz)), case
    assert S.signed_volume(xyz, tri) > 0, case


def test_c1_padded_grid_gives_a_closed_outward_mesh(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(100)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), 1.25 * h)
    rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
    assert rho[0].max() < rho.max() * 1e-3 and rho[-1].max() < rho.max() * 1e-3
    iso = iso_of(rho)
    xyz, nrm, tri = w.extract_surface(origin, spacing, dims, iso)
    _closed_outward(xyz, tri, "c1")
    want = S.extract(rho, grad, origin, spacing, dims, iso)
    _closed_outward(want[0], want[2], "c1 restatement")
    assert same_bits(tri, want[2]) and same_bits(xyz, want[0])
    w.close()


def test_c3_settled_padded_half_h_grid_gives_a_closed_outward_mesh(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(400)
    h = F32(params.smoothing_radius)
    mn = np.asarray(params.ext_min[:3], F32) - F32(1.25 * h)
    mx = np.asarray(params.ext_max[:3], F32) + F32(1.25 * h)
    dims = (512, 288, 288)
    spacing = ((mx - mn) / (np.asarray(dims, F32) - 1)).astype(F32)
    xyz, nrm, tri = w.extract_surface(mn, spacing, dims, F32(0.5 * params.target_density))
    _closed_outward(xyz, tri, "c3 settled 512x288x288")
    fn = S.face_normals(xyz, tri)
    big = np.linalg.norm(fn, axis=1) > 1e-12
    mean_n = nrm.astype(np.float64)[tri.astype(np.int64)].sum(1)
    assert np.mean(np.einsum("ij,ij->i", fn[big], mean_n[big]) > 0) > 0.99
    w.close()


def _one_particle_ball(ws, centres):
    params = ws.make_params(container_size=(8.0, 8.0, 8.0))
    h = F32(params.smoothing_radius)
    k = ws.get_smoothing_kernel(params)
    r = h / F32(2)
    iso = F32((h - r) * (h - r) * F32(k.pow2))  # rho(h / 2): the surface is the sphere of radius h / 2
    pos = np.asarray(centres, F32)
    # the rest of a 4096-particle handle far away (x >= 2.5, more than 2 h from every node of the grid below)
    rest = ws.workloads.uniform_cloud(4096 - len(pos), 7, [2.5, -3.9, -3.9], [3.9, 3.9, 3.9])
    w = ws.FluidWorker(np.concatenate([pos, np.asarray(rest, F32)]).astype(F32), params)
    sp = h / F32(16)
    lo = pos.min(0) - F32(1.25) * h
    hi = pos.max(0) + F32(1.25) * h
    dims = tuple(int(v) for v in np.ceil((hi - lo) / sp).astype(np.int64) + 1)
    mesh = w.extract_surface(lo, np.full(3, sp, F32), dims, iso)
    w.close()
    return mesh, pos, float(h), float(r), float(sp)


def _sphere_tolerance(h, r, sp):
    """Radial error bound of a vertex on an edge of length <= L = sqrt(3) sp for f(d) = pow2 (h - d)^2 (in units of
    pow2): |f(v) - iso| <= L^2 / 8 * max|f''| along the edge, f'' <= 2 + |f'| / d; divided by min |f'| = 2 (h - r - L)."""
    L = np.sqrt(3.0) * sp
    dmin = r - L
    m = 2.0 + 2.0 * (h - dmin) / dmin
    return L * L / 8.0 * m / (2.0 * (h - r - L)) + 1e-5 * h


def test_a_single_particle_gives_the_analytic_sphere(ws):
    (xyz, nrm, tri), pos, h, r, sp = _one_particle_ball(ws, [[0.3, -0.2, 0.1]])
    p = pos[0].astype(np.float64)
    dv = xyz.astype(np.float64) - p
    dist = np.linalg.norm(dv, axis=1)
    tol = _sphere_tolerance(h, r, sp)
    assert np.max(np.abs(dist - r)) <= tol, (np.max(np.abs(dist - r)), tol)
    assert np.all(np.einsum("ij,ij->i", nrm.astype(np.float64), dv) > 0)
    assert S.closed_and_oriented(tri, len(xyz))
    assert S.euler_characteristic(tri, len(xyz)) == 2
    vol = S.signed_volume(xyz, tri)
    assert abs(vol - 4.0 / 3.0 * np.pi * r ** 3) / (4.0 / 3.0 * np.pi * r ** 3) < 0.03, vol


def test_two_far_apart_particles_give_two_closed_components(ws):
    (xyz, nrm, tri), pos, h, r, sp = _one_particle_ball(ws, [[-1.0, 0.0, 0.0], [1.0, 0.5, 0.0]])
    lab = S.components(tri, len(xyz))
    roots = np.unique(lab)
    assert len(roots) == 2
    for root in roots:
        on = lab[tri[:, 0].astype(np.int64)] == root
        part = tri[on]
        used = np.unique(part)
        remap = np.full(len(xyz), -1, np.int64)
        remap[used] = np.arange(len(used))
        sub = remap[part.astype(np.int64)].astype(np.uint32)
        assert S.closed_and_oriented(sub, len(used))
        assert S.euler_characteristic(sub, len(used)) == 2
        c = xyz[used].astype(np.float64).mean(0)
        assert np.min(np.linalg.norm(pos.astype(np.float64) - c, axis=1)) < 0.1 * r


def _trajectory(ws, pos, params, steps, extract, graph=False, regrid_at=None, small=None):
    w = ws.FluidWorker(pos, params, graph=graph)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    for t in range(steps):
        if regrid_at is not None and t == regrid_at:
            w.set_params(small)
        w.run(1)
        if extract:
            w.extract_surface(origin, spacing, dims, F32(2.0), normals=(t % 2 == 0))
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_extracting_every_step_leaves_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _ = _trajectory(ws, pos, params, 200, False, graph)
    got, stats = _trajectory(ws, pos, params, 200, True, graph)
    if graph:
        assert stats["graph_steps"] > 0
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


def test_extracting_across_a_regrid_leaves_the_trajectory_bitwise_unchanged(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    small = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.2))
    want, _ = _trajectory(ws, pos, params, 80, False, regrid_at=40, small=small)
    got, _ = _trajectory(ws, pos, params, 80, True, regrid_at=40, small=small)
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_extract_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    steps = 30
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    iso = F32(0.5 * params.target_density)
    w = ws.FluidWorker(pos, params)
    w.run(steps)
    want = w.extract_surface(origin, spacing, dims, iso)
    w.close()
    assert len(want[2]) > 0
    owner = ws.slab.assign(params, pos, world)
    hub = ws.slab.LoopbackHub(world)
    got = [None] * world
    errors = []

    def body(r):
        try:
            sel = np.flatnonzero(owner == r).astype(np.uint32)
            s = ws.slab.SlabWorker(pos[sel], sel, pos.shape[0], params, r, world, hub.transport(r))
            s.run(steps)
            got[r] = s.extract_surface(origin, spacing, dims, iso, want=(r != 1))  # rank 1 only contributes
            s.run(2)  # nobody was left waiting
            s.close()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not any(t.is_alive() for t in ts)
    assert not errors, errors
    for r in range(world):
        if r == 1:
            assert got[r] == (None, None, None)
            continue
        for a, b in zip(got[r], want):
            assert same_bits(a, b), r


def _raw(w, origin, spacing, dims, iso, cap_v, cap_t, xyz, nrm, tri, counts=True):
    o = np.ascontiguousarray(origin, F32)
    s = np.ascontiguousarray(spacing, F32)
    d = np.ascontiguousarray(dims, np.uint32)
    nv, nt = C.c_uint32(0xDEAD), C.c_uint32(0xBEEF)
    st = w._L.ws_extract_surface(w._h, o.ctypes.data, s.ctypes.data, d.ctypes.data, C.c_float(iso), cap_v, cap_t,
                                 None if xyz is None else xyz.ctypes.data, None if nrm is None else nrm.ctypes.data,
                                 None if tri is None else tri.ctypes.data, C.byref(nv) if counts else None,
                                 C.byref(nt) if counts else None)
    return st, nv.value, nt.value


def test_the_capacity_protocol(ws):
    pos, params = ws.workloads.make_workload("c1", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(20)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    rho = w.sample_density_grid(origin, spacing, dims)
    iso = iso_of(rho)
    v, n, t = w.extract_surface(origin, spacing, dims, iso)
    V, T = len(v), len(t)
    assert V > 0 and T > 0
    # counts only
    assert _raw(w, origin, spacing, dims, iso, 0, 0, None, None, None) == (0, V, T)
    sentinel = F32(-12345.0)

    def bufs(cv, ct):
        return (np.full((cv + 1, 3), sentinel, F32), np.full((cv + 1, 3), sentinel, F32),
                np.full((ct + 1, 3), 0xFFFFFFFF, np.uint32))

    for cv, ct in ((V - 1, T), (V, T - 1), (0, 0)):
        xyz, nrm, tri = bufs(cv, ct)
        assert _raw(w, origin, spacing, dims, iso, cv, ct, xyz, nrm, tri) == (0, V, T)
        assert np.all(xyz == sentinel) and np.all(nrm == sentinel) and np.all(tri == 0xFFFFFFFF)
    # one of the two mesh pointers NULL: counts only
    xyz, nrm, tri = bufs(V, T)
    assert _raw(w, origin, spacing, dims, iso, V, T, xyz, nrm, None) == (0, V, T)
    assert np.all(xyz == sentinel) and np.all(nrm == sentinel)
    # exact capacity fills exactly V vertices and T triangles
    xyz, nrm, tri = bufs(V, T)
    assert _raw(w, origin, spacing, dims, iso, V, T, xyz, nrm, tri) == (0, V, T)
    assert same_bits(xyz[:V], v) and same_bits(nrm[:V], n) and np.array_equal(tri[:T], t)
    assert np.all(xyz[V] == sentinel) and np.all(nrm[V] == sentinel) and np.all(tri[T] == 0xFFFFFFFF)
    # without normals the normal buffer is not touched
    xyz, nrm, tri = bufs(V, T)
    assert _raw(w, origin, spacing, dims, iso, V, T, xyz, None, tri) == (0, V, T)
    assert same_bits(xyz[:V], v) and np.array_equal(tri[:T], t)
    # an iso above every density: no surface
    top = np.nextafter(F32(rho.max()), F32(np.inf))
    xyz, nrm, tri = bufs(4, 4)
    assert _raw(w, origin, spacing, dims, top, 4, 4, xyz, nrm, tri) == (0, 0, 0)
    assert np.all(xyz == sentinel) and np.all(tri == 0xFFFFFFFF)
    v0, n0, t0 = w.extract_surface(origin, spacing, dims, top)
    assert v0.shape == (0, 3) and n0.shape == (0, 3) and t0.shape == (0, 3)
    w.close()


def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _ = _trajectory(ws, pos, params, 20, False)
    w = ws.FluidWorker(pos, params)
    o = np.zeros(3, F32)
    s = np.full(3, 0.1, F32)
    d = np.full(3, 8, np.uint32)
    xyz = np.empty((4096, 3), F32)
    tri = np.empty((4096, 3), np.uint32)

    def bad(v, i, x):
        v = v.copy()
        v[i] = x
        return v

    def call(o=o, s=s, d=d, iso=1.0, counts=True):
        return _raw(w, o, s, d, iso, 4096, 4096, xyz, None, tri, counts)[0]

    L, h = w._L, w._h
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    assert call() == 0
    assert L.ws_extract_surface(h, None, s.ctypes.data, d.ctypes.data, C.c_float(1.0), 0, 0, None, None, None,
                                C.byref(nv), C.byref(nt)) == 1
    assert L.ws_extract_surface(h, o.ctypes.data, None, d.ctypes.data, C.c_float(1.0), 0, 0, None, None, None,
                                C.byref(nv), C.byref(nt)) == 1
    assert L.ws_extract_surface(h, o.ctypes.data, s.ctypes.data, None, C.c_float(1.0), 0, 0, None, None, None,
                                C.byref(nv), C.byref(nt)) == 1
    assert L.ws_extract_surface(h, o.ctypes.data, s.ctypes.data, d.ctypes.data, C.c_float(1.0), 0, 0, None, None, None,
                                C.byref(nv), None) == 1
    assert call(counts=False) == 1
    # every output NULL: a single handle always needs the counts (refused before anything is sampled)
    assert L.ws_extract_surface(h, o.ctypes.data, s.ctypes.data, d.ctypes.data, C.c_float(1.0), 0, 0, None, None, None,
                                None, None) == 1
    assert L.ws_extract_surface(h, None, None, None, C.c_float(1.0), 0, 0, None, None, None, None, None) == 1
    for a in range(3):
        assert call(d=bad(d, a, 1)) == 1 and call(d=bad(d, a, 0)) == 1
    assert call(o=bad(o, 2, np.nan)) == 1 and call(o=bad(o, 0, np.inf)) == 1
    assert call(s=bad(s, 0, 0.0)) == 1 and call(s=bad(s, 1, -0.1)) == 1 and call(s=bad(s, 2, np.inf)) == 1
    assert call(s=bad(s, 1, np.nan)) == 1
    for iso in (0.0, -1.0, np.inf, np.nan):
        assert call(iso=iso) == 1, iso
    assert call(d=np.array([1024, 1024, 257], np.uint32)) == 1  # 2^28 + 2^20 nodes
    w.run(20)
    got = w.read_vec("particles")
    w.close()
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    xyz = np.empty((16, 3), F32)
    tri = np.empty((16, 3), np.uint32)
    assert _raw(w, origin, spacing, dims, 2.0, 16, 16, xyz, None, tri)[0] == 6  # WS_ERR_UNSUPPORTED
    with pytest.raises(ws.WsError) as e:
        w.extract_surface(origin, spacing, dims, 2.0)
    assert e.value.status == 6
    w.run(2)  # the handle steps on
    w.close()


def test_a_slab_rank_without_a_query_fails_after_the_gather(ws):
    """A rank that wants output but passes no origin is refused only after the collective gather: its peer's call
    completes with the single handle's counts, and both step on."""
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    iso = F32(0.5 * params.target_density)
    w = ws.FluidWorker(pos, params)
    w.run(10)
    want_v, _, want_t = w.extract_surface(origin, spacing, dims, iso)
    w.close()
    world = 2
    owner = ws.slab.assign(params, pos, world)
    hub = ws.slab.LoopbackHub(world)
    got = [None] * world
    errors = []

    def body(r):
        try:
            sel = np.flatnonzero(owner == r).astype(np.uint32)
            s = ws.slab.SlabWorker(pos[sel], sel, pos.shape[0], params, r, world, hub.transport(r))
            s.run(10)
            nv, nt = C.c_uint32(0), C.c_uint32(0)
            d = np.asarray(dims, np.uint32)
            if r == 0:
                st = s._L.ws_extract_surface(s._h, None, spacing.ctypes.data, d.ctypes.data, C.c_float(iso), 0, 0, None,
                                             None, None, C.byref(nv), C.byref(nt))
            else:
                st = s._L.ws_extract_surface(s._h, origin.ctypes.data, spacing.ctypes.data, d.ctypes.data, C.c_float(iso), 0,
                                             0, None, None, None, C.byref(nv), C.byref(nt))
            s.run(2)  # nobody was left waiting
            got[r] = (st, nv.value, nt.value)
            s.close()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not any(t.is_alive() for t in ts), "a rank is still waiting"
    assert not errors, errors
    assert got[0] == (1, 0, 0)
    assert got[1] == (0, len(want_v), len(want_t))


def test_a_dead_handle_refuses_to_extract(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = padded(params, h / F32(2), h)
    w.extract_surface(origin, spacing, dims, 2.0)
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    with pytest.raises(ws.WsError) as e:
        w.extract_surface(origin, spacing, dims, 2.0)
    assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()


def test_repeated_extraction_then_destroy_then_a_new_handle(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    origin = np.asarray(params.ext_min[:3], F32)
    spacing = np.full(3, F32(params.smoothing_radius), F32)
    dims = (256, 144, 144)
    first = None
    for _ in range(3):
        mesh = w.extract_surface(origin, spacing, dims, F32(0.5 * params.target_density))
        if first is None:
            first = mesh
        w.run(2)
    assert len(first[2]) > 0 and len(mesh[2]) > 0
    w.close()
    w2 = ws.FluidWorker(pos, params)
    again = w2.extract_surface(origin, spacing, dims, F32(0.5 * params.target_density))
    for a, b in zip(again, first):
        assert same_bits(a, b)
    w2.close()
