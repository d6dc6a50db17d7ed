"""ws_cast_rays / ws_cast_camera on the GPU: bit for bit against a host march that samples the field with the library's
own points calls (tests/rays_ref.py), lane independence, camera == rays, the isotropic limit, no effect on the
simulation, slabs, errors.

Setup unless a test says otherwise: a 16 x 9 x 9 container, a 65 536-particle uniform cloud (seed 1234), 30 steps,
dt = h / 2, steps = 160, refine = 6, iso = target_density / 2."""
import ctypes as C
import threading

import numpy as np
import pytest

import rays_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS = 30


def _setup(ws):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    return pos, params


def _march(ws, params, **kw):
    h = F32(params.smoothing_radius)
    m = dict(t_start=0.0, dt=float(h / F32(2)), steps=160, refine=6, iso=float(F32(params.target_density) / F32(2)))
    m.update(kw)
    return ws.fluid.ray_params(m["t_start"], m["dt"], m["steps"], m["refine"], m["iso"])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def make_rays(cur, params, seed=7, radius=11.0, far=(60.0, 64.0), centre=None):
    """About 2 000 rays in six classes (the class of each ray in `cls`): (a) from a sphere around the container at a
    particle, (b) from a particle, (c) away from the container, (d) axis-parallel, (e) from 50 units outside the grid,
    (f) grazing the container's faces.  Directions are deliberately not unit vectors.  The spheres have the radii
    `radius` and `far` (for this file's 16 x 9 x 9 container) about `centre` (the origin)."""
    rng = np.random.default_rng(seed)
    mn = np.asarray(params.ext_min[:3], np.float64)
    mx = np.asarray(params.ext_max[:3], np.float64)
    h = float(params.smoothing_radius)
    O, V, cls = [], [], []
    shift = np.zeros(3) if centre is None else np.asarray(centre, np.float64)

    def add(c, o, v):
        O.append(np.asarray(o, np.float64))
        V.append(np.asarray(v, np.float64))
        cls.extend([c] * len(o))

    # (a) radius 11 > the container's half diagonal (10.05); |v| >= 1.2 reaches 24 > 11 + 10.05 in 160 steps of h / 2
    o = shift + radius * _sphere(rng, 700)
    target = cur[rng.choice(len(cur), 700, replace=False)].astype(np.float64)
    add("a", o, _unit(target - o) * rng.uniform(1.2, 1.6, (700, 1)))
    # (b) the origin IS a particle's position
    add("b", cur[rng.choice(len(cur), 200, replace=False)].astype(np.float64), _sphere(rng, 200) * rng.uniform(0.5, 1.5, (200, 1)))
    # (c) outwards from the same sphere
    o = radius * _sphere(rng, 300)
    add("c", shift + o, _unit(o) * rng.uniform(0.5, 1.5, (300, 1)))
    # (d) two direction components exactly zero, from one unit outside a face towards it
    for axis in range(3):
        for sign in (-1.0, 1.0):
            o = mn + rng.random((50, 3)) * (mx - mn)
            o[:, axis] = (mx[axis] + 1.0) if sign > 0 else (mn[axis] - 1.0)
            v = np.zeros((50, 3))
            v[:, axis] = -sign * rng.uniform(0.6, 1.4, 50)
            add("d", o, v)
    # (e) 50 units and more outside the grid, at a point of the container: |v| = 3.6 reaches 72 in 160 steps
    o = shift + rng.uniform(far[0], far[1], (200, 1)) * _sphere(rng, 200)
    target = mn + rng.random((200, 3)) * (mx - mn)
    add("e", o, _unit(target - o) * 3.6)
    # (f) along a face, within h of its plane (inside and outside), slightly tilted
    for axis in range(3):
        for side in (mn, mx):
            along = (axis + 1) % 3
            o = mn + rng.random((50, 3)) * (mx - mn)
            o[:, axis] = side[axis] + rng.uniform(-h, h, 50)
            o[:, along] = mn[along] - 1.0
            v = rng.normal(0.0, 0.01, (50, 3))
            v[:, along] = rng.uniform(0.8, 1.3, 50)
            add("f", o, v)
    O = np.concatenate(O).astype(F32)
    V = np.concatenate(V).astype(F32)
    cls = np.asarray(cls)
    assert np.all((O[cls == "b"][:, None, :] == cur[None, :, :]).all(2).any(1))  # (float32 -> float64 -> float32 is exact)
    assert not np.any((V == 0).all(1))
    return O, V, cls


class _Scene:
    """One worker per arithmetic at step 30, its rays, and the library's casts of them (computed once, shared, never
    modified)."""

    def __init__(self, ws):
        self.ws = ws
        self.pos, self.params = _setup(ws)
        self.march = _march(ws, self.params)
        self.workers, self.rays, self.casts = {}, {}, {}

    def worker(self, ieee):
        if ieee not in self.workers:
            w = self.ws.FluidWorker(self.pos, self.params, ieee_division=ieee)
            w.run(STEPS)
            self.workers[ieee] = w
            self.rays[ieee] = make_rays(w.read_positions(), self.params)
        return self.workers[ieee]

    def aniso(self, field):
        return self.ws.fluid.aniso_params() if field == "aniso" else None

    def cast(self, ieee, field):
        """(t, normal) of the library for the rays of this arithmetic."""
        if (ieee, field) not in self.casts:
            w = self.worker(ieee)
            o, v, _ = self.rays[ieee]
            t, n = w.cast_rays(self.march, o, v, aniso=self.aniso(field))
            t.setflags(write=False)
            n.setflags(write=False)
            self.casts[ieee, field] = (t, n)
        return self.casts[ieee, field]

    def close(self):
        for w in self.workers.values():
            w.close()


@pytest.fixture(scope="module")
def scene(ws):
    s = _Scene(ws)
    yield s
    s.close()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


FIELDS = pytest.mark.parametrize("field", ["density", "aniso"])
ARITH = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])


@ARITH
@FIELDS
def test_bit_for_bit_against_a_host_march(scene, ieee, field):
    w = scene.worker(ieee)
    o, v, cls = scene.rays[ieee]
    a = scene.aniso(field)
    if a is None:
        def host_field(p):
            return w.sample_density_points(p, gradient=True)
    else:
        def host_field(p):
            return w.sample_aniso_points(p, gradient=True, aniso=a)
    want_t, want_n, K = R.cast(host_field, scene.march, o, v)
    m = len(o)
    shares = {"K>=1": np.count_nonzero(K >= 1) / m, "miss": np.count_nonzero(K < 0) / m, "K=0": np.count_nonzero(K == 0) / m}
    print("rays %d, shares %s, per class K>=1/K=0/miss: %s" % (m, shares, {
        c: (int(np.count_nonzero(K[cls == c] >= 1)), int(np.count_nonzero(K[cls == c] == 0)), int(np.count_nonzero(K[cls == c] < 0)))
        for c in "abcdef"}))
    # the host march's own result, so the comparison below cannot pass vacuously
    assert shares["K>=1"] >= 0.25 and shares["miss"] >= 0.05 and shares["K=0"] >= 0.05, shares
    assert np.all(K[cls == "c"] < 0)
    if field == "density":  # the self term h^2 * pow2 ~ 153 is far above iso
        assert np.all(K[cls == "b"] == 0) and np.all(K[cls == "a"] >= 1)
    t, n = scene.cast(ieee, field)
    assert t.shape == (m,) and n.shape == (m, 3)
    bad = np.flatnonzero(t.view(np.uint32) != want_t.view(np.uint32))
    assert bad.size == 0, (bad[:8], t[bad[:8]], want_t[bad[:8]], cls[bad[:8]])
    bad = np.flatnonzero((n.view(np.uint32) != want_n.view(np.uint32)).any(1))
    assert bad.size == 0, (bad[:8], n[bad[:8]], want_n[bad[:8]], cls[bad[:8]])
    assert np.all(np.isposinf(t[K < 0])) and not n[K < 0].any()
    # a hit has a zero normal only where g.g == 0: a ray that starts at the very centre of a particle without neighbours
    unit = n.any(1)
    assert np.all(K[~unit] <= 0) and unit[K >= 0].mean() > 0.9
    assert np.max(np.abs(np.linalg.norm(n[unit].astype(np.float64), axis=1) - 1.0)) < 1e-6
    # the distance alone (out_normal NULL) is the distance with normals
    t_only, none = w.cast_rays(scene.march, o, v, normals=False, aniso=a)
    assert none is None and _same(t_only, t)


@ARITH
@FIELDS
def test_a_ray_keeps_its_bits_whatever_shares_its_wave(scene, ieee, field):
    """The rays of the first test in a shuffled order, cast as prefixes: every ray keeps the bits it had in the full cast
    (which the first test ties to the host march)."""
    w = scene.worker(ieee)
    o, v, _ = scene.rays[ieee]
    t, n = scene.cast(ieee, field)
    order = np.random.default_rng(11).permutation(len(o))
    for length in (1, 63, 64, 65, 1000):
        sel = order[:length]
        ts, ns = w.cast_rays(scene.march, o[sel], v[sel], aniso=scene.aniso(field))
        assert _same(ts, t[sel]) and _same(ns, n[sel]), length


def _camera_45(ws):
    """Looks down at 45 degrees from above and in front of the container; right / up carry a 90 degree horizontal field
    of view and the 70 : 50 aspect."""
    s = np.sqrt(0.5)
    eye = np.array([0.5, 10.0, 10.0], F32)
    forward = np.array([0.0, -s, -s], F32)
    right = np.array([1.0, 0.0, 0.0], F32)
    up = (np.array([0.0, s, -s]) * (50.0 / 70.0)).astype(F32)
    return ws.fluid.camera(eye, forward, right, up), (eye, forward, right, up)


@ARITH
@FIELDS
def test_the_camera_equals_the_rays_of_its_formula(scene, ieee, field):
    w = scene.worker(ieee)
    cam, vectors = _camera_45(scene.ws)
    size = (70, 50)  # not a multiple of the 8 x 8 tile on either axis
    a = scene.aniso(field)
    t, n = w.cast_camera(scene.march, cam, size, aniso=a)
    assert t.shape == (50, 70) and n.shape == (50, 70, 3)
    o, v = R.camera_rays(*vectors, size)
    want_t, want_n = w.cast_rays(scene.march, o, v, aniso=a)
    assert _same(t.reshape(-1), want_t) and _same(n.reshape(-1, 3), want_n)
    hit = np.isfinite(t)
    print("camera 70 x 50: %.1f %% hit" % (100.0 * hit.mean()))
    assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05
    t_only, none = w.cast_camera(scene.march, cam, size, normals=False, aniso=a)
    assert none is None and _same(t_only, t)


@ARITH
def test_the_isotropic_limit_is_the_density_field(scene, ieee):
    w = scene.worker(ieee)
    o, v, _ = scene.rays[ieee]
    t, n = scene.cast(ieee, "density")
    limit = scene.ws.fluid.aniso_params(smoothing=0.0, lone_scale=1.0, min_neighbours=0xFFFFFFFF)
    tl, nl = w.cast_rays(scene.march, o, v, aniso=limit)
    assert _same(tl, t) and _same(nl, n)
    cam, _ = _camera_45(scene.ws)
    tc, nc = w.cast_camera(scene.march, cam, (70, 50))
    tcl, ncl = w.cast_camera(scene.march, cam, (70, 50), aniso=limit)
    assert _same(tcl, tc) and _same(ncl, nc)


def _trajectory(ws, pos, params, steps, cast, graph):
    w = ws.FluidWorker(pos, params, graph=graph)
    march = _march(ws, params)
    # above the thin C1 sheet (16 x 18 x 0.2), looking at it along -z
    cam = ws.fluid.camera((0.0, 0.0, 12.0), (0.0, 0.0, -1.0), (0.8, 0.0, 0.0), (0.0, 0.9, 0.0))
    hits = 0
    for t in range(steps):
        w.run(1)
        if cast:
            d, _ = w.cast_camera(march, cam, (32, 24), normals=(t % 2 == 0))
            hits += int(np.isfinite(d).sum())
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats, hits


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_casting_every_step_leaves_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _, _ = _trajectory(ws, pos, params, 100, False, graph)
    got, stats, hits = _trajectory(ws, pos, params, 100, True, graph)
    assert hits > 0
    if graph:
        assert stats["graph_steps"] > 0
    assert got.dtype.itemsize == 80
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_slabs_cast_the_same_bits_as_a_single_handle(scene):
    ws = scene.ws
    world = 2
    o, v, _ = scene.rays[False]
    cam, _ = _camera_45(ws)
    single = scene.worker(False)
    want = [scene.cast(False, "density"), single.cast_camera(scene.march, cam, (70, 50)), scene.cast(False, "aniso")]
    owner = ws.slab.assign(scene.params, scene.pos, world)
    hub = ws.slab.LoopbackHub(world)
    got = [None] * world
    errors = []

    def body(r):
        try:
            sel = np.flatnonzero(owner == r).astype(np.uint32)
            s = ws.slab.SlabWorker(scene.pos[sel], sel, scene.pos.shape[0], scene.params, r, world, hub.transport(r))
            s.run(STEPS)
            wanted = r != 1  # rank 1 only contributes
            got[r] = [s.cast_rays(scene.march, o, v, want=wanted), s.cast_camera(scene.march, cam, (70, 50), want=wanted),
                      s.cast_rays(scene.march, o, v, want=wanted, aniso=ws.fluid.aniso_params())]
            s.close()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not errors, errors
    assert got[1] == [(None, None)] * 3
    for (t, n), (wt, wn) in zip(got[0], want):
        assert _same(t.reshape(-1), wt.reshape(-1)) and _same(n.reshape(-1, 3), wn.reshape(-1, 3))


def test_invalid_arguments_are_refused_and_the_handle_steps_on_and_casts(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    good = dict(t_start=0.0, dt=0.125, steps=160, refine=6, iso=5.0)
    o = np.tile(np.array([0.0, 0.0, 12.0], F32), (4, 1))
    v = np.tile(np.array([0.1, 0.2, -1.0], F32), (4, 1))
    out_t = np.empty(64, F32)
    out_n = np.empty((64, 3), F32)
    cam_good = dict(eye=(0.0, 0.0, 12.0), forward=(0.0, 0.0, -1.0), right=(0.8, 0.0, 0.0), up=(0.0, 0.9, 0.0))
    size = np.array([8, 8], np.uint32)

    def rays(o=o, v=v, m=4, t=out_t, n=out_n, r=True, **kw):
        p = dict(good)
        p.update(kw)
        march = ws.fluid.ray_params(p["t_start"], p["dt"], p["steps"], p["refine"], p["iso"])
        return L.ws_cast_rays(h, None, C.byref(march) if r else None, None if o is None else o.ctypes.data,
                              None if v is None else v.ctypes.data, m, None if t is None else t.ctypes.data,
                              None if n is None else n.ctypes.data)

    def camera(size=size, cam=True, r=True, t=out_t, n=out_n, **kw):
        c = dict(cam_good)
        c.update({k: kw.pop(k) for k in list(kw) if k in c})
        p = dict(good)
        p.update(kw)
        march = ws.fluid.ray_params(p["t_start"], p["dt"], p["steps"], p["refine"], p["iso"])
        cs = ws.fluid.camera(c["eye"], c["forward"], c["right"], c["up"])
        return L.ws_cast_camera(h, None, C.byref(march) if r else None, C.byref(cs) if cam else None,
                                None if size is None else size.ctypes.data, None if t is None else t.ctypes.data,
                                None if n is None else n.ctypes.data)

    def bad(x, i, val):
        x = x.copy()
        x[i] = val
        return x

    assert rays() == 0 and camera() == 0
    march_cases = [dict(steps=0), dict(steps=65536), dict(refine=25), dict(dt=0.0), dict(dt=-0.125), dict(dt=np.inf),
                   dict(dt=np.nan), dict(iso=0.0), dict(iso=-1.0), dict(iso=np.nan), dict(iso=np.inf), dict(t_start=np.nan),
                   dict(t_start=-np.inf), dict(t_start=2e15), dict(t_start=-2e15), dict(dt=1e11, steps=65535)]
    for kw in march_cases:
        assert rays(**kw) == 1, kw
        assert camera(**kw) == 1, kw
    assert rays(r=False) == 1 and camera(r=False) == 1
    assert rays(t=None, n=None) == 1 and camera(t=None, n=None) == 1  # both outputs NULL on a single handle
    assert rays(o=None) == 1 and rays(v=None) == 1 and rays(m=0) == 1
    assert rays(m=(1 << 28) + 1) == 1  # refused before a ray is read
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        assert rays(o=bad(o, (2, 1), val)) == 1, val
        assert rays(v=bad(v, (3, 0), val)) == 1, val
        for name in ("eye", "forward", "right", "up"):
            assert camera(**{name: (0.3, val, -1.0)}) == 1, (name, val)
    assert rays(v=bad(v, 1, 0.0)) == 1  # one direction is (0, 0, 0)
    assert camera(forward=(0.0, 0.0, 0.0)) == 1
    assert camera(cam=False) == 1 and camera(size=None) == 1
    assert camera(size=np.array([0, 8], np.uint32)) == 1 and camera(size=np.array([8, 0], np.uint32)) == 1
    assert camera(size=np.array([1 << 15, 1 << 14], np.uint32)) == 1  # 2^29 rays
    bad_aniso = ws.fluid.aniso_params(max_ratio=0.5)
    march = ws.fluid.ray_params(**good)
    assert L.ws_cast_rays(h, C.byref(bad_aniso), C.byref(march), o.ctypes.data, v.ctypes.data, 4, out_t.ctypes.data, None) == 1
    assert rays() == 0 and camera() == 0
    # the handle steps on and casts what a handle that saw no refusal casts
    fresh = ws.FluidWorker(pos, params)
    cs = ws.fluid.camera(**cam_good)
    for x in (w, fresh):
        x.run(20)
    a, b = w.read_vec("particles"), fresh.read_vec("particles")
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    ta, na = w.cast_camera(march, cs, (32, 24))
    tb, nb = fresh.cast_camera(march, cs, (32, 24))
    assert np.isfinite(ta).any() and _same(ta, tb) and _same(na, nb)
    w.close()
    fresh.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    march = _march(ws, params)
    cam = ws.fluid.camera((0.0, 0.0, 12.0), (0.0, 0.0, -1.0), (0.8, 0.0, 0.0), (0.0, 0.9, 0.0))
    for call in (lambda: w.cast_rays(march, [[0.0, 0.0, 12.0]], [[0.0, 0.0, -1.0]]), lambda: w.cast_camera(march, cam, (8, 8))):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.close()


def test_a_dead_handle_refuses_both_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    march = _march(ws, params)
    cam = ws.fluid.camera((0.0, 0.0, 12.0), (0.0, 0.0, -1.0), (0.8, 0.0, 0.0), (0.0, 0.9, 0.0))
    t, _ = w.cast_camera(march, cam, (8, 8))
    assert np.isfinite(t).any()
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in (lambda: w.cast_rays(march, [[0.0, 0.0, 12.0]], [[0.0, 0.0, -1.0]]), lambda: w.cast_camera(march, cam, (8, 8))):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
