"""ws_body_forces on the GPU: every output bit for bit against the numpy restatement (tests/bodies_ref.py) applied to what
ws_sample_velocity_points returns at the samples -- at every chunk shape of the summation tree, in both arithmetics, on
every cell grid --, a sample's outputs independent of how the samples are grouped, the call leaving the trajectory alone (a
captured step included), slabs, refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import bodies_ref as B
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_forces import _scene as forces_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK = 256  # samples per workgroup of k_body_forces (WS_BLOCK): one node of a body's tree at level 8
# an empty body, one sample, chunks short of / at / past a wave and a chunk, 4 chunks short of a power of two, 17 chunks
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097)
ABOVE, DEEP = SIZES.index(255), SIZES.index(256)
OUTPUTS = ("force", "torque", "volume", "wet", "sample_force", "sample_fraction")


def boxes(rng, sizes, lo, hi):
    """Jittered samples in one box per body: (xyz (m, 3), velocity (m, 3), volume (m,), body_start, centres (nb, 3));
    lo, hi: (nb, 3) corners.  A body's material velocity is a rigid motion about its centre."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    xyz, vel, vol = [], [], []
    centres = (0.5 * (lo + hi)).astype(F32)
    for b, c in enumerate(sizes):
        p = lo[b] + rng.random((c, 3)) * (hi[b] - lo[b])
        lin, ang = rng.normal(0.0, 0.5, 3), rng.normal(0.0, 1.0, 3)
        xyz.append(p)
        vel.append(lin + np.cross(ang, p - centres[b].astype(np.float64)))
        vol.append(np.full(c, np.prod(hi[b] - lo[b]) / max(c, 1)) * rng.uniform(0.5, 1.5, c))
    return (np.concatenate(xyz).astype(F32), np.concatenate(vel).astype(F32), np.concatenate(vol).astype(F32), start, centres)


@functools.lru_cache(maxsize=None)
def pool_scene():
    """4 096 particles in the lower half of a 4 x 4 x 4 container with random velocities, and the twelve bodies: most
    straddle the fluid's top at y = 0, one hangs wholly above it, one lies deep inside."""
    import water_sandbox_amd as ws

    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    lo, hi = list(params.ext_min), list(params.ext_max)
    hi[1] = 0.0
    pos = ws.workloads.uniform_cloud(4096, 77, lo, hi)
    rng = np.random.default_rng(2024)
    vel = rng.normal(0.0, 1.5, (4096, 3)).astype(F32)
    nb = len(SIZES)
    cx = rng.uniform(-1.3, 1.3, (nb, 3))
    cx[:, 1] = rng.uniform(-0.1, 0.1, nb)                 # straddling y = 0 ...
    half = np.tile([0.35, 0.45, 0.35], (nb, 1))
    cx[ABOVE, 1], half[ABOVE, 1] = 1.2, 0.3               # ... wholly above: further than h from every particle
    cx[DEEP, 1], half[DEEP, 1] = -1.0, 0.2                # ... deep inside
    return (pos, vel, params) + boxes(rng, SIZES, cx - half, cx + half)


def load_velocities(w, vel):
    rec = w.read_vec("particles")
    rec["velocity"][:, :3] = vel
    w.write_slice("particles", rec)


def restated(w, params, bp, xyz, vel, vol, start, centres):
    """The restatement on the handle's own field at the samples."""
    u, rho = w.sample_velocity_points(xyz, density=True)
    par = dict(fluid_density=F32(bp.fluid_density), drag=F32(bp.drag), rest_density=F32(bp.rest_density))
    return B.forces(par, list(params.gravity)[:3], params.target_density, u, rho, xyz, vel, vol, start, centres), rho


def assert_same(got, want, what):
    for k in OUTPUTS:
        g, x = getattr(got, k), want[k]
        if k == "wet":
            assert g.dtype == np.uint32 and np.array_equal(g, x), (what, k, g, x)
        else:
            assert same_bits(g, x), (what, k, int(np.count_nonzero(g.view(np.uint32) != x.view(np.uint32))))


def no_minus_zero(got):
    for k in OUTPUTS:
        a = getattr(got, k)
        if a.dtype == F32:
            assert not np.any(np.signbit(a) & (a == 0)), k


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_every_output_has_the_restatements_bits(ws, ieee):
    pos, vel, params, xyz, wv, vol, start, centres = pool_scene()
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    load_velocities(w, vel)
    sizes = np.diff(start.astype(np.int64))
    assert tuple(sizes) == SIZES and len(xyz) == sum(SIZES)
    # rest_density 0 takes the handle's target_density; the other case saturates more samples
    for bp in (ws.fluid.body_params(), ws.fluid.body_params(fluid_density=650.0, drag=80.0, rest_density=4.0)):
        want, rho = restated(w, params, bp, xyz, wv, vol, start, centres)
        got = w.body_forces(bp, xyz, wv, vol, start, centres, samples=True)
        assert_same(got, want, (ieee, bp.rest_density))
        # what the scene is built for
        f = got.sample_fraction
        assert np.any((f > 0) & (f < 1)) and np.any(f == 1) and np.any(f == 0)
        assert got.wet[ABOVE] == 0 and not got.force[ABOVE].view(np.uint32).any() and not got.torque[ABOVE].view(np.uint32).any()
        assert not got.volume[ABOVE:ABOVE + 1].view(np.uint32).any()
        assert got.wet[DEEP] == SIZES[DEEP]
        assert np.count_nonzero((got.wet > 0) & (got.wet < sizes)) >= 3
        assert got.wet[0] == 0 and not got.force[0].view(np.uint32).any()  # the empty body
        assert got.wet.sum() == np.count_nonzero(rho > 0)
        no_minus_zero(got)
        assert np.all(got.force[got.wet > 0, 1] > 0)  # gravity points down: the lift wins over this scene's drag
        # without the per-sample outputs: the same per-body bits
        plain = w.body_forces(bp, xyz, wv, vol, start, centres)
        assert plain.sample_force is None and plain.sample_fraction is None
        for k in OUTPUTS[:4]:
            assert np.array_equal(getattr(plain, k).view(np.uint32), getattr(got, k).view(np.uint32)), k
    w.close()


def test_single_outputs_and_every_body_size_as_one_call_each(ws):
    """Each output alone (the others NULL), and each body as a call of its own: a body's bits do not depend on its
    neighbours in the call."""
    pos, vel, params, xyz, wv, vol, start, centres = pool_scene()
    w = ws.FluidWorker(pos, params)
    load_velocities(w, vel)
    bp = ws.fluid.body_params()
    all_ = w.body_forces(bp, xyz, wv, vol, start, centres, samples=True)
    L, h = w._L, w._h
    for k, name in enumerate(OUTPUTS):
        out = np.empty_like(getattr(all_, name))
        ptrs = [None] * 6
        ptrs[k] = out.ctypes.data
        assert L.ws_body_forces(h, C.byref(bp), xyz.ctypes.data, wv.ctypes.data, vol.ctypes.data, len(xyz), start.ctypes.data,
                                centres.ctypes.data, len(SIZES), *ptrs) == 0, name
        assert np.array_equal(out.view(np.uint32), getattr(all_, name).view(np.uint32)), name
    for b in range(1, len(SIZES)):
        s = slice(int(start[b]), int(start[b + 1]))
        one = w.body_forces(bp, xyz[s], wv[s], vol[s], [0, SIZES[b]], centres[b:b + 1], samples=True)
        for name in OUTPUTS[:4]:
            assert np.array_equal(getattr(one, name)[0].view(np.uint32), getattr(all_, name)[b].view(np.uint32)), (b, name)
        assert same_bits(one.sample_force, all_.sample_force[s]) and same_bits(one.sample_fraction, all_.sample_fraction[s])
    w.close()


def test_bodies_of_more_chunks_than_a_wave_finishes_at_a_time(ws):
    """The finishing kernel takes a body's chunk partials 64 at a time and merges the blocks' nodes like the carries of a
    binary counter: 129 chunks (three blocks: the last fold meets two stack levels), 193 chunks (four blocks: a merge
    through two levels) and exactly 64 (one full block: the padded level is the fold's own +0)."""
    pos, vel, params = pool_scene()[:3]
    w = ws.FluidWorker(pos, params)
    load_velocities(w, vel)
    rng = np.random.default_rng(64)
    sizes = (2 * 64 * CHUNK + 1, 7, 3 * 64 * CHUNK + 5, 64 * CHUNK)
    lo = np.tile([-1.5, -0.6, -1.5], (len(sizes), 1))
    hi = np.tile([1.5, 0.4, 1.5], (len(sizes), 1))
    xyz, wv, vol, start, centres = boxes(rng, sizes, lo, hi)
    bp = ws.fluid.body_params()
    want, rho = restated(w, params, bp, xyz, wv, vol, start, centres)
    got = w.body_forces(bp, xyz, wv, vol, start, centres, samples=True)
    assert_same(got, want, "many chunks")
    big = [0, 2, 3]
    assert np.all(got.wet[big] > 10000) and np.all(got.wet[big] < np.asarray(sizes)[big])
    w.close()


# ---- 2. grouping -----------------------------------------------------------------------------------------------------------------
def test_grouping_does_not_matter_to_a_sample(ws):
    pos, vel, params, xyz, wv, vol, start, centres = pool_scene()
    w = ws.FluidWorker(pos, params)
    load_velocities(w, vel)
    bp = ws.fluid.body_params()
    m = len(xyz)
    par = dict(fluid_density=F32(bp.fluid_density), drag=F32(bp.drag), rest_density=F32(0.0))
    _, rho = w.sample_velocity_points(xyz, density=True)
    first = None
    for grouping in ([0, m], list(range(0, m, 100)) + [m], [0, 0, 1, CHUNK + 1, CHUNK + 1, 3 * CHUNK, m, m]):
        bs = np.asarray(grouping, np.uint32)
        c = np.random.default_rng(len(bs)).uniform(-1.0, 1.0, (len(bs) - 1, 3)).astype(F32)
        got = w.body_forces(bp, xyz, wv, vol, bs, c, samples=True)
        if first is None:
            first = got
        assert same_bits(got.sample_force, first.sample_force) and same_bits(got.sample_fraction, first.sample_fraction)
        # the per-body sums are the canonical sums of the per-sample outputs
        T = B.torque_terms(xyz, c[B.body_of_sample(bs)], got.sample_force)
        T[~(rho > 0)] = 0
        sv = np.where(rho > 0, (vol * got.sample_fraction).astype(F32), F32(0.0)).astype(F32)
        force, torque, volume, count = B.reduce(bs, got.sample_force, T, sv, rho > 0)
        assert same_bits(got.force, force) and same_bits(got.torque, torque) and same_bits(got.volume, volume)
        assert np.array_equal(got.wet, count)
    assert first.wet[0] > 1000
    w.close()


# ---- 3. every cell grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_merged_cells_and_a_regridded_handle(ws, ieee):
    rng = np.random.default_rng(31)
    bp = ws.fluid.body_params(rest_density=0.0)
    # 16 x 9 x 9 at h = 0.04: merged cells; the fluid is a cube of edge 0.32 in the lowest corner
    pos, params, _, centre, reach = forces_scene(ws, "merged-4096")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    assert w.stats()["cells_merged"] != (1, 1, 1)
    load_velocities(w, rng.normal(0.0, 0.5, (len(pos), 3)).astype(F32))
    sizes = (5, 300, 0, 257, 64)
    c = centre + rng.uniform(-0.4, 0.4, (len(sizes), 3)) * reach
    c[:, 1] = centre[1] + 0.5 * reach                          # straddling the cube's top
    half = np.full((len(sizes), 3), 0.25 * reach)
    xyz, wv, vol, start, centres = boxes(rng, sizes, c - half, c + half)
    want, _ = restated(w, params, bp, xyz, wv, vol, start, centres)
    got = w.body_forces(bp, xyz, wv, vol, start, centres, samples=True)
    assert_same(got, want, "merged")
    assert np.count_nonzero((got.wet > 0) & (got.wet < np.asarray(sizes))) >= 2
    w.close()
    # the pool, re-gridded to another radius
    pos, vel, params, xyz, wv, vol, start, centres = pool_scene()
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    load_velocities(w, vel)
    before = w.body_forces(bp, xyz, wv, vol, start, centres)
    other = ws.make_params(container_size=(4.0, 4.0, 4.0), smoothing_radius=F32(0.2))
    w.set_params(other)
    want, _ = restated(w, other, bp, xyz, wv, vol, start, centres)
    got = w.body_forces(bp, xyz, wv, vol, start, centres, samples=True)
    assert_same(got, want, "regrid")
    assert not same_bits(got.force, before.force) and got.wet[DEEP] > 0
    w.close()


# ---- 4. reads only ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_the_call_every_step_leaves_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    rng = np.random.default_rng(6)
    sizes = (300, 64, 0, 700)
    c = rng.uniform(-4.0, 4.0, (len(sizes), 3))
    c[:, 2] = 0.0
    half = np.tile([1.5, 1.5, 0.05], (len(sizes), 1))
    xyz, wv, vol, start, centres = boxes(rng, sizes, c - half, c + half)
    bp = ws.fluid.body_params()
    plain = ws.FluidWorker(pos, params, graph=graph)
    called = ws.FluidWorker(pos, params, graph=graph)
    replayed, wet = [], 0
    for t in range(20):
        done = called.steps_done()
        got = called.body_forces(bp, xyz, wv, vol, start, centres, samples=(t % 2 == 0))
        assert called.steps_done() == done == t
        wet += int(got.wet.sum())
        called.run(1)
        plain.run(1)
        if graph:
            replayed.append(called.stats()["graph_steps"])
    assert wet > 20 * 100
    want, have = plain.read_vec("particles"), called.read_vec("particles")
    assert np.array_equal(have.view(np.uint8), want.view(np.uint8))
    if graph:  # the captured step was neither dropped nor bypassed: one replay per step from the second step on
        assert all(replayed[t] - replayed[t - 1] == 1 for t in range(1, 20)), replayed
        assert plain.stats()["graph_steps"] > 0
    # between the two halves of an asynchronous readback
    buf = np.empty((called.n, 3), F32)
    called.read_positions_begin(buf)
    again = called.body_forces(bp, xyz, wv, vol, start, centres)
    called.read_positions_end()
    assert same_bits(buf, plain.read_positions())
    want, _ = restated(called, params, bp, xyz, wv, vol, start, centres)
    assert same_bits(again.force, want["force"]) and same_bits(again.torque, want["torque"])
    plain.close()
    called.close()


# ---- 5. slabs --------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 4


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    rng = np.random.default_rng(12)
    # the cuts of 2 and 3 slabs of the 16-wide container lie at x = 0 and near +-2.7: the boxes straddle them; the last
    # one also sticks out of the container's top
    sizes = (600, 0, 257, 1, 900)
    lo = np.array([[-1.0, -3.0, -1.0], [0.0, 0.0, 0.0], [-3.5, -1.0, 1.0], [2.6, 0.0, 0.0], [1.5, 3.0, -2.0]])
    hi = np.array([[1.0, -2.0, 1.0], [0.0, 0.0, 0.0], [-2.0, 0.5, 2.5], [2.8, 0.2, 0.2], [4.0, 6.0, 0.0]])
    xyz, wv, vol, start, centres = boxes(rng, sizes, lo, hi)
    bp = ws.fluid.body_params(rest_density=6.0)
    w = ws.FluidWorker(pos, params)
    want = []
    for t in range(SLAB_STEPS):
        w.run(1)
        want.append(w.body_forces(bp, xyz, wv, vol, start, centres, samples=True))
    w.close()
    assert 0 < want[-1].wet[4] < sizes[4] and want[-1].wet[0] > sizes[0] // 2 and want[0].force.any()
    decreasing = start.copy()
    decreasing[2] = decreasing[1] - 1

    def program(s, r):
        out = []
        for t in range(SLAB_STEPS):
            s.run(1)
            if t == 2 and r == 0:
                # this rank passes a decreasing body_start: it alone is refused, after the gather -- no peer is left waiting
                f = np.full((len(sizes), 3), 7, F32)
                st = s._L.ws_body_forces(s._h, C.byref(bp), xyz.ctypes.data, wv.ctypes.data, vol.ctypes.data, len(xyz),
                                         decreasing.ctypes.data, centres.ctypes.data, len(sizes), f.ctypes.data, None, None, None,
                                         None, None)
                assert st == 1 and np.all(f == 7), (r, t, st)
                out.append("refused")
            else:
                out.append(s.body_forces(bp, xyz, wv, vol, start, centres, samples=True, want=(r != 1)))  # rank 1 only contributes
        return out

    got = _slab_run(ws, params, pos, world, 0, program)
    for r in range(world):
        assert len(got[r]) == SLAB_STEPS
        for t, (a, b) in enumerate(zip(got[r], want)):
            if r == 1:
                assert a is None
            elif r == 0 and t == 2:
                assert a == "refused"
            else:
                for k in OUTPUTS:
                    assert np.array_equal(getattr(a, k).view(np.uint32), getattr(b, k).view(np.uint32)), (r, t, k)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    rng = np.random.default_rng(3)
    xyz, wv, vol, start, centres = boxes(rng, (5, 0, 300), [[-1, -1, -0.05]] * 3, [[1, 1, 0.05]] * 3)
    m, nb = len(xyz), 3
    steps = 0

    def ptr(x):
        return None if x is None else x.ctypes.data

    def call(p=True, xyz=xyz, vel=wv, vol=vol, m=m, start=start, centres=centres, nb=nb, outs=True, **fields):
        par = ws.fluid.WsBodyParams(1000.0, 500.0, 0.0, 0)
        for k, v in fields.items():
            setattr(par, k, v)
        ms = len(vol) if vol is not None else 1
        out = [np.full((3, 3), 7, F32), np.full((3, 3), 7, F32), np.full(3, 7, F32), np.full(3, 7, np.uint32),
               np.full((ms, 3), 7, F32), np.full(ms, 7, F32)]
        st = L.ws_body_forces(h, C.byref(par) if p else None, ptr(xyz), ptr(vel), ptr(vol), m, ptr(start), ptr(centres), nb,
                              *((ptr(o) for o in out) if outs else (None,) * 6))
        assert st == 0 or all(np.all(o == 7) for o in out)  # a refusal writes nothing
        return st

    def bad(x, i, val):
        x = x.copy()
        x[i] = val
        return x

    cases = [("NULL p", dict(p=False)), ("NULL xyz", dict(xyz=None)), ("NULL velocity", dict(vel=None)),
             ("NULL volume", dict(vol=None)), ("NULL body_start", dict(start=None)), ("NULL centres", dict(centres=None)),
             ("every output NULL", dict(outs=False)), ("m 0", dict(m=0)), ("m > 2^28", dict(m=(1 << 28) + 1)),
             ("nb 0", dict(nb=0)), ("nb > 2^24", dict(nb=(1 << 24) + 1)),
             ("start[0] != 0", dict(start=bad(start, 0, 1))), ("start[nb] != m", dict(start=bad(start, 3, m - 1))),
             ("start[nb] > m", dict(start=bad(start, 3, m + 1))), ("decreasing", dict(start=np.array([0, 9, 5, m], np.uint32))),
             ("negative volume", dict(vol=bad(vol, 7, -1e-6))), ("reserved", dict(reserved=1))]
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        cases += [("xyz %r" % val, dict(xyz=bad(xyz, (2, 1), val))), ("velocity %r" % val, dict(vel=bad(wv, (300, 0), val))),
                  ("centre %r" % val, dict(centres=bad(centres, (1, 2), val)))]
        if not val < 0:
            cases.append(("volume %r" % val, dict(vol=bad(vol, m - 1, val))))
    for name in ("fluid_density", "drag", "rest_density"):
        for val in (np.nan, np.inf, -np.inf, -0.5):
            cases.append(("%s %r" % (name, val), {name: val}))
    for what, kw in cases:
        assert call(**kw) == 1, what
        w.run(2)  # ... followed by two good steps
        steps += 2
    fresh.run(steps)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # allowed: the largest magnitudes, samples that stand for no volume, no drag, no lift, an explicit rest density
    assert call() == 0
    assert call(xyz=bad(xyz, (0, 0), 1e15)) == 0 and call(vel=bad(wv, (0, 1), -1e15)) == 0 and call(vol=bad(vol, 0, 1e15)) == 0
    assert call(centres=bad(centres, (0, 0), -1e15)) == 0
    assert call(vol=np.zeros_like(vol)) == 0 and call(drag=0.0) == 0 and call(fluid_density=0.0) == 0
    assert call(rest_density=3.0) == 0
    w.run(2)
    fresh.run(2)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    w.close()
    fresh.close()


def _a_call(ws, w):
    q = np.zeros((1, 3), F32)
    return lambda: w.body_forces(ws.fluid.body_params(), q, q, np.ones(1, F32), [0, 1], q)


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    with pytest.raises(ws.WsError) as e:
        _a_call(ws, w)()
    assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_the_call(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    assert _a_call(ws, w)().wet[0] == 1
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    with pytest.raises(ws.WsError) as e:
        _a_call(ws, w)()
    assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
