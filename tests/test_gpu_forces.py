"""ws_apply_forces on the GPU: bit for bit against the numpy restatement (tests/forces_ref.py) at every launch shape, the
step picking the new velocities up exactly as it picks up a host edit through ws_write_particles, a call that reaches
nothing changing nothing (a captured step included), the views the call must leave alone, slabs, refusals."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as F
from test_gpu_aniso_surface import _slab_run, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
BLOCK = 256  # threads per workgroup of k_edit_current (WS_BLOCK)


def _xyz(rec, field):
    return np.ascontiguousarray(rec[field][:, :3])


def _load(w, rec, vel, pred=None):
    """Route B of the issue: the state with new velocities (and predicted positions) through ws_write_particles."""
    rec = rec.copy()
    rec["velocity"][:, :3] = vel
    if pred is not None:
        rec["predicted_position"][:, :3] = pred
    w.write_slice("particles", rec)


def _host_apply(w, forces, dt):
    """ws_read_particles, the restatement on the host, ws_write_particles: what a host without the call has to do."""
    rec = w.read_vec("particles")
    vel, pred, counts = F.apply(_xyz(rec, "position"), _xyz(rec, "velocity"), forces, dt)
    _load(w, rec, vel, pred)
    return counts


# ---- 1. bits against the restatement ------------------------------------------------------------------------------------------
def _emitter_sets():
    rng = np.random.default_rng(42)
    sets = {
        "radial": [F.emitter(F.RADIAL, (0, 0, 0), 0.5, 9.0, damping=1.5)],
        "jet": [F.emitter(F.JET, (0, 0, 0), 0.5, 7.0, axis=(0.3, 1.0, -0.2))],
        "vortex": [F.emitter(F.VORTEX, (0, 0, 0), 0.5, -11.0, axis=(0.0, 2.0, 0.5), damping=0.75)],
    }
    mixed = [F.emitter(F.RADIAL, (0, 0, 0), 0.5, -6.0)]
    for e in range(1, 15):
        mixed.append(F.emitter(e % 3, rng.uniform(-0.7, 0.7, 3), rng.uniform(0.3, 1.2), rng.normal(0.0, 20.0),
                               rng.normal(0.0, 1.5, 3), rng.uniform(0.0, 3.0) if e % 2 else 0.0))
    mixed.append(F.emitter(F.JET, (50.0, 50.0, 50.0), 1.0, 5.0, axis=(1, 0, 0)))  # sees nothing
    sets["mixed16"] = mixed
    return sets


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000, 4097])
def test_the_call_gives_the_restatements_bits(ws, n):
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(n)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    pos[0] = 0.0                      # exactly at the centre of every set's first emitter
    if n > 1:
        pos[1] = (0.5, 0.0, 0.0)      # exactly d == R of it: out
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    vel[::5, 0] = F32(-0.0)
    vel[2::7] = F32(-0.0)
    w = ws.FluidWorker(pos, params)
    rec = w.read_vec("particles")
    dt = F32(1.0 / 60.0)
    for name, forces in _emitter_sets().items():
        _load(w, rec, vel)
        counts = w.apply_forces(F.to_ws(ws, forces), dt)
        got = w.read_vec("particles")
        want_v, want_p, want_c = F.apply(pos, vel, forces, dt)
        _, hit, _ = F.accelerate(pos, vel, forces)
        assert np.array_equal(counts, want_c), (name, counts, want_c)
        assert same_bits(_xyz(got, "position"), pos), name
        assert same_bits(_xyz(got, "velocity"), want_v), name
        assert same_bits(_xyz(got, "predicted_position"), want_p), name
        first = F.accelerate(pos, vel, forces[:1])[1]  # the centre is in reach of the set's first emitter, d == R is not
        assert first[0] and (n == 1 or not first[1]), name
        if name == "mixed16":
            assert counts[-1] == 0 and len(counts) == 16
            assert n < 64 or (counts[:15] > 0).sum() >= 12
        if n >= 63 and name != "mixed16":  # most particles are out of reach, some of them with -0 components: kept as they are
            assert 0 < hit.sum() < n, name
            v_out = _xyz(got, "velocity")[~hit]
            assert np.any(np.signbit(v_out) & (v_out == 0)), name
        # without counts: the same state
        _load(w, rec, vel)
        assert w.apply_forces(F.to_ws(ws, forces), dt, counts=False) is None
        assert same_bits(_xyz(w.read_vec("particles"), "velocity"), want_v), name
    w.close()


# ---- 2. the step picks it up exactly as a host edit ---------------------------------------------------------------------------
def _moving(t, centre, reach, h):
    """A RADIAL puller, a JET and a VORTEX that move with the step number t."""
    c = np.asarray(centre, np.float64)
    s = 0.35 * reach
    return [F.emitter(F.RADIAL, c + s * np.array([np.cos(0.3 * t), 0.2, np.sin(0.3 * t)]), 0.6 * reach, 4.0 * h / 0.25, damping=1.0),
            F.emitter(F.JET, c + s * np.array([-0.5, 0.1 * t / 20.0, 0.4]), 0.5 * reach, 6.0 * h / 0.25, axis=(0.2, 1.0, 0.1)),
            F.emitter(F.VORTEX, c + s * np.array([0.3, -0.2, 0.05 * t / 20.0]), 0.8 * reach, 3.0, axis=(0.0, 1.0, 0.0), damping=0.5)]


def _scene(ws, which):
    if which == "merged-4096":
        # 16 x 9 x 9 at h = 0.04: the product library merges cells on its own; a jittered lattice in the lowest corner
        h = F32(0.04)
        params = ws.make_params(container_size=(16.0, 9.0, 9.0), smoothing_radius=h)
        ijk = np.stack(np.meshgrid(*(np.arange(16),) * 3, indexing="ij"), -1).reshape(-1, 3)
        lo = np.asarray(params.ext_min[:3], np.float64)
        pos = (lo + (ijk + 0.5 * np.random.default_rng(8).random((4096, 3))) * (float(h) / 2)).astype(F32)
        return pos, params, None, lo + 8 * float(h) / 2, 16 * float(h) / 2
    # 31 646 = twice the x prime of hash_cell: the handle takes the multiplicity path of the neighbour kernels
    params = ws.make_params(container_size=(6.0, 4.0, 4.0))
    pos = ws.workloads.uniform_cloud(31646, 99, list(params.ext_min), list(params.ext_max))
    regrid = ws.make_params(container_size=(6.0, 4.0, 4.0), smoothing_radius=F32(0.2))
    return pos, params, regrid, np.zeros(3), 3.0


@pytest.mark.parametrize("which", ["merged-4096", "regrid-31646"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_step_picks_the_call_up_exactly_as_a_host_edit(ws, which, ieee):
    pos, params, regrid, centre, reach = _scene(ws, which)
    a = ws.FluidWorker(pos, params, ieee_division=ieee)
    b = ws.FluidWorker(pos, params, ieee_division=ieee)
    if which == "merged-4096":
        assert a.stats()["cells_merged"] != (1, 1, 1)
    dt = F32(params.delta_time)
    seen = 0
    for t in range(20):
        if regrid is not None and t == 10:
            a.set_params(regrid)
            b.set_params(regrid)
        forces = _moving(t, centre, reach, float(params.smoothing_radius))
        ca = a.apply_forces(F.to_ws(ws, forces), dt)
        cb = _host_apply(b, forces, dt)
        assert np.array_equal(ca, cb), (t, ca, cb)
        seen += int(ca.sum())
        a.run(1)
        b.run(1)
        assert same_bits(a.read_positions(), b.read_positions()), t
        assert same_bits(a.read_velocities(), b.read_velocities()), t
    assert seen > 20 * 50 and a.steps_done() == 20
    a.close()
    b.close()


# ---- 3. nothing in reach changes nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_a_call_that_reaches_nothing_changes_nothing(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    outside = ws.fluid.force("radial", (100.0, 100.0, 100.0), 1.0, 50.0, damping=3.0)
    plain = ws.FluidWorker(pos, params, graph=graph)
    called = ws.FluidWorker(pos, params, graph=graph)
    replayed = []
    for t in range(50):
        counts = called.apply_forces(outside, F32(params.delta_time), counts=(t % 2 == 0))
        assert counts is None or counts[0] == 0
        called.run(1)
        plain.run(1)
        if graph:
            replayed.append(called.stats()["graph_steps"])
    want, got = plain.read_vec("particles"), called.read_vec("particles")
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if graph:  # the captured step was neither dropped nor bypassed: one replay per step from the second step on
        assert all(replayed[t] - replayed[t - 1] == 1 for t in range(1, 50)), replayed
        assert plain.stats()["graph_steps"] > 0
    plain.close()
    called.close()


# ---- 4. views ---------------------------------------------------------------------------------------------------------------------
def test_the_views_of_the_last_step_stay_and_the_readers_see_the_new_velocities(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(12)
    before = w.read_vec("particles")
    forces = _moving(3, np.zeros(3), 6.0, 0.25)
    dt = F32(params.delta_time)
    counts = w.apply_forces(F.to_ws(ws, forces), dt)
    after = w.read_vec("particles")
    want_v, want_p, want_c = F.apply(_xyz(before, "position"), _xyz(before, "velocity"), forces, dt)
    assert np.array_equal(counts, want_c) and counts.min() > 0
    assert before["density"].any() and before["acceleration"].any()
    for field in ("position", "density", "pressure", "acceleration"):
        assert same_bits(after[field], before[field]), field
    assert same_bits(_xyz(after, "velocity"), want_v) and same_bits(_xyz(after, "predicted_position"), want_p)
    assert not same_bits(want_v, _xyz(before, "velocity"))
    assert w.steps_done() == 12
    assert same_bits(w.read_velocities(), want_v)
    # the velocity field sums the new velocities: the bits of a handle that was loaded with them
    q = _xyz(before, "position")[::16] + F32(0.01)
    other = ws.FluidWorker(pos, params)
    _load(other, before, want_v, want_p)
    got, ref = w.sample_velocity_points(q, density=True), other.sample_velocity_points(q, density=True)
    assert ref[0].any() and same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])
    # ... between the two halves of an asynchronous readback too
    buf = np.empty((w.n, 3), F32)
    w.read_positions_begin(buf)
    w.apply_forces(F.to_ws(ws, forces), dt, counts=False)
    w.read_positions_end()
    assert same_bits(buf, _xyz(before, "position"))
    w.close()
    other.close()


# ---- 5. before the first step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_the_call_works_on_a_fresh_handle(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    a = ws.FluidWorker(pos, params, graph=graph)
    b = ws.FluidWorker(pos, params, graph=graph)
    forces = _moving(0, np.zeros(3), 6.0, 0.25)
    dt = F32(params.delta_time)
    ca, cb = a.apply_forces(F.to_ws(ws, forces), dt), _host_apply(b, forces, dt)
    assert np.array_equal(ca, cb) and ca.min() > 0
    rec = a.read_vec("particles")
    assert _xyz(rec, "velocity").any() and not rec["density"].any() and a.steps_done() == 0
    for t in range(3):
        a.run(1)
        b.run(1)
        assert same_bits(a.read_positions(), b.read_positions()) and same_bits(a.read_velocities(), b.read_velocities()), t
    a.close()
    b.close()


# ---- 6. slabs ---------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 10


def _slab_forces(t):
    # the cuts of 2 and 3 slabs of the 16-wide container lie at x = 0 and near +-2.7: both emitters straddle them
    return [F.emitter(F.RADIAL, (0.3 * np.cos(t), -2.5, 0.0), 3.5, 12.0, damping=1.0),
            F.emitter(F.VORTEX, (-0.5, -3.0, 0.5), 3.0, 4.0, axis=(0.0, 1.0, 0.0))]


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    dt = F32(params.delta_time)
    w = ws.FluidWorker(pos, params)
    want = []
    for t in range(SLAB_STEPS):
        counts = w.apply_forces(F.to_ws(ws, _slab_forces(t)), dt) if t % 2 == 0 else None
        w.run(1)
        if t in (2, SLAB_STEPS - 1):
            want.append((w.read_positions(), w.read_velocities()))
        if counts is not None:
            want.append(counts)
    assert min(int(c.min()) for c in want if isinstance(c, np.ndarray)) > 100
    w.close()

    def program(s, r):
        out = []
        for t in range(SLAB_STEPS):
            good = F.to_ws(ws, _slab_forces(t))
            counts = None
            if t % 2 == 0:
                counts = s.apply_forces(good, dt, counts=(r != 1))  # rank 1 passes out_affected = NULL and still applies
            elif t == 3:
                # one rank passes an invalid emitter: every rank refuses, nothing changes
                bad = F.to_ws(ws, _slab_forces(t))
                if r == 0:
                    bad[1].radius = -1.0
                arr = (ws.fluid.WsForce * 2)(*bad)
                assert s._L.ws_apply_forces(s._h, C.byref(arr), 2, dt, None) == 1, (r, t)
            elif t == 5:
                # one rank passes a different, valid emitter: every rank refuses, nothing changes
                other = F.to_ws(ws, _slab_forces(t))
                if r == world - 1:
                    other[0].strength = 13.0
                arr = (ws.fluid.WsForce * 2)(*other)
                n = np.full(2, 7, np.uint32)
                assert s._L.ws_apply_forces(s._h, C.byref(arr), 2, dt, n.ctypes.data) == 1, (r, t)
                assert np.all(n == 7)
            s.run(1)
            if t in (2, SLAB_STEPS - 1):
                out.append((s.read_positions(), s.read_velocities()))
            if t % 2 == 0:
                out.append(counts)
        return out

    got = _slab_run(ws, params, pos, world, 0, program)
    for r in range(world):
        assert len(got[r]) == len(want)
        for a, b in zip(got[r], want):
            if isinstance(b, tuple):
                assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), r
            elif r == 1:
                assert a is None
            else:
                assert np.array_equal(a, b), (r, a, b)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    steps = 0

    def call(edit=None, k=1, dt=0.01, null=False, at=0):
        f = [ws.fluid.force("vortex", (0.0, 0.0, 0.0), 2.0, 3.0, axis=(0.0, 1.0, 0.0), damping=0.5) for _ in range(max(k, 2))]
        if edit:
            edit(f[at])
        arr = (ws.fluid.WsForce * len(f))(*f)
        n = np.full(17, 7, np.uint32)
        st = L.ws_apply_forces(h, None if null else C.byref(arr), k, dt, n.ctypes.data)
        assert st != 0 and np.all(n == 7) or st == 0
        return st

    def set_(name, value, index=None):
        def edit(f):
            if index is None:
                setattr(f, name, value)
            else:
                getattr(f, name)[index] = value
        return edit

    cases = [("NULL f", dict(null=True)), ("k 0", dict(k=0)), ("k 17", dict(k=17)), ("kind 3", dict(edit=set_("kind", 3))),
             ("reserved 0", dict(edit=set_("reserved", 1, 0))), ("reserved 1", dict(edit=set_("reserved", 9, 1))),
             ("damping < 0", dict(edit=set_("damping", -0.5))), ("radius 0", dict(edit=set_("radius", 0.0))),
             ("radius < 0", dict(edit=set_("radius", -1.0))), ("second emitter", dict(edit=set_("radius", 0.0), k=2, at=1))]
    for val in (np.nan, np.inf, -np.inf, 0.0, -0.01, 2e15):
        cases.append(("dt %r" % val, dict(dt=val)))
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        cases += [("centre %r" % val, dict(edit=set_("centre", val, 1))), ("axis %r" % val, dict(edit=set_("axis", val, 2))),
                  ("strength %r" % val, dict(edit=set_("strength", val))), ("radius %r" % val, dict(edit=set_("radius", val)))]
        if not val < 0:
            cases.append(("damping %r" % val, dict(edit=set_("damping", val))))
    for what, kw in cases:
        assert call(**kw) == 1, what
        w.run(2)  # ... followed by two good steps
        steps += 2
    fresh.run(steps)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # allowed: the largest magnitudes, no brake, a zero axis, sixteen emitters
    assert call(edit=set_("centre", 1e15, 0)) == 0 and call(edit=set_("axis", 0.0, 1)) == 0 and call(k=16) == 0
    assert call(edit=set_("damping", 0.0)) == 0
    w.run(2)
    w.close()
    fresh.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    with pytest.raises(ws.WsError) as e:
        w.apply_forces(ws.fluid.force("jet", (0, 0, 0), 1.0, 1.0, axis=(0, 1, 0)), 0.01)
    assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_the_call(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    f = ws.fluid.force("jet", (0, 0, 0), 4.0, 1.0, axis=(0, 1, 0))
    assert w.apply_forces(f, 0.01)[0] > 0
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    with pytest.raises(ws.WsError) as e:
        w.apply_forces(f, 0.01)
    assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
