"""ws_read_cohesion and ws_apply_cohesion on the GPU: the stage bit for bit against the numpy restatement
(tests/cohesion_ref.py) in both arithmetics of the handle and at every launch shape, the apply equal to the read, the step
picking the new velocities up exactly as it picks up a host edit through ws_write_particles (a captured step included),
strengths of 0 changing no bit, a fresh handle, slabs, merged cell grids, refusals, an untouched simulation.

Scene A is tests/test_gpu_whitewater.py's: the dam break at step 40 plus an isolated particle and a coincident pair, 4 099
particles.  Scene B (slabs only) is the 65 536-particle cloud at step 30 of the whitewater and velocity slab tests."""
import ctypes as C

import numpy as np
import pytest

import aniso_ref as A
import cohesion_ref as Co
from forces_ref import LOOKAHEAD
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_field_grids import STEPS as GRID_STEPS
from test_gpu_field_grids import cell_budget
from test_gpu_field_grids import scene as grid_scene
from test_gpu_whitewater import N_BLOCK, SHAPES, _SceneA, load_state

pytestmark = pytest.mark.gpu
F32 = np.float32
ARITH = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
GRAPH = pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
DT = F32(1.0 / 60.0)
# the defaults, each strength alone, an explicit rest density
PARAM_SETS = {"defaults": Co.defaults(),
              "cohesion": dict(cohesion=2.5, curvature=0.0, xsph=0.0, rest_density=0.0),
              "curvature": dict(cohesion=0.0, curvature=0.75, xsph=0.0, rest_density=0.0),
              "xsph": dict(cohesion=0.0, curvature=0.0, xsph=0.5, rest_density=0.0),
              "rest-density": dict(Co.defaults(), rest_density=6.5)}
ZERO = dict(cohesion=0.0, curvature=0.0, xsph=0.0, rest_density=0.0)


def cparams(ws, d):
    return ws.fluid.cohesion_params(**d)


def same_stage(got, want, case=""):
    for k in Co.OUTPUTS:
        assert same_bits(got[k], want[k]), (case, k)


def _xyz(rec, field):
    return np.ascontiguousarray(rec[field][:, :3])


@pytest.fixture(scope="module")
def scene(ws):
    s = _SceneA(ws)
    # pass A is the same for every parameter set: computed once, shared, never modified
    s.fed = Co.normals(s.params, s.pos)
    for a in s.fed:
        a.setflags(write=False)
    yield s
    s.close()


# ---- 1. the stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(PARAM_SETS))
def test_the_stage_has_the_restatements_bits_in_both_arithmetics(ws, scene, which):
    cp = PARAM_SETS[which]
    want = Co.stage(scene.params, scene.pos, scene.vel, cp, DT, fed=scene.fed)
    got = {ieee: scene.get(ieee).read_cohesion(cparams(ws, cp), DT) for ieee in (False, True)}
    for ieee in (False, True):
        same_stage(got[ieee], want, (which, ieee))
    same_stage(got[False], got[True], which)  # the stage is IEEE under either flag
    # what the scene must contain (from the restatement)
    nb = want["neighbours"]
    assert np.all(nb[N_BLOCK:] == 0) and np.count_nonzero(nb == 0) >= 3 and nb.max() > 30
    assert same_bits(want["dv"][N_BLOCK:], np.zeros((3, 3), F32)) and not want["normal"][N_BLOCK:].any()
    assert np.all(want["density"] > 0) and want["density"][-1] == 2 * want["density"][N_BLOCK]  # the coincident pair
    assert np.all(np.any(want["dv"][nb > 0] != 0, 1))
    if which == "defaults":
        # both branches of the spline occur, and any subset of the outputs may be asked for alone
        h = float(scene.params.smoothing_radius)
        d = np.linalg.norm(scene.pos[:64, None, :].astype(np.float64) - scene.pos[None, :, :], axis=2)
        assert np.any((d > 0) & (d < 0.5 * h)) and np.any((d > 0.5 * h) & (d < h))
        w = scene.get(False)
        only = np.empty((scene.n, 3), F32)
        assert w._L.ws_read_cohesion(w._h, C.byref(cparams(ws, cp)), DT, None, None, only.ctypes.data, None) == 0
        assert same_bits(only, want["dv"])
        cnt = np.empty(scene.n, np.uint32)
        assert w._L.ws_read_cohesion(w._h, C.byref(cparams(ws, cp)), DT, None, None, None, cnt.ctypes.data) == 0
        assert np.array_equal(cnt, nb)
    if which == "rest-density":
        assert not same_bits(want["dv"], Co.stage(scene.params, scene.pos, scene.vel, Co.defaults(), DT, fed=scene.fed)["dv"])


# ---- 2. launch shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_every_particle_count_gives_the_restatements_bits(ws, scene, n):
    """The first n particles of the scene as a handle of their own: n = 1 has no neighbour at all, 63 / 64 / 65 straddle a
    wave, 4 097 is one lane into a new workgroup.  The stage, and the velocities after the apply."""
    pos, vel = scene.pos[:n], scene.vel[:n]
    cp = PARAM_SETS["defaults"]
    want = Co.stage(scene.params, pos, vel, cp, DT)
    w = ws.FluidWorker(pos, scene.params)
    load_state(w, pos, vel)
    same_stage(w.read_cohesion(cparams(ws, cp), DT), want, n)
    affected = w.apply_cohesion(cparams(ws, cp), DT)
    assert affected == np.count_nonzero(want["neighbours"]) and (affected > 0) == (n > 1)
    assert same_bits(w.read_velocities(), Co.apply(vel, want)) and same_bits(w.read_positions(), pos)
    w.close()


# ---- 3. apply equals read -----------------------------------------------------------------------------------------------------
@ARITH
def test_apply_adds_what_read_returns_and_leaves_the_rest(ws, scene, ieee):
    vel = scene.vel.copy()
    vel[N_BLOCK:] = F32(-0.0)  # the three particles without a neighbour: a -0 must stay
    w = ws.FluidWorker(scene.pos, scene.params, ieee_division=ieee)
    load_state(w, scene.pos, vel)
    cp = cparams(ws, Co.defaults())
    st = w.read_cohesion(cp, DT)
    has = st["neighbours"] > 0
    assert same_bits(st["dv"][~has], np.zeros(((~has).sum(), 3), F32)) and (~has).sum() >= 3
    affected = w.apply_cohesion(cp, DT)
    got = w.read_vec("particles")
    want_v = np.where(has[:, None], (vel + st["dv"]).astype(F32), vel)
    assert affected == has.sum()
    assert same_bits(w.read_velocities(), want_v) and same_bits(_xyz(got, "velocity"), want_v)
    assert np.all(np.signbit(w.read_velocities()[N_BLOCK:]))
    assert same_bits(w.read_positions(), scene.pos) and same_bits(_xyz(got, "position"), scene.pos)
    assert same_bits(_xyz(got, "predicted_position"), (scene.pos + (want_v * LOOKAHEAD).astype(F32)).astype(F32))
    # without the count: the same state
    load_state(w, scene.pos, vel)
    assert w.apply_cohesion(cp, DT, count=False) is None
    assert same_bits(w.read_velocities(), want_v)
    w.close()


def test_the_views_of_the_last_step_stay(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(12)
    before = w.read_vec("particles")
    cp = cparams(ws, Co.defaults())
    st = w.read_cohesion(cp, DT)
    assert w.apply_cohesion(cp, DT) == np.count_nonzero(st["neighbours"]) > 1000
    after = w.read_vec("particles")
    assert before["density"].any() and before["acceleration"].any()
    for field in ("position", "density", "pressure", "acceleration"):
        assert same_bits(after[field], before[field]), field
    want_v = np.where((st["neighbours"] > 0)[:, None], (_xyz(before, "velocity") + st["dv"]).astype(F32), _xyz(before, "velocity"))
    assert same_bits(_xyz(after, "velocity"), want_v) and not same_bits(want_v, _xyz(before, "velocity"))
    assert w.steps_done() == 12
    # between the two halves of an asynchronous readback too
    buf = np.empty((w.n, 3), F32)
    w.read_positions_begin(buf)
    w.apply_cohesion(cp, DT, count=False)
    w.read_positions_end()
    assert same_bits(buf, _xyz(before, "position"))
    w.close()


# ---- 4. the step picks it up exactly as a host edit --------------------------------------------------------------------------------
def _host_apply(w, params, cp, dt):
    """ws_read_particles, the restatement on the host, ws_write_particles: what a host without the call has to do."""
    rec = w.read_vec("particles")
    pos, vel = _xyz(rec, "position"), _xyz(rec, "velocity")
    st = Co.stage(params, pos, vel, cp, dt)
    new = Co.apply(vel, st)
    rec["velocity"][:, :3] = new
    rec["predicted_position"][:, :3] = (pos + (new * LOOKAHEAD).astype(F32)).astype(F32)
    w.write_slice("particles", rec)
    return int(np.count_nonzero(st["neighbours"]))


@ARITH
@GRAPH
def test_the_step_picks_the_call_up_exactly_as_a_host_edit(ws, ieee, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    a = ws.FluidWorker(pos, params, ieee_division=ieee, graph=graph)
    b = ws.FluidWorker(pos, params, ieee_division=ieee, graph=graph)
    cp = dict(cohesion=0.5, curvature=0.5, xsph=0.25, rest_density=0.0)
    dt = F32(params.delta_time)
    for x in (a, b):
        x.run(6)
    replays = a.stats()["graph_steps"]
    for t in range(3):
        ca = a.apply_cohesion(cparams(ws, cp), dt)
        cb = _host_apply(b, params, cp, dt)
        assert ca == cb > 1000, (t, ca, cb)
        for k in range(3):
            a.run(1)
            b.run(1)
            assert same_bits(a.read_positions(), b.read_positions()), (t, k)
            assert same_bits(a.read_velocities(), b.read_velocities()), (t, k)
    assert a.steps_done() == 15
    if graph:  # the captured step was neither dropped nor bypassed by the call
        assert a.stats()["graph_steps"] - replays == 9
    a.close()
    b.close()


# ---- 5. all strengths 0; a fresh handle ----------------------------------------------------------------------------------------
def test_strengths_of_zero_change_no_velocity_bit(ws, scene):
    vel = scene.vel.copy()
    vel[N_BLOCK:] = F32(-0.0)
    w = ws.FluidWorker(scene.pos, scene.params)
    load_state(w, scene.pos, vel)
    st = w.read_cohesion(cparams(ws, ZERO), DT)
    assert same_bits(st["dv"], np.zeros((scene.n, 3), F32))  # +0 everywhere
    before = w.read_vec("particles")
    assert w.apply_cohesion(cparams(ws, ZERO), DT) == np.count_nonzero(st["neighbours"]) > scene.n // 2  # (all of them "affected")
    after = w.read_vec("particles")
    for field in ("velocity", "position", "density", "pressure", "acceleration"):
        assert same_bits(after[field], before[field]), field
    # (the predicted position is the library's own rule on the unchanged velocity, not what the host had loaded)
    assert same_bits(_xyz(after, "predicted_position"), (scene.pos + (vel * LOOKAHEAD).astype(F32)).astype(F32))
    assert same_bits(w.read_velocities(), vel) and np.all(np.signbit(w.read_velocities()[N_BLOCK:]))
    w.close()


@GRAPH
def test_the_call_works_on_a_fresh_handle(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    a = ws.FluidWorker(pos, params, graph=graph)
    b = ws.FluidWorker(pos, params, graph=graph)
    cp = Co.defaults()
    dt = F32(params.delta_time)
    assert a.apply_cohesion(cparams(ws, cp), dt) == _host_apply(b, params, cp, dt) > 1000
    rec = a.read_vec("particles")
    assert _xyz(rec, "velocity").any() and not rec["density"].any() and a.steps_done() == 0
    for t in range(3):
        a.run(1)
        b.run(1)
        assert same_bits(a.read_positions(), b.read_positions()) and same_bits(a.read_velocities(), b.read_velocities()), t
    a.close()
    b.close()


# ---- 6. slabs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    steps = 30
    cp = dict(Co.defaults(), xsph=0.2)
    dt = F32(params.delta_time)
    w = ws.FluidWorker(pos, params)
    w.run(steps)
    want = dict(stage=w.read_cohesion(cparams(ws, cp), dt), unchanged=(w.read_positions(), w.read_velocities()))
    want["affected"] = w.apply_cohesion(cparams(ws, cp), dt)
    want["applied"] = w.read_velocities()
    w.run(2)
    want["after"] = (w.read_positions(), w.read_velocities())
    w.close()
    assert want["affected"] > 30000 and not same_bits(want["applied"], want["unchanged"][1])

    def refused(s, p, count):
        n = C.c_uint32(7)
        assert s._L.ws_apply_cohesion(s._h, C.byref(p), dt, C.byref(n) if count else None) == 1
        assert n.value == 7

    def program(s, r):
        out = dict(stage=s.read_cohesion(cparams(ws, cp), dt, want=(r != 1)))  # rank 1 only contributes
        # one rank with bad arguments to the read: it alone is refused, nobody waits
        bad = cparams(ws, dict(cp, xsph=1.5 if r == 0 else cp["xsph"]))
        out["bad read"] = s._L.ws_read_cohesion(s._h, C.byref(bad), dt, None, out["stage"]["density"].ctypes.data if r != 1 else None,
                                                None, None)
        # ranks given different parameters, then one rank given bad ones: all refuse, nothing changes
        refused(s, cparams(ws, dict(cp, cohesion=1.0 + r)), True)
        refused(s, cparams(ws, dict(cp, curvature=-1.0 if r == world - 1 else 1.0)), r != 1)
        p = cparams(ws, cp)
        assert s._L.ws_apply_cohesion(s._h, C.byref(p), F32(dt * (2 if r == 0 else 1)), None) == 1  # dt is agreed on too
        out["unchanged"] = (s.read_positions(), s.read_velocities())
        out["affected"] = s.apply_cohesion(cparams(ws, cp), dt, count=(r != 1))
        out["applied"] = s.read_velocities()
        s.run(2)
        out["after"] = (s.read_positions(), s.read_velocities())
        return out

    got = _slab_run(ws, params, pos, world, steps, program)
    for r in range(world):
        g = got[r]
        assert g["bad read"] == (1 if r == 0 else 0), r
        if r == 1:
            assert g["stage"] is None and g["affected"] is None
        else:
            same_stage(g["stage"], want["stage"], r)
            assert g["affected"] == want["affected"], r
        for k in ("unchanged", "after"):
            assert same_bits(g[k][0], want[k][0]) and same_bits(g[k][1], want[k][1]), (r, k)
        assert same_bits(g["applied"], want["applied"]), r


# ---- 7. merged cell grids --------------------------------------------------------------------------------------------------------
@ARITH
def test_merged_cells(ws, devlib, ieee):
    pos, params = grid_scene(ws, 0.25)
    with cell_budget("800"):
        w = ws.FluidWorker(pos, params, ieee_division=ieee, library=devlib)
    w.run(GRID_STEPS)
    merged = w.stats()["cells_merged"]
    assert merged[1] > 1 and merged[2] > 1
    assert tuple(int(v) for v in A.Grid(params, merged).dim) == tuple(w.grid_dims())
    cur, vel = w.read_positions(), w.read_velocities()
    ids = np.random.default_rng(4).choice(len(cur), 1500, replace=False)
    cp = Co.defaults()
    want = Co.stage(params, cur, vel, cp, DT, merged, ids)
    got = w.read_cohesion(cparams(ws, cp), DT)
    assert want["neighbours"].max() > 8 and want["dv"].any()
    for k in Co.OUTPUTS:
        assert same_bits(got[k][ids], want[k]), k
    affected = w.apply_cohesion(cparams(ws, cp), DT)
    assert affected == np.count_nonzero(got["neighbours"])
    assert same_bits(w.read_velocities()[ids], Co.apply(vel[ids], want))
    w.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    for x in (w, fresh):
        x.run(5)
    L, h = w._L, w._h
    n = len(pos)
    dv = np.full((n, 3), 7.0, F32)

    def read(dt=0.01, null=False, out=dv, **fields):
        p = cparams(ws, fields)
        return L.ws_read_cohesion(h, None if null else C.byref(p), dt, None, None, None if out is None else out.ctypes.data, None)

    def apply(dt=0.01, null=False, **fields):
        p = cparams(ws, fields)
        k = C.c_uint32(7)
        st = L.ws_apply_cohesion(h, None if null else C.byref(p), dt, C.byref(k))
        assert st == 0 or k.value == 7
        return st

    cases = [("NULL p", dict(null=True)), ("reserved", dict(reserved=1)), ("xsph < 0", dict(xsph=-0.01)), ("xsph > 1", dict(xsph=1.01))]
    for name in ("cohesion", "curvature", "rest_density"):
        cases.append(("%s < 0" % name, {name: -0.5}))
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        for name in ("cohesion", "curvature", "xsph", "rest_density"):
            cases.append(("%s %r" % (name, val), {name: val}))
    for val in (np.nan, np.inf, -np.inf, 0.0, -0.01, 2e15):
        cases.append(("dt %r" % val, dict(dt=val)))
    steps = 5
    for what, kw in cases:
        dv[:] = 7.0
        assert read(**kw) == 1 and np.all(dv == 7.0), what
        assert apply(**kw) == 1, what
        w.run(1)  # ... followed by a good step
        steps += 1
    dv[:] = 7.0
    assert read(out=None) == 1, "every output NULL"
    fresh.run(steps - 5)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # allowed: the limits themselves, strengths of 0, the largest magnitudes (read only: they are not meant to be stepped)
    assert read(xsph=0.0) == 0 and read(xsph=1.0) == 0 and read(cohesion=0.0, curvature=0.0) == 0 and not np.all(dv == 7.0)
    assert read(cohesion=1e15, rest_density=1e15) == 0 and read(dt=1e15) == 0
    assert apply(xsph=1.0) == 0 and apply(rest_density=3.0) == 0
    w.run(2)
    w.close()
    fresh.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    for call in (lambda: w.read_cohesion(cparams(ws, {}), 0.01), lambda: w.apply_cohesion(cparams(ws, {}), 0.01)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_both_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    assert w.apply_cohesion(cparams(ws, {}), 0.01) > 0
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in (lambda: w.read_cohesion(cparams(ws, {}), 0.01), lambda: w.apply_cohesion(cparams(ws, {}), 0.01)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()


# ---- 9. the simulation is untouched by the read ------------------------------------------------------------------------------------
@GRAPH
def test_reading_every_step_leaves_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    regrid = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=F32(0.2))
    out = []
    for calls in (False, True):
        w = ws.FluidWorker(pos, params, graph=graph)
        seen = 0
        for t in range(60):
            if t == 30:
                w.set_params(regrid)
            w.run(1)
            if calls:
                seen += int(np.count_nonzero(w.read_cohesion(cparams(ws, {}), DT)["dv"]))
        assert seen > 0 or not calls
        if graph:
            assert w.stats()["graph_steps"] > 0
        out.append(w.read_vec("particles"))
        w.close()
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
