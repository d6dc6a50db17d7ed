"""The HIP step at every parameter set of tests/param_sets.py: each scalar fluid property of ws_params off its default.

(a) one teacher-forced step per set against the float64 restatement (per-particle bound; pressures, K6 and the sort view
    bit for bit) and against the oracle (reorder-noise tolerance);
(b) listed kernels == simple kernels bit for bit at four of the sets;
(c) delivery: a handle that is handed the set by ws_set_params in mid-run equals a handle created with it -- direct
    launches, a captured step (dropped and captured again), two loopback slabs;
(d) the record view (ws_read_particles) after a parameter change reports the LAST STEP's six float fields, pressure
    included, on single and slab handles, and the read leaves no trace in the next step."""
import os

import numpy as np
import pytest

import param_sets as PS
from test_gpu_f64_step import BOTH_ARITHMETICS, _arith, gpu_step_check
from util import FLOAT_FIELDS, assert_particles_close, reorder_noise_tolerances

pytestmark = pytest.mark.gpu

EVERY_SET = pytest.mark.parametrize("name", PS.NAMES)


def _loaded(ws, oracle, params, **kw):
    """A handle at `params` holding the scene."""
    w = ws.FluidWorker(PS.start_positions(ws), params, **kw)
    w.write_slice("particles", PS.scene(oracle, ws))
    return w


def _differing(a, b, fields=None):
    """The fields of two record arrays that are not equal bit for bit."""
    return [f for f in (fields or a.dtype.names) if not np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32))]


# ---- (a) ------------------------------------------------------------------------------------------------------------
@BOTH_ARITHMETICS
@EVERY_SET
def test_one_step_per_set_every_particle(oracle, ws, name, ieee):
    params = PS.params(ws, name)
    out = gpu_step_check(ws, PS.start_positions(ws), params, ieee, "param set %s" % name, state=PS.scene(oracle, ws))
    want = PS.oracle_step(oracle, ws, name)[0]
    tol = reorder_noise_tolerances(want, PS.oracle_step_reversed(oracle, ws, name))
    assert_particles_close(out["got"], want, tol, "param set %s (oracle)" % name, _arith(ieee))


# ---- (b) ------------------------------------------------------------------------------------------------------------
@BOTH_ARITHMETICS
@pytest.mark.parametrize("name", ["all", "dt-1/30", "damping-0", "pressure-500-near-18"])
def test_listed_kernels_equal_simple_kernels_bitwise_at_the_set(oracle, ws, devlib, name, ieee):
    """As tests/test_gpu_parity.py does at the default parameters: the one-thread-per-particle kernels of the developer
    build against the product library's listed kernels, four free-running steps from the scene, every field."""
    params = PS.params(ws, name)
    os.environ["WS_VARIANT"] = "simple"
    try:
        simple = _loaded(ws, oracle, params, ieee_division=ieee, library=devlib)
    finally:
        os.environ.pop("WS_VARIANT", None)
    listed = _loaded(ws, oracle, params, ieee_division=ieee)
    for w in (simple, listed):
        w.run(4)
    a, b = simple.read_vec("particles"), listed.read_vec("particles")
    simple.close()
    listed.close()
    assert not _differing(a, b)


# ---- (c) ------------------------------------------------------------------------------------------------------------
@BOTH_ARITHMETICS
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@EVERY_SET
def test_set_params_delivers_the_set(oracle, ws, name, graph, ieee):
    """Three steps at the default parameters, ws_set_params(set), two more: every field equals a handle CREATED with the
    set (launching directly) that is written the first handle's state as read back just before the change and makes the
    same two steps.  graph: the first handle replays a captured step (steps 2 and 3); the change must drop it -- step 4
    is launched directly (the read refreshed the predicted positions), step 5 is captured anew and replayed."""
    params = PS.params(ws, name)
    first = _loaded(ws, oracle, PS.params(ws, "default"), ieee_division=ieee, graph=graph)
    first.run(3)
    state = first.read_vec("particles")
    first.set_params(params)
    first.run(2)
    got, stats = first.read_vec("particles"), first.stats()
    first.close()
    second = ws.FluidWorker(PS.start_positions(ws), params, ieee_division=ieee)
    second.write_slice("particles", state)
    second.run(2)
    want = second.read_vec("particles")
    second.close()
    assert stats["graph_steps"] == (3 if graph else 0), stats
    assert not _differing(got, want), name


@BOTH_ARITHMETICS
@pytest.mark.parametrize("name", ["all", "dt-1/30"])
def test_set_params_delivers_the_set_to_two_slabs(oracle, ws, name, ieee):
    params, default = PS.params(ws, name), PS.params(ws, "default")
    w = _loaded(ws, oracle, default, ieee_division=ieee)
    w.run(3)
    w.set_params(params)
    w.run(2)
    want = w.read_vec("particles")
    w.close()
    got, owned = ws.slab.run_loopback(PS.start_positions(ws), default, 2, 5, ieee_division=ieee, change_params=(3, params),
                                      state=PS.scene(oracle, ws))
    assert sum(owned) == PS.N and min(owned) > 0
    assert not _differing(got, want), name


# ---- (d) ------------------------------------------------------------------------------------------------------------
GRAVITY = (3.0, -7.0, 1.5)
# name -> the ws_set_params calls made between the fifth step and the read, as overrides on the scene's parameters
CHANGES = {
    "target-55": [dict(target_density=55.0)],
    "near-0": [dict(near_pressure_scalar=0.0)],
    "pressure-500-near-18": [dict(pressure_scalar=500.0, near_pressure_scalar=18.0)],
    "viscosity-2": [dict(viscosity_strength=2.0)],
    "gravity-then-viscosity": [dict(gravity=GRAVITY), dict(gravity=GRAVITY, viscosity_strength=2.0)],
    "pressure-500-and-back": [dict(pressure_scalar=500.0), {}],
    "radius-0.35-then-target-0": [dict(smoothing_radius=0.35), dict(smoothing_radius=0.35, target_density=0.0)],
}
_unchanged = {}


def _five_steps(ws, oracle, ieee):
    """The record view of a handle that made five steps from the scene and no change (once per arithmetic)."""
    if ieee not in _unchanged:
        w = _loaded(ws, oracle, PS.params(ws, "default"), ieee_division=ieee)
        w.run(5)
        _unchanged[ieee] = w.read_vec("particles")
        w.close()
        assert np.abs(_unchanged[ieee]["acceleration"][:, :3]).max() > 0
    return _unchanged[ieee]


@BOTH_ARITHMETICS
@pytest.mark.parametrize("change", list(CHANGES))
def test_record_view_reports_the_last_step_after_a_parameter_change(oracle, ws, change, ieee):
    """include/wsfluid.h, ws_read_particles: "density/pressure/acceleration are the values the last step computed".
    Five steps, one or two ws_set_params, two reads: all six float fields carry the bits a handle without the change
    reports -- the pressure is the last step's function of the last step's density, not the new parameters'.  Then one
    more step equals a handle given the same calls without the reads."""
    calls = [ws.make_params(container_size=PS.CONTAINER, **over) for over in CHANGES[change]]
    want = _five_steps(ws, oracle, ieee)

    def changed():
        w = _loaded(ws, oracle, PS.params(ws, "default"), ieee_division=ieee)
        w.run(5)
        for p in calls:
            w.set_params(p)
        return w

    w = changed()
    out = w.read_vec("particles")
    again = w.read_vec("particles")
    w.run(1)
    after_read = w.read_vec("particles")
    w.close()
    w = changed()
    w.run(1)
    unread = w.read_vec("particles")
    w.close()
    assert not _differing(out, again), "two reads differ"
    assert not _differing(out, want, FLOAT_FIELDS), "the record view after %s differs from the last step's" % change
    assert not _differing(after_read, unread), "the read changed the next step"


@BOTH_ARITHMETICS
@pytest.mark.parametrize("change", ["target-55", "near-0", "pressure-500-near-18"])
def test_slab_record_views_report_the_last_step_after_a_parameter_change(oracle, ws, change, ieee):
    """The same on two loopback slabs, through both slab views: the id-ordered collective ws_read_particles (k_slab_pack)
    and the owned records of ws_slab_read_particles (k_gather_slab).  (A re-grid RELOADS a slab handle, so the radius
    change is a single-handle case.)"""
    params = ws.make_params(container_size=PS.CONTAINER, **CHANGES[change][0])
    want = _five_steps(ws, oracle, ieee)
    w = _loaded(ws, oracle, PS.params(ws, "default"), ieee_division=ieee)
    w.run(5)
    w.set_params(params)
    w.run(1)
    want_next = w.read_vec("particles")
    w.close()
    scene = PS.scene(oracle, ws)

    def program(s, rank):
        s.write_particles(scene)
        s.run(5)
        s.set_params(params)
        by_id = s.read_vec("particles")
        again = s.read_vec("particles")
        rec, ids = s.read()
        s.run(1)
        return by_id, again, rec, ids, s.read_vec("particles")

    seen = np.zeros(PS.N, np.int32)
    wrong = []  # (rank, view, fields): every view of every rank is looked at before the test fails
    results = ws.slab.run_loopback_program(PS.start_positions(ws), PS.params(ws, "default"), 2, program, ieee_division=ieee)
    for rank, (by_id, again, rec, ids, nxt) in enumerate(results):
        assert len(ids) > 0
        np.add.at(seen, ids, 1)
        for view, fields in (("two reads differ", _differing(by_id, again)),
                             ("ws_read_particles", _differing(by_id, want, FLOAT_FIELDS)),
                             ("ws_slab_read_particles", _differing(rec, want[ids], FLOAT_FIELDS)),
                             ("the reads changed the next step", _differing(nxt, want_next))):
            if fields:
                wrong.append((rank, view, fields))
    assert np.all(seen == 1)
    assert not wrong, "slab record views after %s" % change
