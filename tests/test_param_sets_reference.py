"""CPU tier of tests/param_sets.py: the oracle at every parameter set against the float64 restatement (so the bound of
tests/test_gpu_param_sets.py is calibrated with no GPU), proof that the scene's one step reaches every face of the
container (counted from the oracle's result, never from the library), and proof that no set is a no-op."""
import numpy as np
import pytest

import f64_step as F
import param_sets as PS
from test_f64_step_reference import HEADROOM, _check_oracle
from util import oracle_from_params


@pytest.mark.parametrize("name", PS.NAMES)
def test_oracle_within_the_per_particle_bound_at_every_set(oracle, ws, name):
    """One oracle step of the scene at each set through f64_step.check_step: K4 / K5 within HEADROOM of the per-particle
    bound, pressures and K6 bit for bit, the sort view equal to the recomputation -- the references themselves hold at
    dt <= 0, damping 0 and above 1, target 0, negative and zero pressure multipliers."""
    params = PS.params(ws, name)
    orc = oracle_from_params(oracle, PS.start_positions(ws), params)
    worst = _check_oracle(oracle, ws, orc, PS.scene(oracle, ws), params, "param set %s" % name, oracle.SORT_FAST)
    print("%s: density %.3f acceleration %.3f of the bound" % (name, worst["density"], worst["acceleration"]))
    assert HEADROOM == 0.5
    # the step the other tests (and the GPU tier) share is this one
    want = PS.oracle_step(oracle, ws, name)[0]
    for f in want.dtype.names:
        assert np.array_equal(orc.particles[f].view(np.uint32), want[f].view(np.uint32)), f


def test_the_scene_is_what_the_tests_assume(oracle, ws):
    state = PS.scene(oracle, ws)
    params = PS.params(ws, "default")
    assert len(state) == PS.N and float(params.smoothing_radius) == 0.25
    assert np.array_equal(state["predicted_position"][:, :3], state["position"][:, :3] + state["velocity"][:, :3] * np.float32(0.02))
    ref = F.StepReference(state, params, ws.get_smoothing_kernel(params), PS.oracle_step(oracle, ws, "default")[0])
    print("pairs per particle: median %d, max %d" % (np.median(ref.pairs), ref.pairs.max()))
    assert np.median(ref.pairs) >= 32 and ref.pairs.max() < 2048  # a settled fluid, no particle near K4's mask limit


@pytest.mark.parametrize("name", PS.WALL_HIT_SETS)
def test_one_step_hits_every_face(oracle, ws, name):
    """At least 3 particles arrive on each of the six faces in the one step the GPU tests make: the K6 reflection
    (velocity * -collision_damping, position = the face) runs on both ends of every axis.  Sets with dt = 0 or 1/240
    (PS.NO_WALL_HITS_EXPECTED) are exempt: they move nothing, or a quarter of the way."""
    assert name not in PS.NO_WALL_HITS_EXPECTED
    want = PS.oracle_step(oracle, ws, name)[0]
    hits = PS.wall_hits(PS.scene(oracle, ws), want, PS.params(ws, name))
    print("%s: hits per face %s" % (name, hits))
    assert min(hits) >= 3, (name, hits)


def test_the_damping_sets_reflect_differently(oracle, ws):
    """The particles that hit a wall leave it with velocity * -damping on that axis: 0, sign kept at damping 0 (-0.0 is
    still zero), the mirror image at 1, faster than they came at 1.5."""
    state = PS.scene(oracle, ws)
    base = PS.oracle_step(oracle, ws, "default")[0]
    p = PS.params(ws, "default")
    mn, mx = np.float32(list(p.ext_min)[:3]), np.float32(list(p.ext_max)[:3])
    # before the walls: the damping enters nowhere else, so the accelerations are the default's
    dt = np.float32(p.delta_time)
    v_in = (state["velocity"] + (np.float32(list(p.gravity)) + base["acceleration"]) * dt)[:, :3]
    p_in = state["position"][:, :3] + v_in * dt
    hit = (p_in < mn) | (p_in > mx)  # (the resting floor layer is pushed into the floor by gravity every step, too)
    assert hit.sum() >= 18
    for name, damping in (("default", 0.95), ("damping-0", 0.0), ("damping-1", 1.0), ("damping-1.5", 1.5)):
        got = PS.oracle_step(oracle, ws, name)[0]
        assert np.array_equal(got["position"], base["position"])  # the wall's position whatever the damping
        assert np.array_equal(got["acceleration"].view(np.uint32), base["acceleration"].view(np.uint32))
        v_out = np.where(hit, v_in * (np.float32(-1.0) * np.float32(damping)), v_in)
        assert np.array_equal(got["velocity"][:, :3].view(np.uint32), v_out.view(np.uint32)), name


@pytest.mark.parametrize("name", [n for n in PS.NAMES if n != "default"])
def test_each_set_changes_what_it_is_meant_to_change(oracle, ws, name):
    """No set is a no-op that lends false coverage: the oracle's output differs from `default`'s in the fields the set
    is expected to move first (PS.MOVES)."""
    base = PS.oracle_step(oracle, ws, "default")[0]
    got = PS.oracle_step(oracle, ws, name)[0]
    for f in PS.MOVES[name]:
        differ = int(np.sum(np.any((got[f] != base[f]).reshape(len(got), -1), axis=1)))
        print("%s: %s differs for %d particles" % (name, f, differ))
        # the damping touches the particles that hit a wall alone; everything else moves (almost) every particle
        assert differ >= (18 if name.startswith("damping-") else PS.N // 2), (name, f, differ)


def test_the_sets_cover_every_scalar_property():
    moved = set()
    for over in PS.SETS.values():
        moved |= set(over)
    assert {"delta_time", "collision_damping", "target_density", "pressure_scalar", "near_pressure_scalar",
            "viscosity_strength"} <= moved
    assert len(PS.SETS) >= 17 and set(PS.MOVES) == set(PS.NAMES) - {"default"}
