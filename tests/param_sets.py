"""One scene and a list of parameter sets that move every scalar fluid property of ws_params off its default.

The reference's update() re-uploads fluid_props every frame (src/fluid_compute.rs:479-481), so a host may change any of
delta_time, collision_damping, target_density, pressure_scalar, near_pressure_scalar and viscosity_strength at any
time; the references of the suite (util.oracle_from_params, f64_step.check_step, f64_step.integrate_f32) take arbitrary
values of all of them.  This module supplies the inputs: tests/test_param_sets_reference.py runs them through the oracle
(no GPU), tests/test_gpu_param_sets.py through the HIP step.

Pure Python and numpy: nothing here imports the library or the oracle; callers hand in `ws` (the package, for
make_params and uniform_cloud) and `O` (the oracle module).

The scene.  8192 particles of uniform_cloud(8192, seed 5) in a 3 x 2 x 2 container at h = 0.25, advanced 30 oracle
steps at the default parameters (the cloud has collapsed onto the floor: median 47 pairs per particle, at most 70); then
N(0, 6) is added to the velocity components of 2048 particles drawn by a seeded generator, and the predicted positions
are recomputed as position + velocity * f32(0.02).  The kicks send particles into all six faces within one step at
dt = 1/60, so K6's reflection (collision_damping) is exercised on every face by ONE teacher-forced step."""
import numpy as np

from util import oracle_from_params, oracle_one_step

N = 8192
CONTAINER = (3.0, 2.0, 2.0)
WARM_STEPS = 30
KICKED = 2048
KICK_SIGMA = 6.0

# name -> overrides on make_params(container_size=CONTAINER).  May be extended, not shortened.
SETS = {
    "default": {},
    "dt-1/30": dict(delta_time=1.0 / 30.0),
    "dt-1/240": dict(delta_time=1.0 / 240.0),
    "dt-0": dict(delta_time=0.0),
    "dt-neg-1/60": dict(delta_time=-1.0 / 60.0),
    "damping-0": dict(collision_damping=0.0),
    "damping-1": dict(collision_damping=1.0),
    "damping-1.5": dict(collision_damping=1.5),
    "target-0": dict(target_density=0.0),
    "target-55": dict(target_density=55.0),
    "pressure-0-near-0": dict(pressure_scalar=0.0, near_pressure_scalar=0.0),
    "pressure-neg-22": dict(pressure_scalar=-22.0),
    "pressure-500-near-18": dict(pressure_scalar=500.0, near_pressure_scalar=18.0),
    "near-0": dict(near_pressure_scalar=0.0),
    "viscosity-0": dict(viscosity_strength=0.0),
    "viscosity-2": dict(viscosity_strength=2.0),
    "all": dict(delta_time=1.0 / 90.0, collision_damping=0.5, target_density=6.5, pressure_scalar=35.5,
                near_pressure_scalar=3.25, viscosity_strength=0.45, gravity=(3.0, -7.0, 1.5)),
}
NAMES = tuple(SETS)
# the fields a set is expected to move first (tests/test_param_sets_reference.py asserts every one of them): the time
# step moves velocity and position; the damping only the velocity of the particles that hit a wall (their position is
# the wall's whatever the damping); the density -> pressure parameters the pressures and through them the acceleration
MOVES = {name: (("velocity", "position") if name.startswith("dt-") else
                ("velocity",) if name.startswith("damping-") else
                ("pressure", "acceleration") if name.startswith(("target-", "pressure-", "near-")) else
                ("acceleration",) if name.startswith("viscosity-") else
                ("velocity", "position", "pressure", "acceleration"))
         for name in NAMES if name != "default"}
# one step at these moves no particle (dt = 0) or too few of them (1/240: a quarter of the default's reach) into a wall
NO_WALL_HITS_EXPECTED = ("dt-0", "dt-1/240")
WALL_HIT_SETS = ("default", "damping-0", "damping-1", "damping-1.5", "all")

_cache = {}


def params(ws, name):
    """The ws_params of one set."""
    return ws.make_params(container_size=CONTAINER, **SETS[name])


def start_positions(ws):
    p = params(ws, "default")
    return ws.workloads.uniform_cloud(N, 5, list(p.ext_min), list(p.ext_max))


def scene(O, ws):
    """The state every test starts from (80-byte records, id order).  Built once per process; callers must not modify it."""
    if "scene" not in _cache:
        p = params(ws, "default")
        orc = oracle_from_params(O, start_positions(ws), p)
        state = orc.particles.copy()
        for _ in range(WARM_STEPS):
            state = oracle_one_step(O, orc, state, mode=O.SORT_FAST)
        rng = np.random.default_rng(20261020)
        kicked = rng.choice(N, KICKED, replace=False)
        state["velocity"][kicked, :3] += rng.normal(0.0, KICK_SIGMA, (KICKED, 3)).astype(np.float32)
        state["predicted_position"][:, :3] = state["position"][:, :3] + state["velocity"][:, :3] * np.float32(0.02)
        state.setflags(write=False)
        _cache["scene"] = state
    return _cache["scene"]


def _oracle(O, ws, name):
    return oracle_from_params(O, start_positions(ws), params(ws, name))


def oracle_step(O, ws, name):
    """One oracle step of the scene at the set `name`: (want, (keys, perm, cell offsets)).  Once per set and process."""
    key = ("oracle", name)
    if key not in _cache:
        orc = _oracle(O, ws, name)
        want = oracle_one_step(O, orc, scene(O, ws), mode=O.SORT_FAST)
        sort = (orc.particle_cell_indicies.copy(), orc.particle_indicies.copy(), orc.cell_offsets.copy())
        for a in (want,) + sort:
            a.setflags(write=False)
        _cache[key] = (want, sort)
    return _cache[key]


def oracle_step_reversed(O, ws, name):
    """The same step with every particle's neighbours visited in reversed order (util.reorder_noise_tolerances' unit)."""
    key = ("reversed", name)
    if key not in _cache:
        rev = oracle_one_step(O, _oracle(O, ws, name), scene(O, ws), reverse=True, mode=O.SORT_FAST)
        rev.setflags(write=False)
        _cache[key] = rev
    return _cache[key]


def wall_hits(state, after, p):
    """Per face (x-, x+, y-, y+, z-, z+): the particles whose new position sits on the face and whose old one did not."""
    mn = np.array([p.ext_min[k] for k in range(3)], np.float32)
    mx = np.array([p.ext_max[k] for k in range(3)], np.float32)
    hits = []
    for k in range(3):
        for bound in (mn[k], mx[k]):
            hits.append(int(np.sum((after["position"][:, k] == bound) & (state["position"][:, k] != bound))))
    return hits
