"""Every particle of one teacher-forced HIP step against the float64 restatement of tests/f64_step.py, in both
arithmetics: density and near density within the per-particle bound, acceleration within it (computed from the step's
own densities and pressures), pressures and K6 bit for bit, and the sort view equal to a numpy recomputation."""
import numpy as np
import pytest

import f64_step as F
from test_f64_step_reference import clump, coincident

pytestmark = pytest.mark.gpu

BOTH_ARITHMETICS = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
SAMPLE = 1 << 19  # query particles of a sampled check (the full C3 population costs ~3.5 min of numpy)


def _arith(ieee):
    return "ieee-division" if ieee else "hw-rcp-sqrt"


def gpu_step_check(ws, pos, params, ieee, what, warm=0, state=None, queries=None, library=None):
    """Build a handle on `pos`, run `warm` free steps (or write `state`), then ONE step from the state read back
    (teacher forcing: the handle's input is exactly the state the restatement starts from); check it particle by
    particle.  queries: a callable (state) -> particle ids for a sampled check, or None for every particle."""
    w = ws.FluidWorker(pos, params, ieee_division=ieee, library=library)
    try:
        if warm:
            w.run(warm)
        if state is None:
            state = w.read_vec("particles")
        w.write_slice("particles", state)
        w.run()
        got = w.read_vec("particles")
        sort = w.sort_view()
        stats = w.stats()
    finally:
        w.close()
    q = queries(state) if callable(queries) else queries
    worst = F.check_step(state, got, params, ws.get_smoothing_kernel(params), what, _arith(ieee), queries=q, check_sort=sort)
    worst["stats"] = stats
    worst["got"] = got
    return worst


def settled_sample(state, params, size=SAMPLE, seed=7):
    """Query particles of a sampled check: every particle of the 64 densest cells, every particle over K4's mask limit
    (more than 2048 candidates), every particle touching a wall (its position on a bound of the container), and a
    uniform random fill up to `size`."""
    n = len(state)
    cl = F.CellList(state["predicted_position"][:, :3], params.smoothing_radius)
    _, inv, cnt = np.unique(cl.key, return_inverse=True, return_counts=True)
    dense = np.flatnonzero(np.isin(inv, np.argsort(-cnt)[:64]))
    over = np.flatnonzero(cl.candidates(np.arange(n)) > 2048)
    p = state["position"][:, :3]
    wall = np.flatnonzero(np.any((p <= np.float32(list(params.ext_min)[:3])) | (p >= np.float32(list(params.ext_max)[:3])), axis=1))
    must = np.unique(np.concatenate([dense, over, wall]))
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(rng.choice(n, min(n, size + len(must)), replace=False), must)[:max(0, size - len(must))]
    return np.sort(np.concatenate([must, rest]))


@BOTH_ARITHMETICS
@pytest.mark.parametrize("name,dist,warm", [("c1", "cloud", 0), ("c1", "lattice", 0), ("c1", "lattice", 66),
                                            ("ref", "lattice", 0), ("ref", "lattice", 100)])
def test_small_configs_every_particle(ws, name, dist, warm, ieee):
    pos, params = ws.workloads.make_workload(name, dist)
    gpu_step_check(ws, pos, params, ieee, "f64 %s-%s warm %d" % (name, dist, warm), warm)


@BOTH_ARITHMETICS
@pytest.mark.parametrize("warm", [0, 400])
def test_c2_every_particle(ws, warm, ieee):
    pos, params = ws.workloads.make_workload("c2", "cloud")
    gpu_step_check(ws, pos, params, ieee, "f64 c2-cloud warm %d" % warm, warm)


@BOTH_ARITHMETICS
def test_c3_initial_cloud_every_particle(ws, ieee):
    pos, params = ws.workloads.make_workload("c3", "cloud")
    gpu_step_check(ws, pos, params, ieee, "f64 c3-cloud warm 0", 0)


@BOTH_ARITHMETICS
def test_c3_settled_sampled(ws, ieee):
    """The bench line's settled window (400 steps in): 2^19 particles, among them every particle of the 64 densest
    cells, every one over the mask limit and every one on a wall; K6, pressures and the sort view over all of them."""
    pos, params = ws.workloads.make_workload("c3", "cloud")
    gpu_step_check(ws, pos, params, ieee, "f64 c3-cloud warm 400 (sampled)", 400,
                   queries=lambda st: settled_sample(st, params))


@BOTH_ARITHMETICS
def test_edge_coincident_pairs(ws, ieee):
    pos, params = ws.workloads.make_workload("c1", "lattice")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(20)
    state = coincident(w.read_vec("particles"))
    w.close()
    gpu_step_check(ws, pos, params, ieee, "f64 coincident pairs", state=state)


@BOTH_ARITHMETICS
def test_edge_overflow_clump(ws, ieee):
    pos, params = clump(ws)
    worst = gpu_step_check(ws, pos, params, ieee, "f64 overflow clump")
    assert worst["stats"]["mask_overflow"] > 1000
    assert int((worst["ref"].candidates > 2048).sum()) > 1000


@BOTH_ARITHMETICS
def test_edge_alias_15823(ws, ieee):
    n = 15823
    assert F.stencil_aliases(n)
    params = ws.make_params(container_size=(6.0, 4.0, 4.0))
    pos = ws.workloads.uniform_cloud(n, 99, list(params.ext_min), list(params.ext_max))
    gpu_step_check(ws, pos, params, ieee, "f64 alias n=15823", 3)
