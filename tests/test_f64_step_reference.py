"""CPU tier of the per-particle check (tests/f64_step.py): the float32 oracle against the float64 restatement of one
step, particle by particle -- this calibrates the bound's constant with no GPU -- and proof that the per-particle bound
catches a lost or doubled neighbour that the global reorder-noise tolerance of util.assert_particles_close lets through."""
import numpy as np
import pytest

import f64_step as F
from util import assert_particles_close, oracle_from_params, oracle_one_step, reorder_noise_tolerances

HEADROOM = 0.5  # the oracle may use at most half of the bound: the GPU sums in another order, with 1-ulp rcp / sqrt


def _advance(O, orc, state, steps, mode=None):
    for _ in range(steps):
        state = oracle_one_step(O, orc, state, mode=mode)
    return state


def _check_oracle(O, ws, orc, state, params, what, mode=None):
    want = oracle_one_step(O, orc, state, mode=mode)
    sort = (orc.particle_cell_indicies.copy(), orc.particle_indicies.copy(), orc.cell_offsets.copy())
    worst = F.check_step(state, want, params, ws.get_smoothing_kernel(params), what, "oracle", check_sort=sort)
    assert worst["density"] < HEADROOM and worst["acceleration"] < HEADROOM, (what, worst["density"], worst["acceleration"])
    return worst


def clump(ws):
    """tests/test_gpu_overflow.py's state: ~5000 particles inside one 27-cell neighbourhood (> 2048 candidates each)."""
    params = ws.make_params(container_size=(6.0, 6.0, 6.0))
    rng = np.random.default_rng(3)
    clump = rng.uniform(-0.3, 0.3, (5000, 3)).astype(np.float32)
    back = ws.workloads.uniform_cloud(3192, 9, list(params.ext_min), list(params.ext_max))
    return np.concatenate([clump, back]), params


def coincident(state, pairs=((100, 101), (2000, 2064), (3000, 3001), (3001, 3002))):
    """A copy of `state` in which particle b sits exactly on particle a (same position, predicted position, velocity)
    for each (a, b): pairs at d == 0, whose K5 direction is (0, 1, 0); (3000, 3001, 3002) is a triple."""
    st = state.copy()
    for a, b in pairs:
        for f in ("position", "predicted_position", "velocity"):
            st[f][b] = st[f][a]
    return st


@pytest.mark.parametrize("name,dist,warm", [("c1", "cloud", 0), ("c1", "cloud", 40), ("c1", "lattice", 0),
                                            ("c1", "lattice", 66), ("ref", "lattice", 0), ("ref", "lattice", 12)])
def test_oracle_within_the_per_particle_bound(oracle, ws, name, dist, warm):
    pos, params = ws.workloads.make_workload(name, dist)
    orc = oracle_from_params(oracle, pos, params)
    state = _advance(oracle, orc, orc.particles.copy(), warm)
    _check_oracle(oracle, ws, orc, state, params, "%s-%s after %d steps" % (name, dist, warm))


@pytest.mark.parametrize("n", [8, 15823])
def test_oracle_within_the_bound_where_the_stencil_aliases(oracle, ws, n):
    """N = 8 (every stencil offset aliases) and N = 15 823 (the x prime: x-neighbour cells share a bucket, and the
    reference counts such neighbours three times): the restatement's multiplicities reproduce the reference's sums."""
    assert F.stencil_aliases(n)
    if n == 8:
        pos, params = ws.cube_fluid(2, 2, 2), ws.make_params(container_size=(4.0, 4.0, 4.0))
    else:
        params = ws.make_params(container_size=(6.0, 4.0, 4.0))
        pos = ws.workloads.uniform_cloud(n, 99, list(params.ext_min), list(params.ext_max))
    orc = oracle_from_params(oracle, pos, params)
    state = _advance(oracle, orc, orc.particles.copy(), 3, oracle.SORT_FAST)
    worst = _check_oracle(oracle, ws, orc, state, params, "alias n=%d" % n, oracle.SORT_FAST)
    if n == 8:  # 7x + 5y + 5z mod 8: three offsets of every stencil share the own cell's bucket -- self counts 3 times
        assert np.all(worst["ref"].pairs >= 3)


def test_oracle_within_the_bound_in_the_overflow_clump(oracle, ws):
    pos, params = clump(ws)
    orc = oracle_from_params(oracle, pos, params)
    worst = _check_oracle(oracle, ws, orc, orc.particles.copy(), params, "overflow clump")
    assert int((worst["ref"].candidates > 2048).sum()) > 1000


def test_oracle_within_the_bound_with_coincident_pairs(oracle, ws):
    pos, params = ws.workloads.make_workload("c1", "lattice")
    orc = oracle_from_params(oracle, pos, params)
    state = coincident(_advance(oracle, orc, orc.particles.copy(), 20))
    _check_oracle(oracle, ws, orc, state, params, "coincident pairs")


def test_the_multiplicity_predicate_matches_the_bucket_count():
    """stencil_aliases (the replica of the library's upload_mult) is true exactly when some cell's 27-stencil reaches a
    bucket twice -- checked directly on a few thousand cells for sizes either side of it."""
    rng = np.random.default_rng(1)
    cells = rng.integers(-300, 300, (4000, 3))
    for n in (8, 64, 15823, 31646, 131009, 1 << 18, 1 << 20, 2097025):
        buckets = np.stack([F._linear(cells[:, 0] + o[0], cells[:, 1] + o[1], cells[:, 2] + o[2]) % np.uint32(n)
                            for o in F.OFFSETS], 1)
        seen = any(len(np.unique(b)) < 27 for b in buckets)
        assert seen == F.stencil_aliases(n), n


# The state of the sensitivity test: the C1 lattice after 66 oracle steps.  At step 0 (and for the first ~40 steps) no
# pair of the lattice sits at d >= 0.85 h whose term is below the global tolerance; once the sheet has hit the floor the
# global tolerance is set by the dense floor layer and the wall hits (4 ulp of max |acceleration| and 4 x the reorder
# noise of the densest piles), and far-pair terms of quiet particles fall under it.
SENSITIVITY_WARM = 66


def _sensitivity_case(oracle, ws, field):
    """(state, oracle result, reorder-noise tolerance, reference, particle p, pair index s): p is the particle with the
    smallest non-zero |acceleration| among those with a neighbour at d >= 0.85 h whose pair term in `field` lies below
    half the global tolerance of that field (all components) and above twice the particle's own bound -- the particles
    where the gap is.  (The issue's first choice, the quietest particle with any neighbour at d >= 0.85 h, picks pairs at
    d ~ 0.9995 h whose density term is below the rounding of d itself; hence the second condition.)"""
    pos, params = ws.workloads.make_workload("c1", "lattice")
    orc = oracle_from_params(oracle, pos, params)
    state = _advance(oracle, orc, orc.particles.copy(), SENSITIVITY_WARM)
    want = oracle_one_step(oracle, orc, state)
    tol = reorder_noise_tolerances(want, oracle_one_step(oracle, orc, state, reverse=True))
    ref = F.StepReference(state, params, ws.get_smoothing_kernel(params), want, keep_pairs=True)
    i, j, m, d, td, ta = ref.pair_terms
    terms = td if field == "density" else ta
    h = float(params.smoothing_radius)
    amag = np.linalg.norm(want["acceleration"][:, :3].astype(np.float64), axis=1)
    ok = (d >= 0.85 * h) & (i != j) & (amag[i] > 0) & np.all(np.abs(terms) <= tol[field] / 2, axis=1)
    # a pair so close to h that its term is below the distance-rounding part of the bound cannot be told from its own
    # rounding by ANY check: the case is a pair whose term is also above twice the particle's own bound
    own = ref.density_tol if field == "density" else ref.acceleration_tol
    ok &= np.any(np.abs(terms) > 2 * own[i], axis=1)
    cand = np.flatnonzero(ok)
    assert cand.size, "no far pair below the global tolerance"
    # the quietest particle; of its far pairs the one with the largest term
    p = i[cand[np.argmin(amag[i[cand]])]]
    mine = cand[i[cand] == p]
    s = mine[np.argmax(np.abs(terms[mine]).max(axis=1))]
    return state, want, tol, ref, p, s


@pytest.mark.parametrize("field", ["density", "acceleration"])
@pytest.mark.parametrize("fault", ["dropped", "doubled"])
def test_per_particle_check_catches_what_the_global_check_misses(oracle, ws, field, fault):
    state, want, tol, ref, p, s = _sensitivity_case(oracle, ws, field)
    i, j, m, d, td, ta = ref.pair_terms
    term = (td if field == "density" else ta)[s]
    bad = want.copy()
    comp = bad[field][p, :len(term)].astype(np.float64)
    bad[field][p, :len(term)] = (comp - term if fault == "dropped" else comp + term).astype(np.float32)
    assert not np.array_equal(bad[field][p].view(np.uint32), want[field][p].view(np.uint32))
    # the global check of util.py accepts the faulty result ...
    assert_particles_close(bad, want, tol, "sensitivity %s %s (global)" % (fault, field))
    # ... the per-particle bound rejects it, and accepts the true result
    r_bad = ref.ratios(bad)[0 if field == "density" else 1]
    r_ok = ref.ratios(want)[0 if field == "density" else 1]
    qp = int(np.flatnonzero(ref.queries == p)[0])
    assert r_bad[qp].max() > 1.0, ("particle %d, pair (%d, %d) at d = %.4f h: err/tol %.3f"
                                   % (p, i[s], j[s], d[s] / 0.25, r_bad[qp].max()))
    assert r_ok.max() <= HEADROOM


@pytest.mark.parametrize("name", ["c1", "ref"])
def test_integration_restatement_is_bit_exact(oracle, ws, name):
    """K6 restated in numpy float32 reproduces the oracle's integration bit for bit on every particle, through wall
    hits (the C1 sheet reaches the floor within its first 40 steps)."""
    pos, params = ws.workloads.make_workload(name, "lattice")
    orc = oracle_from_params(oracle, pos, params)
    state = orc.particles.copy()
    hits = 0
    for step in range(45 if name == "c1" else 4):
        want = oracle_one_step(oracle, orc, state)
        p, v, q = F.integrate_f32(state, want["acceleration"], params)
        for f, x in (("position", p), ("velocity", v), ("predicted_position", q)):
            assert np.array_equal(x.view(np.uint32), want[f].view(np.uint32)), (step, f)
        hits += int(np.sum(p[:, :3] == np.array(list(params.ext_min)[:3], np.float32)))
        state = want
    if name == "c1":
        assert hits > 0
