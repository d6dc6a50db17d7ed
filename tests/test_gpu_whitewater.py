"""ws_read_whitewater, ws_emit_whitewater and ws_step_whitewater on the GPU: every output bit for bit against the numpy
restatement (tests/whitewater_ref.py) in both arithmetics of the handle, equal velocities, emission counts, parameters and
capacity, the diffuse step with all four classes and the wall rule, launch shapes, an untouched simulation, slabs, other
cell grids, errors.

Scene A: a dam-break block of 16^3 lattice particles (spacing 0.12) in the lowest corner of a (6, 4, 3) container at
h = 0.25, stepped 40 times, with three hand-placed particles appended (one isolated, a coincident pair, all at rest).
Scene B (slabs only): tests/test_gpu_velocity.py's 65 536-particle cloud at step 30."""
import ctypes as C

import numpy as np
import pytest

import aniso_ref as A
import whitewater_ref as W
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_field_grids import OFFSETS, STEPS as GRID_STEPS
from test_gpu_field_grids import cell_budget
from test_gpu_field_grids import scene as grid_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
ARITH = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
N_BLOCK = 4096
SHAPES = (1, 63, 64, 65, 4097)


def _box(params):
    return np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)


def same_stage(got, want, case=""):
    for k in W.OUTPUTS:
        assert same_bits(got[k], want[k]), (case, k)


def same_spawns(got, want, case=""):
    assert got["count"] == want["count"], case
    for k in ("xyz", "velocity", "life", "source"):
        assert same_bits(got[k], want[k]), (case, k)


def load_state(w, pos, vel):
    """Positions and velocities by id through ws_write_particles (the other fields as the handle has them)."""
    rec = w.read_vec("particles")
    rec["position"][:, :3] = pos
    rec["velocity"][:, :3] = vel
    w.write_slice("particles", rec)


class _SceneA:
    """The dam break at step 40 plus the three hand-placed particles: one state (positions, velocities), loaded into one
    handle per arithmetic, and the restatement of its stage -- computed once, shared, never modified."""

    def __init__(self, ws):
        self.ws = ws
        self.params = ws.make_params(container_size=(6.0, 4.0, 3.0))
        lo, hi = _box(self.params)
        block = ws.cube_fluid(16, 16, 16, 0.06).astype(np.float64)
        block += lo + 0.05 - block.min(0)
        # the extras start (and stay: they are loaded again below) in the air under the lid, 2 h and more from anything
        extra = np.array([hi - 0.4, hi - (1.4, 0.4, 0.4), hi - (1.4, 0.4, 0.4)])
        start = np.concatenate([block, extra]).astype(F32)
        w = ws.FluidWorker(start, self.params)
        w.run(40)
        pos, vel = w.read_positions(), w.read_velocities()
        w.close()
        assert np.abs(pos[:N_BLOCK] - start[:N_BLOCK]).max() > 0.5  # it moved and broke
        pos[N_BLOCK:], vel[N_BLOCK:] = start[N_BLOCK:], 0.0
        self.pos, self.vel = pos, vel
        self.n = len(pos)
        self.stage = W.stage(self.params, pos, vel)
        for a in (self.pos, self.vel) + tuple(self.stage.values()):
            a.setflags(write=False)
        self.made = {}

    def get(self, ieee):
        if ieee not in self.made:
            w = self.ws.FluidWorker(self.pos, self.params, ieee_division=ieee)
            load_state(w, self.pos, self.vel)
            self.made[ieee] = w
        return self.made[ieee]

    def emit_dict(self, **kw):
        """Emission parameters with the taus at the 20th and 80th percentile of each potential of this very state."""
        st = self.stage
        taus = {k: tuple(float(q) for q in np.quantile(st[name], (0.2, 0.8)))
                for k, name in (("tau_trapped", "trapped"), ("tau_crest", "crest"), ("tau_energy", "energy"))}
        return dict(W.emit_defaults(), **taus, **kw)

    def close(self):
        for w in self.made.values():
            w.close()


@pytest.fixture(scope="module")
def scene(ws):
    s = _SceneA(ws)
    yield s
    s.close()


def emit_params(ws, d):
    return ws.fluid.whitewater_emit_params(**d)


def step_params(ws, d):
    return ws.fluid.whitewater_step_params(**d)


# ---- 1. the stage ------------------------------------------------------------------------------------------------------------
def test_the_stage_has_the_restatements_bits_in_both_arithmetics(ws, scene):
    st = scene.stage
    got = {ieee: scene.get(ieee).read_whitewater() for ieee in (False, True)}
    for ieee in (False, True):
        assert same_bits(scene.get(ieee).read_positions(), scene.pos) and same_bits(scene.get(ieee).read_velocities(), scene.vel)
        same_stage(got[ieee], st, ieee)
    same_stage(got[False], got[True])  # the stage is IEEE under either flag
    # what the scene must contain (from the restatement)
    nb, nrm = st["neighbours"], st["normal"]
    speed0 = ~scene.vel.any(1)
    assert np.all(nb[N_BLOCK:] == 0) and not nrm[N_BLOCK:].any() and np.all(speed0[N_BLOCK:])
    assert np.count_nonzero(nb == 0) >= 3 and nb.max() > 30
    assert same_bits(st["align"][N_BLOCK:], np.zeros(3, F32)) and same_bits(st["energy"][N_BLOCK:], np.zeros(3, F32))
    assert np.any((st["crest_terms"] > 0) & (st["crest_terms"] < nb))  # both signs of the half-space test at one particle
    assert np.any(st["trapped"] > 0) and np.any(st["crest"] > 0) and np.any(st["align"] > 0) and np.any(st["align"] < 0)
    # any subset of the outputs, each alone
    w = scene.get(False)
    only = np.empty(scene.n, F32)
    assert w._L.ws_read_whitewater(w._h, None, only.ctypes.data, None, None, None, None) == 0
    assert same_bits(only, st["crest"])
    cnt = np.empty(scene.n, np.uint32)
    assert w._L.ws_read_whitewater(w._h, None, None, None, None, None, cnt.ctypes.data) == 0
    assert np.array_equal(cnt, nb)


def test_equal_velocities_trap_no_air(ws, scene):
    w = ws.FluidWorker(scene.pos, scene.params)
    load_state(w, scene.pos, np.tile(np.array([1.5, -0.3, 0.7], F32), (scene.n, 1)))
    got = w.read_whitewater()
    w.close()
    assert same_bits(got["trapped"], np.zeros(scene.n, F32))  # +0
    assert same_bits(got["crest"], scene.stage["crest"]) and same_bits(got["normal"], scene.stage["normal"])
    assert np.all(got["energy"] == got["energy"][0]) and got["energy"][0] > 0


# ---- 2. emission -------------------------------------------------------------------------------------------------------------
@ARITH
def test_emission_counts_and_spawns_are_the_restatements(ws, scene, ieee):
    e = scene.emit_dict(max_per_particle=4, k_trapped=150.0, k_crest=150.0, seed=5)
    m = W.counts(scene.stage, scene.vel, e)
    want = W.spawn(scene.pos, scene.vel, m, e)
    total = int(m.sum())
    assert 0 < total < scene.n * 4 and np.any(m == 4) and np.any(m == 0) and np.any((m > 0) & (m < 4))
    assert not m[N_BLOCK:].any()  # at rest: no axis
    w = scene.get(ieee)
    got = w.emit_whitewater(emit_params(ws, e))
    same_spawns(got, want, ieee)
    assert np.array_equal(np.bincount(got["source"], minlength=scene.n), m)  # every m_i
    assert np.all(np.diff(got["source"].astype(np.int64)) >= 0)
    # a generous capacity in one call; each output alone
    same_spawns(w.emit_whitewater(emit_params(ws, e), cap=total + 1000), want, ieee)
    k = C.c_uint32(0)
    life = np.empty(total, F32)
    assert w._L.ws_emit_whitewater(w._h, C.byref(emit_params(ws, e)), total, None, None, life.ctypes.data, None, C.byref(k)) == 0
    assert k.value == total and same_bits(life, want["life"])


def test_emission_parameters_and_capacity(ws, scene):
    w = scene.get(False)
    e = scene.emit_dict(max_per_particle=4, k_trapped=150.0, k_crest=150.0, seed=5)
    base = w.emit_whitewater(emit_params(ws, e))
    # both rates 0: nothing
    none = w.emit_whitewater(emit_params(ws, dict(e, k_trapped=0.0, k_crest=0.0)))
    assert none["count"] == 0 and len(none["xyz"]) == 0
    # another seed: other spawns
    other = w.emit_whitewater(emit_params(ws, dict(e, seed=6)))
    assert other["count"] > 0
    assert other["count"] != base["count"] or not same_bits(other["xyz"], base["xyz"])
    same_spawns(other, W.spawn(scene.pos, scene.vel, W.counts(scene.stage, scene.vel, dict(e, seed=6)), dict(e, seed=6)))
    # one short of the count: the count comes back, nothing is written
    total = base["count"]
    xyz, vel = np.full((total, 3), 7.0, F32), np.full((total, 3), 7.0, F32)
    life, src = np.full(total, 7.0, F32), np.full(total, 7, np.uint32)
    k = C.c_uint32(0)
    assert w._L.ws_emit_whitewater(w._h, C.byref(emit_params(ws, e)), total - 1, xyz.ctypes.data, vel.ctypes.data, life.ctypes.data,
                                   src.ctypes.data, C.byref(k)) == 0
    assert k.value == total
    assert np.all(xyz == 7.0) and np.all(vel == 7.0) and np.all(life == 7.0) and np.all(src == 7)
    short = w.emit_whitewater(emit_params(ws, e), cap=total - 1)
    assert short["count"] == total and short["xyz"] is None
    # the crest term alone, gated by the alignment; the trapped term alone
    for d in (dict(e, k_trapped=0.0), dict(e, k_crest=0.0), dict(e, crest_align=-2.0), dict(e, crest_align=2.0)):
        m = W.counts(scene.stage, scene.vel, d)
        assert m.any(), d
        same_spawns(w.emit_whitewater(emit_params(ws, d)), W.spawn(scene.pos, scene.vel, m, d), d)


# ---- 3. the diffuse step -----------------------------------------------------------------------------------------------------
def diffuse(cur, params, seed=3, n=(1500, 900, 128, 300)):
    """Diffuse particles like tests/test_gpu_velocity.py's probes(): near particles, uniform in the box, 12 h and more
    outside, and on the container's walls moving outwards; velocities N(0, 2), lives straddling dt = 1 / 60."""
    rng = np.random.default_rng(seed)
    h = float(params.smoothing_radius)
    lo, hi = _box(params)
    near = cur[rng.choice(len(cur), n[0], replace=len(cur) < n[0])] + rng.normal(0.0, h / 5, (n[0], 3))
    inside = lo + rng.random((n[1], 3)) * (hi - lo)
    far = hi + 12.0 * h + rng.exponential(2.0, (n[2], 3))
    wall = lo + rng.random((n[3], 3)) * (hi - lo)
    axis, side = rng.integers(0, 3, n[3]), rng.integers(0, 2, n[3])
    wall[np.arange(n[3]), axis] = np.where(side == 1, hi[axis], lo[axis])
    p = np.concatenate([near, inside, far, wall]).astype(F32)
    v = rng.normal(0.0, 2.0, p.shape)
    rows = np.arange(len(p) - n[3], len(p))
    v[rows, axis] = np.where(side == 1, 1.0, -1.0) * (1.0 + rng.random(n[3]))
    life = rng.uniform(-0.01, 0.06, len(p))
    return p, v.astype(F32), life.astype(F32)


def check_step(ws, w, params, cur, sp, p, v, life, case, rounds=5):
    """One step, then four more fed with the results: each bit for bit the restatement driven by the library's own
    velocity field at the points and a brute-force accept count.  Returns the classes seen and whether a wall reflected."""
    seen, bounced = set(), False
    spp = step_params(ws, sp)
    for r in range(rounds):
        u, _ = w.sample_velocity_points(p, density=True)
        c = W.accept_count(params, cur, p)
        want = W.step(params, sp, p, v, life, u, c)
        got = w.step_whitewater(spp, p, v, life)
        for a, b, what in zip(got, want[:4], ("xyz", "velocity", "life", "class")):
            assert a.dtype == b.dtype and a.shape == b.shape, (case, r, what)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (case, r, what)
        # in place == out of place
        bp, bv, bl = p.copy(), v.copy(), life.copy()
        inplace = w.step_whitewater(spp, bp, bv, bl, in_place=True)
        assert np.shares_memory(inplace[0], bp) and same_bits(bp, got[0]) and same_bits(bv, got[1]) and same_bits(bl, got[2]), (case, r)
        assert np.array_equal(inplace[3], got[3]), (case, r)
        seen |= set(int(k) for k in np.unique(got[3]))
        bounced = bounced or bool(want[4].any())
        p, v, life = got[0], got[1], got[2]
    return seen, bounced


@ARITH
def test_the_step_has_the_restatements_bits(ws, scene, ieee):
    w = scene.get(ieee)
    p, v, life = diffuse(scene.pos, scene.params)
    life[:64] = 5.0  # (some live through the five rounds whatever their class)
    seen, bounced = check_step(ws, w, scene.params, scene.pos, W.step_defaults(), p, v, life, ieee)
    assert seen == {0, 1, 2, 3} and bounced


def test_a_diffuse_particles_bits_do_not_depend_on_the_others(ws, scene):
    w = scene.get(False)
    p, v, life = diffuse(scene.pos, scene.params, seed=9, n=(2400, 1200, 197, 300))
    assert len(p) == SHAPES[-1]
    spp = step_params(ws, W.step_defaults())
    whole = w.step_whitewater(spp, p, v, life)
    order = np.random.default_rng(11).permutation(len(p))
    for a, b in zip(w.step_whitewater(spp, p[order], v[order], life[order]), whole):
        assert np.array_equal(a, b[order])
    for m in SHAPES[:-1]:
        for a, b in zip(w.step_whitewater(spp, p[-m:], v[-m:], life[-m:]), whole):
            assert np.array_equal(a.view(np.uint8), b[-m:].view(np.uint8)), m


# ---- 4. launch shapes of the per-particle kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_every_particle_count_gives_the_restatements_bits(ws, scene, n):
    """n fluid particles (the first n of a 4 097 cloud dense enough to have neighbours): the stage and the spawns of a
    handle of that size.  A spawn depends on its emitter alone: the spawns of particle i are those the restatement makes
    for it on its own."""
    params = ws.make_params(container_size=(3.0, 2.0, 2.0))
    pos = ws.workloads.uniform_cloud(SHAPES[-1], 77, list(params.ext_min), list(params.ext_max))[:n]
    vel = np.random.default_rng(78).normal(0.0, 2.0, (SHAPES[-1], 3)).astype(F32)[:n]
    w = ws.FluidWorker(pos, params)
    load_state(w, pos, vel)
    st = W.stage(params, pos, vel)
    same_stage(w.read_whitewater(), st, n)
    e = dict(W.emit_defaults(), tau_trapped=(0.0, 1.0), tau_crest=(0.0, 1.0), tau_energy=(0.0, 1.0), k_trapped=120.0,
             max_per_particle=64, seed=n)
    m = W.counts(st, vel, e)
    got = w.emit_whitewater(emit_params(ws, e))
    w.close()
    same_spawns(got, W.spawn(pos, vel, m, e), n)
    if n > 1:
        assert m.any() and m.max() <= 64
        i = int(np.flatnonzero(m)[-1])
        alone = W.spawn(pos[i:i + 1], vel[i:i + 1], m[i:i + 1], e, ids=[i])
        mine = got["source"] == i
        assert mine.sum() == m[i] and same_bits(got["xyz"][mine], alone["xyz"]) and same_bits(got["life"][mine], alone["life"])


# ---- 5. the simulation is untouched ------------------------------------------------------------------------------------------
def _trajectory(ws, pos, params, regrid, steps, calls, graph):
    w = ws.FluidWorker(pos, params, graph=graph)
    lo, hi = _box(params)
    rng = np.random.default_rng(2)
    q = (lo + rng.random((64, 3)) * (hi - lo)).astype(F32)
    qv = rng.normal(0.0, 1.0, (64, 3)).astype(F32)
    ql = np.full(64, 1.0, F32)
    e = ws.fluid.whitewater_emit_params(tau_trapped=(0.0, 1.0), tau_crest=(0.0, 1.0), tau_energy=(0.0, 1.0))
    sp = ws.fluid.whitewater_step_params()
    seen = 0
    for t in range(steps):
        if t == steps // 2:
            w.set_params(regrid)
        w.run(1)
        if calls:
            seen += int(np.count_nonzero(w.read_whitewater()["trapped"]))
            seen += w.emit_whitewater(e)["count"]
            seen += int(np.count_nonzero(w.step_whitewater(sp, q, qv, ql)[0] != q))
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats, seen


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_the_calls_every_step_leave_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    assert len(pos) == 4096
    regrid = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=F32(0.2))
    want, _, _ = _trajectory(ws, pos, params, regrid, 200, False, graph)
    got, stats, seen = _trajectory(ws, pos, params, regrid, 200, True, graph)
    assert seen > 0
    if graph:
        assert stats["graph_steps"] > 0
    assert got.dtype.itemsize == 80
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- 6. slabs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    steps = 30
    w = ws.FluidWorker(pos, params)
    w.run(steps)
    cur = w.read_positions()
    p, v, life = diffuse(cur, params)
    e = ws.fluid.whitewater_emit_params(tau_trapped=(0.0, 2.0), tau_crest=(0.0, 2.0), tau_energy=(0.0, 2.0), seed=3)
    sp = ws.fluid.whitewater_step_params()
    cap = 8 * len(pos)

    def calls(x, wanted=True):
        kw = {} if wanted is None else {"want": wanted}
        return [x.read_whitewater(**kw), x.emit_whitewater(e, cap=cap, **kw), x.step_whitewater(sp, p, v, life, **kw)]

    want = calls(w, None)
    w.close()
    assert want[0]["trapped"].any() and 0 < want[1]["count"] < cap and len(set(want[2][3].tolist())) >= 3
    got = _slab_run(ws, params, pos, world, steps, lambda s, r: calls(s, r != 1))
    assert got[1] == [None, None, None]  # rank 1 only contributed
    for r in [k for k in range(world) if k != 1]:
        same_stage(got[r][0], want[0], r)
        same_spawns(got[r][1], want[1], r)
        for a, b in zip(got[r][2], want[2]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), r


# ---- 7. other cell grids -----------------------------------------------------------------------------------------------------
def _other_grid_checks(ws, w, params, ieee, case):
    merged = w.stats()["cells_merged"]
    cur, vel = w.read_positions(), w.read_velocities()
    ids = np.random.default_rng(4).choice(len(cur), 1500, replace=False)
    st = W.stage(params, cur, vel, merged, ids)
    got = w.read_whitewater()
    assert st["neighbours"].max() > 8 and st["trapped"].any() and st["crest"].any()
    for k in W.OUTPUTS:
        assert same_bits(got[k][ids], st[k]), (case, k)
    p, v, life = diffuse(cur, params, seed=5, n=(500, 300, 64, 136))
    seen, bounced = check_step(ws, w, params, cur, W.step_defaults(), p, v, life, case, rounds=2)
    assert {0, 3} <= seen and len(seen) >= 3 and bounced, (case, seen)


@ARITH
def test_merged_cells(ws, devlib, ieee):
    pos, params = grid_scene(ws, 0.25)
    with cell_budget("800"):
        w = ws.FluidWorker(pos, params, ieee_division=ieee, library=devlib)
    w.run(GRID_STEPS)
    merged = w.stats()["cells_merged"]
    assert merged[1] > 1 and merged[2] > 1
    assert tuple(int(v) for v in A.Grid(params, merged).dim) == tuple(w.grid_dims())
    _other_grid_checks(ws, w, params, ieee, "merged zy")
    w.close()


@ARITH
def test_a_container_far_from_the_origin(ws, ieee):
    pos, params = grid_scene(ws, 0.2, OFFSETS["east"])
    assert OFFSETS["east"] == (37.35, -21.7, 5.47)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(GRID_STEPS)
    assert w.stats()["cells_merged"] == (1, 1, 1)
    _other_grid_checks(ws, w, params, ieee, "offset east h0.2")
    w.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(5)
    L, h = w._L, w._h
    n = len(pos)
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.05], [-3.0, 1.0, 0.0], [50.0, 0.0, 0.0]], F32)
    vel = np.ones((4, 3), F32)
    life = np.ones(4, F32)
    op, ov, ol, oc = np.empty((4, 3), F32), np.empty((4, 3), F32), np.empty(4, F32), np.empty(4, np.uint8)
    T = np.empty(n, F32)
    cap = 8 * n
    sx, sl, ss = np.empty((cap, 3), F32), np.empty(cap, F32), np.empty(cap, np.uint32)
    k = C.c_uint32(0)

    def ptr(x):
        return None if x is None else x.ctypes.data

    def read(out=T):
        return L.ws_read_whitewater(h, ptr(out), None, None, None, None, None)

    def emit(e=True, count=True, xyz=sx, **fields):
        par = ws.fluid.whitewater_emit_params(**dict(dict(tau_trapped=(0.0, 1.0), tau_energy=(0.0, 1.0)), **fields))
        return L.ws_emit_whitewater(h, C.byref(par) if e else None, cap, ptr(xyz), ptr(sx), ptr(sl), ptr(ss),
                                    C.byref(k) if count else None)

    def step(s=True, xyz=pts, velocity=vel, lives=life, m=4, outs=(op, ov, ol, oc), **fields):
        par = ws.fluid.whitewater_step_params(**fields)
        return L.ws_step_whitewater(h, C.byref(par) if s else None, ptr(xyz), ptr(velocity), ptr(lives), m, *(ptr(o) for o in outs))

    def bad(x, i, val):
        x = x.copy()
        x[i] = val
        return x

    def refused(call, what):
        assert call() == 1, what
        assert read() == 0 and emit() == 0 and step() == 0, what  # ... and the next call succeeds

    assert read() == 0 and emit() == 0 and k.value > 0 and step() == 0
    refused(lambda: read(out=None), "every output NULL")
    refused(lambda: emit(e=False), "NULL params")
    refused(lambda: emit(count=False), "NULL n_emitted")
    for name in ("tau_trapped", "tau_crest", "tau_energy"):
        for pair in ((1.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (0.0, np.inf), (np.nan, 1.0)):
            refused(lambda: emit(**{name: pair}), (name, pair))
    for name in ("k_trapped", "k_crest"):
        for val in (-1.0, np.inf, np.nan):
            refused(lambda: emit(**{name: val}), (name, val))
    for val in (np.nan, np.inf):
        refused(lambda: emit(crest_align=val), ("crest_align", val))
    for name in ("dt", "radius"):
        for val in (0.0, -0.1, np.inf, np.nan):
            refused(lambda: emit(**{name: val}), (name, val))
    for pair in ((2.0, 1.0), (-1.0, 1.0), (0.0, np.inf), (np.nan, 1.0)):
        refused(lambda: emit(lifetime=pair), ("lifetime", pair))
    for val in (0, 65):
        refused(lambda: emit(max_per_particle=val), ("max_per_particle", val))
    refused(lambda: step(s=False), "NULL params")
    refused(lambda: step(xyz=None), "NULL xyz")
    refused(lambda: step(velocity=None), "NULL velocity")
    refused(lambda: step(lives=None), "NULL life")
    refused(lambda: step(m=0), "m == 0")
    refused(lambda: step(m=(1 << 28) + 1), "more than 2^28")  # refused before a particle is read
    refused(lambda: step(outs=(None, None, None, None)), "every output NULL")
    for val in (0.0, -0.1, np.inf, np.nan):
        refused(lambda: step(dt=val), ("dt", val))
    for val in (np.inf, np.nan):
        refused(lambda: step(buoyancy=val), ("buoyancy", val))
    for val in (-0.1, 1.1, np.nan):
        refused(lambda: step(drag=val), ("drag", val))
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        refused(lambda: step(xyz=bad(pts, (2, 1), val)), ("coordinate", val))
        refused(lambda: step(velocity=bad(vel, (1, 2), val)), ("velocity", val))
    for val in (np.nan, np.inf):
        refused(lambda: step(lives=bad(life, 3, val)), ("life", val))
    # allowed: the limits themselves, single outputs, lifetime[0] == lifetime[1], equal class thresholds
    assert emit(max_per_particle=1) == 0 and emit(max_per_particle=64) == 0 and emit(lifetime=(3.0, 3.0)) == 0
    assert emit(xyz=None) == 0 and emit(k_trapped=0.0, k_crest=0.0) == 0 and k.value == 0
    assert step(drag=0.0) == 0 and step(drag=1.0) == 0 and step(xyz=bad(pts, (0, 0), 1e15)) == 0
    assert step(outs=(None, None, None, oc)) == 0 and step(spray_max=0, bubble_min=0) == 0
    # the handle steps on and gives what a handle that saw no refusal gives
    fresh = ws.FluidWorker(pos, params)
    fresh.run(5)
    for x in (w, fresh):
        x.run(20)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    same_stage(w.read_whitewater(), fresh.read_whitewater())
    w.close()
    fresh.close()


def _all_calls(ws, w):
    q = np.zeros((1, 3), F32)
    return (lambda: w.read_whitewater(), lambda: w.emit_whitewater(ws.fluid.whitewater_emit_params()),
            lambda: w.step_whitewater(ws.fluid.whitewater_step_params(), q, q, np.ones(1, F32)))


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    for call in _all_calls(ws, w):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.close()


def test_a_dead_handle_refuses_every_call(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    assert w.read_whitewater()["energy"].any()
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in _all_calls(ws, w):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
