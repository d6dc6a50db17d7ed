"""The attribute calls on the GPU: write / read, paint and diffusion bit for bit against the numpy restatement
(tests/attributes_ref.py) in both arithmetics of the handle and at every launch shape, the field against the restatement
and against the density sampler, merged cell grids, an untouched simulation, slabs, refusals.

Scene A is tests/test_gpu_whitewater.py's: the dam break at step 40 plus an isolated particle and a coincident pair, 4 099
particles; the three hand-placed particles carry -0 in every channel.  The slab scene is test_gpu_field_grids' 16 384-particle
cloud at step 25, the smallest the slab field tests use."""
import ctypes as C

import numpy as np
import pytest

import aniso_ref as A
import attributes_ref as At
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
RATES = (30.0, 12.0, 0.0, 3.5)  # r = 0.5 (the limit), 0.2, 0 (the channel keeps its bits), 0.058


def to_ws(ws, brushes):
    return [ws.fluid.brush(b["kind"], b["centre"], b["radius"], b["value"], b["strength"], b["falloff"], b["channels"])
            for b in brushes]


def dparams(ws, rate=RATES, iterations=1):
    return ws.fluid.diffuse_params(rate=rate, iterations=iterations)


def random_attr(n, seed=21):
    """Seeded values in [-1, 2), every 17th particle with a -0 in channel 1."""
    a = (np.random.default_rng(seed).random((n, 4)) * 3.0 - 1.0).astype(F32)
    a[::17, 1] = F32(-0.0)
    return a


def sixteen_brushes(pos, seed=4):
    """Both kinds, falloff 0 / 0.5 / 1, partial masks, overlapping spheres around particles of the block (the first two
    share a centre), one on the isolated particle alone, one that reaches nobody, one negative ADD."""
    rng = np.random.default_rng(seed)
    at = pos[rng.choice(N_BLOCK, 13, replace=False)].astype(np.float64)
    at[1] = at[0]
    out = []
    for e in range(13):
        out.append(At.brush(("mix", "add")[e % 2], at[e] + rng.normal(0.0, 0.02, 3), 0.15 + 0.05 * (e % 5),
                            rng.normal(0.0, 1.0, 4), strength=(0.25, 0.5, 1.0)[e % 3] if e % 2 == 0 else -1.5 + 0.5 * e,
                            falloff=(0.0, 0.5, 1.0)[(e // 2) % 3], channels=(15, 1, 6, 8, 10, 5, 3)[e % 7]))
    out.append(At.brush("mix", pos[N_BLOCK].astype(np.float64), 0.05, (0.5, 0.25, -4.0, 9.0), strength=1.0, channels=5))
    out.append(At.brush("add", (1e3, 1e3, 1e3), 1.0, (1.0, 1.0, 1.0, 1.0)))
    out.append(At.brush("add", at[3], 0.4, (-0.125, 0.0, 3.0, 1e-3), strength=-2.0, falloff=1.0, channels=13))
    assert len(out) == 16
    return out


@pytest.fixture(scope="module")
def scene(ws):
    s = _SceneA(ws)
    s.attr = random_attr(s.n)
    s.attr[N_BLOCK:] = F32(-0.0)
    # pass A is the same for every call on this state: computed once, shared, never modified
    s.rho = At.densities(s.params, s.pos)
    s.brushes = sixteen_brushes(s.pos)
    for a in (s.attr, s.rho):
        a.setflags(write=False)
    yield s
    s.close()


# ---- 1. scene A: write / read, paint, diffusion ----------------------------------------------------------------------------
@ARITH
def test_write_then_read_round_trips_the_bits(ws, scene, ieee):
    w = scene.get(ieee)
    a = scene.attr.copy()
    a[5] = (np.nan, np.inf, -np.inf, F32(1e-42))  # used as given
    w.write_attributes(a)
    assert same_bits(w.read_attributes(), a) and np.all(np.signbit(w.read_attributes()[N_BLOCK:]))
    w.write_attributes(None)
    assert same_bits(w.read_attributes(), np.zeros((scene.n, 4), F32))  # NULL: all +0


def test_paint_has_the_restatements_bits_in_both_arithmetics(ws, scene):
    want, counts = At.paint(scene.pos, scene.attr, scene.brushes)
    for ieee in (False, True):
        w = scene.get(ieee)
        w.write_attributes(scene.attr)
        got_counts = w.paint_attributes(to_ws(ws, scene.brushes))
        assert np.array_equal(got_counts, counts), ieee
        assert same_bits(w.read_attributes(), want), ieee
        # without the counts: the same bits
        w.write_attributes(scene.attr)
        assert w.paint_attributes(to_ws(ws, scene.brushes), counts=False) is None
        assert same_bits(w.read_attributes(), want), ieee
    # what the brushes must cover (from the restatement)
    assert counts[13] == 1 and counts[14] == 0 and np.count_nonzero(counts) == 15
    reached = np.zeros(scene.n, bool)
    for b in scene.brushes:
        reached |= np.linalg.norm(scene.pos.astype(np.float64) - np.asarray(b["centre"], np.float64), axis=1) < 0.999 * b["radius"]
    assert counts.sum() > 1.03 * reached.sum() > 100  # overlapping spheres: particles painted more than once
    assert same_bits(want[N_BLOCK + 1:], scene.attr[N_BLOCK + 1:])  # out of every reach: the -0 stays
    assert same_bits(want[N_BLOCK, [1, 3]], scene.attr[N_BLOCK, [1, 3]]) and list(want[N_BLOCK, [0, 2]]) == [0.5, -4.0]
    kinds = {(b["kind"], b["falloff"]) for b in scene.brushes}
    assert {(k, f) for k in (0, 1) for f in (0.0, 0.5, 1.0)} <= kinds
    # a second pass runs on the running value
    again, _ = At.paint(scene.pos, want, scene.brushes[:3])
    w = scene.get(True)
    w.paint_attributes(to_ws(ws, scene.brushes[:3]))
    assert same_bits(w.read_attributes(), again) and not same_bits(again, want)


@pytest.mark.parametrize("iterations", [1, 5])
def test_diffusion_has_the_restatements_bits_in_both_arithmetics(ws, scene, iterations):
    want, cnt = At.diffuse(scene.params, scene.pos, scene.attr, RATES, DT, iterations, fed=scene.rho)
    for ieee in (False, True):
        w = scene.get(ieee)
        w.write_attributes(scene.attr)
        affected = w.diffuse_attributes(dparams(ws, iterations=iterations), DT)
        assert affected == np.count_nonzero(cnt), ieee
        assert same_bits(w.read_attributes(), want), ieee
    # what the scene must contain (from the restatement)
    assert np.all(cnt[N_BLOCK:] == 0) and cnt.max() > 30 and np.count_nonzero(cnt) > scene.n // 2
    assert same_bits(want[cnt == 0], scene.attr[cnt == 0]) and np.all(np.signbit(want[N_BLOCK:]))
    assert same_bits(want[:, 2], scene.attr[:, 2])  # rate 0
    moved = cnt > 0
    for c in (0, 1, 3):
        assert np.mean(want[moved, c] != scene.attr[moved, c]) > 0.9, c
    if iterations == 5:
        # ... equals five calls of 1, and without the count the same bits
        w = scene.get(False)
        w.write_attributes(scene.attr)
        for _ in range(5):
            assert w.diffuse_attributes(dparams(ws), DT) == np.count_nonzero(cnt)
        assert same_bits(w.read_attributes(), want)
        w.write_attributes(scene.attr)
        assert w.diffuse_attributes(dparams(ws, iterations=5), DT, count=False) is None
        assert same_bits(w.read_attributes(), want)
        once, _ = At.diffuse(scene.params, scene.pos, scene.attr, RATES, DT, 1, fed=scene.rho)
        assert not same_bits(once, want)


# ---- 2. launch shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_every_particle_count_gives_the_restatements_bits(ws, scene, n):
    """The first n particles of the scene as a handle of their own: n = 1 has no neighbour at all, 63 / 64 / 65 straddle a
    wave, 4 097 is one lane into a new workgroup (and holds the isolated particle)."""
    pos, attr = scene.pos[:n], scene.attr[:n]
    w = ws.FluidWorker(pos, scene.params)
    load_state(w, pos, scene.vel[:n])
    assert same_bits(w.read_attributes(), np.zeros((n, 4), F32))
    w.write_attributes(attr)
    brushes = [At.brush("mix", pos[0].astype(np.float64), 0.3, (1.0, 0.5, 0.25, 2.0), strength=0.75, falloff=0.5, channels=7),
               At.brush("add", pos[n // 2].astype(np.float64), 0.2, (0.0, -1.0, 0.0, 1.0), strength=2.0, channels=10),
               At.brush("mix", pos[n - 1].astype(np.float64), 0.1, (3.0, 3.0, 3.0, 3.0), falloff=1.0)]
    painted, counts = At.paint(pos, attr, brushes)
    assert np.array_equal(w.paint_attributes(to_ws(ws, brushes)), counts) and counts.min() >= 1
    assert same_bits(w.read_attributes(), painted)
    want, cnt = At.diffuse(scene.params, pos, painted, RATES, DT, 2)
    assert w.diffuse_attributes(dparams(ws, iterations=2), DT) == np.count_nonzero(cnt)
    assert (np.count_nonzero(cnt) > 0) == (n > 1)
    assert same_bits(w.read_attributes(), want)
    q = np.concatenate([pos[:: max(1, n // 16)], pos[:8] + F32(0.03)])
    val, rho = w.sample_attribute_points(q, density=True)
    assert same_bits(rho, w.sample_density_points(q))
    w.close()


# ---- 3. the field ----------------------------------------------------------------------------------------------------------------
def probes(pos, params, seed=6):
    """257 points: 128 at particles + N(0, 0.05), 64 uniform in the container, 33 exactly at particles (the three
    hand-placed ones included), 32 far outside the grid."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    near = pos[rng.choice(N_BLOCK, 128, replace=False)] + rng.normal(0.0, 0.05, (128, 3))
    inside = lo + rng.random((64, 3)) * (hi - lo)
    at = np.concatenate([pos[rng.choice(N_BLOCK, 30, replace=False)], pos[N_BLOCK:]]).astype(np.float64)
    far = hi + 5.0 + rng.exponential(3.0, (32, 3))
    q = np.concatenate([near, inside, at, far]).astype(F32)
    assert len(q) == 257
    return q


def close_to(got, want, scale):
    """The hardware sqrt is within one ulp of the correctly rounded one, which moves every weight by parts in 10^6: two
    orders of magnitude inside this."""
    return np.all(np.abs(got.astype(np.float64) - want) <= 1e-4 * scale)


@ARITH
def test_the_field_at_points_and_on_a_grid(ws, scene, ieee):
    w = scene.get(ieee)
    w.write_attributes(scene.attr)
    q = probes(scene.pos, scene.params)
    want, want_rho, _, cnt = At.field(scene.params, scene.pos, scene.attr, q)
    val, rho = w.sample_attribute_points(q, density=True)
    assert val.shape == (257, 4) and same_bits(rho, w.sample_density_points(q))
    assert same_bits(w.sample_attribute_points(q), val)  # without the density: the same bits
    assert np.all(rho[-32:] == 0) and same_bits(val[rho == 0], np.zeros((np.count_nonzero(rho == 0), 4), F32))
    assert np.all(rho[-65:-32] > 0) and np.mean(cnt >= 8) > 0.25 and np.count_nonzero(cnt == 0) >= 32
    # at the three hand-placed particles the moments are +0 + fl(w * -0) = +0: the field of a -0 is +0
    assert same_bits(val[-35:-32], np.zeros((3, 4), F32))
    scale = np.abs(scene.attr).max()
    if ieee:
        assert same_bits(val, want) and same_bits(rho, want_rho)
    else:
        assert close_to(val, want, scale) and close_to(rho, want_rho, want_rho.max())
    h = F32(scene.params.smoothing_radius)
    dims = (9, 7, 5)
    centre = np.median(scene.pos[:N_BLOCK].astype(np.float64), 0)
    for per_h in (0.5, 1.5):  # the brick form, and the points form on a grid
        spacing = np.full(3, h * F32(per_h), F32)
        origin = (centre - spacing.astype(np.float64) * (4, 3, 2)).astype(F32)
        nodes = At.grid_nodes(origin, spacing, dims)
        gval, grho = w.sample_attribute_grid(origin, spacing, dims, density=True)
        assert gval.shape == (5, 7, 9, 4) and grho.shape == (5, 7, 9)
        pval, prho = w.sample_attribute_points(nodes, density=True)
        assert same_bits(gval.reshape(-1, 4), pval) and same_bits(grho.reshape(-1), prho), per_h
        assert same_bits(grho, w.sample_density_grid(origin, spacing, dims)), per_h
        assert same_bits(w.sample_attribute_grid(origin, spacing, dims), gval), per_h
        assert np.count_nonzero(grho) > 30, per_h
        gw, gw_rho, _, _ = At.field(scene.params, scene.pos, scene.attr, nodes)
        if ieee:
            assert same_bits(pval, gw) and same_bits(prho, gw_rho), per_h
        else:
            assert close_to(pval, gw, scale), per_h
    # only the density: the value may be NULL
    only = np.empty(257, F32)
    assert w._L.ws_sample_attribute_points(w._h, q.ctypes.data, 257, None, only.ctypes.data) == 0 and same_bits(only, rho)


def test_merged_cells(ws, devlib):
    pos, params = grid_scene(ws, 0.25)
    with cell_budget("800"):
        w = ws.FluidWorker(pos, params, ieee_division=True, library=devlib)
    w.run(GRID_STEPS)
    merged = w.stats()["cells_merged"]
    assert merged[1] > 1 and merged[2] > 1
    assert tuple(int(v) for v in A.Grid(params, merged).dim) == tuple(w.grid_dims())
    cur = w.read_positions()
    attr = random_attr(len(cur), 8)
    w.write_attributes(attr)
    rng = np.random.default_rng(5)
    q = np.concatenate([cur[rng.choice(len(cur), 200, replace=False)] + rng.normal(0.0, 0.05, (200, 3)).astype(F32),
                        cur[:57]]).astype(F32)
    want, want_rho, _, cnt = At.field(params, cur, attr, q, merged)
    val, rho = w.sample_attribute_points(q, density=True)
    assert cnt.max() > 8 and same_bits(val, want) and same_bits(rho, want_rho)
    h = F32(params.smoothing_radius)
    origin, spacing, dims = cur.mean(0).astype(F32), np.full(3, h / F32(2), F32), (9, 7, 5)
    gval, grho = w.sample_attribute_grid(origin, spacing, dims, density=True)
    gw, gw_rho, _, _ = At.field(params, cur, attr, At.grid_nodes(origin, spacing, dims), merged)
    assert same_bits(gval.reshape(-1, 4), gw) and same_bits(grho.reshape(-1), gw_rho) and np.count_nonzero(gw_rho) > 100
    # the same bits as the same state on the unmerged grid would give is NOT promised (the order differs); the pairs are
    plain = At.field(params, cur, attr, q)
    assert np.array_equal(plain[3], cnt)
    w.close()


# ---- 4. an untouched simulation ---------------------------------------------------------------------------------------------------
@GRAPH
def test_the_calls_leave_the_trajectory_bitwise_unchanged_and_the_attributes_survive(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    regrid = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=F32(0.2))
    n = len(pos)
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    b = to_ws(ws, [At.brush("mix", 0.5 * (lo + hi), 4.0, (1.0, 0.0, 0.5, 300.0), falloff=1.0)])  # (c1 is 16 x 18 x 0.2)
    q = pos[::61]
    out = []
    for calls in (False, True):
        w = ws.FluidWorker(pos, params, graph=graph)
        if not calls:
            assert same_bits(w.read_attributes(), np.zeros((n, 4), F32))  # never written: all +0
        for t in range(20):
            w.run(1)
            if calls:
                assert w.paint_attributes(b)[0] > 100
                assert w.diffuse_attributes(dparams(ws, (10.0, 10.0, 10.0, 10.0), 2), DT) > 1000
                assert w.sample_attribute_points(q).any()
        assert w.steps_done() == 20
        if graph:
            assert w.stats()["graph_steps"] > 0
        out.append(w.read_vec("particles"))
        if calls:
            a = w.read_attributes()
            assert a.any()
            buf = np.empty((n, 3), F32)
            w.read_positions_begin(buf)  # between the two halves of an asynchronous readback too
            w.paint_attributes(b, counts=False)
            a = w.read_attributes()
            w.read_positions_end()
            assert same_bits(buf, np.ascontiguousarray(out[1]["position"][:, :3]))
            w.run(3)
            assert same_bits(w.read_attributes(), a)  # the steps carry them along
            w.set_params(regrid)
            assert same_bits(w.read_attributes(), a)  # ... a re-grid
            w.run(1)
            assert w.diffuse_attributes(dparams(ws), DT) > 0  # (and the calls work on the new grid)
            a = w.read_attributes()
            rec = w.read_vec("particles")
            w.write_slice("particles", rec)
            assert same_bits(w.read_attributes(), a)  # ... ws_write_particles
            w.reset(pos)
            assert same_bits(w.read_attributes(), np.zeros((n, 4), F32))  # ws_reset: +0
            w.run(2)
        w.close()
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))


# ---- 5. slabs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_as_a_single_handle(ws, world):
    pos, params = grid_scene(ws, 0.25)
    n = len(pos)
    attr = random_attr(n, 31)
    w = ws.FluidWorker(pos, params)
    w.run(GRID_STEPS)
    cur = w.read_positions()
    rng = np.random.default_rng(2)
    brushes = [At.brush(("mix", "add")[e % 2], cur[rng.integers(n)].astype(np.float64), 0.5 + 0.1 * e, rng.normal(0.0, 1.0, 4),
                        strength=0.5, falloff=(0.0, 0.5, 1.0)[e % 3], channels=(15, 5, 10, 3)[e]) for e in range(4)]
    q = np.concatenate([cur[::257], cur[::509] + F32(0.04)]).astype(F32)
    want = {}
    w.write_attributes(attr)
    want["counts"] = w.paint_attributes(to_ws(ws, brushes))
    want["painted"] = w.read_attributes()
    want["affected"] = w.diffuse_attributes(dparams(ws, iterations=5), DT)
    want["mixed"] = w.read_attributes()
    want["field"] = w.sample_attribute_points(q, density=True)
    w.close()
    assert want["counts"].min() > 10 and want["affected"] > n // 2 and not same_bits(want["mixed"], want["painted"])

    def program(s, r):
        out = {}
        assert same_bits(s.read_attributes(), np.zeros((n, 4), F32))
        s.write_attributes(attr)
        active = r != 1  # rank 1 only contributes: it asks for no output, and keeps its replica current
        out["counts"] = s.paint_attributes(to_ws(ws, brushes), counts=active)
        out["painted"] = s.read_attributes()
        # ranks given different brushes, then one rank given a bad one, then different arrays: all refuse, nothing changes
        mine = to_ws(ws, [dict(brushes[0], strength=0.25 + 0.125 * r)])
        k = np.full(1, 7, np.uint32)
        assert s._L.ws_paint_attributes(s._h, C.byref((ws.fluid.WsBrush * 1)(*mine)), 1, k.ctypes.data) == 1 and k[0] == 7
        bad = to_ws(ws, [dict(brushes[0], radius=-1.0 if r == world - 1 else 1.0)])
        assert s._L.ws_paint_attributes(s._h, C.byref((ws.fluid.WsBrush * 1)(*bad)), 1, None) == 1
        p = dparams(ws, iterations=1 + r)
        assert s._L.ws_diffuse_attributes(s._h, C.byref(p), DT, None) == 1
        other = attr + F32(r)
        assert s._L.ws_write_attributes(s._h, other.ctypes.data) == 1
        out["unchanged"] = s.read_attributes()
        out["affected"] = s.diffuse_attributes(dparams(ws, iterations=5), DT, count=active)
        out["mixed"] = s.read_attributes()
        out["field"] = s.sample_attribute_points(q, density=True, want=active)
        return out

    got = _slab_run(ws, params, pos, world, GRID_STEPS, program)
    for r in range(world):
        g = got[r]
        if r == 1:
            assert g["counts"] is None and g["affected"] is None and g["field"] == (None, None)
        else:
            assert np.array_equal(g["counts"], want["counts"]) and g["affected"] == want["affected"], r
            assert same_bits(g["field"][0], want["field"][0]) and same_bits(g["field"][1], want["field"][1]), r
        assert same_bits(g["painted"], want["painted"]) and same_bits(g["unchanged"], want["painted"]), r
        assert same_bits(g["mixed"], want["mixed"]), r


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    for x in (w, fresh):
        x.run(5)
    L, h = w._L, w._h
    n = len(pos)
    attr = random_attr(n, 2)
    w.write_attributes(attr)
    good = dict(kind=0, centre=(0.0, 0.0, 0.0), radius=1.0, value=(1.0, 1.0, 1.0, 1.0), strength=0.5, falloff=0.5, channels=15)
    cnt = np.full(16, 7, np.uint32)

    def paint(k=1, null=False, **fields):
        b = dict(good, **fields)
        arr = (ws.fluid.WsBrush * 16)(*([ws.fluid.brush(good["kind"], good["centre"], good["radius"], good["value"], good["strength"],
                                                        good["falloff"], good["channels"])] * 15
                                        + [ws.fluid.WsBrush(b["kind"], (C.c_float * 3)(*b["centre"]), b["radius"], b["falloff"],
                                                            b["strength"], b["channels"], (C.c_float * 4)(*b["value"]))]))
        # (the brush under test is the LAST of k: the ones before it are good)
        first = 16 - k if 1 <= k <= 16 else 0
        ptr = None if null else C.byref(arr, first * C.sizeof(ws.fluid.WsBrush))
        return L.ws_paint_attributes(h, ptr, k, cnt.ctypes.data)

    def diffuse(dt=0.01, null=False, rate=(1.0, 1.0, 1.0, 1.0), iterations=1, reserved=0):
        p = ws.fluid.WsDiffuseParams((C.c_float * 4)(*rate), iterations, reserved)
        k = C.c_uint32(7)
        st = L.ws_diffuse_attributes(h, None if null else C.byref(p), dt, C.byref(k))
        assert st == 0 or k.value == 7
        return st

    bad_paint = [("NULL b", dict(null=True)), ("k = 0", dict(k=0)), ("k = 17", dict(k=17)), ("kind 2", dict(kind=2)),
                 ("channels 0", dict(channels=0)), ("channels 16", dict(channels=16)), ("radius 0", dict(radius=0.0)),
                 ("radius < 0", dict(radius=-1.0)), ("falloff < 0", dict(falloff=-0.01)), ("falloff > 1", dict(falloff=1.01)),
                 ("MIX strength < 0", dict(strength=-0.01)), ("MIX strength > 1", dict(strength=1.01)),
                 ("third of three", dict(k=3, radius=0.0))]
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        for name in ("radius", "falloff", "strength"):
            bad_paint.append(("%s %r" % (name, val), {name: val, "kind": 1}))
        bad_paint.append(("centre %r" % val, dict(centre=(0.0, val, 0.0))))
        bad_paint.append(("value %r" % val, dict(value=(0.0, 0.0, 0.0, val))))
    bad_diffuse = [("NULL p", dict(null=True)), ("reserved", dict(reserved=1)), ("iterations 0", dict(iterations=0)),
                   ("iterations 65", dict(iterations=65)), ("rate < 0", dict(rate=(1.0, -0.01, 1.0, 1.0))),
                   ("r > 0.5", dict(rate=(1.0, 1.0, 1.0, 50.1))), ("r > 0.5 by dt", dict(dt=0.51))]
    for val in (np.nan, np.inf, -np.inf, 2e15):
        bad_diffuse.append(("rate %r" % val, dict(rate=(val, 1.0, 1.0, 1.0))))
    for val in (np.nan, np.inf, -np.inf, 0.0, -0.01):
        bad_diffuse.append(("dt %r" % val, dict(dt=val)))
    steps = 5
    for call, cases in ((paint, bad_paint), (diffuse, bad_diffuse)):
        for what, kw in cases:
            assert call(**kw) == 1 and np.all(cnt == 7), what
            w.run(1)  # ... followed by a good step
            steps += 1
    assert L.ws_read_attributes(h, None) == 1
    out = np.full((4, 4), 7.0, F32)
    q = np.zeros((4, 3), F32)
    dims = np.array([2, 2, 1], np.uint32)
    one = np.ones(3, F32)
    assert L.ws_sample_attribute_points(h, q.ctypes.data, 4, None, None) == 1  # both outputs NULL
    assert L.ws_sample_attribute_points(h, None, 4, out.ctypes.data, None) == 1
    assert L.ws_sample_attribute_points(h, q.ctypes.data, 0, out.ctypes.data, None) == 1
    q[2, 1] = np.nan
    assert L.ws_sample_attribute_points(h, q.ctypes.data, 4, out.ctypes.data, None) == 1
    assert L.ws_sample_attribute_grid(h, one.ctypes.data, one.ctypes.data, dims.ctypes.data, None, None) == 1
    assert L.ws_sample_attribute_grid(h, None, one.ctypes.data, dims.ctypes.data, out.ctypes.data, None) == 1
    none = np.zeros(3, F32)
    assert L.ws_sample_attribute_grid(h, one.ctypes.data, none.ctypes.data, dims.ctypes.data, out.ctypes.data, None) == 1
    dims[2] = 0
    assert L.ws_sample_attribute_grid(h, one.ctypes.data, one.ctypes.data, dims.ctypes.data, out.ctypes.data, None) == 1
    assert np.all(out == 7.0)
    # nothing was touched: the attributes, and the state against a handle that made no call
    assert same_bits(w.read_attributes(), attr)
    fresh.run(steps - 5)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # allowed: the limits themselves
    assert paint(falloff=0.0) == 0 and paint(falloff=1.0, strength=1.0) == 0 and paint(strength=0.0) == 0 and np.all(cnt[1:] == 7)
    assert paint(kind=1, strength=-1e15) == 0 and paint(k=16) == 0 and paint(channels=1) == 0
    assert diffuse(rate=(50.0, 0.0, 0.0, 0.0)) == 0 and diffuse(iterations=64, rate=(0.0, 0.0, 0.0, 1e-3)) == 0
    assert diffuse(dt=0.5) == 0
    w.run(2)
    w.close()
    fresh.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    b = to_ws(ws, [At.brush("mix", (0.0, 0.0, 0.0), 1.0, (1.0, 1.0, 1.0, 1.0))])
    for call in (lambda: w.write_attributes(None), lambda: w.read_attributes(), lambda: w.paint_attributes(b),
                 lambda: w.diffuse_attributes(dparams(ws), 0.01), lambda: w.sample_attribute_points(pos[:4]),
                 lambda: w.sample_attribute_grid((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2, 2, 2))):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 6
    w.run(2)
    w.close()
