"""ws_add_particles, ws_remove_particles and ws_remove_particle_ids on the GPU.  Every comparison is bit for bit: the
handle's contents after each call against the numpy restatement (tests/population_ref.py), and the steps that follow
against a SHADOW -- a fresh handle created at the new count and loaded with the records the changed handle reports.
Sizes sit where the kernels can go wrong: one and two particles, either side of a wave, a power-of-two count flipping the
hash-alias path, several scan tiles with a ragged tail, the tile schedule's threshold crossed in both directions."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as F
import population_ref as P
from test_gpu_aniso_surface import same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID_ARG, UNSUPPORTED = 1, 6
STEP_KERNELS = ("cell_scan", "cell_scatter", "reorder", "density", "force_integrate_bin")  # test_gpu_profile.py's


def _xyz(rec, field):
    return np.ascontiguousarray(rec[field][:, :3])


def _state(w):
    """(pos, vel, attr) by id, as the restatement takes it."""
    rec = w.read_vec("particles")
    return _xyz(rec, "position"), _xyz(rec, "velocity"), w.read_attributes()


def _same_state(got, want):
    return all(same_bits(g, x) for g, x in zip(got, want))


def _bytes(w):
    """Everything the views show: the 80-byte records (all six fields) and the three arrays of the sort view."""
    return (w.read_vec("particles").tobytes(),) + tuple(a.tobytes() for a in w.sort_view())


def _probe(params, m=65, seed=77):
    lo, hi = np.asarray(params.ext_min[:3], F32), np.asarray(params.ext_max[:3], F32)
    return (lo + np.random.default_rng(seed).random((m, 3)).astype(F32) * (hi - lo)).astype(F32)


def _after_a_change(w, want):
    """The handle right after a count change: the restatement's contents, every predicted position from the library's
    own rule, the last step's fields gone as after ws_write_particles."""
    rec = w.read_vec("particles")
    assert w.n == len(want[0]) == rec.shape[0]
    assert _same_state((_xyz(rec, "position"), _xyz(rec, "velocity"), w.read_attributes()), want)
    assert same_bits(_xyz(rec, "predicted_position"), P.predicted(want))
    for field in ("density", "pressure", "acceleration"):
        assert not rec[field].any(), field
    keys, perm, off = w.sort_view()
    assert np.array_equal(keys, np.arange(w.n)) and np.array_equal(perm, keys) and np.array_equal(off, keys)


def _shadow(ws, w, steps=3, **kw):
    """A fresh handle at w's count, loaded with w's records and attributes; `steps` steps on both; identical bits in every
    field, identical attributes, and the density field at 65 points identical (the field scratch's particle count)."""
    rec = w.read_vec("particles")
    s = ws.FluidWorker(_xyz(rec, "position"), w.params, **kw)
    try:
        s.write_slice("particles", rec)
        s.write_attributes(w.read_attributes())
        q = _probe(w.params)
        assert same_bits(w.sample_density_points(q), s.sample_density_points(q))
        w.run(steps)
        s.run(steps)
        a, b = w.read_vec("particles"), s.read_vec("particles")
        assert a.tobytes() == b.tobytes()
        assert a["density"][:, 0].any() or w.n == 1
        assert same_bits(w.sample_density_points(q), s.sample_density_points(q))
        assert same_bits(w.read_attributes(), s.read_attributes())
        assert all(np.array_equal(x, y) for x, y in zip(w.sort_view(), s.sort_view()))
    finally:
        s.close()


def _lattice(ws, ni, nj, nk):
    return ws.cube_fluid(ni, nj, nk), ws.make_params(container_size=(4.0, 4.0, 4.0))


def _cloud(ws, n, seed, size=(16.0, 9.0, 9.0)):
    params = ws.make_params(container_size=size)
    return ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max)), params


def _attrs(n, seed):
    a = np.random.default_rng(seed).uniform(0.0, 1.0, (n, 4)).astype(F32)
    a[::3, 1] = F32(-0.0)
    return a


def _moving(w, seed):
    """A few steps and random velocities' worth of history: the records are no longer what ws_create wrote."""
    w.write_attributes(_attrs(w.n, seed))
    w.run(2)


def _slab_sinks(params, frac, k):
    """k boxes side by side that together cover the low `frac` of the container along x (each claims its own share)."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    width = (hi[0] - lo[0]) * frac / k
    mid, half = (lo + hi) / 2, (hi - lo) / 2 + 1.0
    return [P.sink(P.BOX, (lo[0] + (e + 0.5) * width, mid[1], mid[2]), (width / 2, half[1], half[2])) for e in range(k)]


# ---- 1. contents and shadow at the sizes where the kernels can go wrong ---------------------------------------------------------
def _remove_ids_case(ws, w, ids):
    before = _state(w)
    want, want_new = P.remove(before, P.keep_of_ids(w.n, ids))
    new = w.remove_particle_ids(ids)
    assert np.array_equal(new, want_new)
    _after_a_change(w, want)
    _shadow(ws, w)


def _add_case(ws, w, pos, vel=None, attr=None):
    want = P.add(_state(w), pos, vel, attr)
    assert w.add_particles(pos, vel, attr) == len(want[0])
    _after_a_change(w, want)
    _shadow(ws, w)


def _sinks_case(ws, w, sinks):
    before = _state(w)
    want, want_counts, want_new = P.remove_by_sinks(before, sinks)
    counts, new = w.remove_particles(P.to_ws(ws, sinks))
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    assert np.array_equal(new, want_new)
    _after_a_change(w, want)
    _shadow(ws, w)
    return counts


def test_two_particles_to_one_and_back(ws):
    pos, params = _lattice(ws, 2, 1, 1)
    w = ws.FluidWorker(pos, params)
    _moving(w, 1)
    _remove_ids_case(ws, w, [0])
    assert w.n == 1
    _add_case(ws, w, pos[:1] + F32(0.01), vel=[(0.5, 0.0, -0.5)], attr=[(1.0, 2.0, 3.0, 4.0)])
    assert w.n == 2
    w.close()


def test_either_side_of_a_wave(ws):
    pos, params = _lattice(ws, 5, 13, 1)
    w = ws.FluidWorker(pos, params)
    _moving(w, 2)
    _remove_ids_case(ws, w, [64, 3])
    assert w.n == 63
    _add_case(ws, w, pos[[3, 64]], attr=_attrs(2, 9))
    assert w.n == 65
    w.close()


def test_a_power_of_two_count_flips_the_alias_path(ws):
    pos, params = _lattice(ws, 16, 16, 16)
    w = ws.FluidWorker(pos, params)
    _moving(w, 3)
    _add_case(ws, w, [(0.05, 0.05, 0.05)], vel=[(0.0, 1.0, 0.0)])
    assert w.n == 4097
    _remove_ids_case(ws, w, [1234])
    assert w.n == 4096
    w.close()


def test_several_scan_tiles_with_a_ragged_tail(ws):
    pos, params = _cloud(ws, 70001, 5)
    w = ws.FluidWorker(pos, params)
    _moving(w, 4)
    sinks = _slab_sinks(params, 0.01, 15) + [P.sink(P.SPHERE, (0.0, 0.0, 0.0), 1.5)]
    counts = _sinks_case(ws, w, sinks)
    assert (counts > 0).all() and 500 < counts.sum() < 70001
    gone = 70001 - w.n
    _add_case(ws, w, pos[:gone], vel=np.full((gone, 3), 0.25, F32), attr=_attrs(gone, 11))
    assert w.n == 70001
    w.close()


def test_the_schedule_threshold_is_crossed_down_and_back(ws):
    """300 001 particles: the tile schedule drives K4 / K5 (2^18 <= n < 2^20).  Draining the low 15 % of the container
    takes the count below 2^18 -- the schedule is dropped -- and pouring the particles back rebuilds it."""
    pos, params = _cloud(ws, 300001, 6)
    w = ws.FluidWorker(pos, params)
    _moving(w, 5)
    assert w.stats()["tile_schedule"]
    counts = _sinks_case(ws, w, _slab_sinks(params, 0.15, 16))
    assert w.n < (1 << 18) and (counts > 0).all() and not w.stats()["tile_schedule"]
    gone = 300001 - w.n
    _add_case(ws, w, pos[:gone], attr=_attrs(gone, 12))
    assert w.n == 300001 and w.stats()["tile_schedule"]
    w.close()


# ---- 2. removal extremes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all-but-one", "first-and-last", "a-range", "every-second"])
def test_removal_extremes(ws, which):
    n = 4097
    pos, params = _cloud(ws, n, 21, size=(4.0, 4.0, 4.0))
    ids = {"all-but-one": np.delete(np.arange(n), 2049), "first-and-last": np.array([0, n - 1]),
           "a-range": np.arange(1000, 3100), "every-second": np.arange(0, n, 2)}[which]
    w = ws.FluidWorker(pos, params)
    _moving(w, 6)
    _remove_ids_case(ws, w, ids)
    assert w.n == n - len(ids)
    w.close()


# ---- 3. no-ops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_no_ops_leave_the_handle_exactly_as_it_was(ws, graph):
    pos, params = _cloud(ws, 4097, 22, size=(4.0, 4.0, 4.0))
    w, twin = (ws.FluidWorker(pos, params, graph=graph) for _ in range(2))  # the twin makes every call but the no-ops
    for x in (w, twin):
        _moving(x, 7)
        x.run(1)
    before, attr = _bytes(w), w.read_attributes()
    assert _bytes(twin) == before and w.read_vec("particles")["density"].any()
    replayed = w.stats()["graph_steps"]
    assert replayed == (2 if graph else 0)  # the first step after the load is launched directly
    assert w.add_particles(np.zeros((0, 3), F32)) == 4097
    new = w.remove_particle_ids(np.zeros(0, np.uint32))
    assert np.array_equal(new, np.arange(4097))
    far = [P.sink(P.SPHERE, (100.0, 100.0, 100.0), 1.0), P.sink(P.BOX, (-50.0, 0.0, 0.0), (1.0, 1.0, 1.0))]
    counts, new = w.remove_particles(P.to_ws(ws, far))
    assert list(counts) == [0, 0] and np.array_equal(new, np.arange(4097))
    assert _bytes(w) == before and same_bits(w.read_attributes(), attr)
    assert w.n == 4097 and w.steps_done() == 3 and w.capacity() == 4097
    w.run(3)
    twin.run(3)
    # the captured step is still the one replayed (a step that follows a read of the records is launched directly, on
    # either handle), and the steps are the steps of a handle nobody called
    assert w.stats()["graph_steps"] == twin.stats()["graph_steps"] == (replayed + 2 if graph else 0)
    assert _bytes(twin) == _bytes(w)
    twin.close()
    w.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(ws):
    pos, params = _cloud(ws, 4097, 23, size=(4.0, 4.0, 4.0))
    w = ws.FluidWorker(pos, params)
    _moving(w, 8)
    before = _bytes(w)
    everything = [P.sink(P.BOX, (0.0, 0.0, 0.0), (10.0, 10.0, 10.0))]
    L, h = w._L, w._h
    counts, ids = np.full(16, 7, np.uint32), np.full(4097, 7, np.uint32)

    def refused(call, status=INVALID_ARG):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert w.n == 4097 == L.ws_num_particles(h) and _bytes(w) == before

    arr = (ws.fluid.WsSink * 1)(*P.to_ws(ws, everything))
    refused(lambda: w._check(L.ws_remove_particles(h, C.byref(arr), 1, counts.ctypes.data, ids.ctypes.data)))
    assert np.all(counts == 7) and np.all(ids == 7)  # emptying: decided after the scan, the outputs untouched
    refused(lambda: w.remove_particle_ids(np.arange(4097)))
    refused(lambda: w.remove_particle_ids([5, 4097]))
    refused(lambda: w.remove_particle_ids([0xFFFFFFFF]))
    bad = np.zeros((3, 3), F32)
    bad[1, 2] = np.nan
    refused(lambda: w.add_particles(bad))
    refused(lambda: w.add_particles(np.zeros((3, 3), F32), velocities=bad))
    refused(lambda: w.add_particles(np.zeros((3, 3), F32), attributes=np.full((3, 4), np.inf, F32)))
    refused(lambda: w.remove_particles([ws.fluid.sink("box", (0, 0, 0), (1.0, 0.0, 1.0))]))
    refused(lambda: w.remove_particles([ws.fluid.sink("sphere", (0, 0, 0), (1.0, 1.0, 0.0))]))
    refused(lambda: w.remove_particles([]))
    refused(lambda: w.remove_particles([ws.fluid.sink("sphere", (0, 0, 0), 1.0)] * 17))
    # a readback in flight: every count-changing call waits for ws_read_positions_end
    buf = np.empty((4097, 3), F32)
    w.read_positions_begin(buf)
    for call in (lambda: w.add_particles(pos[:2]), lambda: w.remove_particle_ids([1]),
                 lambda: w.remove_particles(P.to_ws(ws, everything[:1])), lambda: w.reserve(9000)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == INVALID_ARG and w.n == 4097 == L.ws_num_particles(h)
    w.read_positions_end()
    assert _bytes(w) == before and w.capacity() == 4097
    assert same_bits(buf, _xyz(w.read_vec("particles"), "position"))
    _remove_ids_case(ws, w, [1])  # ... and after it they work
    w.close()


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------------
def test_capacity(ws):
    n = 4097
    pos, params = _cloud(ws, n, 24, size=(4.0, 4.0, 4.0))
    w = ws.FluidWorker(pos, params)
    _moving(w, 9)
    assert w.capacity() == n
    before, attr = _bytes(w), w.read_attributes()
    w.reserve(2 * n)
    assert w.capacity() == 2 * n and w.n == n
    assert _bytes(w) == before and same_bits(w.read_attributes(), attr)  # the last step's views included
    w.reserve(n)  # never lowered
    assert w.capacity() == 2 * n
    twin = ws.FluidWorker(pos, params)
    _moving(twin, 9)
    w.run(2)
    twin.run(2)
    assert _bytes(w) == _bytes(twin)  # ... and the steps of the larger arrays are the steps
    twin.close()
    extra, _ = _cloud(ws, 2 * n, 25, size=(4.0, 4.0, 4.0))
    _add_case(ws, w, extra[:1000], attr=_attrs(1000, 13))
    _add_case(ws, w, extra[1000:n])
    assert w.n == 2 * n == w.capacity()
    _remove_ids_case(ws, w, np.arange(10, 500))
    assert w.capacity() == 2 * n  # a removal never shrinks
    now = w.n
    _add_case(ws, w, extra[n:n + 1500], vel=np.full((1500, 3), -0.125, F32))  # beyond: grows to n' + n' / 2
    assert w.n == now + 1500 and w.capacity() == w.n + w.n // 2
    # a handle that never had attributes gets them with the first addition that carries some
    bare = ws.FluidWorker(pos[:63], params)
    bare.run(1)
    rec = bare.read_vec("particles")
    before = (_xyz(rec, "position"), _xyz(rec, "velocity"), np.zeros((63, 4), F32))  # (no attribute call so far)
    want = P.add(before, extra[:70], attr=_attrs(70, 14))
    assert bare.add_particles(extra[:70], attributes=_attrs(70, 14)) == 133 and bare.capacity() == 133 + 66
    _after_a_change(bare, want)
    _shadow(ws, bare)
    bare.close()
    w.close()


# ---- 6. handle flavours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["graph", "profile", "ieee_division"])
def test_the_shadow_on_every_flavour_of_handle(ws, flavour):
    kw = {flavour: True}
    pos, params = _cloud(ws, 4097, 26, size=(4.0, 4.0, 4.0))
    w = ws.FluidWorker(pos, params, **kw)
    _moving(w, 10)
    if flavour == "profile":
        stepped = lambda k, b: dict({name: k for name in STEP_KERNELS}, bin=b)  # noqa: E731
        counts = lambda: {k: c for k, (_, c) in w.profile().items()}  # noqa: E731
        assert counts() == stepped(2, 1)  # ws_create's binning
    sinks = [P.sink(P.SPHERE, (0.5, 0.0, 0.0), 1.0), P.sink(P.BOX, (-1.0, -1.0, 0.0), (0.5, 0.5, 2.5))]
    before = _state(w)
    want, want_counts, want_new = P.remove_by_sinks(before, sinks)
    got_counts, new = w.remove_particles(P.to_ws(ws, sinks))
    assert np.array_equal(got_counts, want_counts) and np.array_equal(new, want_new) and (got_counts > 0).all()
    if flavour == "profile":
        assert counts() == stepped(2, 2)  # a count change bins once, as a write does
    _after_a_change(w, want)
    _shadow(ws, w, **kw)
    if flavour == "profile":
        assert counts() == stepped(5, 2)  # and a step after it launches what a step launches
    if flavour == "graph":
        assert w.stats()["graph_steps"] >= 1 + 2  # captured again and replayed (but for a step that follows a read)
    want = P.add(_state(w), pos[:300], attr=_attrs(300, 15))
    w.add_particles(pos[:300], attributes=_attrs(300, 15))
    if flavour == "profile":
        assert counts() == stepped(5, 3)
    _after_a_change(w, want)
    _shadow(ws, w, **kw)
    if flavour == "profile":
        assert counts() == stepped(8, 3)
    w.close()


# ---- 7. a seeded sequence of every kind of call against the restatement and a shadow -----------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_a_seeded_sequence_against_a_shadow_rebuilt_at_every_count_change(ws, seed):
    rng = np.random.default_rng(1000 + seed)
    size = (4.0, 4.0, 4.0)
    pos, params = _cloud(ws, 4097, 30 + seed, size=size)
    pool, _ = _cloud(ws, 4000, 40 + seed, size=size)
    regrids = [ws.make_params(container_size=size, smoothing_radius=F32(0.2)), ws.make_params(container_size=size)]
    w = ws.FluidWorker(pos, params)
    w.write_attributes(_attrs(4097, seed))
    box = {"s": None}

    def rebuild():
        if box["s"] is not None:
            box["s"].close()
        rec = w.read_vec("particles")
        s = ws.FluidWorker(_xyz(rec, "position"), w.params)
        s.write_slice("particles", rec)
        s.write_attributes(w.read_attributes())
        box["s"] = s

    def both(call):
        a, b = call(w), call(box["s"])
        return a, b

    rebuild()
    ops = ["add", "sink", "ids", "step", "step", "forces", "regrid", "paint", "field"]
    done = {op: 0 for op in ops}
    script = list(rng.permutation(ops * 4))[:30]
    taken = 0
    for t, op in enumerate(script):
        done[op] += 1
        if op == "add":
            m = int(rng.integers(1, 400))
            new = pool[taken:taken + m]
            taken += m
            vel = rng.normal(0.0, 0.5, (m, 3)).astype(F32) if t % 2 else None
            att = _attrs(m, t) if t % 3 else None
            want = P.add(_state(w), new, vel, att)
            w.add_particles(new, vel, att)
            _after_a_change(w, want)
            rebuild()
        elif op == "sink":
            c = rng.uniform(-1.5, 1.5, 3)
            sinks = [P.sink(P.SPHERE, c, rng.uniform(0.3, 0.8)), P.sink(P.BOX, c + 0.3, rng.uniform(0.2, 0.6, 3))]
            before = _state(w)
            want, want_counts, want_new = P.remove_by_sinks(before, sinks)
            counts, new = w.remove_particles(P.to_ws(ws, sinks))
            assert np.array_equal(counts, want_counts) and np.array_equal(new, want_new), t
            if counts.sum():
                _after_a_change(w, want)
                rebuild()
        elif op == "ids":
            ids = rng.integers(0, w.n, int(rng.integers(1, 200)))
            before = _state(w)
            want, want_new = P.remove(before, P.keep_of_ids(w.n, ids))
            assert np.array_equal(w.remove_particle_ids(ids), want_new), t
            _after_a_change(w, want)
            rebuild()
        elif op == "step":
            both(lambda x: x.run(1))
        elif op == "forces":
            f = [F.emitter(F.VORTEX, rng.uniform(-1, 1, 3), 1.5, 8.0, axis=(0.0, 1.0, 0.0), damping=0.5),
                 F.emitter(F.RADIAL, rng.uniform(-1, 1, 3), 1.0, -6.0)]
            a, b = both(lambda x: x.apply_forces(F.to_ws(ws, f), F32(1.0 / 60.0)))
            assert np.array_equal(a, b), t
        elif op == "regrid":
            p = regrids[(done[op] - 1) % 2]
            both(lambda x: x.set_params(p))
        elif op == "paint":
            br = [ws.fluid.brush("mix", rng.uniform(-1, 1, 3), 1.2, (1.0, 0.5, 0.25, 0.0), strength=0.5, falloff=0.5)]
            a, b = both(lambda x: x.paint_attributes(br))
            assert np.array_equal(a, b), t
        else:
            q = _probe(w.params, seed=t)
            a, b = both(lambda x: x.sample_density_points(q))
            assert same_bits(a, b), t
        s = box["s"]
        assert w.n == s.n and w.read_vec("particles").tobytes() == s.read_vec("particles").tobytes(), (t, op)
        assert same_bits(w.read_attributes(), s.read_attributes()), (t, op)
    assert all(done[op] >= 2 for op in ops), done
    both(lambda x: x.run(3))
    assert w.read_vec("particles").tobytes() == box["s"].read_vec("particles").tobytes()
    box["s"].close()
    w.close()


# ---- 8. handles that keep their count -------------------------------------------------------------------------------------------
def test_a_slab_handle_refuses(ws):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0))
    pos = ws.workloads.uniform_cloud(4096, 50, list(params.ext_min), list(params.ext_max))
    hub = ws.slab.LoopbackHub(1)
    s = ws.slab.SlabWorker(pos, np.arange(4096, dtype=np.uint32), 4096, params, 0, 1, hub.transport(0))
    s.run(2)
    L, h = s._L, s._h
    sink = ws.fluid.sink("sphere", (0, 0, 0), 1.0)
    ids = np.zeros(1, np.uint32)
    assert L.ws_add_particles(h, pos.ctypes.data, None, None, 1) == UNSUPPORTED
    assert L.ws_remove_particles(h, C.byref(sink), 1, None, None) == UNSUPPORTED
    assert L.ws_remove_particle_ids(h, ids.ctypes.data, 1, None) == UNSUPPORTED
    assert L.ws_reserve_particles(h, 8192) == UNSUPPORTED
    assert b"slab" in L.ws_last_error(h)
    assert L.ws_particle_capacity(h) >= 4096  # answers on every handle
    s.run(2)
    assert s.num_owned() == 4096
    s.close()
