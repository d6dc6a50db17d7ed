"""ws_measure and ws_select_particles on the GPU.  Every comparison is bit for bit: every field of every gauge and the id
list against the numpy restatement (tests/gauges_ref.py), and a handle that measures and selects between its steps
against a shadow that does not.  Sizes sit where the kernels can go wrong: one particle, either side of a wave and of a
workgroup, either side of the particles one workgroup of the reduction takes, several scan tiles with a ragged tail and
many workgroups meeting in the atomics."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gauges_ref as G
from test_gpu_aniso_surface import _slab_run, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID_ARG, HIP, UNSUPPORTED = 1, 4, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    """Particles per workgroup of the reduction kernel, from its source: WS_BLOCK x GAUGE_ITEMS."""
    csrc = os.path.join(ROOT, "water-sandbox_amd", "csrc")
    items = int(re.search(r"^#define GAUGE_ITEMS (\d+)u", open(os.path.join(csrc, "ws_gauges.hip")).read(), flags=re.M).group(1))
    block = int(re.search(r"^#define WS_BLOCK (\d+)", open(os.path.join(csrc, "ws_device.h")).read(), flags=re.M).group(1))
    return items * block


TILE = _tile()
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, 1000, 4097, TILE - 1, TILE, TILE + 1, 70001})


def _xyz(rec, field):
    return np.ascontiguousarray(rec[field][:, :3])


def _cloud(ws, n, seed):
    size = (4.0, 4.0, 4.0) if n <= 5000 else (16.0, 9.0, 9.0)
    params = ws.make_params(container_size=size)
    return ws.workloads.uniform_cloud(n, seed, list(params.ext_min), list(params.ext_max)), params


def _attrs(n, seed):
    a = np.random.default_rng(seed).uniform(0.0, 1.0, (n, 4)).astype(F32)
    a[::3, 1] = F32(-0.0)
    return a


def _regions(params, seed=5):
    """16 regions over the container: spheres and boxes that overlap one another, one that is empty (far outside), one
    that is everything (half 1e15), one thin slab and one small ball."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    mid, ext = (lo + hi) / 2, hi - lo
    rng = np.random.default_rng(seed)
    out = [G.region(G.BOX, mid, (1e15, 1e15, 1e15)), G.region(G.SPHERE, hi + 50.0, 1.0),
           G.region(G.BOX, (mid[0], lo[1] + 0.05 * ext[1], mid[2]), (ext[0], 0.05 * ext[1], ext[2])),
           G.region(G.SPHERE, mid, 0.04 * ext.min())]
    while len(out) < 16:
        c = lo + rng.random(3) * ext
        if len(out) % 2:
            out.append(G.region(G.SPHERE, c, rng.uniform(0.15, 0.45) * ext.min()))
        else:
            out.append(G.region(G.BOX, c, rng.uniform(0.1, 0.4, 3) * ext))
    return out


def _disjoint(params):
    """Three regions no two of which share a particle: the low quarter along x, a box in the high half, a ball between."""
    lo, hi = np.asarray(params.ext_min[:3], np.float64), np.asarray(params.ext_max[:3], np.float64)
    mid, ext = (lo + hi) / 2, hi - lo
    return [G.region(G.BOX, (lo[0], mid[1], mid[2]), (0.25 * ext[0], ext[1], ext[2])),
            G.region(G.BOX, (lo[0] + 0.8 * ext[0], mid[1], mid[2]), (0.1 * ext[0], 0.3 * ext[1], 0.3 * ext[2])),
            G.region(G.SPHERE, (lo[0] + 0.5 * ext[0], mid[1], mid[2]), 0.15 * ext[0])]


def _worker(ws, n, seed, attributes=True, steps=3, **kw):
    """A handle with a few steps of history: `cur` is in the last step's cell order, not in id order."""
    pos, params = _cloud(ws, n, seed)
    w = ws.FluidWorker(pos, params, **kw)
    if attributes:
        w.write_attributes(_attrs(n, seed))
    w.run(steps)
    return w


def _state(w):
    rec = w.read_vec("particles")
    return _xyz(rec, "position"), _xyz(rec, "velocity")


def _bytes(w):
    """Everything the views show: the 80-byte records (all six fields) and the three arrays of the sort view."""
    return (w.read_vec("particles").tobytes(),) + tuple(a.tobytes() for a in w.sort_view())


def _measured(ws, w, regions, attr):
    """Both forms of the call against the restatement, every field of every gauge.  attr: the handle's attributes or None."""
    pos, vel = _state(w)
    arr = G.to_ws(ws, regions)
    for flag in (False, True):
        got = w.measure(arr, attributes=flag)
        want = G.measure(pos, vel, regions, attr if flag else None)
        assert G.same(got, want) == [], (flag, G.same(got, want))
    return want


# ---- 1. bits against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_every_field_of_16_mixed_gauges_is_the_restatements(ws, n):
    w = _worker(ws, n, 100 + n % 97)
    regions = _regions(w.params)
    want = _measured(ws, w, regions, w.read_attributes())
    assert want["count"][0] == n and want["count"][1] == 0  # everything, and nothing
    if n >= 1000:
        assert np.count_nonzero(want["count"]) >= 14 and want["sum_attr"].any() and want["sum_ang"].any()
    one = w.measure(G.to_ws(ws, regions[:1]), attributes=True)  # k = 1 is the same gauge
    assert G.same(one, {name: v[:1] for name, v in want.items()}) == []
    w.close()


def test_a_handle_without_attributes_sums_none(ws):
    w = _worker(ws, 257, 7, attributes=False)
    regions = _regions(w.params)
    want = _measured(ws, w, regions, None)  # with the flag too: sum_attr stays 0
    assert not want["sum_attr"].any() and want["count"][0] == 257
    w.close()


# ---- 2. read-only ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["profile", "graph", "ieee_division"])
def test_neither_call_changes_anything_and_the_steps_between_them_are_the_steps(ws, flavour):
    n = 4097
    w, shadow = (_worker(ws, n, 31, **{flavour: True}) for _ in range(2))
    regions = G.to_ws(ws, _regions(w.params))
    before, stats = _bytes(w), w.stats()
    assert _bytes(shadow) == before
    counts = lambda x: {k: c for k, (_, c) in x.profile().items()}  # noqa: E731
    launched = counts(w) if flavour == "profile" else None
    assert launched is None or launched["density"] == 3
    for flag in (False, True):
        w.measure(regions, attributes=flag)
    ids, total = w.select_particles(regions[2:])
    assert 0 < total < n and len(ids) == total
    assert _bytes(w) == before and w.stats() == stats and w.steps_done() == 3 and w.n == n
    assert launched is None or counts(w) == launched  # no launch is counted under any kernel id
    replayed = w.stats()["graph_steps"]
    for _ in range(5):
        w.run(1)
        shadow.run(1)
        w.measure(regions, attributes=True)
        w.select_particles(regions[2:], cap=100)
    assert w.stats() == shadow.stats() and w.steps_done() == shadow.steps_done() == 8
    if flavour == "graph":
        assert w.stats()["graph_steps"] >= replayed + 4  # the captured step went on being replayed
    if flavour == "profile":
        assert counts(w) == counts(shadow) and counts(w)["density"] == 8
    assert _bytes(w) == _bytes(shadow)
    assert same_bits(w.read_attributes(), shadow.read_attributes())
    shadow.close()
    w.close()


# ---- 3. ws_select_particles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4097, 70001])
def test_the_selected_ids_and_what_removing_them_removes(ws, n):
    w, twin = (_worker(ws, n, 41) for _ in range(2))
    pos, _ = _state(w)
    for regions in (_regions(w.params)[2:], _regions(w.params)[1:2], _disjoint(w.params)):
        want = G.select(pos, regions)
        arr = G.to_ws(ws, regions)
        ids, total = w.select_particles(arr)
        assert total == len(want) and np.array_equal(ids, want)
        none, total0 = w.select_particles(arr, cap=0)  # a count only
        assert total0 == len(want) and none.size == 0
        if len(want) > 1:
            few, total1 = w.select_particles(arr, cap=len(want) // 2)  # a prefix
            assert total1 == len(want) and np.array_equal(few, want[:len(want) // 2])
        more, total2 = w.select_particles(arr, cap=len(want) + 3)
        assert total2 == len(want) and np.array_equal(more, want)
    # the list into ws_remove_particle_ids removes exactly what ws_remove_particles over the same, disjoint, regions reports
    regions = _disjoint(w.params)
    want = G.select(pos, regions)
    assert 0 < len(want) < n
    ids, _ = w.select_particles(G.to_ws(ws, regions))
    new = w.remove_particle_ids(ids)
    removed, twin_new = twin.remove_particles(G.to_ws(ws, regions))
    assert int(removed.sum()) == len(want) == n - w.n and [int(c) for c in removed] == [int(G.contains(pos, s).sum()) for s in regions]
    assert np.array_equal(new, twin_new) and w.n == twin.n
    assert w.read_vec("particles").tobytes() == twin.read_vec("particles").tobytes()
    twin.close()
    w.close()


# ---- 4. between ws_read_positions_begin and _end --------------------------------------------------------------------------------
def test_both_are_allowed_while_a_readback_is_in_flight(ws):
    w = _worker(ws, 4097, 51)
    regions = _regions(w.params)
    pos, vel = _state(w)
    buf = np.empty((4097, 3), F32)
    w.read_positions_begin(buf)
    got = w.measure(G.to_ws(ws, regions), attributes=True)
    ids, total = w.select_particles(G.to_ws(ws, regions[2:]))
    w.read_positions_end()
    assert same_bits(buf, pos)  # the readback keeps its positions
    assert G.same(got, G.measure(pos, vel, regions, w.read_attributes())) == []
    assert np.array_equal(ids, G.select(pos, regions[2:])) and total == len(ids)
    w.close()


# ---- 5. slabs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_every_slab_rank_measures_the_single_handles_bits(ws, world):
    n, steps = 4099, 3
    pos, params = _cloud(ws, 5001, 61)  # (the 16 x 9 x 9 container: enough cell layers for three slabs)
    pos = pos[:n]
    attr = _attrs(n, 61)
    regions = _regions(params)
    w = ws.FluidWorker(pos, params)
    w.write_attributes(attr)
    w.run(steps)
    arr = G.to_ws(ws, regions)
    want = [w.measure(arr, attributes=flag) for flag in (False, True)]
    x, v = _state(w)
    assert G.same(want[1], G.measure(x, v, regions, attr)) == [] and want[1]["count"][0] == n
    w.close()

    def calls(s, r):
        s.write_attributes(attr)
        got = [s.measure(arr, attributes=flag) for flag in (False, True)]
        quiet = s.measure(arr, want=False)  # a rank that only contributes
        # ranks whose regions differ all refuse, and so do all when one rank's arguments are bad
        shifted = G.to_ws(ws, [G.region(G.SPHERE, (float(r), 0.0, 0.0), 1.0)])
        bad = G.to_ws(ws, [G.region(G.SPHERE, (0.0, 0.0, 0.0), 1.0 if r else 0.0)])
        statuses = []
        for these in (shifted, bad):
            with pytest.raises(ws.WsError) as e:
                s.measure(these)
            statuses.append(e.value.status)
        total = C.c_uint32(7)
        one = (ws.fluid.WsSink * 1)(*arr[:1])
        statuses.append(s._L.ws_select_particles(s._h, C.byref(one), 1, 0, None, C.byref(total)))
        assert total.value == 7
        again = s.measure(arr, attributes=True)  # ... and the handle measures on
        return got, quiet, statuses, again

    for got, quiet, statuses, again in _slab_run(ws, params, pos, world, steps, calls):
        assert quiet is None and statuses == [INVALID_ARG, INVALID_ARG, UNSUPPORTED]
        for a, b in zip(got + [again], want + [want[1]]):
            assert G.same(a, b) == [], G.same(a, b)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_handle_steps_on(ws):
    w, twin = (_worker(ws, 4097, 71) for _ in range(2))
    before = _bytes(w)
    L, h = w._L, w._h
    good = ws.fluid.region("sphere", (0.0, 0.0, 0.0), 1.0)
    out = np.full(17 * 152, 7, np.uint8)
    ids = np.full(4097, 7, np.uint32)
    total = C.c_uint32(7)

    def both(regions, k):
        arr = (ws.fluid.WsSink * max(len(regions), 1))(*regions)
        a = L.ws_measure(h, C.byref(arr), k, 0, out.ctypes.data)
        b = L.ws_select_particles(h, C.byref(arr), k, 4097, ids.ctypes.data, C.byref(total))
        assert np.all(out == 7) and np.all(ids == 7) and total.value == 7
        return a, b

    def edited(**fields):
        r = ws.fluid.region("box", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        for name, value in fields.items():
            if isinstance(value, tuple):
                getattr(r, name)[value[0]] = value[1]
            else:
                setattr(r, name, value)
        return [good, r]

    assert both([good], 0) == (INVALID_ARG, INVALID_ARG)
    assert both([good] * 17, 17) == (INVALID_ARG, INVALID_ARG)
    one = (ws.fluid.WsSink * 1)(good)
    for flags in (2, 3, 0x80000000):  # (ws_select_particles takes no flags)
        assert L.ws_measure(h, C.byref(one), 1, flags, out.ctypes.data) == INVALID_ARG and np.all(out == 7), flags
    for fields in (dict(kind=2), dict(reserved=1), dict(centre=(1, float("nan"))), dict(half=(2, 1e16)), dict(half=(0, 0.0)),
                   dict(centre=(0, float("inf"))), dict(half=(1, -1.0))):
        assert both(edited(**fields), 2) == (INVALID_ARG, INVALID_ARG), fields
    ball = ws.fluid.region("sphere", (0.0, 0.0, 0.0), 1.0)
    ball.half[0] = 0.0
    assert both([ball], 1) == (INVALID_ARG, INVALID_ARG)  # radius 0
    ball = ws.fluid.region("sphere", (0.0, 0.0, 0.0), (1.0, 0.5, 0.0))
    assert both([ball], 1) == (INVALID_ARG, INVALID_ARG)
    assert L.ws_measure(h, None, 1, 0, out.ctypes.data) == INVALID_ARG and L.ws_measure(h, C.byref(one), 1, 0, None) == INVALID_ARG
    assert L.ws_select_particles(h, None, 1, 0, None, C.byref(total)) == INVALID_ARG
    assert L.ws_select_particles(h, C.byref(one), 1, 0, None, None) == INVALID_ARG
    assert L.ws_select_particles(h, C.byref(one), 1, 5, None, C.byref(total)) == INVALID_ARG
    assert np.all(out == 7) and np.all(ids == 7) and total.value == 7
    assert b"select" in L.ws_last_error(h)
    assert _bytes(w) == before == _bytes(twin)
    assert L.ws_measure(h, C.byref(one), 1, 0, out.ctypes.data) == 0 and not np.all(out[:152] == 7) and np.all(out[152:] == 7)
    w.run(2)
    twin.run(2)
    assert _bytes(w) == _bytes(twin)
    twin.close()
    w.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    r = ws.fluid.region("sphere", (0, 0, 0), 1.0)
    for call in (lambda: w.measure(r), lambda: w.select_particles(r)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_both_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    r = ws.fluid.region("sphere", (0, 0, 0), 4.0)
    assert w.measure(r)["count"][0] > 0 and w.select_particles(r)[1] > 0
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in (lambda: w.measure(r), lambda: w.select_particles(r)):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == HIP and "unusable" in str(e.value)
    w.close()
