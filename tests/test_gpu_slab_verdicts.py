"""The common verdict of the eight collective calls that validate their arguments on slab handles: ws_apply_forces,
ws_apply_cohesion, ws_collide_solids, ws_collide_volumes, ws_write_attributes, ws_paint_attributes,
ws_diffuse_attributes and ws_measure.  A rank that left such a call early would keep its peers waiting inside the
transport, so every rank refuses or goes on alike.  Pinned here, per call: the status, the words of ws_last_error on
every rank, and the precedence "own argument error, then a refusal elsewhere, then a difference"; that a refused call
changes nothing and writes no output; and that afterwards every rank still makes every call with the single handle's
results.  The expected texts are literals: they are what a host's log shows."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_aniso_surface import _slab_run

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID_ARG = 1
N = 4099  # the smallest set the slab tests use: enough cell layers of the 16 x 9 x 9 container for three slabs
DT = 0.01
SUFFIX = "; nothing was changed"

# kind: (this rank's own argument error for the "bad" variant below, <tag>, <things>, whether the call changes state)
TEXTS = {
    "forces": ("forces: radius must be finite, > 0 and at most 1e15", "forces", "emitters", True),
    "cohesion": ("cohesion: xsph must lie in [0, 1]", "cohesion", "parameters", True),
    "solids": ("solids: a radius or half extent must be > 0", "solids", "solids", True),
    "volumes": ("volumes: margin must be >= 0", "volumes", "poses or volumes", True),
    "write": (None, "attributes", "arguments", True),  # (ws_write_attributes has no invalid argument: NULL is all +0)
    "paint": ("attributes: radius must be > 0", "attributes", "arguments", True),
    "diffuse": ("attributes: iterations must lie in 1 .. 64", "attributes", "arguments", True),
    "measure": ("regions: unknown flag bits", "measure", "regions or flags", False),
}


def _refused(kind):
    _, tag, _, mutates = TEXTS[kind]
    return tag + ": another slab refused its arguments" + (SUFFIX if mutates else "")


def _different(kind):
    _, tag, things, mutates = TEXTS[kind]
    return tag + ": the slabs were given different " + things + (SUFFIX if mutates else "")


# case: (the variant rank r of `world` passes, the text it must report)
CASES = {
    "a": (lambda r, world: "bad" if r == 0 else "good",
          lambda kind, r, world: TEXTS[kind][0] if r == 0 else _refused(kind)),
    "b": (lambda r, world: "other" if r == world - 1 else "good",
          lambda kind, r, world: _different(kind)),
    "c": (lambda r, world: "bad" if r == 0 else "other" if r == world - 1 else "good",  # a refusal outranks a difference
          lambda kind, r, world: TEXTS[kind][0] if r == 0 else _refused(kind)),
}


def _sevens(shape, dtype):
    return np.full(shape, 7, dtype)


def _call(ws, L, h, kind, variant, attr):
    """One call of `kind` with the good arguments, an invalid one ("bad") or valid but different ones ("other"), every
    output pre-filled with 7.  Returns (status, outputs)."""
    fl = ws.fluid
    pick = lambda good, bad, other: {"good": good, "bad": bad, "other": other}[variant]  # noqa: E731
    if kind == "forces":
        arr = (fl.WsForce * 1)(fl.force("radial", (0.0, 0.0, 0.0), pick(5.0, 0.0, 5.0), pick(4.0, 4.0, 6.0)))
        outs = [_sevens(1, np.uint32)]
        return L.ws_apply_forces(h, C.byref(arr), 1, DT, outs[0].ctypes.data), outs
    if kind == "cohesion":
        p = fl.cohesion_params(xsph=pick(0.1, 2.0, 0.25))
        outs = [_sevens(1, np.uint32)]
        return L.ws_apply_cohesion(h, C.byref(p), DT, outs[0].ctypes.data), outs
    if kind in ("solids", "volumes"):
        outs = [_sevens(1, np.uint32), _sevens((1, 3), np.float64), _sevens((1, 3), np.float64)]
        ptrs = [o.ctypes.data for o in outs]
        if kind == "solids":
            arr = (fl.WsSolid * 1)(fl.solid("sphere", (0.0, -2.0, 0.0), pick(2.0, 0.0, 2.0), restitution=pick(0.0, 0.0, 0.5)))
            return L.ws_collide_solids(h, C.byref(arr), 1, *ptrs), outs
        arr = (fl.WsVolumePose * 1)(fl.volume_pose(0, (3.0, 1.0, 0.0), restitution=pick(0.0, 0.0, 0.5), margin=pick(0.0, -1.0, 0.0)))
        return L.ws_collide_volumes(h, C.byref(arr), 1, *ptrs), outs
    if kind == "write":
        values = np.array(attr, dtype=F32, order="C", copy=True)
        if variant == "other":
            values[5, 2] = F32(0.5)
        return L.ws_write_attributes(h, values.ctypes.data), []
    if kind == "paint":
        arr = (fl.WsBrush * 1)(fl.brush("mix", (0.0, 0.0, 0.0), pick(4.0, 0.0, 4.0), (1.0, 0.5, 0.25, 0.0), strength=pick(1.0, 1.0, 0.5)))
        outs = [_sevens(1, np.uint32)]
        return L.ws_paint_attributes(h, C.byref(arr), 1, outs[0].ctypes.data), outs
    if kind == "diffuse":
        p = fl.diffuse_params(iterations=pick(2, 0, 3))
        outs = [_sevens(1, np.uint32)]
        return L.ws_diffuse_attributes(h, C.byref(p), DT, outs[0].ctypes.data), outs
    assert kind == "measure"
    arr = (fl.WsSink * 1)(fl.region("sphere", (0.0, 0.0, 0.0), pick(4.0, 4.0, 2.0)))
    outs = [_sevens(152, np.uint8)]
    return L.ws_measure(h, C.byref(arr), 1, pick(fl.WS_GAUGE_ATTRIBUTES, 2, fl.WS_GAUGE_ATTRIBUTES), outs[0].ctypes.data), outs


def _ball_volume():
    """A ball of radius 1.5 as a signed-distance array on 9^3 nodes."""
    x = np.arange(9, dtype=np.float64) * 0.5 - 2.0
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    return [-2.0, -2.0, -2.0], [0.5, 0.5, 0.5], (np.sqrt(xx * xx + y * y + z * z) - 1.5).astype(F32)


def _state(w):
    """Positions, velocities and attributes by id (on slab handles three collective reads)."""
    return w.read_positions().tobytes(), w.read_velocities().tobytes(), w.read_attributes().tobytes()


def _every_call_once(ws, w, attr):
    """One valid call of each kind; the write first, so that the painted and diffused attributes are what is left."""
    out = []
    for kind in ("write", "measure", "forces", "cohesion", "solids", "volumes", "paint", "diffuse"):
        status, outs = _call(ws, w._L, w._h, kind, "good", np.ascontiguousarray(attr[::-1]))
        out.append((kind, status, [o.tobytes() for o in outs]))
    return out, _state(w)


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_reports_the_common_verdict_in_the_calls_own_words(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0))
    pos = ws.workloads.uniform_cloud(N, 61, list(params.ext_min), list(params.ext_max))
    attr = np.random.default_rng(61).uniform(0.0, 1.0, (N, 4)).astype(F32)
    volume = _ball_volume()

    w = ws.FluidWorker(pos, params)
    w.upload_volume(0, *volume)
    w.write_attributes(attr)
    want_calls, want_state = _every_call_once(ws, w, attr)
    w.close()
    assert all(status == 0 for _, status, _ in want_calls), want_calls
    counts = {kind: int(np.frombuffer(outs[0], np.uint32 if kind != "measure" else np.uint64)[0]) for kind, _, outs in want_calls if outs}
    assert all(counts[kind] > 0 for kind in ("measure", "forces", "solids", "volumes", "paint", "diffuse")), counts

    # an upload frees and allocates device memory, which waits for the whole device: with every rank a thread of this
    # process on one GPU, a rank uploads only while no peer is inside a collective
    together = threading.Barrier(world)

    def program(s, r):
        together.wait(120)
        s.upload_volume(0, *volume)  # LOCAL: every rank its own copy
        together.wait(120)
        s.write_attributes(attr)
        before = _state(s)
        report = []
        for kind in TEXTS:
            for case, (variant, _) in CASES.items():
                if TEXTS[kind][0] is None and case != "b":
                    continue
                status, outs = _call(ws, s._L, s._h, kind, variant(r, world), attr)
                text = (s._L.ws_last_error(s._h) or b"").decode()
                report.append((kind, case, status, text, all(np.all(o == 7) for o in outs), _state(s) == before))
        return report, _every_call_once(ws, s, attr)  # nobody was left waiting: every rank makes every call

    got = _slab_run(ws, params, pos, world, 0, program)
    for r, (report, (calls, state)) in enumerate(got):
        assert len(report) == 7 * 3 + 1
        for kind, case, status, text, untouched, unchanged in report:
            where = (kind, case, r)
            assert status == INVALID_ARG, where
            assert text == CASES[case][1](kind, r, world), where
            assert untouched and unchanged, where
        assert calls == want_calls, r
        assert state == want_state, r
