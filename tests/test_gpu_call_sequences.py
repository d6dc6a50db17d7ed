"""Seeded sequences of every single-handle call against a quiet shadow handle (tests/call_sequences.py has the generator,
the driver and the property): the noisy handle executes every op, the quiet one only the ops that change the state, and
every read on the noisy handle must give a fresh handle's bits.  The noisy handle is plain, captured (WS_FLAG_GRAPH),
profiled (WS_FLAG_PROFILE: its launch counts are checked at every op too), in IEEE division, on the cost-guided tile schedule, or on merged cells; the quiet one is always direct and unscheduled, in
the same arithmetic (and on the same grid: the summation order follows it).  Each sequence is also replayed on two
loopback slabs against what its plain run recorded.

Scene: tests/test_gpu_field_scratch.py's -- 16^3 lattice particles in the corner of a (6, 4, 3) container at h = 0.25,
stepped 20 times -- and a 24^3 signed-distance sphere (tests/volumes_ref.py).  Both handles start from the lattice and
make those 20 steps themselves, so the first op meets a stepped handle, not a loaded one.

Against vacuity: at the first occurrence of each edit kind in a sequence the quiet handle's new state must have the
bits of the numpy restatement (forces_ref.apply, solids_ref.collide, volumes_ref.collide, cohesion_ref.stage + apply)
applied to the verified state before it, and the restatement itself must reach at least 64 particles.

Everything is compared bit for bit: no tolerances."""
import collections
import json
import os

import numpy as np
import pytest

import call_sequences as Q
import cohesion_ref as Co
import forces_ref as F
import solids_ref as S
import volumes_ref as V
from test_call_sequences_driver import LENGTH, SEEDS
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_field_grids import cell_budget
from test_gpu_field_scratch import STEPS, _Scene
from test_gpu_solids import _ext
from test_gpu_whitewater import load_state
from test_volumes_reference import sphere_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
DT = F32(1.0 / 60.0)
REACHED = 64  # particles the restatement of an anchored edit must reach
TILT = S.rotation((1.0, 2.0, -0.5), 0.7)


class _Kit:
    """The recipes of tests/call_sequences.py bound to the library and to the scene (its field calls are the scratch
    test's, at its sizes and inputs)."""

    def __init__(self, ws, scene):
        self.ws, self.scene, self.start = ws, scene, scene.start
        # (the ball of ws_collide_volumes sits at the centroid, the solids beside it: an edit clears the room it takes, and
        # the first edit of each kind must still find water where it lands)
        self.volumes = {"a": sphere_volume(24, 0.45, 0.6), "b": sphere_volume(24, 0.5, 0.6)}

    def params(self, cur):
        kw = dict(smoothing_radius=F32(0.2)) if cur["small"] else {}
        return self.ws.make_params(container_size=(6.0, 4.0, 3.0), gravity=(6.0 * cur["gx"], -9.8, 0.0, 0.0), **kw)

    def forces(self, c, off):
        at = c + np.asarray(off, F32)
        f = [F.emitter(F.RADIAL, at, 0.6, 4.0, damping=0.5),
             F.emitter(F.VORTEX, at + np.array([0.2, 0.0, 0.0], F32), 0.5, 3.0, axis=(0.0, 1.0, 0.0)),
             F.emitter(F.JET, at + np.array([0.0, 0.3, 0.0], F32), 0.3, 2.0, axis=(1.0, 0.0, 0.0), damping=0.25)]
        return F.to_ws(self.ws, f), DT, (f, DT)

    def solids(self, c, off):
        at = c + np.asarray(off, F32)
        s = [S.solid(S.SPHERE, at + np.array([-0.5, -0.1, 0.0], F32), 0.35, velocity=(0.5, 0.0, 0.0), restitution=0.3, friction=0.2,
                     margin=0.02),
             S.solid(S.BOX, at + np.array([0.55, -0.2, 0.1], F32), (0.2, 0.3, 0.2), rot=TILT, angular_velocity=(0.0, 2.0, 0.0),
                     restitution=0.5, friction=0.1, margin=0.01)]
        return S.to_ws(self.ws, s), s

    def poses(self, c, off, cur):
        p = [V.pose(0, c + np.asarray(off, F32), rot=TILT, velocity=(0.0, 0.3, 0.0), angular_velocity=(0.0, 0.0, 1.0),
                    restitution=0.4, friction=0.2, margin=0.02)]
        return V.to_ws(self.ws, p), (p, [self.volumes[cur["volumes"][0]]])

    def volume(self, which):
        vol = self.volumes[which]
        return [float(x) for x in vol["origin"]], [float(x) for x in vol["spacing"]], vol["sdf"]

    def cohesion(self, cur):
        return self.ws.fluid.cohesion_params(**Co.defaults()), DT, (Co.defaults(), DT, dict(cur))

    def records(self, pos, vel, seed):
        """What a host writes back: the positions moved a little, the velocities halved, predicted positions that are
        deliberately not p + 0.02 v; density, pressure and acceleration as zeros (ws_write_particles ignores them)."""
        rec = np.zeros(len(pos), self.ws.fluid.PARTICLE_DTYPE)
        rec["position"][:, :3] = pos + np.random.default_rng(seed).uniform(-0.002, 0.002, pos.shape).astype(F32)
        rec["velocity"][:, :3] = vel * F32(0.5)
        rec["predicted_position"][:, :3] = rec["position"][:, :3] + rec["velocity"][:, :3] * F32(0.03)
        return rec

    def read(self, w, cur, kind, m, **kw):
        return self.scene.call(w, self.params(cur), kind, m, **kw)


class _Anchor:
    """The first edit of each kind in a sequence against its numpy restatement; how many particles each reached."""

    def __init__(self, kit, merged):
        self.kit, self.merged, self.reached = kit, merged, {}

    def __call__(self, i, op, ref, before, after, out):
        if op.name in self.reached:
            return
        (pos, vel), (pos1, vel1) = before, after
        ext = _ext(self.kit.scene.params)  # (the container and its damping: the same under every parameter set in use)
        if op.name == "apply_forces":
            vel_r, _, counts = F.apply(pos, vel, *ref)
            pos_r, reached = pos, int(F.accelerate(pos, vel, ref[0])[1].sum())
            want = [counts]
        elif op.name == "apply_cohesion":
            cp, dt, cur = ref
            st = Co.stage(self.kit.params(cur), pos, vel, cp, dt, self.merged(cur))
            pos_r, vel_r, reached = pos, Co.apply(vel, st), int(np.count_nonzero(st["neighbours"]))
            want = [np.asarray(reached)]
        else:
            a = S.collide(pos, vel, ref, *ext) if op.name == "collide_solids" else V.collide(pos, vel, ref[1], ref[0], *ext)
            pos_r, vel_r, reached = a["pos"], a["vel"], int(a["touched"].sum())
            want = [a["contacts"], a["impulse"], a["angular"]]
        self.reached[op.name] = reached
        assert reached >= REACHED, "the restatement reaches %d particles" % reached
        assert same_bits(vel1, vel_r), "velocities: %d differ" % np.count_nonzero((vel1.view(np.uint32) != vel_r.view(np.uint32)).any(1))
        assert same_bits(pos1, pos_r), "positions differ"
        assert not same_bits(vel1, vel) and (op.name in ("apply_forces", "apply_cohesion") or not same_bits(pos1, pos))
        if out is not None:
            assert all(np.array_equal(g, w) for g, w in zip(out, want)), "counts or reaction sums differ"


@pytest.fixture(scope="module")
def scene(ws):
    return _Scene(ws)


@pytest.fixture(scope="module")
def kit(ws, scene):
    return _Kit(ws, scene)


RECORDS = {}  # seed -> what the plain run verified (the slab test replays one)


def _sequence_run(ws, kit, seed, label, noisy=None, **both):
    """The seeded sequence; noisy(positions, params, **both) makes the noisy handle (default: as the quiet one), the
    quiet and the fresh handles are FluidWorker(.., **both).  (sequence, record, the noisy handle's stats at the end, its
    graph steps before the first op)."""
    base = kit.params(dict(small=False, gx=0))
    seq = Q.sequence(seed, LENGTH)
    merged = {}

    def fresh(cur, pos, vel):
        w = ws.FluidWorker(pos, kit.params(cur), **both)
        load_state(w, pos, vel)
        for slot, which in cur["volumes"].items():
            w.upload_volume(slot, *kit.volume(which))
        return w

    def merged_of(cur):  # the cells merged per grid cell at the parameters of the moment, from a handle made for the question
        if cur["small"] not in merged:
            f = fresh(cur, kit.start, np.zeros_like(kit.start))
            merged[cur["small"]] = f.stats()["cells_merged"]
            f.close()
        return merged[cur["small"]]

    loud = (noisy or ws.FluidWorker)(kit.start, base, **both)
    quiet = ws.FluidWorker(kit.start, base, **both)
    try:
        loud.run(STEPS)
        quiet.run(STEPS)
        g0 = loud.stats()["graph_steps"]
        anchor = _Anchor(kit, merged_of)
        rec = Q.run(loud, quiet, fresh, seq, anchor, kit=kit)
        stats = loud.stats()
    finally:
        loud.close()
        quiet.close()
    assert sum(rec.counts.values()) == LENGTH
    assert set(anchor.reached) == {op.name for op in seq if op.cls == "edit"}, anchor.reached
    print("CALLSEQ " + json.dumps(dict(configuration=label, seed=seed, ops=dict(rec.counts), reached=anchor.reached,
                                       graph_steps=stats["graph_steps"], tile_schedule=stats["tile_schedule"],
                                       cells_merged=stats["cells_merged"])))
    return seq, rec, stats, g0


@pytest.mark.parametrize("seed", SEEDS)
def test_plain(ws, kit, seed):
    seq, rec, stats, _ = _sequence_run(ws, kit, seed, "plain")
    assert stats["graph_steps"] == 0 and not stats["tile_schedule"] and stats["cells_merged"] == (1, 1, 1)
    RECORDS[seed] = (seq, rec)


@pytest.mark.parametrize("seed", SEEDS)
def test_captured_steps(ws, kit, seed):
    """graph=True on the noisy handle.  ws_step replays its capture whenever the predicted positions are the library's
    to recompute (pred_stale, csrc/ws_api.cpp): after a step and after an edit -- an edit leaves every array where it
    is, so the capture is replayed as it is -- but not for the first step after ws_write_particles, ws_reset, a re-grid
    or ws_read_particles, which leave predicted positions to be taken as they are.  ws_set_params with unchanged
    parameters must keep the capture, changed gravity drops it and the next step captures again: replayed either way.
    So every step op's replays are known from the ops before it; tests/test_call_sequences_driver.py holds that the
    seeds' lists contain edit -> step and step -> unchanged parameters -> step."""
    seq, rec, stats, g0 = _sequence_run(ws, kit, seed, "graph", lambda *a, **kw: ws.FluidWorker(*a, graph=True, **kw))
    before, stale, replays = g0, True, collections.Counter()  # (the 20 steps before the first op leave pred_stale set)
    for i, op in enumerate(seq):
        if op.cls == "edit":
            stale = True
        elif op.name in ("write", "reset", "read_vec") or Q.regrids(op):
            stale = False
        elif op.cls == "step":
            replayed, before = rec.graph_steps[i] - before, rec.graph_steps[i]
            assert replayed == op.variant - (0 if stale else 1), (i, op, replayed)
            if stale:
                replays["after an edit"] += seq[i - 1].cls == "edit"
                replays["after unchanged parameters"] += seq[i - 1].variant == "same"
            stale = True
    assert stats["graph_steps"] == before > g0
    print("CALLSEQ " + json.dumps(dict(configuration="graph", seed=seed, fully_replayed_step_ops=dict(replays))))


@pytest.mark.parametrize("seed", SEEDS)
def test_profiled(ws, kit, seed):
    """profile=True on the noisy handle: its steps carry event brackets and K4 / K5 go through the launch that takes a
    start / stop event pair (csrc/ws_kernels.hip WS_LAUNCH); the quiet and the fresh handles are unprofiled.  Same bits
    at every op, and the launch counts after EVERY op are the ones the op list asks for (Q.expected_launches: nothing is
    read back from the library to make the expectation): the handle's creation binned once and the 20 steps before the
    first op ran each step kernel 20 times; a step op of variant v adds v to each, a write, a reset and a re-grid one
    `bin`, edits and reads nothing -- not the unprofiled force pass of ws_read_particles, not the field calls that
    drain the pending pairs."""
    seq, rec, stats, _ = _sequence_run(ws, kit, seed, "profiled", lambda *a, **kw: ws.FluidWorker(*a, profile=True, **kw))
    assert stats["graph_steps"] == 0 and not stats["tile_schedule"]
    Q.check_profile_counts(seq, rec, STEPS)
    last = {k: n for k, (_, n) in rec.profile[len(seq) - 1].items()}
    assert last["density"] == STEPS + sum(op.variant for op in seq if op.cls == "step") > STEPS
    assert last["bin"] == 1 + sum(op.name in ("write", "reset") or Q.regrids(op) for op in seq) > 1


@pytest.mark.parametrize("seed", SEEDS)
def test_ieee_division(ws, kit, seed):
    _sequence_run(ws, kit, seed, "ieee", ieee_division=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_tile_schedule(ws, kit, devlib, seed):
    """The developer library's WS_TILE_SCHEDULE=1 puts a handle of this size on the cost-guided schedule (parity, costs
    and cuts change with every step and with nothing else); the quiet handle is the product library's, unscheduled."""
    def scheduled(*a, **kw):  # the hook is read when a handle is created
        os.environ["WS_TILE_SCHEDULE"] = "1"
        try:
            return ws.FluidWorker(*a, library=devlib, **kw)
        finally:
            os.environ.pop("WS_TILE_SCHEDULE", None)

    _, _, stats, _ = _sequence_run(ws, kit, seed, "schedule", scheduled)
    assert stats["tile_schedule"]


@pytest.mark.parametrize("seed", SEEDS)
def test_merged_cells(ws, kit, devlib, seed):
    """The developer library's WS_CELL_BUDGET=800 merges reference cells at both radii; the quiet handle and the fresh
    ones are on the same grid, because a sum's order follows the grid."""
    with cell_budget("800"):
        _, _, stats, _ = _sequence_run(ws, kit, seed, "merged", library=devlib)
    assert max(stats["cells_merged"]) > 1


class _SlabAsWorker:
    """A SlabWorker under FluidWorker's names: write_slice("particles", .) is write_particles there."""

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        return getattr(self._s, name)

    def write_slice(self, name, records):
        assert name == "particles"
        self._s.write_particles(records)


@pytest.mark.parametrize("seed", SEEDS)
def test_two_slabs_replay_the_plain_run(ws, kit, seed):
    """Two loopback slabs make the 20 steps and then every op of the sequence (a slab handle offers each of them, all
    collective; only write_slice is spelled write_particles there, and a split read brackets the next op only if that is
    a step: a slab handle refuses every call that gathers while a readback is in flight, so before any other op the
    readback is ended first).  Rank 1 only contributes to every second read --
    except read_vec, sort_view, read_speeds and the split read, which have no contribute-only form.  Every state, every
    returned count and sum, and every wanted read is what the single plain run recorded -- but for the views of the last
    step after a reload (include/wsfluid.h: an edit or a re-grid reloads a slab handle, and until the next step
    ws_read_particles then reports zero density, pressure and acceleration and ws_read_sort_view the identity)."""
    if seed not in RECORDS:
        RECORDS[seed] = _sequence_run(ws, kit, seed, "plain")[:2]
    seq, rec = RECORDS[seed]
    nth = {i: k for k, i in enumerate(i for i, op in enumerate(seq) if op.cls == "read")}

    def body(s, r):
        Q.replay(_SlabAsWorker(s), seq, rec, kit=kit, wants=lambda i: r == 0 or nth[i] % 2 == 0, reloads=True,
                 brackets=lambda op: op.cls == "step")
        return True

    assert _slab_run(ws, kit.params(dict(small=False, gx=0)), kit.start, 2, STEPS, body) == [True, True]


def test_the_driver_tells_real_handles_apart(ws, kit):
    """Against vacuity on the library's side: the same driver with a noisy handle in the OTHER arithmetic is refused
    before the first op (20 steps of hardware reciprocals against IEEE division), and so is a quiet handle that lags one
    step behind."""
    seq = Q.sequence(SEEDS[0], LENGTH)
    base = kit.params(dict(small=False, gx=0))

    def pair(steps, **noisy_args):
        noisy, quiet = ws.FluidWorker(kit.start, base, **noisy_args), ws.FluidWorker(kit.start, base)
        noisy.run(STEPS)
        quiet.run(steps)
        return noisy, quiet

    for (noisy, quiet), index in ((pair(STEPS, ieee_division=True), -1), (pair(STEPS - 1), -1)):
        with pytest.raises(Q.SequenceMismatch) as e:
            Q.run(noisy, quiet, None, seq, kit=kit)
        assert e.value.index == index and "differ between the noisy and the quiet handle" in e.value.what
        noisy.close()
        quiet.close()
