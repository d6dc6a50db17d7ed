"""tests/call_sequences.py without a GPU: what the generated lists of the seeds in use contain, and that the driver can
fail -- numpy stand-ins for a handle (a toy "state = positions, velocities" model with FluidWorker's method names)
carry planted history dependence, and each fault must be reported at the first op where it shows.  A faithful stand-in
passes every seeded sequence.  Nothing here touches the library."""
import numpy as np
import pytest

import call_sequences as Q
from call_sequences import Op

F32 = np.float32
SEEDS = (0, 1, 3)  # fixed: tests/test_gpu_call_sequences.py runs these
LENGTH = 48
REC = np.dtype([("position", F32, 4), ("velocity", F32, 4), ("acceleration", F32, 4), ("predicted_position", F32, 4)])
DT = F32(1.0 / 60.0)


# ---- the generator's guarantees, on the lists ------------------------------------------------------------------------------
def test_the_seeded_lists_cover_the_catalogue_the_class_pairs_and_the_named_triples():
    seqs = [Q.sequence(s, LENGTH) for s in SEEDS]
    assert all(len(s) == LENGTH for s in seqs)
    lacking = Q.coverage(seqs)
    assert lacking == dict(ops=[], pairs=[], triples=[], early_volumes=[]), lacking
    assert len({k for c in Q.CATALOGUE.values() for k in c}) == 2 + 8 + 4 + 4 + 23
    for s in seqs:
        small = False
        for i, op in enumerate(s):
            assert op.key in Q.CATALOGUE[op.cls]
            if op.name == "split":  # it brackets the next op: there is one, and it is not another split
                assert i + 1 < len(s) and s[i + 1].name != "split"
            if Q.regrids(op):  # every such call changes the radius
                assert small == (op.variant == "h=0.25")
                small = not small
            if op.variant == "replace":
                assert any(o.variant == "first" for o in s[:i])
        assert sum(o.variant == "first" for o in s) <= 1


def test_a_seed_gives_the_same_list_every_time_and_another_seed_another():
    assert Q.sequence(SEEDS[0], LENGTH) == Q.sequence(SEEDS[0], LENGTH) != Q.sequence(SEEDS[1], LENGTH)


def test_the_field_kinds_are_the_scratch_tests():
    import test_gpu_field_scratch as T

    assert Q.FIELD_KINDS == T.KINDS and Q.SIZES == T.SIZES


# ---- the stand-in ------------------------------------------------------------------------------------------------------------
class Toy:
    """State = positions, velocities; parameters h and g; resident "volumes" (a radius per slot).  Every result is a
    function of those alone -- unless a fault is planted:
      nudge    a read leaves a flag behind that moves the next step's result by one ulp
      stale    a re-grid leaves a table stale that the next read rebuilds; an edit on the stale table is twice as strong
      accel    the acceleration of the record view is computed late, from the velocities of THAT moment: at a re-grid
               or a read, so after step -> edit -> re-grid it depends on whether something read in between
      scratch  a field read's result remembers the size of the read before it"""

    def __init__(self, pos, params, fault=None):
        self.pos, self.vel = np.array(pos, F32), np.zeros_like(pos, dtype=F32)
        self.acc = np.zeros_like(self.pos)
        self.p, self.vol, self.fault = dict(params), {}, fault
        self.flag = self.stale = self.late = False
        self.last_m = 0

    def close(self):
        pass

    def stats(self):
        return {"graph_steps": 0}

    def _accel(self):
        return (np.asarray(self.p["g"], F32) - F32(0.1) * self.vel).astype(F32)

    def _read(self):
        self.flag, self.stale = True, False
        if self.late:
            self.acc, self.late = self._accel(), False

    # state-changing
    def run(self, steps=1):
        for _ in range(steps):
            if self.fault == "nudge" and self.flag:
                self.vel[0, 0] = np.nextafter(self.vel[0, 0], F32(np.inf))
            self.flag = False
            self.vel = (self.vel + DT * self._accel()).astype(F32)
            self.pos = (self.pos + DT * self.vel).astype(F32)
            self.acc, self.late = self._accel(), False  # (of the new velocities: what a late evaluation gives too)
            if self.fault == "accel":
                self.late = True

    def _near(self, centre, radius):
        q = (self.pos - np.asarray(centre, F32)).astype(F32)
        d = np.sqrt((q * q).sum(1)).astype(F32)
        return q, d, d < F32(radius)

    def apply_forces(self, forces, dt, counts=True):
        out = np.zeros(len(forces), np.uint32)
        for e, f in enumerate(forces):
            _, _, seen = self._near(f["centre"], f["radius"])
            s = f["strength"] * F32(2 if self.fault == "stale" and self.stale else 1)
            self.vel[seen] = (self.vel[seen] + F32(dt) * s).astype(F32)
            out[e] = seen.sum()
        return out if counts else None

    def _push(self, centres, radii, reaction):
        contacts, impulse = np.zeros(len(centres), np.uint32), np.zeros((len(centres), 3))
        for e, (c, r) in enumerate(zip(centres, radii)):
            q, d, seen = self._near(c, r)
            seen &= d > 0
            moved = (np.asarray(c, F32) + q[seen] / d[seen, None] * F32(r)).astype(F32)
            impulse[e] = (moved - self.pos[seen]).sum(0, dtype=np.float64)
            self.pos[seen] = moved
            self.vel[seen] = (self.vel[seen] * F32(0.5)).astype(F32)
            contacts[e] = seen.sum()
        return (contacts, impulse, -impulse) if reaction else None

    def collide_solids(self, solids, reaction=True):
        return self._push([s["centre"] for s in solids], [s["radius"] for s in solids], reaction)

    def collide_volumes(self, poses, reaction=True):
        assert all(p["slot"] in self.vol for p in poses), "ws_collide_volumes before an upload"
        return self._push([p["centre"] for p in poses], [self.vol[p["slot"]][0] for p in poses], reaction)

    def apply_cohesion(self, cp, dt, count=True):
        self.vel = (self.vel + F32(cp) * (self.vel.mean(0, dtype=np.float64).astype(F32) - self.vel)).astype(F32)
        return len(self.pos) if count else None

    def write_slice(self, name, rec):
        assert name == "particles"
        self.pos, self.vel = rec["position"][:, :3].copy(), rec["velocity"][:, :3].copy()
        self.acc, self.late, self.flag = np.zeros_like(self.pos), False, False

    def reset(self, pos):
        self.pos, self.vel = np.array(pos, F32), np.zeros_like(self.pos)
        self.acc, self.late, self.flag = np.zeros_like(self.pos), False, False

    def upload_volume(self, slot, origin, spacing, sdf):
        self.vol[slot] = np.array(sdf, F32)

    def set_params(self, p):
        if p["h"] != self.p["h"]:
            self.stale = True
            if self.late:
                self.acc, self.late = self._accel(), False
        self.p = dict(p)

    # the two readers that touch no hidden state, as in the library
    def read_positions(self, want=True):
        return self.pos.copy() if want else None

    def read_velocities(self, want=True):
        return self.vel.copy() if want else None

    # read-only
    def read_speeds(self):
        self._read()
        return np.sqrt((self.vel * self.vel).sum(1)).astype(F32)

    def read_vec(self, name="particles"):
        self._read()
        rec = np.zeros(len(self.pos), REC)
        rec["position"][:, :3], rec["velocity"][:, :3], rec["acceleration"][:, :3] = self.pos, self.vel, self.acc
        rec["predicted_position"][:, :3] = (self.pos + (self.vel * F32(0.02)).astype(F32)).astype(F32)
        return rec

    def sort_view(self):
        keys = (np.floor(self.pos / F32(self.p["h"])).astype(np.int64) % 7).sum(1).astype(np.uint32)
        return keys, np.argsort(keys, kind="stable").astype(np.uint32), np.bincount(keys, minlength=len(keys)).astype(np.uint32)[:len(keys)]

    def read_positions_begin(self, buf):
        self._read()
        buf[:] = self.pos

    def read_positions_end(self):
        pass

    def toy_read(self, kind, m, want=True):
        self._read()
        m_seen, self.last_m = (self.last_m if self.fault == "scratch" else 0), m
        if not want:
            return None
        w = F32(len(kind) + m % 7 + m_seen)
        return [(self.pos * F32(self.p["h"]) + self.vel * w).astype(F32), np.array([m, len(self.vol)], np.uint32)]


class Reloaded(Toy):
    """The views of a slab handle: after a write, a reset, an edit or a re-grid and until the next step, zero
    acceleration and the identity as the sort view."""
    loaded = False

    def run(self, steps=1):
        super().run(steps)
        self.loaded = False

    def read_vec(self, name="particles"):
        rec = super().read_vec(name)
        if self.loaded:
            rec["acceleration"] = 0
        return rec

    def sort_view(self):
        n = len(self.pos)
        return (np.arange(n, dtype=np.uint32),) * 3 if self.loaded else super().sort_view()


def _loads(name):
    def call(self, *a, **kw):
        if name != "set_params" or a[0]["h"] != self.p["h"]:
            self.loaded = True
        return getattr(Toy, name)(self, *a, **kw)

    return call


for _name in ("apply_forces", "collide_solids", "collide_volumes", "apply_cohesion", "write_slice", "reset", "set_params"):
    setattr(Reloaded, _name, _loads(_name))


class ToyKit:
    def __init__(self):
        g = np.arange(4, dtype=F32) * F32(0.3)
        self.start = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)

    def params(self, cur):
        return dict(h=0.2 if cur["small"] else 0.25, g=(6.0 * cur["gx"], -9.8, 0.0))

    def forces(self, c, off):
        f = [dict(centre=c + np.asarray(off, F32), radius=F32(0.6), strength=F32(3.0))]
        return f, DT, ("apply_forces", f, DT)

    def solids(self, c, off):
        s = [dict(centre=c + np.asarray(off, F32), radius=F32(0.35))]
        return s, ("collide_solids", s)

    def poses(self, c, off, cur):
        p = [dict(slot=0, centre=c + np.asarray(off, F32))]
        return p, ("collide_volumes", p, {k: self.volume(v)[2] for k, v in cur["volumes"].items()})

    def volume(self, which):
        return (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), np.array([0.4 if which == "a" else 0.3], F32)

    def cohesion(self, cur):
        return F32(0.1), DT, ("apply_cohesion", F32(0.1), DT)

    def records(self, pos, vel, seed):
        rec = np.zeros(len(pos), REC)
        rec["position"][:, :3] = pos + np.random.default_rng(seed).uniform(-0.01, 0.01, pos.shape).astype(F32)
        rec["velocity"][:, :3] = vel * F32(0.5)
        rec["predicted_position"][:, :3] = pos  # deliberately not p + 0.02 v
        return rec

    def read(self, w, cur, kind, m, **kw):
        return w.toy_read(kind, m, **kw)


KIT = ToyKit()


def handles(fault):
    p = KIT.params(dict(small=False, gx=0))

    def fresh(cur, pos, vel):
        f = Toy(pos, KIT.params(cur), fault)
        f.vel = np.array(vel, F32)
        for slot, which in cur["volumes"].items():
            f.upload_volume(slot, *KIT.volume(which))
        return f

    noisy, quiet = Toy(KIT.start, p, fault), Toy(KIT.start, p, fault)
    for w in (noisy, quiet):
        w.run(5)
    return noisy, quiet, fresh


def restated(i, op, ref, before, after, out):
    """The faithful model of an edit on the state before it."""
    m = Toy(before[0], dict(h=0.25, g=(0.0, -9.8, 0.0)))
    m.vel = before[1].copy()
    if ref[0] == "collide_volumes":
        m.vol = dict(ref[2])
        m.collide_volumes(ref[1])
    else:
        getattr(m, ref[0])(*ref[1:])
    assert not Q.differing([m.pos, m.vel], list(after)), "positions or velocities differ"


STEP, READ_VEC = Op("step", "run", 1, None), Op("read", "read_vec", None, None)
FORCES = Op("edit", "apply_forces", True, (0.0, 0.0, 0.0))
REGRID, BACK = Op("params", "set_params", "h=0.2", None), Op("params", "set_params", "h=0.25", None)


def FIELD(kind="density_points", m=65):
    return Op("read", "read", kind, m)


# ---- a faithful stand-in passes, a faulty one is reported where the fault shows ------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_a_faithful_stand_in_passes_the_seeded_sequence_and_its_replay(seed):
    seq = Q.sequence(seed, LENGTH)
    noisy, quiet, fresh = handles(None)
    rec = Q.run(noisy, quiet, fresh, seq, restated, kit=KIT)
    assert sum(rec.counts.values()) == LENGTH and set(rec.counts) == set(Q.CLASSES)
    assert sorted(rec.states) == [-1] + [i for i, op in enumerate(seq) if op.cls != "read"]
    assert sorted(rec.reads) == [i for i, op in enumerate(seq) if op.cls == "read" and op.name != "split"]
    assert sorted(rec.splits) == [i for i, op in enumerate(seq) if op.name == "split"]
    # the recorded run against a third handle, as a slab rank replays it: every read, and every second one
    for wants in (lambda i: True, lambda i: i % 2 == 0):
        third = Toy(KIT.start, KIT.params(dict(small=False, gx=0)))
        third.run(5)
        Q.replay(third, seq, rec, kit=KIT, wants=wants)
    # a stand-in with a slab handle's views: an edit or a re-grid reloads it like a write does
    third = Reloaded(KIT.start, KIT.params(dict(small=False, gx=0)))
    third.run(5)
    Q.replay(third, seq, rec, kit=KIT, reloads=True, brackets=lambda op: op.cls == "step")
    # ... and the replay can fail too
    third = Toy(KIT.start, KIT.params(dict(small=False, gx=0)), "nudge")
    third.run(5)
    with pytest.raises(Q.SequenceMismatch):
        Q.replay(third, seq, rec, kit=KIT)


CASES = {
    # fault, sequence, check, index of the first visible difference, a word of the report
    "a read nudges the next step": ("nudge", [FORCES, Op("read", "read_speeds", None, None), STEP, STEP], None, 2, "velocities"),
    # (a read_vec the sequence draws is made on the quiet handle too: the one read that cannot tell)
    "the nudge with nothing but a drawn read_vec in between": ("nudge", [FORCES, READ_VEC, STEP, REGRID, STEP], None, None, None),
    "an edit after a re-grid, healed by a read": ("stale", [STEP, REGRID, FIELD(), FORCES, STEP], None, 3, "velocities"),
    "an edit after a re-grid, nothing read: both handles agree": ("stale", [STEP, REGRID, FORCES, STEP], None, None, None),
    "... and the restatement tells": ("stale", [STEP, REGRID, FORCES, STEP], restated, 2, "restatement"),
    "read_vec differs in the acceleration alone": ("accel", [STEP, FIELD(), FORCES, REGRID, READ_VEC, STEP], None, 4, "outputs [2]"),
    "... at the end when the sequence never reads it": ("accel", [STEP, FIELD(), FORCES, REGRID], None, 4, "['acceleration']"),
    "a field read remembers the read before it": ("scratch", [STEP, FIELD(m=4097), FIELD(m=65), STEP], None, 2, "fresh"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_planted_fault_is_reported_at_the_first_op_where_it_shows(case):
    fault, seq, check, index, word = CASES[case]
    noisy, quiet, fresh = handles(fault)
    if index is None:
        Q.run(noisy, quiet, fresh, seq, check, kit=KIT)
        return
    with pytest.raises(Q.SequenceMismatch) as e:
        Q.run(noisy, quiet, fresh, seq, check, kit=KIT)
    assert e.value.index == index and word in e.value.what, e.value
    assert e.value.op == (seq[index] if index < len(seq) else None)
    # the report names the op and the (up to five) ops before it
    assert str(tuple(seq[index - 1])) in str(e.value) and "op %d" % index in str(e.value)
    # the same sequence on faithful stand-ins passes
    Q.run(*handles(None), seq, check, kit=KIT)


def test_a_split_read_must_hold_the_positions_of_its_begin():
    class Late(Toy):  # gathers at end instead of at begin
        def read_positions_begin(self, buf):
            self.buf = buf

        def read_positions_end(self):
            self.buf[:] = self.pos

    seq = [Op("read", "split", None, None), STEP, STEP]
    noisy, quiet, fresh = handles(None)
    late = Late(KIT.start, noisy.p)
    late.run(5)
    with pytest.raises(Q.SequenceMismatch) as e:
        Q.run(late, quiet, fresh, seq, kit=KIT)
    assert e.value.index == 0 and "split" in e.value.what
    Q.run(*handles(None), seq, kit=KIT)


class Profiled(Toy):
    """A stand-in that counts its launches as a profiled handle does: one of each step kernel per step, one "bin" per
    creation, write, reset and re-grid.  miscount = an op name: a read of that name loses the event pair of one density
    launch (a pair dropped unread); "split": the step after a re-grid counts its density launch twice (an early and a
    late range both counted)."""

    def __init__(self, pos, params, miscount=None):
        super().__init__(pos, params)
        self.miscount, self.counts, self.regridded = miscount, dict({k: 0 for k in Q.STEP_KERNELS}, bin=1), False

    def profile(self):
        return {k: (0.01 * n, n) for k, n in self.counts.items()}

    def run(self, steps=1):
        super().run(steps)
        for k in Q.STEP_KERNELS:
            self.counts[k] += steps
        if self.miscount == "split" and self.regridded:
            self.counts["density"] += 1
        self.regridded = False

    def write_slice(self, name, rec):
        super().write_slice(name, rec)
        self.counts["bin"] += 1

    def reset(self, pos):
        super().reset(pos)
        self.counts["bin"] += 1

    def set_params(self, p):
        if p["h"] != self.p["h"]:
            self.counts["bin"] += 1
            self.regridded = True
        super().set_params(p)

    def read_speeds(self):
        if self.miscount == "read_speeds":
            self.counts["density"] -= 1
        return super().read_speeds()


SPEEDS = Op("read", "read_speeds", None, None)
MISCOUNTS = {
    # planted miscount, sequence, the op at which the counts first differ
    "a read drops a pair": ("read_speeds", [STEP, FORCES, SPEEDS, STEP], 2),
    "the step after a re-grid counts twice": ("split", [STEP, REGRID, FIELD(), Op("step", "run", 3, None), STEP], 3),
    "faithful": (None, [STEP, REGRID, SPEEDS, Op("host", "reset", None, None), Op("step", "run", 3, None), BACK, Op("host", "write", None, 7)], None),
}


@pytest.mark.parametrize("case", list(MISCOUNTS))
def test_a_planted_miscount_is_reported_at_the_op_where_it_happens(case):
    miscount, seq, index = MISCOUNTS[case]
    _, quiet, fresh = handles(None)
    noisy = Profiled(KIT.start, quiet.p, miscount)
    noisy.run(5)
    rec = Q.run(noisy, quiet, fresh, seq, kit=KIT)  # (the state is right: only the counts are not)
    assert sorted(rec.profile) == list(range(-1, len(seq)))
    if index is None:
        Q.check_profile_counts(seq, rec, 5)
        assert Q.expected_launches(seq, 5)[-1] == dict({k: 5 + 1 + 3 for k in Q.STEP_KERNELS}, bin=1 + 4)
        return
    with pytest.raises(Q.SequenceMismatch) as e:
        Q.check_profile_counts(seq, rec, 5)
    assert e.value.index == index and e.value.op == seq[index] and "density" in e.value.what, e.value
    with pytest.raises(Q.SequenceMismatch) as e:  # ... and a wrong claim about the start is refused at the start
        Q.check_profile_counts(seq, rec, 4)
    assert e.value.index == -1


def test_a_handle_without_a_profile_records_none():
    noisy, quiet, fresh = handles(None)
    assert Q.run(noisy, quiet, fresh, [STEP, SPEEDS], kit=KIT).profile == {}


def test_returned_counts_are_compared():
    class Miscount(Toy):
        def apply_forces(self, forces, dt, counts=True):
            out = super().apply_forces(forces, dt, counts)
            return out if out is None else out + np.uint32(self.flag)

    noisy, quiet, fresh = handles(None)
    bad = Miscount(KIT.start, noisy.p)
    bad.run(5)
    with pytest.raises(Q.SequenceMismatch) as e:
        Q.run(bad, quiet, fresh, [STEP, FIELD(), FORCES], kit=KIT)
    assert e.value.index == 2 and "returned outputs" in e.value.what
