"""Seeded sequences drawn from the whole single-handle API, and the driver that runs one on a "noisy" handle (every
op) beside a "quiet" shadow handle (the state-changing ops alone).

The property: the result of a call depends on the parameters, the resident volumes and the positions and velocities of
the moment -- not on which calls came before, not on whether the steps are captured, scheduled or direct, not on how
many read-only calls were made in between.  So after every state-changing op both handles must hold the same bits, and
every read on the noisy handle must give what the same call gives on a fresh handle loaded with that state.

Pure Python and numpy: nothing here imports the library.  What binds a recipe to a library (parameter structures,
emitters, solids, the field calls) is a `kit`, given to the driver by its caller: tests/test_gpu_call_sequences.py has
the real one, tests/test_call_sequences_driver.py a toy one over numpy stand-ins.

A kit has
    start                       the positions ws_reset goes back to
    params(cur)                 the parameter structure of cur = {"small": bool, "gx": -1 | 0 | 1}
    forces(c, off)              (emitters, dt, ref) around the centroid c;  ref: whatever the kit's check() wants
    solids(c, off)              (solids, ref)
    poses(c, off, cur)          (poses, ref)
    volume(which)               (origin, spacing, sdf) of volume "a" or "b"
    cohesion(cur)               (parameters, dt, ref)
    records(pos, vel, seed)     the perturbed 80-byte records a host writes back
    read(w, cur, kind, m, **kw) the field call `kind` at size m on w at the parameters of cur: a list of arrays
"""
import collections

import numpy as np

F32 = np.float32
CLASSES = ("step", "edit", "host", "params", "read")
# tests/test_gpu_field_scratch.py's KINDS (the CPU tier checks that the two lists agree)
FIELD_KINDS = ("density_grid", "density_points", "aniso_grid", "aniso_points", "anisotropy", "surface", "aniso_surface",
               "cast_rays", "cast_camera", "velocity_grid", "velocity_points", "advect_points", "read_whitewater",
               "emit_whitewater", "step_whitewater", "read_velocities", "read_cohesion", "body_forces")
SIZES = (65, 4097, 1)
VIEWS = ("read_vec", "sort_view")  # they report the LAST STEP's fields by design: compared with the quiet handle's

Op = collections.namedtuple("Op", "cls name variant arg")
Op.key = property(lambda op: (op.name, op.variant))

CATALOGUE = {
    "step": [("run", 1), ("run", 3)],
    "edit": [(name, flag) for name in ("apply_forces", "collide_solids", "collide_volumes", "apply_cohesion")
             for flag in (True, False)],  # with and without the counts / the reaction
    "host": [("write", None), ("reset", None), ("upload_volume", "first"), ("upload_volume", "replace")],
    "params": [("set_params", "h=0.2"), ("set_params", "h=0.25"), ("set_params", "flip"), ("set_params", "same")],
    "read": [("read", k) for k in FIELD_KINDS] + [("read_vec", None), ("read_positions", None), ("read_speeds", None),
                                                  ("sort_view", None), ("split", None)],
}
WEIGHTS = dict(step=0.17, edit=0.2, host=0.13, params=0.12, read=0.38)


# the transitions the hidden state was reasoned about in threes: a slot is a class, an op name or "regrid"
MOTIFS = (("edit", "regrid", "step"), ("edit", "read", "step"), ("write", "edit", "step"), ("edit", "reset", "edit"),
          ("step", "regrid", "read_vec"), ("step", "same", "step"))
MOTIF_RATE = 0.1


def sequence(seed, length=48):
    """`length` ops drawn with default_rng(seed).  Most are free draws: a class by WEIGHTS, then an op of that class
    that is possible at that point (ws_collide_volumes only after an upload, h = 0.25 only from 0.2, a split read
    neither last nor after another), one the sequence has not used yet before one it has.  With MOTIF_RATE a draw is one
    of MOTIFS instead, three ops in a row.  Only the recipe: the driver evaluates it."""
    rng = np.random.default_rng(seed)
    small = uploaded = False
    used, ops = set(), []

    def possible(key):
        name, variant = key
        if name == "collide_volumes":
            return uploaded
        if name == "upload_volume":
            return uploaded == (variant == "replace")
        if variant in ("h=0.2", "h=0.25"):
            return small == (variant == "h=0.25")
        if name == "split":
            return len(ops) < length - 1 and not (ops and ops[-1].name == "split")
        return True

    def draw(slot):
        nonlocal small, uploaded
        every = [(c, k) for c in CLASSES for k in CATALOGUE[c]]
        keys = [(c, k) for c, k in every if possible(k) and (slot in (c, k[0], k[1]) or (slot == "regrid" and k[1] in ("h=0.2", "h=0.25")))]
        keys = [ck for ck in keys if ck[1] not in used] or keys
        cls, (name, variant) = keys[rng.integers(len(keys))]
        used.add((name, variant))
        arg = None
        if cls == "edit":
            arg = tuple(float(x) for x in rng.uniform(-0.15, 0.15, 3).round(3))  # where, from the centroid
        elif name == "read":
            arg = int(SIZES[rng.integers(len(SIZES))])
        elif name == "write":
            arg = int(rng.integers(1 << 16))
        uploaded |= name == "upload_volume"
        if variant in ("h=0.2", "h=0.25"):
            small = variant == "h=0.2"
        ops.append(Op(cls, name, variant, arg))

    while len(ops) < length:
        if rng.random() < MOTIF_RATE and len(ops) + 3 <= length:
            for slot in MOTIFS[rng.integers(len(MOTIFS))]:
                draw(slot)
        else:
            draw(CLASSES[rng.choice(len(CLASSES), p=[WEIGHTS[c] for c in CLASSES])])
    return ops


def regrids(op):
    return op.variant in ("h=0.2", "h=0.25")


class SequenceMismatch(AssertionError):
    def __init__(self, index, op, what, seq):
        self.index, self.op, self.what = index, op, what
        before = [tuple(o) for o in seq[max(0, index - 5):max(0, index)]]
        super().__init__("op %d %s: %s; the five ops before it: %s" % (index, None if op is None else tuple(op), what, before))


def flat(out):
    """A call's results as a list of arrays (None: nothing was asked for)."""
    if out is None:
        return None
    if isinstance(out, dict):
        return [np.asarray(out[k]) for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [np.asarray(a) for a in out if a is not None] or None
    return [np.asarray(out)]


def differing(got, want):
    """Which of two lists of arrays differ in a bit (or in shape or type): the indices, [-1] for another length."""
    if (got is None) != (want is None):
        return [-1]
    if got is None:
        return []
    if len(got) != len(want):
        return [-1]
    return [k for k, (a, b) in enumerate(zip(got, want))
            if a.shape != b.shape or a.dtype != b.dtype or np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes()]


def record_fields(a, b):
    """The fields of two structured arrays that differ in a byte."""
    return [f for f in a.dtype.names if np.ascontiguousarray(a[f]).tobytes() != np.ascontiguousarray(b[f]).tobytes()]


def centroid(pos):
    return np.asarray(pos, np.float64).mean(axis=0).astype(F32)


def _arguments(op, kit, cur, pos, vel):
    """The recipe of a state-changing op evaluated on the state of the moment: (call(w) -> outputs, ref)."""
    c, name, flag = centroid(pos), op.name, op.variant
    if name == "run":
        return (lambda w: w.run(op.variant)), None
    if name == "apply_forces":
        forces, dt, ref = kit.forces(c, op.arg)
        return (lambda w: w.apply_forces(forces, dt, counts=flag)), ref
    if name == "collide_solids":
        solids, ref = kit.solids(c, op.arg)
        return (lambda w: w.collide_solids(solids, reaction=flag)), ref
    if name == "collide_volumes":
        poses, ref = kit.poses(c, op.arg, cur)
        return (lambda w: w.collide_volumes(poses, reaction=flag)), ref
    if name == "apply_cohesion":
        cp, dt, ref = kit.cohesion(cur)
        return (lambda w: w.apply_cohesion(cp, dt, count=flag)), ref
    if name == "write":
        rec = kit.records(pos, vel, op.arg)
        return (lambda w: w.write_slice("particles", rec)), None
    if name == "reset":
        return (lambda w: w.reset(kit.start)), None
    if name == "upload_volume":
        which = "a" if flag == "first" else "b" if cur["volumes"].get(0) == "a" else "a"
        origin, spacing, sdf = kit.volume(which)
        return (lambda w: w.upload_volume(0, origin, spacing, sdf)), which
    assert name == "set_params", op
    new = dict(cur)
    if regrids(op):
        new["small"] = flag == "h=0.2"
    elif flag == "flip":
        new["gx"] = -cur["gx"] if cur["gx"] else 1
    p = kit.params(new)
    return (lambda w: w.set_params(p)), new


def _settle(cur, op, ref):
    """What the op leaves in the description of the moment (parameters, resident volumes)."""
    if op.name == "set_params":
        cur.update(ref)
    elif op.name == "upload_volume":
        cur["volumes"] = {0: ref}


def _read(w, op, kit, cur, **kw):
    """A read-only op on w: a list of arrays."""
    if op.name == "read":
        return kit.read(w, cur, op.variant, op.arg, **kw)
    if op.name == "read_vec":
        rec = w.read_vec("particles")
        return [np.ascontiguousarray(rec[f]) for f in rec.dtype.names]
    if op.name == "read_positions":
        return flat(w.read_positions(**kw))
    if op.name == "read_speeds":
        return flat(w.read_speeds())
    assert op.name == "sort_view", op
    return flat(w.sort_view())


Record = collections.namedtuple("Record", "states outs reads splits final counts graph_steps profile")


def run(noisy, quiet, fresh, seq, check=None, *, kit):
    """The sequence on both handles.

    noisy executes every op; quiet only the step / edit / host / params ops.  After every state-changing op
    read_positions() and read_velocities() of both are compared bit for bit -- ws_read_positions and ws_read_velocities
    gather from `cur` and touch neither pred_stale nor accel_stale (csrc/ws_api.cpp: no refresh_pred, no refresh_accel
    in either), so reading the quiet handle this way leaves its hidden state alone -- and so are the counts and reaction
    sums the op returned.  A read op's expectation is the same call on fresh(cur, pos, vel): a new handle at the
    parameters of the moment holding the verified state and the same resident volumes.  The two views of the LAST STEP,
    read_vec("particles") (density, pressure, acceleration: h->steps, accel_stale) and sort_view (the sort that step
    made), have no such expectation by design; where the sequence draws one, the quiet handle makes the same call and
    the two are compared -- ws_read_sort_view touches none of the flags either, ws_read_particles does, which is the
    point of comparing it -- and read_vec is compared once more at the end.  A split read brackets the next op: begin,
    that op, end, and the buffer must hold the positions of the moment of begin.

    check(index, op, ref, before, after, out) is called after every edit with the verified (pos, vel) around it and
    the quiet handle's outputs.  A difference raises SequenceMismatch at the first op where it shows.  Returns a Record
    of what was verified: states[i] = (pos, vel) after op i (-1: at the start), outs[i], reads[i], splits[i], final,
    the number of ops per class, graph_steps[i] = noisy.stats()["graph_steps"] after step op i, and -- where the noisy
    handle offers profile() -- profile[i] = noisy.profile() after EVERY op i (-1: at the start; check_profile_counts)."""
    rec = Record({}, {}, {}, {}, [], collections.Counter(), {}, {})
    cur = dict(small=False, gx=0, volumes={})

    def state(i, op):
        got = [noisy.read_positions(), noisy.read_velocities()]
        want = [quiet.read_positions(), quiet.read_velocities()]
        for k, what in enumerate(("positions", "velocities")):
            if differing(got[k:k + 1], want[k:k + 1]):
                rows = np.flatnonzero((got[k].view(np.uint32) != want[k].view(np.uint32)).any(axis=1))
                raise SequenceMismatch(i, op, "%s of %d particles differ between the noisy and the quiet handle (first id %d)"
                                       % (what, len(rows), rows[0]), seq)
        rec.states[i] = tuple(want)
        return want

    def note_profile(i):
        if hasattr(noisy, "profile"):
            rec.profile[i] = noisy.profile()

    pos, vel = state(-1, None)
    note_profile(-1)
    split = None

    def end_split():
        nonlocal split
        if split is None:
            return
        k, buf, at_begin = split
        split = None
        noisy.read_positions_end()
        if differing([buf], [at_begin]):
            raise SequenceMismatch(k, seq[k], "the split read does not hold the positions of its begin", seq)
        rec.splits[k] = at_begin

    for i, op in enumerate(seq):
        rec.counts[op.cls] += 1
        if op.name == "split":
            end_split()
            buf = np.empty((len(pos), 3), F32)
            noisy.read_positions_begin(buf)
            split = (i, buf, pos)
            note_profile(i)
            continue
        if op.cls == "read":
            got = _read(noisy, op, kit, cur)
            end_split()
            if op.name in VIEWS:
                want, against = _read(quiet, op, kit, cur), "the quiet handle's"
            else:
                f = fresh(cur, pos, vel)
                want, against = _read(f, op, kit, cur), "a fresh handle's"
                f.close()
            bad = differing(got, want)
            if op.name == "read_positions" and not bad:
                bad, against = differing(got, [pos]), "the verified state"
            if bad:
                raise SequenceMismatch(i, op, "outputs %s differ from %s" % (bad, against), seq)
            rec.reads[i] = want
            note_profile(i)
            continue
        call, ref = _arguments(op, kit, cur, pos, vel)
        out_n, out_q = flat(call(noisy)), flat(call(quiet))
        end_split()
        _settle(cur, op, ref)
        bad = differing(out_n, out_q)
        if bad:
            raise SequenceMismatch(i, op, "returned outputs %s differ between the noisy and the quiet handle" % bad, seq)
        before, (pos, vel) = (pos, vel), state(i, op)
        rec.outs[i] = out_q
        if op.cls == "edit" and check is not None:
            try:
                check(i, op, ref, before, (pos, vel), out_q)
            except SequenceMismatch:
                raise
            except AssertionError as e:
                raise SequenceMismatch(i, op, "the restatement: %s" % (e,), seq) from e
        if op.cls == "step" and hasattr(noisy, "stats"):
            rec.graph_steps[i] = noisy.stats()["graph_steps"]
        note_profile(i)
    end_split()
    a, b = noisy.read_vec("particles"), quiet.read_vec("particles")
    bad = record_fields(a, b)
    if bad:
        raise SequenceMismatch(len(seq), None, "the records at the end differ in %s" % bad, seq)
    rec.final.append(b)
    return rec


STEP_KERNELS = ("cell_scan", "cell_scatter", "reorder", "density", "force_integrate_bin")  # one launch each per step


def expected_launches(seq, steps_before, bins_before=1):
    """The cumulative launch counts a profiled single handle must report after every op, from the op list ALONE:
    [{kernel: launches}] for index -1 (the start: `bins_before` stand-alone binnings -- the handle's creation -- and
    `steps_before` steps) and then one per op.  A step op of variant v adds v to each of STEP_KERNELS; a write, a
    reset and a re-grid bin the particles once more ("bin"); edits, uploads, other parameter pushes and reads add
    nothing."""
    now = dict({k: steps_before for k in STEP_KERNELS}, bin=bins_before)
    out = [dict(now)]
    for op in seq:
        if op.cls == "step":
            for k in STEP_KERNELS:
                now[k] += op.variant
        elif op.name in ("write", "reset") or regrids(op):
            now["bin"] += 1
        out.append(dict(now))
    return out


def check_profile_counts(seq, rec, steps_before, bins_before=1):
    """rec.profile (what run() recorded of noisy.profile() after every op) against expected_launches, at EVERY op: the
    first op whose counts differ raises SequenceMismatch there.  A counted kernel must also carry time, an uncounted
    one none."""
    want = expected_launches(seq, steps_before, bins_before)
    if sorted(rec.profile) != list(range(-1, len(seq))):
        raise SequenceMismatch(-1, None, "the profile was recorded at ops %s" % sorted(rec.profile), seq)
    for i in range(-1, len(seq)):
        got = {k: n for k, (_, n) in rec.profile[i].items()}
        op = seq[i] if i >= 0 else None
        if got != want[i + 1]:
            bad = {k: (got.get(k), want[i + 1].get(k)) for k in set(got) | set(want[i + 1]) if got.get(k) != want[i + 1].get(k)}
            raise SequenceMismatch(i, op, "launch counts (reported, asked for) differ: %s" % bad, seq)
        timeless = [k for k, (ms, n) in rec.profile[i].items() if (ms > 0.0) != (n > 0)]
        if timeless:
            raise SequenceMismatch(i, op, "kernels counted without time, or timed without a count: %s" % timeless, seq)


STEP_FIELDS = ("density", "pressure", "acceleration")  # of the 80-byte record: what only a step computes


def replay(w, seq, rec, *, kit, wants=lambda i: True, reloads=False, brackets=lambda op: True):
    """The same sequence on ONE handle against what run() recorded -- a rank of a slab run, where every call is
    collective: every rank makes it, wants(i) says whether this rank asks for read i's results (else it only
    contributes, and must be handed nothing).  Every state and every wanted read is the recorded one -- with reloads,
    but for the one difference include/wsfluid.h states: an edit and a re-grid RELOAD a slab handle, so that until the
    next step its two views of the last step report what they report after any load -- zero density, pressure and
    acceleration, and the identity as the sort view -- where a single handle goes on reporting the last step's.  The arguments of an op come
    A split read is ended before the next op unless brackets(op) (a slab handle refuses every gathering call while a
    readback is in flight).  The arguments of an op come
    from the recorded states and a difference is raised only after the last op (the first one found), so that a rank
    that has seen one goes on making the calls its peers are waiting in."""
    cur = dict(small=False, gx=0, volumes={})
    pos, vel = rec.states[-1]
    split, found, loaded = None, [], False
    names = rec.final[0].dtype.names

    def view(op, want):  # what a view of the last step reports on a handle that has been reloaded since
        if not (reloads and loaded):
            return want
        if op is None or op.name == "read_vec":
            return [np.zeros_like(a) if f in STEP_FIELDS else a for f, a in zip(names, want)]
        return [np.arange(len(a), dtype=a.dtype) for a in want]

    def differs(i, got, want, what):
        bad = differing(got, want)
        if bad:
            found.append(SequenceMismatch(i, seq[i] if i < len(seq) else None, "%s %s differ from the single handle's" % (what, bad), seq))

    def end_split():
        nonlocal split
        if split is not None:
            k, buf = split
            split = None
            w.read_positions_end()
            differs(k, [buf], [rec.splits[k]], "the split read's positions")

    for i, op in enumerate(seq):
        if op.name == "split":
            end_split()
            buf = np.empty((len(pos), 3), F32)
            w.read_positions_begin(buf)
            split = (i, buf)
            if not brackets(seq[i + 1]):
                end_split()
            continue
        if op.cls == "read":
            # (read_vec, sort_view and read_speeds have no contribute-only form)
            kw = {} if wants(i) or op.name in VIEWS + ("read_speeds",) else dict(want=False)
            got = _read(w, op, kit, cur, **kw)
            end_split()
            differs(i, got, None if kw else view(op, rec.reads[i]) if op.name in VIEWS else rec.reads[i], "outputs")
            continue
        call, ref = _arguments(op, kit, cur, pos, vel)
        out = flat(call(w))
        end_split()
        _settle(cur, op, ref)
        loaded = op.cls != "step" and (loaded or op.cls == "edit" or regrids(op) or op.name in ("write", "reset"))
        differs(i, out, rec.outs[i], "returned outputs")
        pos, vel = rec.states[i]
        differs(i, [w.read_positions(), w.read_velocities()], [pos, vel], "positions / velocities")
    end_split()
    a = w.read_vec("particles")
    differs(len(seq), [np.ascontiguousarray(a[f]) for f in names], view(None, [np.ascontiguousarray(rec.final[0][f]) for f in names]),
            "the records at the end: fields")
    if found:
        first = min(found, key=lambda e: e.index)
        first.what += " (ops with a difference: %s)" % sorted({e.index for e in found})
        raise SequenceMismatch(first.index, first.op, first.what, seq)


# ---- what the lists of a set of seeds contain (tests/test_call_sequences_driver.py asserts it of the seeds in use) -------
TRIPLES = {
    "edit -> params(re-grid) -> step": lambda a, b, c: a.cls == "edit" and regrids(b) and c.cls == "step",
    "edit -> read -> step": lambda a, b, c: a.cls == "edit" and b.cls == "read" and c.cls == "step",
    "host(write) -> edit -> step": lambda a, b, c: a.name == "write" and b.cls == "edit" and c.cls == "step",
    "edit -> host(reset) -> edit": lambda a, b, c: a.cls == "edit" and b.name == "reset" and c.cls == "edit",
    "step -> params(re-grid) -> read_vec": lambda a, b, c: a.cls == "step" and regrids(b) and c.name == "read_vec",
    # (for the captured-step test: a ws_set_params that a capture must survive)
    "step -> params(same) -> step": lambda a, b, c: a.cls == "step" and b.variant == "same" and c.cls == "step",
}


def coverage(seqs):
    """What the lists lack: catalogue ops, ordered pairs of classes and the named triples that never occur, and the
    positions of a ws_collide_volumes before any upload."""
    keys = {op.key for s in seqs for op in s}
    pairs = {(a.cls, b.cls) for s in seqs for a, b in zip(s, s[1:])}
    triples = [(a, b, c) for s in seqs for a, b, c in zip(s, s[1:], s[2:])]
    early = [(k, i) for k, s in enumerate(seqs) for i, op in enumerate(s)
             if op.name == "collide_volumes" and not any(o.name == "upload_volume" for o in s[:i])]
    return dict(ops=sorted(set(k for c in CATALOGUE.values() for k in c) - keys, key=str),
                pairs=sorted({(a, b) for a in CLASSES for b in CLASSES} - pairs),
                triples=sorted(name for name, hit in TRIPLES.items() if not any(hit(*t) for t in triples)),
                early_volumes=early)
