"""numpy restatement of the count-changing calls (include/wsfluid.h "pouring water in and draining it"): which sink contains
which particle, float32 with every operation rounded once in the header's order; which sink claims it; the survivors'
new ids; and the records a handle must hold afterwards.

A sink is a dict {kind, centre, half} (sink() builds one; to_ws() turns a list into the binding's WsSink records).  The
state of a handle is the triple (pos (n, 3), vel (n, 3), attr (n, 4)) by id."""
import numpy as np

from forces_ref import dot

F32 = np.float32
SPHERE, BOX = 0, 1
REMOVED = np.uint32(0xFFFFFFFF)


def sink(kind, centre, half):
    """half: the box's three half extents, or the sphere's radius (a number)."""
    if np.ndim(half) == 0:
        half = (half, 0.0, 0.0)
    return dict(kind=int(kind), centre=np.asarray(centre, F32), half=np.asarray(half, F32))


def to_ws(ws, sinks):
    return [ws.fluid.sink(s["kind"], [float(c) for c in s["centre"]], [float(x) for x in s["half"]]) for s in sinks]


def contains(pos, s):
    """(n,) bool: step 1 of the definition.  The sphere's d is ws_apply_forces' (forces_ref.accelerate)."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    q = (x - s["centre"].astype(F32)).astype(F32)
    with np.errstate(invalid="ignore"):
        if s["kind"] == SPHERE:
            d = np.sqrt(dot(q, q)).astype(F32)
            return d < F32(s["half"][0])
        return np.all(np.abs(q) <= s["half"].astype(F32)[None, :], axis=1)


def claims(pos, sinks):
    """(owner (n,) int32: the first sink that contains the particle, or -1; counts (k,) uint32)."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    owner = np.full(len(x), -1, np.int32)
    for e, s in enumerate(sinks):
        owner[(owner < 0) & contains(x, s)] = e
    counts = np.array([np.count_nonzero(owner == e) for e in range(len(sinks))], np.uint32)
    return owner, counts


def keep_of_ids(n, ids):
    """(n,) bool: who stays when the particles named in ids go (an id may be named more than once)."""
    keep = np.ones(n, bool)
    keep[np.asarray(ids, np.int64)] = False
    return keep


def renumber(keep):
    """(n,) uint32: a survivor's new id = its rank among the survivors by old id; REMOVED for the others."""
    keep = np.asarray(keep, bool)
    new = (np.cumsum(keep) - 1).astype(np.uint32)
    new[~keep] = REMOVED
    return new


def remove(state, keep):
    """The state after the removal and the id map: survivors keep their bits and their attributes, in id order."""
    pos, vel, attr = state
    keep = np.asarray(keep, bool)
    return (pos[keep].copy(), vel[keep].copy(), attr[keep].copy()), renumber(keep)


def remove_by_sinks(state, sinks):
    """(state', counts, new ids)."""
    owner, counts = claims(state[0], sinks)
    after, new = remove(state, owner < 0)
    return after, counts, new


def add(state, pos, vel=None, attr=None):
    """The new particles behind the old ones, ids n .. n+m-1 in the order given; at rest / +0 where nothing is given."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    v = np.zeros_like(p) if vel is None else np.ascontiguousarray(vel, F32).reshape(-1, 3)
    a = np.zeros((len(p), 4), F32) if attr is None else np.ascontiguousarray(attr, F32).reshape(-1, 4)
    return (np.concatenate([state[0], p]), np.concatenate([state[1], v]), np.concatenate([state[2], a]))


def predicted(state):
    """pred = fl(x + fl(v * 0.02f)): what every particle's predicted position is after a count change."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (state[0] + (state[1] * F32(0.02)).astype(F32)).astype(F32)
