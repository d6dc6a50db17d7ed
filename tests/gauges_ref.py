"""numpy restatement of the gauges (include/wsfluid.h "gauges"): ws_measure's count, fixed-point sums and extremes per
region, and ws_select_particles' id list -- float32 with every operation rounded once in the header's order, the sums as
int64 sums that wrap modulo 2^64, the extremes under the key order of the floats' bits.  measure_loop is the same
definition once more as a plain loop over particles and regions with scalar arithmetic, written to share nothing with the
vectorised form but the header: the restatement is checked against it (tests/test_gauges_reference.py).

A region is population_ref's sink dict {kind, centre, half}.  A result is a dict of arrays like the binding's Gauges:
count (k,) uint64; sum_pos, sum_vel, sum_ang (k, 3), sum_speed2 (k,), sum_attr (k, 4) int64; min_pos, max_pos (k, 3),
max_speed2 (k,) float32."""
import struct

import numpy as np

from forces_ref import dot
from population_ref import BOX, SPHERE, contains, sink as region, to_ws  # noqa: F401  (re-exported for the tests)

F32 = np.float32
FIX = 24
CLAMP = F32(2.0 ** 31)
FIELDS = ("count", "sum_pos", "sum_vel", "sum_ang", "sum_speed2", "sum_attr", "min_pos", "max_pos", "max_speed2")


def key(x):
    """The total order of the extremes: bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), uint32."""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F32)


def quantise(t):
    """llrintf(fminf(fmaxf(t, -2^31), 2^31) * 2^24) of float32 values, int64 (fmaxf drops a NaN: -2^31)."""
    t = np.fmin(np.fmax(np.asarray(t, F32), -CLAMP), CLAMP)
    scaled = t.astype(np.float64) * 2.0 ** FIX  # exact: a float32 times a power of two, at most 2^55
    return np.rint(scaled).astype(np.int64)


def wrap(total):
    """A Python integer modulo 2^64 as the int64 the device holds."""
    return ((int(total) + (1 << 63)) % (1 << 64)) - (1 << 63)


def fixed_sum(t, inside):
    """The sum modulo 2^64: numpy's int64 sum wraps, as the device's does (measure_loop adds Python integers and wraps
    once at the end: the same residue)."""
    return int(quantise(np.asarray(t, F32)[inside]).sum(dtype=np.int64))


def empty(k):
    return dict(count=np.zeros(k, np.uint64), sum_pos=np.zeros((k, 3), np.int64), sum_vel=np.zeros((k, 3), np.int64),
                sum_ang=np.zeros((k, 3), np.int64), sum_speed2=np.zeros(k, np.int64), sum_attr=np.zeros((k, 4), np.int64),
                min_pos=np.full((k, 3), np.inf, F32), max_pos=np.full((k, 3), -np.inf, F32), max_speed2=np.zeros(k, F32))


def measure(pos, vel, regions, attr=None):
    """ws_measure.  attr: the (n, 4) attributes with WS_GAUGE_ATTRIBUTES on a handle that has them, else None."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    v = np.ascontiguousarray(vel, F32).reshape(-1, 3)
    out = empty(len(regions))
    with np.errstate(over="ignore", invalid="ignore"):
        s2 = dot(v, v)
        for e, s in enumerate(regions):
            inside = contains(x, s)
            out["count"][e] = np.count_nonzero(inside)
            if not inside.any():
                continue
            q = (x - s["centre"].astype(F32)).astype(F32)
            ang = np.stack([q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1], q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2],
                            q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0]], axis=1).astype(F32)
            for c in range(3):
                out["sum_pos"][e, c] = fixed_sum(x[:, c], inside)
                out["sum_vel"][e, c] = fixed_sum(v[:, c], inside)
                out["sum_ang"][e, c] = fixed_sum(ang[:, c], inside)
                k = key(x[inside, c])
                out["min_pos"][e, c] = unkey(k.min())
                out["max_pos"][e, c] = unkey(k.max())
            out["sum_speed2"][e] = fixed_sum(s2, inside)
            for c in range(4 if attr is not None else 0):
                out["sum_attr"][e, c] = fixed_sum(np.ascontiguousarray(attr, F32).reshape(-1, 4)[:, c], inside)
            fast = s2[inside]
            fast = fast[~np.isnan(fast)]  # fmaxf skips a NaN; the maximum starts from +0
            out["max_speed2"][e] = unkey(max([0x80000000] + [int(t) for t in key(fast)]))  # (0x80000000: the key of +0)
    return out


def select(pos, regions):
    """ws_select_particles with cap >= total: the ids at least one region contains, ascending."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    inside = np.zeros(len(x), bool)
    for s in regions:
        inside |= contains(x, s)
    return np.flatnonzero(inside).astype(np.uint32)


# ---- the same definition as a loop over particles: scalar float32 arithmetic, struct for the bits ---------------------------
def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _order(x):
    b = _bits(x)
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def _fixed(t):
    t = float(t)
    if t != t or t < -2.0 ** 31:  # fmaxf(NaN, -2^31) = -2^31
        t = -2.0 ** 31
    if t > 2.0 ** 31:
        t = 2.0 ** 31
    return round(t * 2.0 ** FIX)  # exact product; round() rounds a tie to even, as llrintf does


def _inside(p, s):
    with np.errstate(over="ignore", invalid="ignore"):
        q = [F32(p[a]) - F32(s["centre"][a]) for a in range(3)]
        if s["kind"] == SPHERE:
            d = np.sqrt(F32(F32(F32(q[0] * q[0]) + F32(q[1] * q[1])) + F32(q[2] * q[2])))
            return bool(d < F32(s["half"][0])), q
        return all(bool(abs(q[a]) <= F32(s["half"][a])) for a in range(3)), q


def measure_loop(pos, vel, regions, attr=None):
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    v = np.ascontiguousarray(vel, F32).reshape(-1, 3)
    out = empty(len(regions))
    for e, s in enumerate(regions):
        count, sums = 0, [0] * 14
        lo, hi, fast = [F32(np.inf)] * 3, [F32(-np.inf)] * 3, F32(0.0)
        for i in range(len(x)):
            yes, q = _inside(x[i], s)
            if not yes:
                continue
            count += 1
            with np.errstate(over="ignore", invalid="ignore"):
                vi = [F32(t) for t in v[i]]
                ang = [F32(F32(q[1] * vi[2]) - F32(q[2] * vi[1])), F32(F32(q[2] * vi[0]) - F32(q[0] * vi[2])),
                       F32(F32(q[0] * vi[1]) - F32(q[1] * vi[0]))]
                s2 = F32(F32(F32(vi[0] * vi[0]) + F32(vi[1] * vi[1])) + F32(vi[2] * vi[2]))
            terms = [x[i, 0], x[i, 1], x[i, 2]] + vi + ang + [s2] + ([F32(t) for t in attr[i]] if attr is not None else [])
            for c, t in enumerate(terms):
                sums[c] += _fixed(t)
            for a in range(3):
                if _order(x[i, a]) < _order(lo[a]):
                    lo[a] = x[i, a]
                if _order(x[i, a]) > _order(hi[a]):
                    hi[a] = x[i, a]
            if s2 == s2 and _order(s2) > _order(fast):
                fast = s2
        out["count"][e] = count
        w = [wrap(t) for t in sums]
        out["sum_pos"][e], out["sum_vel"][e], out["sum_ang"][e] = w[0:3], w[3:6], w[6:9]
        out["sum_speed2"][e], out["sum_attr"][e] = w[9], w[10:14]
        out["min_pos"][e], out["max_pos"][e], out["max_speed2"][e] = lo, hi, fast
    return out


def select_loop(pos, regions):
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    return np.array([i for i in range(len(x)) if any(_inside(x[i], s)[0] for s in regions)], np.uint32)


def same(got, want):
    """Every field of every gauge, bit for bit (the floats by their bits: -0 is not +0)."""
    bad = []
    for name in FIELDS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.tobytes() != b.astype(a.dtype).tobytes():
            bad.append(name)
    return bad
