"""numpy restatement of ws_apply_forces (include/wsfluid.h): the emitters' acceleration and the Euler step in float32
with every operation rounded once, in the header's order -- the library's bits -- and a float64 evaluation of the same
formulas that knows nothing of the roundings.

An emitter is a dict {kind, centre, axis, radius, strength, damping} (emitter() builds one; to_ws() turns a list into the
binding's WsForce records)."""
import numpy as np

F32 = np.float32
RADIAL, JET, VORTEX = 0, 1, 2
LOOKAHEAD = F32(0.02)  # the step's look-ahead: pred = fl(x + fl(v * 0.02f))


def emitter(kind, centre, radius, strength, axis=(0.0, 0.0, 0.0), damping=0.0):
    return dict(kind=int(kind), centre=np.asarray(centre, F32), axis=np.asarray(axis, F32), radius=F32(radius),
                strength=F32(strength), damping=F32(damping))


def to_ws(ws, forces):
    return [ws.fluid.force(f["kind"], [float(c) for c in f["centre"]], float(f["radius"]), float(f["strength"]),
                           [float(a) for a in f["axis"]], float(f["damping"])) for f in forces]


def dot(a, b):
    """fl(fl(fl(a.x b.x) + fl(a.y b.y)) + fl(a.z b.z)) over the last axis, float32 (the whitewater block's dot)."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F32)


def cross(a, q):
    """t = a x q: each product rounded, then the difference."""
    return np.stack([a[1] * q[:, 2] - a[2] * q[:, 1], a[2] * q[:, 0] - a[0] * q[:, 2], a[0] * q[:, 1] - a[1] * q[:, 0]],
                    axis=1).astype(F32)


def accelerate(pos, vel, forces):
    """(A (n, 3) float32, affected (n,) bool, counts (k,) uint32): steps 1-4 of the definition."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    v = np.ascontiguousarray(vel, F32).reshape(-1, 3)
    A = np.zeros_like(x)
    hit = np.zeros(len(x), bool)
    counts = np.zeros(len(forces), np.uint32)
    for e, f in enumerate(forces):
        c, a, R = f["centre"].astype(F32), f["axis"].astype(F32), F32(f["radius"])
        q = (x - c).astype(F32)
        d = np.sqrt(dot(q, q)).astype(F32)
        with np.errstate(invalid="ignore"):
            seen = d < R
        counts[e] = np.count_nonzero(seen)
        hit |= seen
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w = (F32(1) - (d / R).astype(F32)).astype(F32)
            s = (F32(f["strength"]) * w).astype(F32)
            if f["kind"] == RADIAL:
                term = ((q / d[:, None]).astype(F32) * s[:, None]).astype(F32)
                An = np.where((d > 0)[:, None], (A - term).astype(F32), A)
            elif f["kind"] == JET:
                An = (A + (a[None, :] * s[:, None]).astype(F32)).astype(F32)
            else:
                An = (A + (cross(a, q) * s[:, None]).astype(F32)).astype(F32)
            g = (F32(f["damping"]) * w).astype(F32)
            An = (An - (v * g[:, None]).astype(F32)).astype(F32)
        A = np.where(seen[:, None], An, A)
    return A, hit, counts


def apply(pos, vel, forces, dt):
    """(vel', pred', counts): the velocities after the call (unseen particles keep their bits), the predicted positions
    the library derives from them, and the per-emitter counts of affected particles."""
    x = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    v = np.ascontiguousarray(vel, F32).reshape(-1, 3)
    A, hit, counts = accelerate(x, v, forces)
    with np.errstate(over="ignore", invalid="ignore"):
        moved = (v + (F32(dt) * A).astype(F32)).astype(F32)
        vn = np.where(hit[:, None], moved, v)
        pred = (x + (vn * LOOKAHEAD).astype(F32)).astype(F32)
    return vn, pred, counts


def apply64(pos, vel, forces, dt):
    """The same formulas in float64 from the float32 inputs: (vel', affected).  Membership (d < R) is taken from the
    float32 evaluation, which defines it."""
    x = np.asarray(pos, np.float64).reshape(-1, 3)
    v = np.asarray(vel, np.float64).reshape(-1, 3)
    A = np.zeros_like(x)
    hit = np.zeros(len(x), bool)
    for f in forces:
        c, a, R = f["centre"].astype(np.float64), f["axis"].astype(np.float64), float(f["radius"])
        q32 = (np.asarray(pos, F32).reshape(-1, 3) - f["centre"].astype(F32)).astype(F32)
        with np.errstate(invalid="ignore"):
            seen = np.sqrt(dot(q32, q32)).astype(F32) < F32(R)
        q = x - c
        d = np.sqrt((q * q).sum(axis=1))
        w = 1.0 - d / R
        s = float(f["strength"]) * w
        if f["kind"] == RADIAL:
            with np.errstate(divide="ignore", invalid="ignore"):
                term = np.where((d > 0)[:, None], -(q / d[:, None]) * s[:, None], 0.0)
        elif f["kind"] == JET:
            term = a[None, :] * s[:, None]
        else:
            term = np.cross(a[None, :], q) * s[:, None]
        term = term - v * (float(f["damping"]) * w)[:, None]
        A = np.where(seen[:, None], A + term, A)
        hit |= seen
    return np.where(hit[:, None], v + float(dt) * A, v), hit
