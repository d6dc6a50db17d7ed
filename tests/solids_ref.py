"""numpy restatement of ws_collide_solids (include/wsfluid.h): the signed distances, the push-out, the velocity response
and the container rule in float32 with every operation rounded once, in the header's order -- the library's bits -- the
reaction as fixed-point sums in Python integers, and a float64 evaluation of the same formulas that knows nothing of the
roundings.

A solid is a dict {kind, flags, centre, rot (3, 3), size, velocity, angular_velocity, restitution, friction, margin}
(solid() builds one; to_ws() turns a list into the binding's WsSolid records)."""
import numpy as np

F32 = np.float32
SPHERE, BOX, CAPSULE = 0, 1, 2
HOLLOW = 1
LOOKAHEAD = F32(0.02)  # the step's look-ahead: pred = fl(p + fl(v * 0.02f))
FIX = 24               # fractional bits of the fixed-point sums
CLAMP = F32(2.0 ** 31)
MASK64 = (1 << 64) - 1


def solid(kind, centre, size, rot=None, hollow=False, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0),
          restitution=0.0, friction=0.0, margin=0.0):
    size = np.atleast_1d(np.asarray(size, F32))
    return dict(kind=int(kind), flags=HOLLOW if hollow else 0, centre=np.asarray(centre, F32),
                rot=np.asarray(np.eye(3) if rot is None else rot, F32).reshape(3, 3),
                size=np.concatenate([size, np.zeros(3 - len(size), F32)]).astype(F32), velocity=np.asarray(velocity, F32),
                angular_velocity=np.asarray(angular_velocity, F32), restitution=F32(restitution), friction=F32(friction),
                margin=F32(margin))


def rotation(axis, angle):
    """A rotation matrix (rows = the local axes in world coordinates), float32."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt(a @ a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).T.astype(F32)


def to_ws(ws, solids):
    return [ws.fluid.solid(s["kind"], [float(c) for c in s["centre"]], [float(x) for x in s["size"]],
                           rot=[float(x) for x in s["rot"].reshape(-1)], hollow=bool(s["flags"] & HOLLOW),
                           velocity=[float(x) for x in s["velocity"]], angular_velocity=[float(x) for x in s["angular_velocity"]],
                           restitution=float(s["restitution"]), friction=float(s["friction"]), margin=float(s["margin"]))
            for s in solids]


def dot(a, b):
    """fl(fl(fl(a.x b.x) + fl(a.y b.y)) + fl(a.z b.z)) over the last axis (the whitewater block's dot)."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """a x b: each product rounded, then the difference."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def distance(p, s, T=F32):
    """Steps 1-2 of the definition in the arithmetic T: (signed distance s (n,), outward unit normal n (n, 3))."""
    p = np.asarray(p, T).reshape(-1, 3)
    c, R, size = s["centre"].astype(T), s["rot"].astype(T), s["size"].astype(T)
    one, zero = T(1), T(0)
    q = p - c
    with np.errstate(divide="ignore", invalid="ignore"):
        if s["kind"] == SPHERE:
            d = np.sqrt(dot(q, q))
            sd = d - size[0]
            n = np.where((d > 0)[:, None], q / d[:, None], np.array([0, 1, 0], T))
        elif s["kind"] == CAPSULE:
            l1 = dot(R[1][None, :], q)
            t = np.fmin(np.fmax(l1, -size[1]), size[1])
            w = q - t[:, None] * R[1][None, :]
            d = np.sqrt(dot(w, w))
            sd = d - size[0]
            n = np.where((d > 0)[:, None], w / d[:, None], R[0][None, :])
        else:
            l = np.stack([dot(R[i][None, :], q) for i in range(3)], axis=1)
            a = np.abs(l) - size[None, :]
            g = np.fmax(np.fmax(a[:, 0], a[:, 1]), a[:, 2])
            u = np.copysign(np.fmax(a, zero), l)
            d = np.sqrt(dot(u, u))
            outside = g > 0
            star = np.argmax(a == g[:, None], axis=1)  # the lowest i with a_i == g
            face = np.zeros_like(l)
            face[np.arange(len(l)), star] = np.copysign(one, l[np.arange(len(l)), star])
            m = np.where(outside[:, None], u / d[:, None], face)
            sd = np.where(outside, d, g)
            n = (m[:, 0:1] * R[0][None, :] + m[:, 1:2] * R[1][None, :]) + m[:, 2:3] * R[2][None, :]
    if s["flags"] & HOLLOW:
        sd, n = -sd, -n
    return sd.astype(T), n.astype(T)


def quantise(x):
    """llrintf(fminf(fmaxf(x, -2^31), 2^31) * 2^24) of float32 values, as Python integers (object array)."""
    x = np.fmin(np.fmax(np.asarray(x, F32), -CLAMP), CLAMP)
    scaled = x.astype(np.float64) * 2.0 ** FIX  # exact: a float32 times a power of two
    return np.rint(scaled).astype(np.int64).astype(object)


def collide(pos, vel, solids, ext_min, ext_max, damping, T=F32, contact32=None):
    """The call in the arithmetic T.  Returns a dict: pos, vel, pred (n, 3), touched (n,) bool, contacts (k,) uint32,
    hit (k, n) bool, dv (k, n, 3) and r (k, n, 3) (the velocity change and the lever arm of every contact, zero elsewhere),
    impulse / angular (k, 3) float64 from the fixed-point sums, sums (k, 6) Python integers modulo 2^64.
    contact32: the (k, n) contact decisions to use instead of T's own (the float32 evaluation defines them)."""
    p = np.array(pos, T).reshape(-1, 3)
    v = np.array(vel, T).reshape(-1, 3)
    n_p, k = len(p), len(solids)
    touched = np.zeros(n_p, bool)
    hits = np.zeros((k, n_p), bool)
    dvs = np.zeros((k, n_p, 3), T)
    rs = np.zeros((k, n_p, 3), T)
    sums = np.zeros((k, 6), object)
    one = T(1)
    with np.errstate(over="ignore", invalid="ignore"):
        for e, s in enumerate(solids):
            c, V, W = s["centre"].astype(T), s["velocity"].astype(T), s["angular_velocity"].astype(T)
            sd, n = distance(p, s, T)
            hit = (sd < T(s["margin"])) if contact32 is None else contact32[e]
            hits[e] = hit
            touched |= hit
            pn = p + (T(s["margin"]) - sd)[:, None] * n
            r = pn - c
            u = V[None, :] + cross(W[None, :], r)
            rel = v - u
            vn = dot(rel, n)
            kicked = hit & (vn < 0)
            j = (one + T(s["restitution"])) * (-vn)
            tang = rel - vn[:, None] * n
            dv = j[:, None] * n - T(s["friction"]) * tang
            p = np.where(hit[:, None], pn, p).astype(T)
            v = np.where(kicked[:, None], v + dv, v).astype(T)
            dvs[e] = np.where(kicked[:, None], dv, 0)
            rs[e] = np.where(hit[:, None], r, 0)
            if T is F32 and kicked.any():
                I = (-dv[kicked]).astype(F32)
                H = cross(r[kicked].astype(F32), I).astype(F32)
                six = np.concatenate([quantise(I), quantise(H)], axis=1)
                sums[e] = [int(sum(six[:, w])) & MASK64 for w in range(6)]
        nd = T(-1) * T(damping)
        lo, hi = np.asarray(ext_min, T)[:3], np.asarray(ext_max, T)[:3]
        below, above = touched[:, None] & (p < lo), touched[:, None] & ~(p < lo) & (p > hi)
        v = np.where(below | above, v * nd, v).astype(T)
        p = np.where(below, lo, np.where(above, hi, p)).astype(T)
        pred = (p + (v * T(LOOKAHEAD)).astype(T)).astype(T)

    def signed(x):
        return x - (1 << 64) if x >> 63 else x

    flat = np.array([[float(signed(int(x))) * 2.0 ** -FIX for x in row] for row in sums], np.float64).reshape(k, 6)
    return dict(pos=p, vel=v, pred=pred, touched=touched, contacts=hits.sum(axis=1).astype(np.uint32), hit=hits, dv=dvs, r=rs,
                impulse=flat[:, :3].copy(), angular=flat[:, 3:].copy(), sums=sums)
