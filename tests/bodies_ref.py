"""numpy restatement of ws_body_forces (include/wsfluid.h): a sample's terms in float32 with every operation rounded once,
in the header's order, and a body's canonical sum -- the fixed binary tree over the body's samples, padded with +0 to the
smallest power of two above their number -- which are the library's bits; and a float64 evaluation of the same formulas
that knows nothing of the roundings or of the order.

The field (u, rho) at the samples is an input: what ws_sample_velocity_points returns there.  params is a dict
{fluid_density, drag, rest_density} (defaults() has the library's); rho_0 comes from rest_density_of()."""
import math

import numpy as np

F32 = np.float32


def defaults():
    """ws_default_body_params as a dict."""
    return dict(fluid_density=F32(1000.0), drag=F32(500.0), rest_density=F32(0.0))


def rest_density_of(params, target_density):
    """rho_0: rest_density, or the handle's target_density when rest_density is 0."""
    r = F32(params["rest_density"])
    return F32(target_density) if r == 0 else r


def _f32(x):
    return np.asarray(x, F32)


def sample_terms(params, g, rho0, u, rho, p, w, V, c):
    """Steps 2-4 of the definition for m samples: (F (m, 3), T (m, 3), vol (m,), f (m,) float32, wet (m,) bool).
    g: the gravity (3,); rho0: rest_density_of(); u (m, 3), rho (m,): the field at the samples; p, w (m, 3), V (m,): the
    samples; c: the centre of each sample's body, (m, 3) or one (3,) for all."""
    g, rho0 = _f32(g).reshape(3), F32(rho0)
    u, p, w = (_f32(a).reshape(-1, 3) for a in (u, p, w))
    rho, V = _f32(rho).reshape(-1), _f32(V).reshape(-1)
    c = np.broadcast_to(_f32(c), p.shape)
    fd, drag = F32(params["fluid_density"]), F32(params["drag"])
    wet = rho > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = np.fmin((rho / rho0).astype(F32), F32(1.0))              # fminf(rho / rho_0, 1)
        vol = (V * f).astype(F32)
        lift = (fd * vol).astype(F32)
        kd = (drag * vol).astype(F32)
        du = (u - w).astype(F32)
        F = ((kd[:, None] * du).astype(F32) - (lift[:, None] * g[None, :]).astype(F32)).astype(F32)
    T = torque_terms(p, c, F)
    zero = F32(0.0)
    f = np.where(wet, f, zero).astype(F32)
    vol = np.where(wet, vol, zero).astype(F32)
    F = np.where(wet[:, None], F, zero).astype(F32)
    T = np.where(wet[:, None], T, zero).astype(F32)
    return F, T, vol, f, wet


def torque_terms(p, c, F):
    """Step 4 for wet samples: r_a = fl(p_a - c_a), T_x = fl(fl(r_y F_z) - fl(r_z F_y)) and cyclically, (m, 3) float32."""
    p, F = _f32(p).reshape(-1, 3), _f32(F).reshape(-1, 3)
    c = np.broadcast_to(_f32(c), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (p - c).astype(F32)

        def cross(a, b):
            return ((r[:, a] * F[:, b]).astype(F32) - (r[:, b] * F[:, a]).astype(F32)).astype(F32)

        return np.stack([cross(1, 2), cross(2, 0), cross(0, 1)], axis=1)


def tree_sum(t, leaves=None):
    """The canonical sum over axis 0 of t (c,) or (c, k) float32: P = the smallest power of two > c leaves (or `leaves`, a
    larger power of two: further padding), t then +0, every level v[i] = fl(v[2i] + v[2i+1])."""
    t = _f32(t)
    c = t.shape[0]
    P = 1
    while P <= c:
        P *= 2
    if leaves is not None:
        assert leaves >= P and leaves & (leaves - 1) == 0
        P = leaves
    v = np.zeros((P,) + t.shape[1:], F32)
    v[:c] = t
    with np.errstate(over="ignore", invalid="ignore"):
        while v.shape[0] > 1:
            v = (v[0::2] + v[1::2]).astype(F32)
    return v[0]


def reduce(body_start, F, T, vol, wet):
    """The per-body outputs: (force (nb, 3), torque (nb, 3), volume (nb,) float32, wet (nb,) uint32)."""
    bs = np.asarray(body_start, np.int64)
    nb = len(bs) - 1
    force, torque = np.zeros((nb, 3), F32), np.zeros((nb, 3), F32)
    volume, count = np.zeros(nb, F32), np.zeros(nb, np.uint32)
    for b in range(nb):
        s = slice(bs[b], bs[b + 1])
        force[b], torque[b], volume[b] = tree_sum(F[s]), tree_sum(T[s]), tree_sum(vol[s])
        count[b] = np.count_nonzero(wet[s])
    return force, torque, volume, count


def body_of_sample(body_start):
    """(m,) int: the body every sample belongs to."""
    bs = np.asarray(body_start, np.int64)
    return np.repeat(np.arange(len(bs) - 1), np.diff(bs))


def forces(params, g, target_density, u, rho, p, w, V, body_start, centres):
    """The whole call on the field (u, rho): a dict of the six outputs."""
    c = _f32(centres).reshape(-1, 3)[body_of_sample(body_start)]
    F, T, vol, f, wet = sample_terms(params, g, rest_density_of(params, target_density), u, rho, p, w, V, c)
    force, torque, volume, count = reduce(body_start, F, T, vol, wet)
    return dict(force=force, torque=torque, volume=volume, wet=count, sample_force=F, sample_fraction=f)


# ---- float64: the same formulas, no float32 rounding, any order ---------------------------------------------------------
def sample_terms64(params, g, rho0, u, rho, p, w, V, c):
    """sample_terms in float64 from the float32 inputs (wet is rho > 0 either way)."""
    g = np.asarray(g, np.float64).reshape(3)
    u, p, w = (np.asarray(a, np.float64).reshape(-1, 3) for a in (u, p, w))
    rho, V = np.asarray(rho, np.float64).reshape(-1), np.asarray(V, np.float64).reshape(-1)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    wet = rho > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(wet, np.minimum(rho / float(rho0), 1.0), 0.0)
    vol = V * f
    F = (float(params["drag"]) * vol)[:, None] * (u - w) - (float(params["fluid_density"]) * vol)[:, None] * g[None, :]
    F = np.where(wet[:, None], F, 0.0)
    T = np.where(wet[:, None], np.cross(p - c, F), 0.0)
    return F, T, vol, f, wet


def tree_sum64(t):
    """The exact sum of a 1-D array, rounded once to float64 (math.fsum)."""
    return math.fsum(float(x) for x in np.asarray(t).reshape(-1))


def reduce64(body_start, F, T, vol, wet):
    bs = np.asarray(body_start, np.int64)
    nb = len(bs) - 1
    force, torque, volume = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros(nb)
    count = np.zeros(nb, np.uint32)
    for b in range(nb):
        s = slice(bs[b], bs[b + 1])
        for a in range(3):
            force[b, a], torque[b, a] = tree_sum64(F[s, a]), tree_sum64(T[s, a])
        volume[b] = tree_sum64(vol[s])
        count[b] = np.count_nonzero(wet[s])
    return force, torque, volume, count
