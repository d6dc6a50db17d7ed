"""numpy restatement of ws_cast_rays / ws_cast_camera (include/wsfluid.h): the march, the bisection, the normal and the
camera's rays in float32, every operation rounded once, over a field given as a callable

    field(points (m, 3) float32) -> (rho (m,) float32, gradient (m, 3) float32)

-- an analytic field on the CPU, or the library's own ws_sample_density_points / ws_sample_aniso_points on the GPU (then
the restatement and ws_cast_rays must agree bit for bit).  The field is called once per march step and once per
bisection step, on the rays still concerned."""
from collections import namedtuple

import numpy as np

F32 = np.float32

March = namedtuple("March", "t_start dt steps refine iso")


def sample_t(march, k):
    """t_k = fl(t_start + fl((float)k * dt)); k a scalar or an integer array."""
    return (F32(march.t_start) + np.asarray(k).astype(F32) * F32(march.dt)).astype(F32)


def points(o, v, t):
    """p_a(t) = fl(o_a + fl(t * v_a)); t one parameter per ray."""
    t = np.broadcast_to(np.asarray(t, F32), (len(o),))
    return (o + (t[:, None] * v).astype(F32)).astype(F32)


def cast(field, march, origins, directions, normals=True):
    """(t (m,) float32 with +inf on a miss, normal (m, 3) float32 or None, K (m,) int: the hit index, -1 on a miss)."""
    o = np.ascontiguousarray(origins, F32).reshape(-1, 3)
    v = np.ascontiguousarray(directions, F32).reshape(-1, 3)
    m = len(o)
    iso = F32(march.iso)
    K = np.full(m, -1, np.int64)
    alive = np.arange(m)
    for k in range(int(march.steps) + 1):
        if alive.size == 0:
            break
        rho, _ = field(points(o[alive], v[alive], sample_t(march, k)))
        hit = rho >= iso
        K[alive[hit]] = k
        alive = alive[~hit]
    t = np.full(m, np.inf, F32)
    t[K == 0] = sample_t(march, 0)
    b = np.flatnonzero(K >= 1)
    if b.size:
        lo, hi = sample_t(march, K[b] - 1), sample_t(march, K[b])
        for _ in range(int(march.refine)):  # exactly `refine` times, no early exit
            mid = ((lo + hi).astype(F32) * F32(0.5)).astype(F32)
            rho, _ = field(points(o[b], v[b], mid))
            inside = rho >= iso
            hi = np.where(inside, mid, hi)
            lo = np.where(inside, lo, mid)
        t[b] = hi
    if not normals:
        return t, None, K
    n = np.zeros((m, 3), F32)
    h = np.flatnonzero(K >= 0)
    if h.size:
        _, g = field(points(o[h], v[h], t[h]))
        g = np.asarray(g, F32)
        gg = ((g[:, 0] * g[:, 0]).astype(F32) + (g[:, 1] * g[:, 1]).astype(F32)).astype(F32)
        gg = (gg + (g[:, 2] * g[:, 2]).astype(F32)).astype(F32)
        ok = gg != 0
        length = np.sqrt(gg[ok], dtype=F32)
        n[h[ok]] = (-g[ok] / length[:, None]).astype(F32)
    return t, n, K


def camera_rays(eye, forward, right, up, size):
    """(origins, directions), (H * W, 3) float32 each, x fastest: pixel (i, j) of a size = (W, H) image has
    u = ((float)i + 0.5f) * (2.0f / (float)W) - 1.0f, w = 1.0f - ((float)j + 0.5f) * (2.0f / (float)H),
    v = (forward + u * right) + w * up, o = eye."""
    W, H = int(size[0]), int(size[1])
    e, f, r, q = (np.asarray(a, F32).reshape(3) for a in (eye, forward, right, up))
    u = (((np.arange(W, dtype=F32) + F32(0.5)) * (F32(2) / F32(W))).astype(F32) - F32(1)).astype(F32)
    w = (F32(1) - ((np.arange(H, dtype=F32) + F32(0.5)) * (F32(2) / F32(H))).astype(F32)).astype(F32)
    uu = np.tile(u, H)
    ww = np.repeat(w, W)
    v = ((f[None, :] + (uu[:, None] * r[None, :]).astype(F32)).astype(F32) + (ww[:, None] * q[None, :]).astype(F32)).astype(F32)
    return np.tile(e, (W * H, 1)).astype(F32), v
