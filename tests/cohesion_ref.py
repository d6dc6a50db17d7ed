"""numpy restatement of the surface-tension and XSPH calls (include/wsfluid.h, ws_read_cohesion / ws_apply_cohesion): the
per-particle stage in float32 with every operation rounded once and the candidates in the canonical order of the
handle's grid (aniso_ref's Grid / Binned / _near, merged grids included) -- the library's bits --, apply(), which returns
v', and a float64 brute force over ALL pairs that knows nothing of the grid and also returns, per particle and quantity,
the sum of the absolute pair terms a float32 result is judged against."""
import numpy as np

import aniso_ref as A

F32 = np.float32
U32 = np.uint32
OUTPUTS = ("normal", "density", "dv", "neighbours")  # what ws_read_cohesion returns


def defaults():
    """ws_default_cohesion_params as a dict."""
    return dict(cohesion=1.0, curvature=1.0, xsph=0.1, rest_density=0.0)


def _f32(a):
    return np.ascontiguousarray(a, F32)


def constants(h):
    """(kc, h664) of the header, as float32 operations in its order."""
    h = F32(h)
    h3 = F32(F32(h * h) * h)
    h6 = F32(h3 * h3)
    h9 = F32(h6 * h3)
    return F32(F32(32.0) / F32(F32(3.14159274) * h9)), F32(h6 * F32(0.015625))


def rest_density(params, cp):
    rho0 = F32(cp["rest_density"])
    return F32(params.target_density) if rho0 == 0 else rho0


# ---- the stage -----------------------------------------------------------------------------------------------------------
def normals(params, x, merged=(1, 1, 1), bins=None):
    """Pass A: (n (n, 3), rho (n,)) -- the density sampler's IEEE sums at every particle, as n = (h g) / rho and rho."""
    h, p2, p2d = A._kernel(params)
    x = _f32(x).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = bins or A.Binned(grid, x)
    g = np.zeros((len(x), 3), F32)
    rho = np.zeros(len(x), F32)
    for s0 in range(0, len(x), grid.chunk()):
        sl = slice(s0, min(len(x), s0 + grid.chunk()))
        _, acc, e, d2 = A._near(grid, bins, x, x[sl])
        dst = np.sqrt(d2).astype(F32)
        t = (h - dst).astype(F32)
        w = ((t * t).astype(F32) * p2).astype(F32)
        slope = ((dst - h).astype(F32) * p2d).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = (((-e) / dst[..., None]).astype(F32) * slope[..., None]).astype(F32)
        apart = dst > 0
        gs, rs = g[sl].copy(), rho[sl].copy()
        for k in range(acc.shape[1]):
            rs = np.where(acc[:, k], (rs + w[:, k]).astype(F32), rs)
            gs = np.where(acc[:, k, None], (gs + np.where(apart[:, k, None], term[:, k], F32(0))).astype(F32), gs)
        g[sl], rho[sl] = gs, rs
    return ((h * g).astype(F32) / rho[:, None]).astype(F32), rho


def stage(params, x, v, cp, dt, merged=(1, 1, 1), ids=None, fed=None):
    """The stage of the header by id, every array float32 bit for bit: a dict of normal (n, 3), density (n,), dv (n, 3),
    neighbours (n,) uint32 -- and A, X (n, 3), the two sums before dt and xsph (not outputs of the library).  With ids,
    the rows of those particles alone.  fed = (normal, density) by id replaces pass A (float32 arrays)."""
    x = _f32(x).reshape(-1, 3)
    v = _f32(v).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = A.Binned(grid, x)
    h, p2, _ = A._kernel(params)
    nrm, rho = normals(params, x, merged, bins) if fed is None else (_f32(fed[0]), _f32(fed[1]))
    kc, h664 = constants(h)
    gc, gn, eps = F32(cp["cohesion"]), F32(cp["curvature"]), F32(cp["xsph"])
    rho0, dt = rest_density(params, cp), F32(dt)
    two = F32(2)
    sel = np.arange(len(x)) if ids is None else np.asarray(ids, np.int64)
    n = len(sel)
    Aa, Xa = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    cnt = np.zeros(n, U32)
    for s0 in range(0, n, grid.chunk()):
        rows = np.arange(s0, min(n, s0 + grid.chunk()))
        me = sel[rows]
        j, acc, e, d2 = A._near(grid, bins, x, x[me])
        d = np.sqrt(d2).astype(F32)
        con = acc & (d > 0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            xh = ((-e) / d[..., None]).astype(F32)
            q = (two / (rho[me][:, None] + rho[j]).astype(F32)).astype(F32)
            K = (rho0 * q).astype(F32)
            t = (h - d).astype(F32)
            t3 = ((t * t).astype(F32) * t).astype(F32)
            d3 = ((d * d).astype(F32) * d).astype(F32)
            pp = (t3 * d3).astype(F32)
            s = np.where((two * d).astype(F32) > h, pp, ((two * pp).astype(F32) - h664).astype(F32)).astype(F32)
            fc = (gc * (kc * s).astype(F32)).astype(F32)
            dn = (nrm[me][:, None, :] - nrm[j]).astype(F32)
            T = ((fc[..., None] * xh).astype(F32) + (gn * dn).astype(F32)).astype(F32)
            ta = (K[..., None] * T).astype(F32)
            w = ((t * t).astype(F32) * p2).astype(F32)
            tx = (((v[j] - v[me][:, None, :]).astype(F32) * w[..., None]).astype(F32) * q[..., None]).astype(F32)
            a_, x_ = Aa[rows].copy(), Xa[rows].copy()
            for c in range(acc.shape[1]):
                on = con[:, c, None]
                a_ = np.where(on, (a_ - ta[:, c]).astype(F32), a_)
                x_ = np.where(on, (x_ + tx[:, c]).astype(F32), x_)
        Aa[rows], Xa[rows] = a_, x_
        cnt[rows] = con.sum(1).astype(U32)
    with np.errstate(invalid="ignore", over="ignore"):
        dv = ((dt * Aa).astype(F32) + (eps * Xa).astype(F32)).astype(F32)
    dv = np.where((cnt > 0)[:, None], dv, F32(0)).astype(F32)
    return dict(normal=nrm[sel].copy(), density=rho[sel].copy(), dv=dv, neighbours=cnt, A=Aa, X=Xa)


def apply(v, st):
    """ws_apply_cohesion: v' = v + dv where the particle has a contributing neighbour, v's own bits elsewhere."""
    v = _f32(v).reshape(-1, 3)
    return np.where((st["neighbours"] > 0)[:, None], (v + st["dv"]).astype(F32), v).astype(F32)


# ---- float64 brute force ----------------------------------------------------------------------------------------------------
def stage64(ws, params, x, v, cp, dt, fed=None):
    """The stage in float64 over ALL pairs with d <= h (no grid, no float32 accept test): normal, density, A, X, dv,
    neighbours; A_abs, X_abs, dv_abs (n, 3) -- the sums of the absolute values of every part of every pair term, what a
    float32 sum's error is proportional to --, and near (n,) bool: some pair of the particle sits within 1e-4 h of the
    accept radius or of the spline's branch 2 d = h, where float32 and float64 may decide differently.
    fed = (normal, density) replaces pass A in pass B."""
    X = _f32(x).reshape(-1, 3).astype(np.float64)
    V = _f32(v).reshape(-1, 3).astype(np.float64)
    n = len(X)
    k = ws.get_smoothing_kernel(params)
    h = float(F32(params.smoothing_radius))
    p2, p2d = float(F32(k.pow2)), float(F32(k.pow2_der))
    kc, h664 = 32.0 / (float(F32(3.14159274)) * h ** 9), h ** 6 / 64.0
    gc, gn, eps = (float(F32(cp[key])) for key in ("cohesion", "curvature", "xsph"))
    rho0, dt = float(rest_density(params, cp)), float(F32(dt))
    qi, pj = [], []
    rows = max(1, (1 << 21) // max(1, n))
    for s0 in range(0, n, rows):
        e = X[None, :, :] - X[s0:s0 + rows, None, :]
        a, b = np.nonzero((e * e).sum(2) <= h * h * (1 + 1e-3))
        qi.append(a + s0)
        pj.append(b)
    qi, pj = np.concatenate(qi), np.concatenate(pj)
    e = X[pj] - X[qi]
    d = np.sqrt((e * e).sum(1))
    near = np.zeros(n, bool)
    np.logical_or.at(near, qi, (np.abs(d - h) < 1e-4 * h) | (np.abs(2 * d - h) < 1e-4 * h))
    keep = d <= h
    qi, pj, e, d = qi[keep], pj[keep], e[keep], d[keep]
    t = h - d
    w = t * t * p2
    rho = np.bincount(qi, w, minlength=n)
    apart = d > 0
    qi, pj, e, d, t, w = qi[apart], pj[apart], e[apart], d[apart], t[apart], w[apart]
    xh = -e / d[:, None]
    g = np.stack([np.bincount(qi, xh[:, a] * ((d - h) * p2d), minlength=n) for a in range(3)], 1)
    nrm = h * g / rho[:, None]
    if fed is not None:
        nrm, rho = np.asarray(fed[0], np.float64), np.asarray(fed[1], np.float64)
    q = 2.0 / (rho[qi] + rho[pj])
    K = rho0 * q
    pp = t ** 3 * d ** 3
    far = 2 * d > h
    s = np.where(far, pp, 2 * pp - h664)
    s_abs = np.where(far, pp, 2 * pp + h664)
    dn = nrm[qi] - nrm[pj]
    ta = -K[:, None] * ((gc * kc * s)[:, None] * xh + gn * dn)
    ta_abs = K[:, None] * ((gc * kc * s_abs)[:, None] * np.abs(xh) + gn * (np.abs(nrm[qi]) + np.abs(nrm[pj])))
    tx = (V[pj] - V[qi]) * (w * q)[:, None]
    tx_abs = (np.abs(V[pj]) + np.abs(V[qi])) * (w * q)[:, None]

    def total(term):
        return np.stack([np.bincount(qi, term[:, a], minlength=n) for a in range(3)], 1)

    Aa, Xa, A_abs, X_abs = total(ta), total(tx), total(ta_abs), total(tx_abs)
    cnt = np.bincount(qi, minlength=n)
    return dict(normal=nrm, density=rho, A=Aa, X=Xa, dv=np.where((cnt > 0)[:, None], dt * Aa + eps * Xa, 0.0),
                neighbours=cnt, A_abs=A_abs, X_abs=X_abs, dv_abs=dt * A_abs + eps * X_abs, near=near)
