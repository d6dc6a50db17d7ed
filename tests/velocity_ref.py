"""numpy restatement of the velocity field and the tracer march (include/wsfluid.h, ws_sample_velocity_* and
ws_advect_points): the field in float32 with every operation rounded once and the candidates in the canonical order of the
handle's grid (aniso_ref's Grid / Binned; grid from stats()["cells_merged"]) -- the library's WS_FLAG_IEEE_DIVISION form bit
for bit --, the march over a field given as a callable, and a float64 brute force of rho and the momentum sums that knows
nothing of the grid."""
import numpy as np

import aniso_ref as A

F32 = np.float32


def field32(params, x, v, q, merged=(1, 1, 1)):
    """(u (m, 3), rho (m,), M (m, 3)) at the points q, float32: per accepted candidate in canonical order d = sqrt(d2),
    w = (h - d)^2 * pow2, rho += w, M_a += fl(w * v_a); u = M / rho where rho > 0, else +0."""
    h, p2, _ = A._kernel(params)
    x = np.ascontiguousarray(x, F32).reshape(-1, 3)
    v = np.ascontiguousarray(v, F32).reshape(-1, 3)
    q = np.ascontiguousarray(q, F32).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = A.Binned(grid, x)
    rho = np.zeros(len(q), F32)
    mom = np.zeros((len(q), 3), F32)
    for s0 in range(0, len(q), grid.chunk()):
        sl = slice(s0, min(len(q), s0 + grid.chunk()))
        j, acc, _, d2 = A._near(grid, bins, x, q[sl])
        t = (h - np.sqrt(d2)).astype(F32)
        w = ((t * t).astype(F32) * p2).astype(F32)
        wv = (w[..., None] * v[j]).astype(F32)
        r, m = rho[sl].copy(), mom[sl].copy()
        for k in range(acc.shape[1]):
            a = acc[:, k]
            r = np.where(a, (r + w[:, k]).astype(F32), r)
            m = np.where(a[:, None], (m + wv[:, k]).astype(F32), m)
        rho[sl], mom[sl] = r, m
    return velocity(mom, rho), rho, mom


def velocity(mom, rho):
    """u = M / rho (float32 division) where rho > 0, else (+0, +0, +0)."""
    has = rho > 0
    u = np.zeros(mom.shape, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        u[has] = (mom[has] / rho[has, None]).astype(F32)
    return u


def advect(field, dt, substeps, xyz):
    """The midpoint march of the header over field(points (m, 3) float32) -> (u (m, 3), rho (m,)) float32.  Returns the
    final points and, per tracer, whether it ever took each branch: {"air": rho1 == 0 (it stayed), "euler": the midpoint
    left the fluid, "ordinary": a full midpoint step}.  The field is called on the tracers still moving only."""
    p = np.array(xyz, F32).reshape(-1, 3)
    m = len(p)
    dt = F32(dt)
    hdt = F32(F32(0.5) * dt)
    took = {k: np.zeros(m, bool) for k in ("air", "euler", "ordinary")}
    alive = np.arange(m)
    for _ in range(int(substeps)):
        if alive.size == 0:
            break
        u1, rho1 = field(p[alive])
        out = rho1 == 0
        took["air"][alive[out]] = True
        alive, u1 = alive[~out], np.asarray(u1, F32)[~out]
        if alive.size == 0:
            break
        mid = (p[alive] + (hdt * u1).astype(F32)).astype(F32)
        u2, rho2 = field(mid)
        left = rho2 == 0
        took["euler"][alive[left]] = True
        took["ordinary"][alive[~left]] = True
        u2 = np.where(left[:, None], u1, np.asarray(u2, F32))
        p[alive] = (p[alive] + (dt * u2).astype(F32)).astype(F32)
    return p, took


def _pairs(q, x, h):
    """(query, particle) index pairs that pass the library's float32 accept test, sorted by query then particle id, from
    a float64 cell list of edge h around the data (not the handle's grid)."""
    hq = np.float64(h)
    pc = np.floor(x.astype(np.float64) / hq).astype(np.int64)
    qc = np.floor(q.astype(np.float64) / hq).astype(np.int64)
    lo = np.minimum(pc.min(0), qc.min(0)) - 2
    span = np.maximum(pc.max(0), qc.max(0)) - lo + 3

    def key(c):
        c = c - lo
        return (c[:, 0] * span[1] + c[:, 1]) * span[2] + c[:, 2]

    order = np.argsort(key(pc), kind="stable")
    sk = key(pc)[order]
    qi_all, pj_all = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = key(qc + np.array([dx, dy, dz]))
                b = np.searchsorted(sk, k, "left")
                cnt = np.searchsorted(sk, k, "right") - b
                qi_all.append(np.repeat(np.arange(len(q)), cnt))
                off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                pj_all.append(order[np.repeat(b, cnt) + off])
    qi, pj = np.concatenate(qi_all), np.concatenate(pj_all)
    e = x[pj] - q[qi]  # float32, as the kernel forms it
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    ok = ~(d2 > A.accept(F32(h)))
    qi, pj = qi[ok], pj[ok]
    s = np.lexsort((pj, qi))
    return qi[s], pj[s]


def field64(ws, params, x, v, q):
    """float64 brute force at q: (rho (m,), M (m, 3), noise (4,), count (m,)).  noise = the float32 summation noise of
    these very terms, per column (rho, Mx, My, Mz): the largest difference between the sequential float32 sums taken
    forwards, backwards and the float64 sum -- the unit tests/test_gpu_density_field.py builds its tolerance from."""
    x = np.ascontiguousarray(x, F32).reshape(-1, 3)
    v = np.ascontiguousarray(v, F32).reshape(-1, 3)
    q = np.ascontiguousarray(q, F32).reshape(-1, 3)
    k = ws.get_smoothing_kernel(params)
    h = np.float64(params.smoothing_radius)
    qi, pj = _pairs(q, x, params.smoothing_radius)
    diff = q[qi].astype(np.float64) - x[pj].astype(np.float64)
    d = np.sqrt((diff * diff).sum(1))
    w = (h - d) ** 2 * np.float64(k.pow2)
    terms = np.concatenate([w[:, None], w[:, None] * v[pj].astype(np.float64)], 1)
    m = len(q)
    exact = np.stack([np.bincount(qi, terms[:, c], minlength=m) for c in range(4)], 1)
    cnt = np.bincount(qi, minlength=m)
    starts = np.searchsorted(qi, np.arange(m))
    t32 = terms.astype(F32)
    fw = np.zeros((m, 4), F32)
    rv = np.zeros((m, 4), F32)
    for i in np.flatnonzero(cnt):  # sequential float32 sums (np.add.reduce would sum pairwise)
        a, e = starts[i], starts[i] + cnt[i]
        fw[i] = np.cumsum(t32[a:e], axis=0, dtype=F32)[-1]
        rv[i] = np.cumsum(t32[a:e][::-1], axis=0, dtype=F32)[-1]
    noise = (np.maximum(np.abs(fw.astype(np.float64) - rv), np.maximum(np.abs(fw - exact), np.abs(rv - exact))).max(0)
             if m else np.zeros(4))
    return exact[:, 0], exact[:, 1:], noise, cnt
