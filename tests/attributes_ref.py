"""numpy restatement of the attribute calls (include/wsfluid.h, ws_paint_attributes / ws_diffuse_attributes /
ws_sample_attribute_*): paint, diffusion (with iterations) and the field in float32 with every operation rounded once and
the candidates in the canonical order of the handle's grid (aniso_ref's Grid / Binned / _near, merged grids included) --
the library's bits --, and a float64 brute force of one diffusion iteration over ALL pairs that knows nothing of the grid
and also returns, per particle and channel, the sum of the absolute pair terms a float32 result is judged against."""
import numpy as np

import aniso_ref as A
import cohesion_ref as Co

F32 = np.float32
U32 = np.uint32
MIX, ADD = 0, 1


def _f32(a):
    return np.ascontiguousarray(a, F32)


def brush(kind, centre, radius, value, strength=1.0, falloff=0.0, channels=15):
    """One ws_brush as a dict (fluid.brush's arguments)."""
    return dict(kind={"mix": MIX, "add": ADD}.get(kind, kind), centre=tuple(centre), radius=radius, value=tuple(value),
                strength=strength, falloff=falloff, channels=int(channels))


def defaults():
    """ws_default_diffuse_params as a dict."""
    return dict(rate=(1.0, 1.0, 1.0, 1.0), iterations=1)


# ---- paint ------------------------------------------------------------------------------------------------------------------
def paint(x, attr, brushes):
    """(A' (n, 4) float32, painted (k,) uint32): the brushes in order on the running value of A."""
    x = _f32(x).reshape(-1, 3)
    a = _f32(attr).reshape(-1, 4).copy()
    counts = np.zeros(len(brushes), U32)
    one = F32(1)
    for e, b in enumerate(brushes):
        c = np.asarray(b["centre"], F32)
        R, fo, st = F32(b["radius"]), F32(b["falloff"]), F32(b["strength"])
        q = (x - c).astype(F32)
        dd = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(F32) + q[:, 2] * q[:, 2]).astype(F32)
        d = np.sqrt(dd).astype(F32)
        hit = d < R
        counts[e] = hit.sum()
        t = (d / R).astype(F32)
        w = (one - (fo * t).astype(F32)).astype(F32)
        s = (st * w).astype(F32)
        keep = (one - s).astype(F32)
        for ch in range(4):
            if not (b["channels"] >> ch) & 1:
                continue
            add = (s * F32(b["value"][ch])).astype(F32)
            with np.errstate(invalid="ignore", over="ignore"):
                if b["kind"] == MIX:
                    new = ((keep * a[:, ch]).astype(F32) + add).astype(F32)
                else:
                    new = (a[:, ch] + add).astype(F32)
            a[:, ch] = np.where(hit, new, a[:, ch])
    return a, counts


# ---- diffusion --------------------------------------------------------------------------------------------------------------
def densities(params, x, merged=(1, 1, 1)):
    """Pass A: the density sampler's IEEE sums at every particle (the cohesion pass A's rho, the same bits)."""
    return Co.normals(params, x, merged)[1]


def diffuse(params, x, attr, rate, dt, iterations=1, merged=(1, 1, 1), fed=None, sums=False):
    """(A' (n, 4) float32, neighbours (n,) uint32): `iterations` passes B over one binning and one pass A.  fed = the
    densities by id in place of pass A.  sums=True: also S (n, 4) of the LAST iteration (not an output of the library)."""
    x = _f32(x).reshape(-1, 3)
    a = _f32(attr).reshape(-1, 4).copy()
    n = len(x)
    grid = A.Grid(params, merged)
    bins = A.Binned(grid, x)
    h, p2, _ = A._kernel(params)
    rho = densities(params, x, merged) if fed is None else _f32(fed)
    r = (_f32(rate) * F32(dt)).astype(F32)
    two = F32(2)
    cnt = np.zeros(n, U32)
    S = np.zeros((n, 4), F32)
    for _ in range(int(iterations)):
        new = a.copy()
        for s0 in range(0, n, grid.chunk()):
            rows = np.arange(s0, min(n, s0 + grid.chunk()))
            j, acc, _, d2 = A._near(grid, bins, x, x[rows])
            d = np.sqrt(d2).astype(F32)
            con = acc & (d > 0)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                q = (two / (rho[rows][:, None] + rho[j]).astype(F32)).astype(F32)
                t = (h - d).astype(F32)
                w = ((t * t).astype(F32) * p2).astype(F32)
                g = (w * q).astype(F32)
                term = ((a[j] - a[rows][:, None, :]).astype(F32) * g[..., None]).astype(F32)
                s_ = np.zeros((len(rows), 4), F32)
                for c in range(acc.shape[1]):
                    s_ = np.where(con[:, c, None], (s_ + term[:, c]).astype(F32), s_)
                upd = (a[rows] + (r[None, :] * s_).astype(F32)).astype(F32)
            cnt[rows] = con.sum(1).astype(U32)
            S[rows] = s_
            on = (cnt[rows] > 0)[:, None] & (r != 0)[None, :]
            new[rows] = np.where(on, upd, a[rows])
        a = new
    return (a, cnt, S) if sums else (a, cnt)


def diffuse64(ws, params, x, attr, rate, dt, fed=None):
    """One iteration in float64 over ALL pairs with 0 < d <= h (no grid, no float32 accept test): a dict of S, A' (n, 4),
    neighbours (n,), S_abs (n, 4) -- the sums of the absolute values of the pair terms' parts --, density (n,), near (n,)
    bool: some pair of the particle sits within 1e-4 h of the accept radius -- and pairs (qi, pj) with their weights g."""
    X = _f32(x).reshape(-1, 3).astype(np.float64)
    At = _f32(attr).reshape(-1, 4).astype(np.float64)
    n = len(X)
    k = ws.get_smoothing_kernel(params)
    h = float(F32(params.smoothing_radius))
    p2 = float(F32(k.pow2))
    r = (_f32(rate) * F32(dt)).astype(F32).astype(np.float64)
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
    np.logical_or.at(near, qi, np.abs(d - h) < 1e-4 * h)
    keep = d <= h
    qi, pj, d = qi[keep], pj[keep], d[keep]
    w = (h - d) ** 2 * p2
    rho = np.bincount(qi, w, minlength=n)
    if fed is not None:
        rho = np.asarray(fed, np.float64)
    apart = d > 0
    qi, pj, w = qi[apart], pj[apart], w[apart]
    g = w * 2.0 / (rho[qi] + rho[pj])
    term = (At[pj] - At[qi]) * g[:, None]
    term_abs = (np.abs(At[pj]) + np.abs(At[qi])) * g[:, None]

    def total(t):
        return np.stack([np.bincount(qi, t[:, c], minlength=n) for c in range(4)], 1)

    S, S_abs = total(term), total(term_abs)
    cnt = np.bincount(qi, minlength=n)
    on = (cnt > 0)[:, None] & (r != 0)[None, :]
    return dict(S=S, S_abs=S_abs, A=np.where(on, At + r * S, At), neighbours=cnt, density=rho, near=near, pairs=(qi, pj, g),
                r=r)


# ---- the field --------------------------------------------------------------------------------------------------------------
def field(params, x, attr, q, merged=(1, 1, 1)):
    """(value (m, 4), rho (m,), M (m, 4), accepted (m,)) at the points q, float32: velocity_ref.field32 with four channels."""
    h, p2, _ = A._kernel(params)
    x = _f32(x).reshape(-1, 3)
    a = _f32(attr).reshape(-1, 4)
    q = _f32(q).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = A.Binned(grid, x)
    rho = np.zeros(len(q), F32)
    mom = np.zeros((len(q), 4), F32)
    cnt = np.zeros(len(q), np.int64)
    for s0 in range(0, len(q), grid.chunk()):
        sl = slice(s0, min(len(q), s0 + grid.chunk()))
        j, acc, _, d2 = A._near(grid, bins, x, q[sl])
        t = (h - np.sqrt(d2)).astype(F32)
        w = ((t * t).astype(F32) * p2).astype(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            wa = (w[..., None] * a[j]).astype(F32)
            r, m = rho[sl].copy(), mom[sl].copy()
            for k in range(acc.shape[1]):
                on = acc[:, k]
                r = np.where(on, (r + w[:, k]).astype(F32), r)
                m = np.where(on[:, None], (m + wa[:, k]).astype(F32), m)
        rho[sl], mom[sl], cnt[sl] = r, m, acc.sum(1)
    has = rho > 0
    val = np.zeros(mom.shape, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        val[has] = (mom[has] / rho[has, None]).astype(F32)
    return val, rho, mom, cnt


def grid_nodes(origin, spacing, dims):
    """The nodes of a grid call, x fastest: fl(origin + fl(i * spacing)) per axis, (nz * ny * nx, 3) float32."""
    o, sp = _f32(origin), _f32(spacing)
    ax = [(o[a] + (np.arange(int(dims[a])).astype(F32) * sp[a]).astype(F32)).astype(F32) for a in range(3)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(F32)
