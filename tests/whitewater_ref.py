"""numpy restatement of the whitewater calls (include/wsfluid.h, ws_read_whitewater / ws_emit_whitewater /
ws_step_whitewater): the per-particle stage, the emission and the diffuse step in float32 with every operation rounded
once and the candidates in the canonical order of the handle's grid (aniso_ref's Grid / Binned) -- the library's bits --,
the counter-based random numbers in 32-bit integers, and a float64 brute force of the stage over all pairs that knows
nothing of the grid."""
import numpy as np

import aniso_ref as A
import velocity_ref as V

F32 = np.float32
U32 = np.uint32
OUTPUTS = ("trapped", "crest", "align", "energy", "normal", "neighbours")  # what ws_read_whitewater returns
_M32 = np.uint64(0xFFFFFFFF)


# ---- random numbers (pure integer) -------------------------------------------------------------------------------------
def mix(x):
    """The header's mixer on uint32 values (arrays or scalars), wrapping."""
    x = np.asarray(x).astype(np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x.astype(U32)


def word(seed, ids, c):
    """word(i, c) = mix(mix(seed + i * 0x9E3779B9) + c), uint32."""
    ids = np.asarray(ids).astype(np.uint64)
    first = mix((np.uint64(int(seed) & 0xFFFFFFFF) + ids * np.uint64(0x9E3779B9)) & _M32)
    return mix((first.astype(np.uint64) + np.asarray(c).astype(np.uint64)) & _M32)


def uniform(seed, ids, c):
    """U(i, c) = (float)(word >> 8) * 2^-24, float32 in [0, 1)."""
    return ((word(seed, ids, c) >> U32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


# ---- float32 helpers -----------------------------------------------------------------------------------------------------
def dot(a, b):
    """fl(fl(fl(a.x b.x) + fl(a.y b.y)) + fl(a.z b.z)) over the last axis, float32."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F32)


def _f32(a):
    return np.ascontiguousarray(a, F32)


# ---- the stage -----------------------------------------------------------------------------------------------------------
def normals(params, x, merged=(1, 1, 1), bins=None):
    """Pass A: (nh (n, 3), g (n, 3)) -- the IEEE density gradient at every particle and the unit normal -g / |g|."""
    h, _, p2d = A._kernel(params)
    x = _f32(x).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = bins or A.Binned(grid, x)
    g = np.zeros((len(x), 3), F32)
    for s0 in range(0, len(x), grid.chunk()):
        sl = slice(s0, min(len(x), s0 + grid.chunk()))
        _, acc, e, d2 = A._near(grid, bins, x, x[sl])
        dst = np.sqrt(d2).astype(F32)
        slope = ((dst - h) * p2d).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = (((-e) / dst[..., None]).astype(F32) * slope[..., None]).astype(F32)
        apart = dst > 0
        gs = g[sl].copy()
        for k in range(acc.shape[1]):
            gs = np.where(acc[:, k, None], (gs + np.where(apart[:, k, None], term[:, k], F32(0))).astype(F32), gs)
        g[sl] = gs
    gg = dot(g, g)
    nh = np.zeros_like(g)
    ok = gg != 0
    with np.errstate(over="ignore", invalid="ignore"):
        nh[ok] = ((-g[ok]) / np.sqrt(gg[ok])[:, None]).astype(F32)
    return nh, g


def stage(params, x, v, merged=(1, 1, 1), ids=None):
    """The stage of the header by id, every array float32 bit for bit: a dict of trapped, crest, align, energy (n,),
    normal (n, 3) and neighbours (n,) uint32 -- and crest_terms (n,), how many neighbours passed the crest's half-space
    test (not an output of the library).  With ids, the rows of those particles alone."""
    x = _f32(x).reshape(-1, 3)
    v = _f32(v).reshape(-1, 3)
    grid = A.Grid(params, merged)
    bins = A.Binned(grid, x)
    nh, _ = normals(params, x, merged, bins)
    sel = np.arange(len(x)) if ids is None else np.asarray(ids, np.int64)
    n = len(sel)
    T, K = np.zeros(n, F32), np.zeros(n, F32)
    cnt = np.zeros(n, U32)
    gated = np.zeros(n, U32)
    one = F32(1)
    for s0 in range(0, n, grid.chunk()):
        rows = np.arange(s0, min(n, s0 + grid.chunk()))
        me = sel[rows]
        j, acc, e, d2 = A._near(grid, bins, x, x[me])
        dst = np.sqrt(d2).astype(F32)
        con = acc & (dst > 0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            xh = ((-e) / dst[..., None]).astype(F32)
            w = (one - (dst / grid.h).astype(F32)).astype(F32)
            r = (v[me][:, None, :] - v[j]).astype(F32)
            s = np.sqrt(dot(r, r)).astype(F32)
            rh = (r / s[..., None]).astype(F32)
            tt = ((s * (one - dot(rh, xh)).astype(F32)).astype(F32) * w).astype(F32)
            ni = np.broadcast_to(nh[me][:, None, :], xh.shape)
            gate = dot(-xh, ni) < 0
            tk = ((one - dot(ni, nh[j])).astype(F32) * w).astype(F32)
        moving = s > 0
        t, k_ = T[rows].copy(), K[rows].copy()
        for c in range(acc.shape[1]):
            t = np.where(con[:, c] & moving[:, c], (t + tt[:, c]).astype(F32), t)
            k_ = np.where(con[:, c] & gate[:, c], (k_ + tk[:, c]).astype(F32), k_)
        T[rows], K[rows] = t, k_
        cnt[rows] = con.sum(1).astype(U32)
        gated[rows] = (con & gate).sum(1).astype(U32)
    vi = v[sel]
    vv = dot(vi, vi)
    sv = np.sqrt(vv).astype(F32)
    al = np.zeros(n, F32)
    ok = sv > 0
    with np.errstate(over="ignore", invalid="ignore"):
        al[ok] = dot((vi[ok] / sv[ok, None]).astype(F32), nh[sel][ok])
    return dict(trapped=T, crest=K, align=al, energy=(F32(0.5) * vv).astype(F32), normal=nh[sel].copy(), neighbours=cnt,
                crest_terms=gated)


# ---- emission --------------------------------------------------------------------------------------------------------------
def emit_defaults():
    """ws_default_whitewater_emit_params as a dict."""
    return dict(tau_trapped=(5.0, 50.0), tau_crest=(0.5, 4.0), tau_energy=(1.0, 25.0), k_trapped=400.0, k_crest=400.0,
                crest_align=0.6, dt=1.0 / 60.0, radius=0.1, lifetime=(2.0, 5.0), max_per_particle=8, seed=0)


def step_defaults():
    """ws_default_whitewater_step_params as a dict."""
    return dict(dt=1.0 / 60.0, spray_max=6, bubble_min=20, buoyancy=2.0, drag=0.5)


def clamp(val, tau):
    lo, hi = F32(tau[0]), F32(tau[1])
    return ((np.fmin(val, hi) - np.fmin(val, lo)).astype(F32) / F32(hi - lo)).astype(F32)


def counts(st, v, emit, ids=None):
    """m_i of the header for the stage st (rows of the particles ids, default all) and their velocities v."""
    v = _f32(v).reshape(-1, 3)
    ids = np.arange(len(v)) if ids is None else np.asarray(ids, np.int64)
    sv = np.sqrt(dot(v, v)).astype(F32)
    kt, kc, dt = F32(emit["k_trapped"]), F32(emit["k_crest"]), F32(emit["dt"])
    c = np.where(st["align"] >= F32(emit["crest_align"]), (kc * clamp(st["crest"], emit["tau_crest"])).astype(F32), F32(0))
    inner = ((kt * clamp(st["trapped"], emit["tau_trapped"])).astype(F32) + c).astype(F32)
    rate = ((clamp(st["energy"], emit["tau_energy"]) * inner).astype(F32) * dt).astype(F32)
    f = np.floor((rate + uniform(emit["seed"], ids, 0)).astype(F32))
    cap = int(emit["max_per_particle"])
    m = np.where(f >= F32(cap), cap, np.where(f >= 1, f, 0)).astype(np.int64)
    return np.where(sv != 0, m, 0).astype(U32)


def frame(vh):
    """(e1, e2) of the header for unit axes vh (k, 3)."""
    a = np.abs(vh)
    q = np.zeros(len(vh), np.int64)
    least = a[:, 0].copy()
    y = a[:, 1] < least
    q[y], least[y] = 1, a[y, 1]
    q[a[:, 2] < least] = 2
    z = np.zeros(len(vh), F32)
    c = np.where((q == 0)[:, None], np.stack([z, -vh[:, 2], vh[:, 1]], 1),
                 np.where((q == 1)[:, None], np.stack([vh[:, 2], z, -vh[:, 0]], 1), np.stack([-vh[:, 1], vh[:, 0], z], 1)))
    c = c.astype(F32)
    e1 = (c / np.sqrt(dot(c, c))[:, None]).astype(F32)
    e2 = np.stack([vh[:, 1] * e1[:, 2] - vh[:, 2] * e1[:, 1], vh[:, 2] * e1[:, 0] - vh[:, 0] * e1[:, 2],
                   vh[:, 0] * e1[:, 1] - vh[:, 1] * e1[:, 0]], 1).astype(F32)
    return e1, e2


def disc(seed, ids, k):
    """The disc point (a, b) of spawn k of the particles ids (arrays of one length), by the header's rejection."""
    ids, k = np.asarray(ids, np.int64), np.asarray(k, np.int64)
    base = 1 + 18 * k
    da, db = np.zeros(len(ids), F32), np.zeros(len(ids), F32)
    done = np.zeros(len(ids), bool)
    for t in range(8):
        a = (F32(2) * uniform(seed, ids, base + 2 + 2 * t) - F32(1)).astype(F32)
        b = (F32(2) * uniform(seed, ids, base + 3 + 2 * t) - F32(1)).astype(F32)
        take = ~done & ((a * a + b * b).astype(F32) <= 1)
        da[take], db[take] = a[take], b[take]
        done |= take
    return da, db


def spawn(x, v, m, emit, ids=None):
    """The spawns of the header for the emitters' positions x, velocities v and counts m (rows of the particles ids,
    default all), ordered by id then k: a dict of xyz, velocity (k, 3), life (k,), source (k,) uint32, count."""
    x, v = _f32(x).reshape(-1, 3), _f32(v).reshape(-1, 3)
    ids = np.arange(len(x)) if ids is None else np.asarray(ids, np.int64)
    m = np.asarray(m, np.int64)
    row = np.repeat(np.arange(len(x)), m)
    k = np.arange(m.sum()) - np.repeat(np.cumsum(m) - m, m)
    src = ids[row]
    xi, vi = x[row], v[row]
    seed = emit["seed"]
    sv = np.sqrt(dot(vi, vi)).astype(F32)
    vh = (vi / sv[:, None]).astype(F32)
    e1, e2 = frame(vh)
    da, db = disc(seed, src, k)
    o = (F32(emit["radius"]) * ((da[:, None] * e1).astype(F32) + (db[:, None] * e2).astype(F32)).astype(F32)).astype(F32)
    along = (uniform(seed, src, 1 + 18 * k) * F32(emit["dt"])).astype(F32)
    p = ((xi + o).astype(F32) + (along[:, None] * vi).astype(F32)).astype(F32)
    l0, l1 = F32(emit["lifetime"][0]), F32(emit["lifetime"][1])
    life = (l0 + (uniform(seed, src, 2 + 18 * k) * F32(l1 - l0)).astype(F32)).astype(F32)
    return dict(xyz=p, velocity=(vi + o).astype(F32), life=life, source=src.astype(U32), count=int(m.sum()))


def emit(params, x, v, emit_params, merged=(1, 1, 1)):
    """ws_emit_whitewater restated: (spawns dict, m (n,) uint32, the stage)."""
    st = stage(params, x, v, merged)
    m = counts(st, v, emit_params)
    return spawn(x, v, m, emit_params), m, st


# ---- the diffuse step --------------------------------------------------------------------------------------------------
def accept_count(params, x, p):
    """Brute force: how many particles x pass the library's float32 accept test around each point p (d == 0 included)."""
    x, p = _f32(x).reshape(-1, 3), _f32(p).reshape(-1, 3)
    t = A.accept(F32(params.smoothing_radius))
    out = np.zeros(len(p), np.int64)
    rows = max(1, (1 << 22) // max(1, len(x)))
    for s0 in range(0, len(p), rows):
        e = (x[None, :, :] - p[s0:s0 + rows, None, :]).astype(F32)
        out[s0:s0 + rows] = (~(dot(e, e) > t)).sum(1)
    return out


def step(params, sp, p, v, life, u, c):
    """One ws_step_whitewater for the field velocity u (m, 3) and accept count c (m,) at p: (p, v, life, class uint8,
    reflected (m,) bool -- the container rule fired)."""
    p, v, u = np.array(p, F32).reshape(-1, 3), np.array(v, F32).reshape(-1, 3), _f32(u).reshape(-1, 3)
    life = np.array(life, F32).reshape(-1)
    c = np.asarray(c, np.int64)
    dt, kb, kd = F32(sp["dt"]), F32(sp["buoyancy"]), F32(sp["drag"])
    g = np.asarray(params.gravity[:3], F32)
    spray = c < int(sp["spray_max"])
    bubble = ~spray & (c > int(sp["bubble_min"]))
    foam = ~spray & ~bubble
    v_s = (v + (dt * g).astype(F32)[None, :]).astype(F32)
    v_b = ((v + (dt * ((-kb) * g).astype(F32)).astype(F32)[None, :]).astype(F32) + (kd * (u - v).astype(F32)).astype(F32)).astype(F32)
    vn = np.where(spray[:, None], v_s, np.where(bubble[:, None], v_b, u)).astype(F32)
    pn = (p + (dt * vn).astype(F32)).astype(F32)
    ln = np.where(foam, (life - dt).astype(F32), life).astype(F32)
    nd = F32(F32(-1) * F32(params.collision_damping))
    lo, hi = np.asarray(params.ext_min[:3], F32), np.asarray(params.ext_max[:3], F32)
    below, above = pn < lo, pn > hi
    vn = np.where(below | above, (vn * nd).astype(F32), vn).astype(F32)
    pn = np.where(below, lo, np.where(above, hi, pn)).astype(F32)
    cls = np.where(spray, 0, np.where(bubble, 2, 1)).astype(np.uint8)
    cls[ln <= 0] = 3
    return pn, vn, ln, cls, (below | above).any(1)


# ---- float64 brute force of the stage ---------------------------------------------------------------------------------
def stage64(ws, params, x, v):
    """The stage in float64 over all pairs that pass the float32 accept test: a dict of trapped, crest, align, energy,
    normal, neighbours and, for judging a float32 result, cond (n,) = |g| / sum |gradient terms| (how well the normal
    is conditioned) and margin (n,) = the smallest |(-xh) . nh_i| over the neighbours (how far the crest gate is from
    flipping)."""
    x32, v32 = _f32(x).reshape(-1, 3), _f32(v).reshape(-1, 3)
    n = len(x32)
    k = ws.get_smoothing_kernel(params)
    h = np.float64(params.smoothing_radius)
    qi, pj = V._pairs(x32, x32, params.smoothing_radius)
    X, Vv = x32.astype(np.float64), v32.astype(np.float64)
    e = X[qi] - X[pj]  # x_i - x_j
    d = np.sqrt((e * e).sum(1))
    keep = d > 0
    qi, pj, e, d = qi[keep], pj[keep], e[keep], d[keep]
    xh = e / d[:, None]
    gterm = xh * ((d - h) * np.float64(k.pow2_der))[:, None]
    g = np.stack([np.bincount(qi, gterm[:, a], minlength=n) for a in range(3)], 1)
    gabs = np.bincount(qi, np.abs(gterm).sum(1), minlength=n)
    gn = np.sqrt((g * g).sum(1))
    nh = np.where(gn[:, None] > 0, -g / np.where(gn > 0, gn, 1)[:, None], 0.0)
    w = 1.0 - d / h
    r = Vv[qi] - Vv[pj]
    s = np.sqrt((r * r).sum(1))
    tt = np.where(s > 0, (s - (r * xh).sum(1)) * w, 0.0)
    dn = -(xh * nh[qi]).sum(1)
    tk = np.where(dn < 0, (1.0 - (nh[qi] * nh[pj]).sum(1)) * w, 0.0)
    margin = np.full(n, np.inf)
    np.minimum.at(margin, qi, np.abs(dn))
    vv = (Vv * Vv).sum(1)
    sv = np.sqrt(vv)
    al = np.where(sv > 0, (Vv * nh).sum(1) / np.where(sv > 0, sv, 1), 0.0)
    return dict(trapped=np.bincount(qi, tt, minlength=n), crest=np.bincount(qi, tk, minlength=n), align=al, energy=0.5 * vv,
                normal=nh, neighbours=np.bincount(qi, minlength=n), cond=gn / np.where(gabs > 0, gabs, 1), margin=margin,
                pairs=(qi, pj), trapped_abs=np.bincount(qi, np.abs(tt), minlength=n),
                crest_abs=np.bincount(qi, np.abs(tk), minlength=n))
