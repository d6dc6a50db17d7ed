"""numpy restatement of ws_collide_volumes (include/wsfluid.h): the trilinear signed distance and its gradient in float32
with every operation rounded once, in the header's order -- the library's bits -- followed by ws_collide_solids' contact
response (tests/solids_ref.py's operations: dot, cross, the fixed-point sums), and the same formulas in float64.

A volume is a dict {origin (3,), spacing (3,), sdf (nz, ny, nx)} (volume() builds one); a pose is a dict {slot, centre,
rot (3, 3), velocity, angular_velocity, restitution, friction, margin} (pose() builds one; to_ws() turns a list into the
binding's WsVolumePose records, upload() makes a list of volumes resident in the slots 0, 1, ...)."""
import numpy as np

import solids_ref as S

F32 = np.float32


def volume(sdf, origin, spacing):
    sdf = np.ascontiguousarray(sdf, F32)
    assert sdf.ndim == 3
    return dict(origin=np.asarray(origin, F32), spacing=np.asarray(spacing, F32), sdf=sdf)


def nodes(dims, origin, spacing):
    """The local coordinates of every node in float64, shape (nz, ny, nx, 3) (dims = (nx, ny, nz))."""
    o, h = np.asarray(origin, F32).astype(np.float64), np.asarray(spacing, F32).astype(np.float64)
    z, y, x = np.meshgrid(*[o[a] + np.arange(dims[a]) * h[a] for a in (2, 1, 0)], indexing="ij")
    return np.stack([x, y, z], axis=-1)


def pose(slot, centre=(0.0, 0.0, 0.0), rot=None, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0), restitution=0.0,
         friction=0.0, margin=0.0):
    return dict(slot=int(slot), centre=np.asarray(centre, F32), rot=np.asarray(np.eye(3) if rot is None else rot, F32).reshape(3, 3),
                velocity=np.asarray(velocity, F32), angular_velocity=np.asarray(angular_velocity, F32), restitution=F32(restitution),
                friction=F32(friction), margin=F32(margin))


def to_ws(ws, poses):
    return [ws.fluid.volume_pose(p["slot"], [float(c) for c in p["centre"]], [float(x) for x in p["rot"].reshape(-1)],
                                 [float(x) for x in p["velocity"]], [float(x) for x in p["angular_velocity"]],
                                 float(p["restitution"]), float(p["friction"]), float(p["margin"])) for p in poses]


def upload(w, volumes):
    for slot, vol in enumerate(volumes):
        w.upload_volume(slot, [float(x) for x in vol["origin"]], [float(x) for x in vol["spacing"]], vol["sdf"])


def grid_coordinate(p, ps, vol, T=F32):
    """Step 1 and the first line of step 2: (g (n, 3), in the domain (n,))."""
    p = np.asarray(p, T).reshape(-1, 3)
    R = ps["rot"].astype(T)
    q = p - ps["centre"].astype(T)
    l = np.stack([S.dot(R[i][None, :], q) for i in range(3)], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        g = ((l - vol["origin"].astype(T)) / vol["spacing"].astype(T)).astype(T)
    nz, ny, nx = vol["sdf"].shape
    top = np.array([nx - 1, ny - 1, nz - 1]).astype(T)
    with np.errstate(invalid="ignore"):
        inside = np.all((g >= 0) & (g <= top), axis=1)
    return g, inside


def sample(p, ps, vol, T=F32):
    """Steps 1-2 in the arithmetic T: (s (n,), outward unit normal n (n, 3) in world coordinates, in the domain (n,), the
    local gradient G (n, 3)).  Outside the domain s and n are those of cell (0, 0, 0) at f = 0 and mean nothing."""
    g, inside = grid_coordinate(p, ps, vol, T)
    sdf = vol["sdf"].astype(T)
    nz, ny, nx = sdf.shape
    h = np.where(inside[:, None], g, T(0)).astype(T)
    i = np.minimum(h.astype(np.int64), np.array([nx - 2, ny - 2, nz - 2]))
    f = (h - i.astype(T)).astype(T)
    c = [[[sdf[i[:, 2] + z, i[:, 1] + y, i[:, 0] + x] for z in (0, 1)] for y in (0, 1)] for x in (0, 1)]  # c[x][y][z]
    f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
    d = [[c[1][y][z] - c[0][y][z] for z in (0, 1)] for y in (0, 1)]           # d[y][z]
    cx = [[c[0][y][z] + f0 * d[y][z] for z in (0, 1)] for y in (0, 1)]        # cx[y][z]
    e = [cx[1][z] - cx[0][z] for z in (0, 1)]
    cy = [cx[0][z] + f1 * e[z] for z in (0, 1)]
    hh = cy[1] - cy[0]
    s = cy[0] + f2 * hh
    dz = [d[0][z] + f1 * (d[1][z] - d[0][z]) for z in (0, 1)]
    sp = vol["spacing"].astype(T)
    G = np.stack([(dz[0] + f2 * (dz[1] - dz[0])) / sp[0], (e[0] + f2 * (e[1] - e[0])) / sp[1], hh / sp[2]], axis=1).astype(T)
    gg = S.dot(G, G)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.where((gg > 0)[:, None], G / np.sqrt(gg)[:, None], np.array([0, 1, 0], T)).astype(T)
    R = ps["rot"].astype(T)
    n = (m[:, 0:1] * R[0][None, :] + m[:, 1:2] * R[1][None, :]) + m[:, 2:3] * R[2][None, :]
    return s.astype(T), n.astype(T), inside, G


def collide(pos, vel, volumes, poses, ext_min, ext_max, damping, T=F32, contact32=None):
    """The call in the arithmetic T; the dict tests/solids_ref.py's collide returns, per pose.  contact32: the (k, n)
    contact decisions to use instead of T's own."""
    p = np.array(pos, T).reshape(-1, 3)
    v = np.array(vel, T).reshape(-1, 3)
    n_p, k = len(p), len(poses)
    touched = np.zeros(n_p, bool)
    hits = np.zeros((k, n_p), bool)
    dvs = np.zeros((k, n_p, 3), T)
    rs = np.zeros((k, n_p, 3), T)
    sums = np.zeros((k, 6), object)
    one = T(1)
    with np.errstate(over="ignore", invalid="ignore"):
        for e, ps in enumerate(poses):
            c, V, W = ps["centre"].astype(T), ps["velocity"].astype(T), ps["angular_velocity"].astype(T)
            sd, n, inside, _ = sample(p, ps, volumes[ps["slot"]], T)
            hit = (inside & (sd < T(ps["margin"]))) if contact32 is None else contact32[e]
            hits[e] = hit
            touched |= hit
            pn = p + (T(ps["margin"]) - sd)[:, None] * n
            r = pn - c
            u = V[None, :] + S.cross(W[None, :], r)
            rel = v - u
            vn = S.dot(rel, n)
            kicked = hit & (vn < 0)
            j = (one + T(ps["restitution"])) * (-vn)
            tang = rel - vn[:, None] * n
            dv = j[:, None] * n - T(ps["friction"]) * tang
            p = np.where(hit[:, None], pn, p).astype(T)
            v = np.where(kicked[:, None], v + dv, v).astype(T)
            dvs[e] = np.where(kicked[:, None], dv, 0)
            rs[e] = np.where(hit[:, None], r, 0)
            if T is F32 and kicked.any():
                I = (-dv[kicked]).astype(F32)
                H = S.cross(r[kicked].astype(F32), I).astype(F32)
                six = np.concatenate([S.quantise(I), S.quantise(H)], axis=1)
                sums[e] = [int(sum(six[:, w])) & S.MASK64 for w in range(6)]
        nd = T(-1) * T(damping)
        lo, hi = np.asarray(ext_min, T)[:3], np.asarray(ext_max, T)[:3]
        below, above = touched[:, None] & (p < lo), touched[:, None] & ~(p < lo) & (p > hi)
        v = np.where(below | above, v * nd, v).astype(T)
        p = np.where(below, lo, np.where(above, hi, p)).astype(T)
        pred = (p + (v * T(S.LOOKAHEAD)).astype(T)).astype(T)

    def signed(x):
        return x - (1 << 64) if x >> 63 else x

    flat = np.array([[float(signed(int(x))) * 2.0 ** -S.FIX for x in row] for row in sums], np.float64).reshape(k, 6)
    return dict(pos=p, vel=v, pred=pred, touched=touched, contacts=hits.sum(axis=1).astype(np.uint32), hit=hits, dv=dvs, r=rs,
                impulse=flat[:, :3].copy(), angular=flat[:, 3:].copy(), sums=sums)
