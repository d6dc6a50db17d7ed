"""tests/volumes_ref.py, the float32 restatement of ws_collide_volumes the GPU tests compare bits with, against a float64
evaluation of the same formulas, and what trilinear interpolation promises (include/wsfluid.h).

The tolerances are derived, not tuned.  eps = 2^-24; every float32 operation is rounded once and errs by at most eps of
its result (second-order terms are left out, as in tests/test_solids_reference.py).  With q = p - c, rn = max(1, the
largest row norm of rot), C = the largest |sdf| of the volume, D_a = the largest |difference| of two nodes adjacent along
axis a, o = origin, h = spacing:

  grid coordinate.  q: 1 rounding; l_a = dot(R_a, q): 6 eps rn |q| in all.  l_a - o_a adds eps |l_a - o_a|, the division
    eps |g_a|; with |l_a - o_a| <= rn |q| + |o_a|:  E_g,a <= eps (8 rn |q| + 2 |o_a|) / h_a.
  interpolation at a given g.  Corners are exact.  d = c_1 - c_0: 2 eps C.  cx = c_0 + f d: d's 2, the product's 2 and the
    sum's 1 (|cx| <= C: a convex combination): 5 eps C.  e = cx_1 - cx_0: 10 + 2 = 12.  cy: 5 + 12 + 2 + 1 = 20.
    hh: 40 + 2 = 42.  s: 20 + 42 + 2 + 1 = 65 eps C.
  The interpolant is continuous across cells and its slope along g_a is at most D_a:
    E_s <= 65 eps C + sum_a E_g,a D_a.
  gradient.  d_1z - d_0z: 4 + 4 = 8 eps C; dz: 2 + 8 + 4 + 2 = 16; dz_1 - dz_0: 32 + 4 = 36; the numerator of G_0: 16 + 36 +
    4 + 2 = 58, the division one more at 2 C: 60 eps C / h_0.  G_1: e_1 - e_0: 24 + 4 = 28; 12 + 28 + 4 + 2 = 46, + 2: 48 eps C
    / h_1.  G_2: 42 + 2 = 44 eps C / h_2.  Within ONE cell a mixed difference is at most 4 C, so G_a moves by at most 4 C
    E_g,b / h_a per axis b:  E_G,a <= (60 eps C + 4 C sum_b E_g,b) / h_a, E_x = |E_G|.
  normal.  m = G / |G| errs by 2 E_x / |G| + 2 eps; n = m R adds 5 roundings at rn:  E_n <= rn (2 E_x / |G| + 7 eps), never
    more than 2.
  push-out and velocity: tests/test_solids_reference.py's E_p and E_v with these E_s and E_n.
  A discrete decision (in the domain, which cell, contact, kicked) can differ between the two arithmetics only where its
  float64 discriminant lies within its error of the threshold: the comparisons leave those particles out and count them."""
import numpy as np

import solids_ref as S
import volumes_ref as V

F32 = np.float32
EPS = 2.0 ** -24
EXT = (np.array([-4, -4, -4], F32), np.array([4, 4, 4], F32), F32(0.95))


def scene(seed, n=3000, half=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-half, half, (n, 3)).astype(F32), rng.normal(0.0, 2.0, (n, 3)).astype(F32)


def bounds(pos, vel, ps, vol, r_len):
    """(E_g (n, 3), E_s, E_n, E_p, E_v, speed, E_x) of the module's text, for the float64 sample at pos."""
    p64 = pos.astype(np.float64)
    q = np.sqrt(((p64 - ps["centre"].astype(np.float64)) ** 2).sum(axis=1))
    R, h, o = ps["rot"].astype(np.float64), vol["spacing"].astype(np.float64), vol["origin"].astype(np.float64)
    rn = max(1.0, float(np.sqrt((R * R).sum(axis=1)).max()))
    sdf = vol["sdf"].astype(np.float64)
    C = float(np.abs(sdf).max())
    D = np.array([np.abs(np.diff(sdf, axis=2)).max(), np.abs(np.diff(sdf, axis=1)).max(), np.abs(np.diff(sdf, axis=0)).max()])
    E_g = EPS * (8 * rn * q[:, None] + 2 * np.abs(o)[None, :]) / h[None, :]
    E_s = 65 * EPS * C + (E_g * D[None, :]).sum(axis=1)
    E_G = (60 * EPS * C + 4 * C * E_g.sum(axis=1))[:, None] / h[None, :]
    E_x = np.sqrt((E_G ** 2).sum(axis=1))
    s64, _, _, G64 = V.sample(pos, ps, vol, np.float64)
    glen = np.sqrt((G64 ** 2).sum(axis=1))
    with np.errstate(divide="ignore"):
        E_n = np.minimum(2.0, rn * (2 * E_x / glen + 7 * EPS))
    out = np.abs(float(ps["margin"]) - s64)
    E_p = np.sqrt(3.0) * (E_s + out * E_n + 3 * EPS * (np.sqrt((p64 ** 2).sum(axis=1)) + out))
    W = float(np.sqrt((ps["angular_velocity"].astype(np.float64) ** 2).sum()))
    Vl = float(np.sqrt((ps["velocity"].astype(np.float64) ** 2).sum()))
    speed = np.sqrt((vel.astype(np.float64) ** 2).sum(axis=1)) + Vl + W * r_len
    e, f = float(ps["restitution"]), float(ps["friction"])
    E_v = 2 * (1 + e + f) * (W * E_p + speed * (2 * E_n + 20 * EPS))
    return E_g, E_s, E_n, E_p, E_v, speed, E_x


def decided(pos, ps, vol, E_g, E_s):
    """Particles whose domain, cell and contact decisions cannot differ between float32 and float64."""
    g64, _ = V.grid_coordinate(pos, ps, vol, np.float64)
    s64, _, inside, _ = V.sample(pos, ps, vol, np.float64)
    nz, ny, nx = vol["sdf"].shape
    top = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    near_face = (np.abs(g64) <= E_g) | (np.abs(g64 - top) <= E_g)
    near_node = np.abs(g64 - np.rint(g64)) <= E_g
    return ~near_face.any(axis=1) & ~(inside & near_node.any(axis=1)) & ~(inside & (np.abs(s64 - float(ps["margin"])) <= E_s))


def sphere_volume(N, r=0.5, half=1.0):
    dims = (N, N, N)
    h = 2.0 * half / (N - 1)
    xyz = V.nodes(dims, (-half,) * 3, (h,) * 3)
    return V.volume(np.sqrt((xyz ** 2).sum(axis=-1)) - r, (-half,) * 3, (h,) * 3)


def terrain_volume(scale=1.0):
    """A 9 x 3 x 9 height field: the distance to y = a bumpy height, not a true distance (a host's terrain rarely is)."""
    dims, origin, spacing = (9, 3, 9), (-1.0, -0.5, -1.0), (0.25, 0.5, 0.25)
    xyz = V.nodes(dims, origin, spacing)
    height = xyz[..., 1] - 0.2 * np.sin(2.0 * xyz[..., 0]) * np.cos(1.5 * xyz[..., 2])
    return V.volume(scale * height, [scale * x for x in origin], [scale * x for x in spacing])


def cases():
    rng = np.random.default_rng(3)
    R = S.rotation((1.0, 2.0, -0.5), 0.7)
    rough = V.volume(rng.uniform(-0.5, 0.5, (3, 4, 5)), (-1.0, -0.375, -0.125), (0.5, 0.25, 0.125))
    return {
        "sphere17": (sphere_volume(17), V.pose(0, (0.1, -0.2, 0.05), restitution=0.5, friction=0.2, margin=0.03)),
        "sphere17-moving": (sphere_volume(17), V.pose(0, (0.0, 0.0, 0.0), rot=R, velocity=(1.0, -0.5, 0.25),
                                                    angular_velocity=(0.5, 3.0, -1.0), restitution=1.0, friction=1.0, margin=0.05)),
        "terrain": (terrain_volume(), V.pose(0, (0.05, 0.0, -0.1), rot=R, restitution=0.25, friction=0.3, margin=0.04)),
        "random-5x4x3": (rough, V.pose(0, (0.0, 0.1, 0.0), rot=S.rotation((0.0, 1.0, 0.3), -0.4), restitution=0.3, friction=0.1,
                                       margin=0.02)),
    }


# ---- (a) the restatement against float64 ----------------------------------------------------------------------------------
def test_the_restatement_is_within_the_derived_bounds_of_float64():
    for seed, (name, (vol, ps)) in enumerate(cases().items()):
        pos, vel = scene(seed)
        if name == "random-5x4x3":  # a flat domain (2 x 0.75 x 0.25): the cloud is squeezed so that enough of it lies inside
            pos = (pos * np.array([1.0, 0.5, 0.25], F32)).astype(F32)
        E_g, E_s, E_n, E_p, E_v, speed, E_x = bounds(pos, vel, ps, vol, 2.0)
        g32, _ = V.grid_coordinate(pos, ps, vol)
        g64, _ = V.grid_coordinate(pos, ps, vol, np.float64)
        assert np.all(np.abs(g32.astype(np.float64) - g64) <= E_g), name
        ok = decided(pos, ps, vol, E_g, E_s)
        s32, n32, in32, _ = V.sample(pos, ps, vol)
        s64, n64, in64, _ = V.sample(pos, ps, vol, np.float64)
        assert np.array_equal(in32[ok], in64[ok]) and 100 < in64.sum(), (name, in64.sum())
        both = ok & in64
        assert np.all(np.abs(s32.astype(np.float64) - s64)[both] <= E_s[both]), name
        en = np.sqrt(((n32.astype(np.float64) - n64) ** 2).sum(axis=1))[both]
        assert np.all(en <= E_n[both]), (name, float((en / E_n[both]).max()))
        a = V.collide(pos, vel, [vol], [ps], *EXT)
        b = V.collide(pos, vel, [vol], [ps], *EXT, T=np.float64)
        r64 = b["pos"] - ps["centre"].astype(np.float64)
        u64 = ps["velocity"].astype(np.float64) + np.cross(ps["angular_velocity"].astype(np.float64), r64)
        vn64 = ((vel.astype(np.float64) - u64) * n64).sum(axis=1)
        ok &= ~(b["hit"][0] & (np.abs(vn64) <= E_v))
        assert ok.mean() > 0.98, (name, ok.mean())  # the undecided are the rare exception
        assert np.array_equal(a["hit"][0][ok], b["hit"][0][ok]), name
        hit = a["hit"][0] & ok
        assert 100 < hit.sum() < len(pos), (name, hit.sum())
        ep = np.abs(a["pos"].astype(np.float64) - b["pos"])[hit]
        ev = np.abs(a["vel"].astype(np.float64) - b["vel"])[hit]
        print("%s: %d contacts, worst position error / bound %.3f, velocity %.3f, normal %.3f" %
              (name, hit.sum(), float((ep / E_p[hit, None]).max()), float((ev / E_v[hit, None]).max()), float((en / E_n[both]).max())))
        assert np.all(ep <= E_p[hit, None]), (name, float((ep / E_p[hit, None]).max()))
        assert np.all(ev <= E_v[hit, None]), (name, float((ev / E_v[hit, None]).max()))
        assert np.array_equal(a["pred"], (a["pos"] + (a["vel"] * F32(0.02)).astype(F32)).astype(F32))
        assert a["contacts"].dtype == np.uint32 and a["contacts"][0] == a["hit"][0].sum()
        out = ~a["touched"]
        assert np.array_equal(a["pos"][out].view(np.uint32), pos[out].view(np.uint32))
        assert np.array_equal(a["vel"][out].view(np.uint32), vel[out].view(np.uint32))


# ---- (b) an affine field is reproduced ------------------------------------------------------------------------------------
def plane_volume(nrm, c, dims=(5, 4, 3), origin=(-1.0, -0.375, -0.125), spacing=(0.5, 0.25, 0.125)):
    """dot(nrm, l) - c, by default on a 5 x 4 x 3 volume with three different spacings: an index-order or axis mix-up shows."""
    return V.volume(V.nodes(dims, origin, spacing) @ np.asarray(nrm, np.float64) - c, origin, spacing)


def node_rounding(vol):
    """The nodes are a field's values rounded to float32: the stored field is within eps C of it, its differences within
    2 eps C, so its gradient within 2 eps C / h_a per axis.  (error of s, error of |G|)."""
    Cmax = float(np.abs(vol["sdf"]).max())
    return EPS * Cmax, float(np.sqrt(((2 * EPS * Cmax / vol["spacing"].astype(np.float64)) ** 2).sum()))


def test_a_tilted_plane_is_reproduced_with_its_normal_and_touched_particles_end_at_the_margin():
    nrm = np.array([0.48, 0.6, 0.64])  # a unit vector
    assert abs(nrm @ nrm - 1.0) < 1e-15
    c = 0.0625
    vol = plane_volume(nrm, c)
    assert vol["sdf"].shape == (3, 4, 5)
    for seed, rot in enumerate((None, S.rotation((1.0, 2.0, -0.5), 0.7))):
        ps = V.pose(0, (0.125, -0.0625, 0.03125), rot=rot, restitution=0.5, friction=0.2, margin=0.05)
        rng = np.random.default_rng(50 + seed)
        local = rng.uniform((-1.0, -0.375, -0.125), (1.0, 0.375, 0.125), (3000, 3))
        R64 = ps["rot"].astype(np.float64)
        pos = (local @ R64 + ps["centre"].astype(np.float64)).astype(F32)  # p = c + sum_i l_i R_i
        vel = rng.normal(0.0, 2.0, pos.shape).astype(F32)
        E_g, E_s, E_n, E_p, E_v, speed, E_x = bounds(pos, vel, ps, vol, 2.0)
        node_s, node_g = node_rounding(vol)

        def exact(p):  # the plane at world positions, in float64; l from the exact rotation of the float32 rot
            return ((np.asarray(p, np.float64) - ps["centre"].astype(np.float64)) @ R64.T) @ nrm - c

        ok = decided(pos, ps, vol, E_g, E_s)
        s32, n32, in32, G32 = V.sample(pos, ps, vol)
        both = ok & in32
        assert both.sum() > 1000
        es = np.abs(s32.astype(np.float64) - exact(pos))[both]
        assert np.all(es <= (E_s + node_s)[both]), float((es / (E_s + node_s)[both]).max())
        s64, n64, _, G64 = V.sample(pos, ps, vol, np.float64)
        eg = np.sqrt(((G64 - nrm) ** 2).sum(axis=1))[both]
        assert np.all(eg <= node_g + 1e-12), float(eg.max())  # trilinear is exact for an affine field: the gradient IS nrm
        eg32 = np.sqrt(((G32.astype(np.float64) - nrm) ** 2).sum(axis=1))[both]
        assert np.all(eg32 <= (E_x + node_g)[both]), float((eg32 / (E_x + node_g)[both]).max())
        a = V.collide(pos, vel, [vol], [ps], *EXT)
        hit = a["hit"][0] & ok
        assert 300 < hit.sum() < both.sum(), hit.sum()
        # after the call a touched particle lies at distance `margin`: the plane extends beyond the domain, so wherever the
        # particle ended its exact value there is s + out * dot(nrm, R n), within the push-out's error E_p of the margin
        # (the plane is 1-Lipschitz); rot is a rotation to a few eps only, which the push-out length carries
        out = np.abs(float(ps["margin"]) - s64)
        tol = (E_p + node_s + out * (node_g + 8 * EPS))[hit]
        short = np.abs(exact(a["pos"]) - float(ps["margin"]))[hit]
        print("plane %d: %d touched, worst |s - margin| / bound %.3f" % (seed, hit.sum(), float((short / tol).max())))
        assert np.all(short <= tol), float((short / tol).max())


# ---- (c) a sphere's exact distance, sampled ----------------------------------------------------------------------------------
def trilinear_bound(d, spacing):
    """|interpolant - (d - r)| for a sphere's distance: per axis h_a^2 / 8 times the second derivative, at most 1 / d' at
    the nearest point d' >= d - |spacing| of the cell."""
    h = np.asarray(spacing, np.float64)
    return (h ** 2).sum() / 8.0 / (d - np.sqrt((h ** 2).sum()))


def test_a_sampled_sphere_is_within_the_trilinear_error_bound_of_the_analytic_one():
    r, half = 0.3, 0.5  # (the bound needs d > |spacing|: 0.2165 at N = 9 on this domain, below the 0.25 the particles keep)
    pos, vel = scene(77, n=4000, half=0.48)
    d = np.sqrt((pos.astype(np.float64) ** 2).sum(axis=1))
    far = d > 0.25
    ps = V.pose(0, (0.0, 0.0, 0.0), restitution=0.5, friction=0.2, margin=0.03)
    for N in (9, 17, 33):
        vol = sphere_volume(N, r, half)
        s64, n64, inside, _ = V.sample(pos, ps, vol, np.float64)
        assert inside.all()
        bound = trilinear_bound(d[far], vol["spacing"]) + EPS * float(np.abs(vol["sdf"]).max())  # (the nodes are float32)
        err = np.abs(s64[far] - (d[far] - r))
        print("N = %d: worst |s - (d - r)| / bound %.3f" % (N, float((err / bound).max())))
        assert np.all(err <= bound), (N, float((err / bound).max()))
    # N = 33: the call against tests/solids_ref.py on the analytic sphere.  p' = p + (margin - s) n in both, so
    #   p'_v - p'_a = (s_a - s_v) n_v + (margin - s_a) (n_v - n_a):
    # the interpolation bound plus the PUSH-OUT LENGTH margin - s_a times the normal's angular error |n_v - n_a|, both
    # measured in float64 here, plus the two restatements' own roundings (E_p of each).  For a particle outside the solid
    # (0 <= s_a < margin: water that came nearer than the margin) the push-out length is at most the margin -- the bound
    # "margin times the angular error"; a particle that starts inside the solid is pushed further than the margin and its
    # normal's error weighs that much more, so it is held to its own push-out length.
    from test_solids_reference import bounds as solid_bounds

    ball = S.solid(S.SPHERE, (0.0, 0.0, 0.0), r, restitution=0.5, friction=0.2, margin=0.03)
    a = V.collide(pos, vel, [vol], [ps], *EXT)
    b = S.collide(pos, vel, [ball], *EXT)
    sa, na = S.distance(pos, ball, np.float64)
    angular = np.sqrt(((n64 - na) ** 2).sum(axis=1))
    margin = float(ps["margin"])
    _, _, _, E_pv, _, _, _ = bounds(pos, vel, ps, vol, 2.0)
    _, _, E_ps, _, _ = solid_bounds(pos, vel, ball, 2.0)
    interp = trilinear_bound(d, vol["spacing"]) + EPS * float(np.abs(vol["sdf"]).max())
    same = far & a["hit"][0] & b["hit"][0]
    undecided = far & (a["hit"][0] != b["hit"][0])
    assert np.all(np.abs(sa[undecided] - margin) <= interp[undecided])  # a contact in one only: within the bound of the margin
    diff = np.sqrt(((a["pos"].astype(np.float64) - b["pos"].astype(np.float64)) ** 2).sum(axis=1))
    outside, inside_solid = same & (sa >= 0), same & (sa < 0)
    assert outside.sum() > 100 and inside_solid.sum() > 100, (outside.sum(), inside_solid.sum())
    tol = interp + margin * angular + E_pv + E_ps
    print("N = 33: %d contacts from outside, worst position difference / bound %.3f" % (outside.sum(), float((diff / tol)[outside].max())))
    assert np.all(diff[outside] <= tol[outside]), float((diff / tol)[outside].max())
    tol = interp + (margin - sa) * angular + E_pv + E_ps
    print("N = 33: %d contacts from inside, worst position difference / bound %.3f" % (inside_solid.sum(), float((diff / tol)[inside_solid].max())))
    assert np.all(diff[inside_solid] <= tol[inside_solid]), float((diff / tol)[inside_solid].max())


# ---- planted cases of the definition ---------------------------------------------------------------------------------------
def test_the_planted_cases_of_the_definition():
    # one cell, node values in binary fractions: s = y - 0.25 exactly on a 2 x 2 x 2 volume over [0, 1]^3
    xyz = V.nodes((2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    cell = V.volume(xyz[..., 1] - 0.25, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    ps = V.pose(0, margin=0.125)
    pos = np.array([[0.5, 0.375, 0.5],                               # s == margin exactly: not a contact
                    [0.5, np.nextafter(F32(0.375), F32(0)), 0.5],    # just below: a contact
                    [1.0, 0.25, 1.0],                                # on the far faces (g == dims - 1, f == 1): in the domain
                    [np.nextafter(F32(1.0), F32(2)), 0.25, 1.0],     # one step beyond: outside, the volume says nothing
                    [0.0, 0.0, 0.0],                                 # exactly at a node
                    [0.5, -0.001, 0.5]], F32)                        # below the domain: outside
    a = V.collide(pos, np.zeros_like(pos), [cell], [ps], *EXT)
    assert list(a["hit"][0]) == [False, True, True, False, True, False]
    assert np.array_equal(a["pos"][2], np.array([1.0, 0.375, 1.0], F32)) and np.array_equal(a["pos"][4], np.array([0.0, 0.375, 0.0], F32))
    assert np.array_equal(a["pos"][[0, 3, 5]].view(np.uint32), pos[[0, 3, 5]].view(np.uint32))
    # a constant negative volume has no gradient: every particle in the domain leaves along local up, R_1
    flat = V.volume(np.full((2, 2, 2), -0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    quarter = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], F32)
    a = V.collide(np.array([[-0.5, 0.5, 0.5]], F32), np.zeros((1, 3), F32), [flat], [V.pose(0, rot=quarter, margin=0.25)], *EXT)
    assert a["hit"][0][0] and np.array_equal(a["pos"][0], np.array([-1.25, 0.5, 0.5], F32))  # R_1 = (-1, 0, 0); out = 0.75
    # an all-zero rot: l = 0 for every particle; in the domain iff the origin is, and the normal is the zero vector
    a = V.collide(pos, np.ones_like(pos), [cell], [V.pose(0, rot=np.zeros((3, 3)), margin=0.125)], *EXT)
    assert a["hit"][0].all() and np.array_equal(a["pos"], pos) and np.array_equal(a["vel"], np.ones_like(pos))


def test_the_order_of_the_poses_is_part_of_the_contract_and_a_slot_may_be_posed_twice():
    pos, vel = scene(31)
    vol = sphere_volume(17)
    p0 = V.pose(0, (0.1, -0.2, 0.05), restitution=0.5, friction=0.2, margin=0.03)
    p1 = V.pose(0, (0.4, 0.1, 0.0), rot=S.rotation((0.0, 0.0, 1.0), 0.5), restitution=0.25, margin=0.05)
    ab, ba = V.collide(pos, vel, [vol], [p0, p1], *EXT), V.collide(pos, vel, [vol], [p1, p0], *EXT)
    assert (ab["hit"][0] & ab["hit"][1]).sum() > 20
    assert np.any(ab["pos"].view(np.uint32) != ba["pos"].view(np.uint32))
    first = V.collide(pos, vel, [vol], [p0], *EXT)
    second = V.collide(first["pos"], first["vel"], [vol], [p1], *EXT)
    assert np.array_equal(second["pos"].view(np.uint32), ab["pos"].view(np.uint32))
    assert np.array_equal(second["vel"].view(np.uint32), ab["vel"].view(np.uint32))
    assert np.array_equal(second["sums"][0], ab["sums"][1])
