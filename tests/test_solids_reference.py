"""tests/solids_ref.py, the float32 restatement of ws_collide_solids the GPU tests compare bits with, against a float64
evaluation of the same formulas, and the properties the definition promises (include/wsfluid.h).

The tolerances are derived, not tuned.  eps = 2^-24; every float32 operation is rounded once and errs by at most eps of
its result.  With q = p - c, rn = max(1, the largest row norm of rot) and the scale M = rn |q| + |size| + margin:

  signed distance.  q: 1 rounding.  A dot product with q: 5 more, at most 6 eps rn |q| in all.
    SPHERE:  d = sqrt(dot(q, q)) is good to 4 eps d, s = d - r adds one: E_s <= 5 eps M.
    BOX:     a_i = |l_i| - b_i: 7 eps M each; inside s = g: 7 eps M; outside d = |u| moves by at most |delta u| <=
             sqrt(3) 7 eps M, plus its own 4 eps d: E_s <= 17 eps M.
    CAPSULE: l_1: 6; t R_1,a and the difference: 2 more on top of q's own: each w_a within 9 eps M, so |w| within
             sqrt(3) 9 eps M, plus its own 4 eps d, plus s = d - r: E_s <= 21 eps M.
    N_S = 21 covers every kind.
  normal.  n = x / |x| for x = q, u or w, known to E_x <= sqrt(3) 9 eps M: the direction errs by E_n <= 2 E_x / |x| + 2 eps
    (never more than 2); a face normal of a box is a row of rot: exact.
  push-out.  p' = p + (margin - s) n: E_p <= E_s + out E_n + 3 eps (|p| + out) per axis, out = margin - s, times sqrt(3)
    for the vector.
  velocity.  With the speed scale S = |v| + |V| + |W| |r|, e = restitution, f = friction: r = p' - c carries E_p, u = V +
    W x r carries |W| E_p and 4 roundings at S, rel one more, vn = dot(rel, n) five more and S E_n; j, tang and dv are
    linear in these with factors (1 + e) and f and 6 more roundings at S:
    E_v <= 2 (1 + e + f) (|W| E_p + S (2 E_n + 20 eps)).
  A discrete decision (contact, inside / outside, the face, kicked or not) can differ between the two arithmetics only
  where its float64 discriminant lies within its error of zero; the comparisons leave those particles out and count them.

What the push-out promises.  p' lies at signed distance exactly `margin` in exact arithmetic for a sphere, a capsule and a
solid box in either sense, and for a HOLLOW box when one wall is involved.  A hollow box is not convex from the inside: a
particle outside it beyond an edge or a corner is pushed through that edge along the diagonal and comes to rest at
distance margin from the EDGE, margin / sqrt(2) or margin / sqrt(3) from the walls; and a particle within `margin` of two
walls is moved away from the nearer one only.  Both are properties of the definition, not of the arithmetic, so the
hollow box is tested with margin = 0 (exact: the particle lands on the surface) and, with a margin, on the particles
that have one wall to deal with."""
import numpy as np

import solids_ref as S

F32 = np.float32
EPS = 2.0 ** -24
N_S = 21


def scene(seed, n=3000):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    return pos, vel


EXT = (np.array([-4, -4, -4], F32), np.array([4, 4, 4], F32), F32(0.95))


def solids():
    R = S.rotation((1.0, 2.0, -0.5), 0.7)
    out = {}
    for hollow in (False, True):
        tag = "-hollow" if hollow else ""
        out["sphere" + tag] = S.solid(S.SPHERE, (0.1, -0.2, 0.05), 0.6, hollow=hollow, restitution=0.5, friction=0.2, margin=0.03)
        out["capsule" + tag] = S.solid(S.CAPSULE, (0.0, 0.1, 0.0), (0.4, 0.5), rot=R, hollow=hollow, restitution=0.3, friction=0.1,
                                       margin=0.02)
        out["box" + tag] = S.solid(S.BOX, (0.05, 0.0, -0.1), (0.5, 0.3, 0.4), rot=R, hollow=hollow, restitution=0.25,
                                   friction=0.3, margin=0.0 if hollow else 0.04)
    out["moving"] = S.solid(S.BOX, (0.0, 0.0, 0.0), (0.5, 0.4, 0.3), rot=R, velocity=(1.0, -0.5, 0.25),
                            angular_velocity=(0.5, 3.0, -1.0), restitution=1.0, friction=1.0, margin=0.05)
    out["spinning-sphere"] = S.solid(S.SPHERE, (0.0, 0.0, 0.0), 0.7, velocity=(0.0, 2.0, 0.0), angular_velocity=(0.0, 0.0, 4.0),
                                     restitution=0.0, friction=0.5, margin=0.01)
    return out


def scales(pos, s):
    """(M, |x| of the vector the normal is the direction of, in float64; inf where the normal is a row of rot)."""
    q = pos.astype(np.float64) - s["centre"].astype(np.float64)
    R, size = s["rot"].astype(np.float64), s["size"].astype(np.float64)
    rn = max(1.0, float(np.sqrt((R * R).sum(axis=1)).max())) if s["kind"] != S.SPHERE else 1.0
    used = {S.SPHERE: size[:1], S.CAPSULE: size[:2], S.BOX: size}[s["kind"]]
    M = rn * np.sqrt((q * q).sum(axis=1)) + np.sqrt((used * used).sum()) + float(s["margin"])
    if s["kind"] == S.SPHERE:
        x = np.sqrt((q * q).sum(axis=1))
    elif s["kind"] == S.CAPSULE:
        t = np.clip(q @ R[1], -size[1], size[1])
        w = q - t[:, None] * R[1][None, :]
        x = np.sqrt((w * w).sum(axis=1))
    else:
        a = np.abs(q @ R.T) - size
        u = np.maximum(a, 0.0)
        x = np.where(a.max(axis=1) > 0, np.sqrt((u * u).sum(axis=1)), np.inf)
    return M, x


def bounds(pos, vel, s, r_len):
    M, x = scales(pos, s)
    with np.errstate(divide="ignore"):
        E_n = np.where(np.isinf(x), 0.0, np.minimum(2.0, 2.0 * np.sqrt(3.0) * 9 * EPS * M / x + 2 * EPS))
    E_s = N_S * EPS * M
    sd64, _ = S.distance(pos, s, np.float64)
    out = np.abs(float(s["margin"]) - sd64)
    pn = np.sqrt((pos.astype(np.float64) ** 2).sum(axis=1))
    E_p = np.sqrt(3.0) * (E_s + out * E_n + 3 * EPS * (pn + out))
    W = float(np.sqrt((s["angular_velocity"].astype(np.float64) ** 2).sum()))
    V = float(np.sqrt((s["velocity"].astype(np.float64) ** 2).sum()))
    speed = np.sqrt((vel.astype(np.float64) ** 2).sum(axis=1)) + V + W * r_len
    e, f = float(s["restitution"]), float(s["friction"])
    E_v = 2 * (1 + e + f) * (W * E_p + speed * (2 * E_n + 20 * EPS))
    return E_s, E_n, E_p, E_v, speed


def decided(pos, vel, s, E_s):
    """Particles whose discrete decisions cannot differ between float32 and float64."""
    sd64, n64 = S.distance(pos, s, np.float64)
    ok = np.abs(sd64 - float(s["margin"])) > E_s
    if s["kind"] == S.BOX:
        q = pos.astype(np.float64) - s["centre"].astype(np.float64)
        a = np.sort(np.abs(q @ s["rot"].astype(np.float64).T) - s["size"].astype(np.float64), axis=1)
        ok &= (np.abs(a[:, 2]) > E_s) & ((a[:, 2] > 0) | (a[:, 2] - a[:, 1] > 2 * E_s))  # inside / outside, and the face
        ok &= ~((a[:, 2] > 0) & (np.abs(a[:, 1]) < E_s))  # ... and which components of u are zero
    return ok


def test_the_restatement_is_within_the_derived_bounds_of_float64():
    for seed, (name, s) in enumerate(solids().items()):
        pos, vel = scene(seed)
        a = S.collide(pos, vel, [s], *EXT)
        E_s, E_n, E_p, E_v, speed = bounds(pos, vel, s, 2.0)
        s32, _ = S.distance(pos, s)
        s64, n64 = S.distance(pos, s, np.float64)
        assert np.all(np.abs(s32.astype(np.float64) - s64) <= E_s), name
        b = S.collide(pos, vel, [s], *EXT, T=np.float64)
        ok = decided(pos, vel, s, E_s)
        # kicked or not: vn64 within its error of zero is undecided
        r64 = b["pos"] - s["centre"].astype(np.float64)
        u64 = s["velocity"].astype(np.float64) + np.cross(s["angular_velocity"].astype(np.float64), r64)
        vn64 = ((vel.astype(np.float64) - u64) * n64).sum(axis=1)
        ok &= ~(b["hit"][0] & (np.abs(vn64) <= E_v))
        assert ok.mean() > 0.98, (name, ok.mean())  # the undecided are the rare exception
        assert np.array_equal(a["hit"][0][ok], b["hit"][0][ok]), name
        hit = a["hit"][0] & ok
        assert 100 < hit.sum() < len(pos), (name, hit.sum())
        ep = np.abs(a["pos"].astype(np.float64) - b["pos"])[hit]
        ev = np.abs(a["vel"].astype(np.float64) - b["vel"])[hit]
        print("%s: %d contacts, worst position error / bound %.3f, velocity %.3f" %
              (name, hit.sum(), float((ep / E_p[hit, None]).max()), float((ev / E_v[hit, None]).max())))
        assert np.all(ep <= E_p[hit, None]), (name, float((ep / E_p[hit, None]).max()))
        assert np.all(ev <= E_v[hit, None]), (name, float((ev / E_v[hit, None]).max()))
        assert np.array_equal(a["pred"], (a["pos"] + (a["vel"] * F32(0.02)).astype(F32)).astype(F32))
        assert a["contacts"].dtype == np.uint32 and a["contacts"][0] == a["hit"][0].sum()


def one_wall(pos, s):
    """For a hollow box with a margin: the particles that have one wall to deal with (see the module's text)."""
    q = pos.astype(np.float64) - s["centre"].astype(np.float64)
    a = np.sort(np.abs(q @ s["rot"].astype(np.float64).T) - s["size"].astype(np.float64), axis=1)
    return a[:, 1] <= -float(s["margin"])  # the second-nearest wall is further than margin inside


def test_a_touched_particle_ends_at_the_margin_and_bounces_with_the_restitution():
    cases = dict(solids())
    R = S.rotation((0.0, 1.0, 0.3), -0.4)
    cases["box-hollow-margin"] = S.solid(S.BOX, (0.0, 0.0, 0.0), (0.7, 0.6, 0.8), rot=R, hollow=True, restitution=0.5,
                                         friction=0.1, margin=0.05)
    for seed, (name, s) in enumerate(cases.items()):
        pos, vel = scene(100 + seed)
        a = S.collide(pos, vel, [s], *EXT)
        hit = a["hit"][0].copy()
        if name == "box-hollow-margin":
            hit &= one_wall(pos, s)
        assert hit.sum() > 100, (name, hit.sum())
        E_s, E_n, E_p, E_v, speed = bounds(pos, vel, s, 2.0)
        after, _ = S.distance(a["pos"], s, np.float64)
        # the distance function is 1-Lipschitz: p' within E_p of the exact push-out is within E_p of `margin`
        slack = float(s["margin"]) - after[hit]
        print("%s: %d touched, worst shortfall / bound %.3f" % (name, hit.sum(), float((slack / E_p[hit]).max())))
        assert np.all(slack <= E_p[hit]), (name, float((slack / E_p[hit]).max()))
        # normal relative velocity: -restitution times the old one (float64 normal at the old position, the solid's
        # surface velocity at the new one, as the definition takes them)
        _, n64 = S.distance(pos, s, np.float64)
        r64 = a["pos"].astype(np.float64) - s["centre"].astype(np.float64)
        u64 = s["velocity"].astype(np.float64) + np.cross(s["angular_velocity"].astype(np.float64), r64)
        vn_old = ((vel.astype(np.float64) - u64) * n64).sum(axis=1)
        vn_new = ((a["vel"].astype(np.float64) - u64) * n64).sum(axis=1)
        kicked = hit & np.any(a["dv"][0] != 0, axis=1)
        tol = E_v + speed * E_n
        assert kicked.sum() > 30 and np.all(vn_old[kicked] < tol[kicked]), name
        err = np.abs(vn_new - (-float(s["restitution"]) * vn_old))[kicked]
        assert np.all(err <= tol[kicked]), (name, float((err / tol[kicked]).max()))
        # moved, not kicked: the velocity keeps its bits
        moved = hit & ~kicked
        assert np.array_equal(a["vel"][moved].view(np.uint32), vel[moved].view(np.uint32)), name
        assert np.all(vn_old[moved] > -tol[moved]), name


def test_a_hollow_box_leaves_a_corner_particle_nearer_than_the_margin_by_definition():
    """The limit of the definition the module's text describes, pinned so that nobody takes it for a rounding error."""
    s = S.solid(S.BOX, (0, 0, 0), (1.0, 1.0, 1.0), hollow=True, margin=0.1)
    a = S.collide(np.array([[1.5, 1.5, 0.0]], F32), np.zeros((1, 3), F32), [s], *EXT)
    after, _ = S.distance(a["pos"], s, np.float64)
    assert a["hit"][0][0] and abs(after[0] - 0.1 / np.sqrt(2.0)) < 1e-6


def test_untouched_particles_keep_their_bits_minus_zero_included():
    pos, vel = scene(7)
    pos[::9] = F32(-0.0) * pos[::9]
    vel[::7] = F32(-0.0)
    vel[3::7, 1] = F32(-0.0)
    s = [S.solid(S.SPHERE, (0.9, 0.9, 0.9), 0.5, margin=0.02), S.solid(S.BOX, (-0.8, 0.0, 0.0), (0.3, 0.3, 0.3), margin=0.01)]
    a = S.collide(pos, vel, s, *EXT)
    out = ~a["touched"]
    assert 0 < out.sum() < len(pos) and a["contacts"].min() > 0
    assert np.array_equal(a["pos"][out].view(np.uint32), pos[out].view(np.uint32))
    assert np.array_equal(a["vel"][out].view(np.uint32), vel[out].view(np.uint32))
    assert np.any(np.signbit(a["vel"][out]) & (a["vel"][out] == 0)) and np.any(np.signbit(a["pos"][out]) & (a["pos"][out] == 0))


def test_the_planted_cases_of_the_definition():
    vel = np.zeros((4, 3), F32)
    sph = S.solid(S.SPHERE, (0.25, 0.5, -0.25), 0.5, margin=0.125)
    pos = np.array([[0.25, 0.5, -0.25], [0.875, 0.5, -0.25], [np.nextafter(F32(0.875), F32(0)), 0.5, -0.25], [3, 3, 3]], F32)
    a = S.collide(pos, vel, [sph], *EXT)
    assert list(a["hit"][0]) == [True, False, True, False]          # s == margin is not a contact
    assert np.array_equal(a["pos"][0], np.array([0.25, 1.125, -0.25], F32))  # the centre leaves along (0, 1, 0)
    hol = S.solid(S.SPHERE, (0.25, 0.5, -0.25), 0.5, hollow=True, margin=0.125)
    a = S.collide(pos, vel, [hol], *EXT)
    assert list(a["hit"][0]) == [False, True, True, True] and np.array_equal(a["pos"][0], pos[0])
    # the tie: equally deep under two faces of a box, the lowest axis wins, with the sign of that coordinate
    box = S.solid(S.BOX, (0, 0, 0), (1.0, 1.0, 1.0), margin=0.25)
    tie = np.array([[0.25, -0.75, -0.75], [-0.5, 0.5, 0.25], [0.0, 0.0, 0.0]], F32)
    a = S.collide(tie, vel[:3], [box], *EXT)
    assert np.array_equal(a["pos"], np.array([[0.25, -1.25, -0.75], [-1.25, 0.5, 0.25], [1.25, 0.0, 0.0]], F32))
    cap = S.solid(S.CAPSULE, (0, 0, 0), (0.5, 1.0), margin=0.0)
    on_axis = np.array([[0.0, 0.5, 0.0], [0.0, 1.25, 0.0]], F32)
    a = S.collide(on_axis, vel[:2], [cap], *EXT)
    assert np.array_equal(a["pos"], np.array([[0.5, 0.5, 0.0], [0.0, 1.5, 0.0]], F32))  # on the axis: out along R_0


def test_the_reaction_is_the_integer_sum_of_the_quantised_velocity_changes():
    pos, vel = scene(21, n=4000)
    vel *= F32(3.0)
    ss = [solids()["moving"], solids()["sphere"], S.solid(S.CAPSULE, (0.5, 0.5, 0.0), (0.3, 0.4), rot=S.rotation((0, 0, 1), 1.0),
                                                          restitution=0.8, friction=0.4, margin=0.02),
          S.solid(S.SPHERE, (9, 9, 9), 0.5)]
    a = S.collide(pos, vel, ss, *EXT)
    assert a["contacts"][:3].min() > 100 and a["contacts"][3] == 0
    for e in range(4):
        dv, r = a["dv"][e], a["r"][e]
        kicked = np.any(dv != 0, axis=1)
        I = (-dv[kicked]).astype(F32)
        H = S.cross(r[kicked], I).astype(F32)
        want = [0] * 6
        for row in np.concatenate([I, H], axis=1):
            for w in range(6):
                x = min(max(float(row[w]), -2.0 ** 31), 2.0 ** 31) * 2.0 ** 24
                assert x == int(x) or abs(x) < 2.0 ** 53
                want[w] += int(np.rint(x))
        assert [int(x) for x in a["sums"][e]] == [w & S.MASK64 for w in want], e
        assert np.array_equal(a["impulse"][e], np.array(want[:3], np.float64) * 2.0 ** -24)
        assert np.array_equal(a["angular"][e], np.array(want[3:], np.float64) * 2.0 ** -24)
        # ... which is the float64 sum of -dv to within the quantum per contact
        assert np.all(np.abs(a["impulse"][e] - (-dv.astype(np.float64)).sum(axis=0)) <= kicked.sum() * 2.0 ** -25 + 1e-300)
    assert np.all(a["impulse"][3] == 0) and np.all(a["angular"][3] == 0)
    # a huge change is clamped, not wrapped; the sum wraps modulo 2^64
    assert [int(x) for x in S.quantise(np.array([3e9, -3e9, 0.5 * 2.0 ** -24, 1.5 * 2.0 ** -24], F32))] == [2 ** 55, -2 ** 55, 0, 2]


def test_the_order_of_the_solids_is_part_of_the_contract():
    pos, vel = scene(31)
    a = solids()["sphere"]
    b = S.solid(S.BOX, (0.3, -0.2, 0.0), (0.5, 0.5, 0.5), margin=0.03, restitution=0.5)
    ab, ba = S.collide(pos, vel, [a, b], *EXT), S.collide(pos, vel, [b, a], *EXT)
    both = ab["hit"][0] & ab["hit"][1]
    assert both.sum() > 20
    assert np.any(ab["pos"].view(np.uint32) != ba["pos"].view(np.uint32))
    # the running position: the second solid sees where the first one put the particle
    first = S.collide(pos, vel, [a], *EXT)
    second = S.collide(first["pos"], first["vel"], [b], *EXT)
    assert np.array_equal(second["pos"].view(np.uint32), ab["pos"].view(np.uint32))
    assert np.array_equal(second["vel"].view(np.uint32), ab["vel"].view(np.uint32))
    assert np.array_equal(second["sums"][0], ab["sums"][1])


def test_the_container_rule_applies_to_touched_particles_only():
    ext = (np.array([-1, -1, -1], F32), np.array([1, 1, 1], F32), F32(0.5))
    s = S.solid(S.SPHERE, (0.9, 0.0, 0.0), 0.5, margin=0.0)
    pos = np.array([[0.95, 0.0, 0.0], [-2.0, 0.0, 0.0]], F32)  # the first is pushed through the wall; the second is outside, untouched
    vel = np.array([[-1.0, 0.5, 0.0], [1.0, 1.0, 1.0]], F32)
    a = S.collide(pos, vel, [s], *ext)
    assert a["pos"][0, 0] == F32(1.0) and np.array_equal(a["pos"][1], pos[1]) and np.array_equal(a["vel"][1], vel[1])
    kick = S.collide(pos, vel, [s], np.array([-9, -9, -9], F32), np.array([9, 9, 9], F32), F32(0.5))
    assert a["vel"][0, 0] == F32(kick["vel"][0, 0] * F32(-0.5)) and a["vel"][0, 1] == kick["vel"][0, 1]
    assert np.array_equal(a["sums"], kick["sums"])  # the wall's velocity change does not enter the reaction
