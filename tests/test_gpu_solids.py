"""ws_collide_solids on the GPU: bit for bit against the numpy restatement (tests/solids_ref.py) at every launch shape --
positions, velocities, predicted positions, contact counts and both reaction sums -- the step picking the edit up exactly
as it picks up a host edit through ws_write_particles, a call that touches nothing changing nothing (a captured step
included), the views the call must leave alone, water that stays out of a sphere and inside a hollow box, slabs, this
call and ws_apply_forces between the same two steps in either order, refusals."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as F
import solids_ref as S
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_forces import _emitter_sets, _host_apply, _scene, _xyz
from test_gpu_forces import _moving as _moving_forces
from test_solids_reference import bounds

pytestmark = pytest.mark.gpu
F32 = np.float32
BLOCK = 256  # threads per workgroup of k_edit_current (WS_BLOCK)


def _ext(params):
    return np.array(params.ext_min[:3], F32), np.array(params.ext_max[:3], F32), F32(params.collision_damping)


def _load(w, rec, pos=None, vel=None, pred=None):
    """The state with new positions, velocities and predicted positions through ws_write_particles."""
    rec = rec.copy()
    for field, val in (("position", pos), ("velocity", vel), ("predicted_position", pred)):
        if val is not None:
            rec[field][:, :3] = val
    w.write_slice("particles", rec)


def _host_collide(w, solids, params):
    """ws_read_particles, the restatement on the host, ws_write_particles: what a host without the call has to do."""
    rec = w.read_vec("particles")
    a = S.collide(_xyz(rec, "position"), _xyz(rec, "velocity"), solids, *_ext(params))
    _load(w, rec, a["pos"], a["vel"], a["pred"])
    return a


def _same_reaction(got, want, what):
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want["contacts"]), (what, got[0], want["contacts"])
    assert np.array_equal(got[1], want["impulse"]), (what, got[1], want["impulse"])
    assert np.array_equal(got[2], want["angular"]), (what, got[2], want["angular"])


# ---- 1. bits against the restatement ------------------------------------------------------------------------------------------
SPHERE = dict(centre=(0.25, 0.5, -0.25), size=0.5, margin=0.125)  # binary fractions: s == margin exactly at x = 0.875
QUARTER = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]                      # a quarter turn about z: exact entries


def _solid_sets():
    rng = np.random.default_rng(42)
    R = S.rotation((1.0, 2.0, -0.5), 0.7)
    # the tie: q = (0.25, -0.25, 0.125) from this box's centre is 0.25 under two faces (l_0 = q_y, l_1 = -q_x)
    tie_box = S.solid(S.BOX, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), rot=QUARTER, restitution=0.5, friction=0.25, margin=0.0625)
    sets = {
        "sphere": [S.solid(S.SPHERE, restitution=0.5, friction=0.2, velocity=(0.5, 0.0, 0.0), **SPHERE)],
        "box": [S.solid(S.BOX, (0.3, 0.1, 0.2), (0.5, 0.3, 0.4), rot=R, restitution=0.25, friction=0.3, margin=0.04,
                        angular_velocity=(0.0, 2.0, 0.5)), tie_box],
        "capsule": [S.solid(S.CAPSULE, (0.0, 0.1, 0.0), (0.3, 0.5), rot=R, restitution=0.3, friction=0.1, margin=0.02)],
        "hollow": [S.solid(S.SPHERE, (0.0, 0.0, 0.0), 1.25, hollow=True, restitution=0.5, friction=0.5, margin=0.05)],
        # rot is the host's: all zeros makes every particle "inside" with a zero normal -- touched, neither moved nor kicked
        "degenerate": [S.solid(S.BOX, (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), rot=np.zeros((3, 3)), margin=0.01),
                       S.solid(S.SPHERE, restitution=1.0, **SPHERE)],
    }
    mixed = [S.solid(S.SPHERE, restitution=0.5, friction=0.2, **SPHERE), tie_box,
             S.solid(S.BOX, (0.6, -0.6, 0.5), (0.2, 0.2, 0.2), rot=0.5 * R, margin=0.01, restitution=0.5),  # half-size rows: a 0.4 box
             S.solid(S.BOX, (0.0, 0.0, 0.0), (0.95, 1.2, 0.9), hollow=True, margin=0.03, friction=1.0)]
    for e in range(4, 15):
        kind = e % 3
        size = {S.SPHERE: rng.uniform(0.1, 0.3, 1), S.BOX: rng.uniform(0.1, 0.3, 3), S.CAPSULE: rng.uniform(0.1, 0.25, 2)}[kind]
        mixed.append(S.solid(kind, rng.uniform(-0.8, 0.8, 3), size, rot=S.rotation(rng.normal(0, 1, 3), rng.uniform(0, 3)),
                             velocity=rng.normal(0, 1, 3), angular_velocity=rng.normal(0, 2, 3) if e % 2 else (0, 0, 0),
                             restitution=rng.uniform(0, 1), friction=rng.uniform(0, 1), margin=rng.uniform(0, 0.05)))
    mixed.append(S.solid(S.CAPSULE, (50.0, 50.0, 50.0), (1.0, 1.0)))  # touches nothing
    sets["mixed16"] = mixed
    return sets


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000, 4097])
def test_the_call_gives_the_restatements_bits(ws, n):
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(n)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    pos[0] = SPHERE["centre"]                     # exactly at the sphere's centre
    if n > 2:
        pos[1] = (0.875, 0.5, -0.25)              # exactly s == margin of it: not a contact
        pos[2] = (-0.25, -0.75, -0.375)           # the tie under two faces of tie_box
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    vel[::5, 0] = F32(-0.0)
    vel[3::7] = F32(-0.0)
    w = ws.FluidWorker(pos, params)
    rec = w.read_vec("particles")
    for name, solids in _solid_sets().items():
        _load(w, rec, vel=vel)
        got = w.collide_solids(S.to_ws(ws, solids))
        state = w.read_vec("particles")
        want = S.collide(pos, vel, solids, *_ext(params))
        _same_reaction(got, want, name)
        assert same_bits(_xyz(state, "position"), want["pos"]), name
        assert same_bits(_xyz(state, "velocity"), want["vel"]), name
        assert same_bits(_xyz(state, "predicted_position"), want["pred"]), name
        assert same_bits(w.read_positions(), want["pos"]) and w.steps_done() == 0, name
        if name in ("sphere", "mixed16"):
            assert want["hit"][0][0] and (n <= 2 or not want["hit"][0][1]), name
            assert want["pos"][0][1] == F32(0.5 + 0.625)  # the centre leaves along (0, 1, 0)
        if name in ("box", "mixed16") and n > 2:
            assert want["hit"][1][2] and want["pos"][2][1] == F32(-0.5 - 0.5 - 0.0625) and want["pos"][2][0] == F32(-0.25), name
        if name == "mixed16":
            assert got[0][-1] == 0 and len(got[0]) == 16 and not got[1][-1].any() and not got[2][-1].any()
            assert n < 1000 or (got[0][:15] > 0).all()
        if name == "degenerate":
            assert got[0][0] == n and not got[1][0].any()
        if n >= 63 and name in ("sphere", "box", "capsule"):  # most particles are untouched, some with -0 components: kept
            out = ~want["touched"]
            assert 0 < out.sum() < n, name
            v_out = _xyz(state, "velocity")[out]
            assert np.any(np.signbit(v_out) & (v_out == 0)), name
            assert n < 1000 or np.abs(got[1][0]).max() > 0 and np.abs(got[2][0]).max() > 0, name
        # without the reaction: the same state
        _load(w, rec, vel=vel)
        assert w.collide_solids(S.to_ws(ws, solids), reaction=False) is None
        state = w.read_vec("particles")
        assert same_bits(_xyz(state, "position"), want["pos"]) and same_bits(_xyz(state, "velocity"), want["vel"]), name
        assert same_bits(_xyz(state, "predicted_position"), want["pred"]), name
    w.close()


def test_any_one_output_is_enough_to_ask_for(ws):
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(5)
    pos = rng.uniform(-1.0, 1.0, (1000, 3)).astype(F32)
    vel = rng.normal(0.0, 2.0, (1000, 3)).astype(F32)
    w = ws.FluidWorker(pos, params)
    rec = w.read_vec("particles")
    solids = _solid_sets()["box"]
    want = S.collide(pos, vel, solids, *_ext(params))
    arr = (ws.fluid.WsSolid * 2)(*S.to_ws(ws, solids))
    for which in range(3):
        _load(w, rec, vel=vel)
        n, imp, ang = np.full(3, 7, np.uint32), np.full((3, 3), 7.0), np.full((3, 3), 7.0)
        ptr = [None, None, None]
        ptr[which] = (n, imp, ang)[which].ctypes.data
        assert w._L.ws_collide_solids(w._h, C.byref(arr), 2, *ptr) == 0
        assert np.array_equal(n[:2], want["contacts"]) if which == 0 else np.all(n == 7)
        assert np.array_equal(imp[:2], want["impulse"]) if which == 1 else np.all(imp == 7.0)
        assert np.array_equal(ang[:2], want["angular"]) if which == 2 else np.all(ang == 7.0)
        assert n[2] == 7 and np.all(imp[2] == 7.0) and np.all(ang[2] == 7.0)  # nothing past k
    w.close()


# ---- 2. the step picks it up exactly as a host edit ---------------------------------------------------------------------------
def _moving(t, centre, reach):
    """A sphere that circles, a rotated box that spins and a capsule that rises with the step number t."""
    c = np.asarray(centre, np.float64)
    s = 0.3 * reach
    return [S.solid(S.SPHERE, c + s * np.array([np.cos(0.3 * t), 0.1, np.sin(0.3 * t)]), 0.2 * reach, restitution=0.5, friction=0.1,
                    velocity=(-0.09 * s * np.sin(0.3 * t) * 50, 0.0, 0.09 * s * np.cos(0.3 * t) * 50), margin=0.01 * reach),
            S.solid(S.BOX, c + s * np.array([-0.6, 0.0, 0.3]), (0.15 * reach, 0.1 * reach, 0.2 * reach),
                    rot=S.rotation((0.2, 1.0, 0.1), 0.15 * t), angular_velocity=(1.0, 5.0, 0.5), restitution=0.2, friction=0.5,
                    margin=0.005 * reach),
            S.solid(S.CAPSULE, c + s * np.array([0.4, -0.5 + 0.05 * t, -0.5]), (0.1 * reach, 0.2 * reach),
                    rot=S.rotation((1.0, 0.0, 0.0), 0.5), velocity=(0.0, 0.05 * s * 50, 0.0), restitution=0.0, friction=0.0,
                    margin=0.0)]


@pytest.mark.parametrize("which", ["merged-4096", "regrid-31646"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_step_picks_the_call_up_exactly_as_a_host_edit(ws, which, ieee):
    pos, params, regrid, centre, reach = _scene(ws, which)
    a = ws.FluidWorker(pos, params, ieee_division=ieee)
    b = ws.FluidWorker(pos, params, ieee_division=ieee)
    if which == "merged-4096":
        assert a.stats()["cells_merged"] != (1, 1, 1)
    seen = 0
    for t in range(20):
        if regrid is not None and t == 10:
            a.set_params(regrid)
            b.set_params(regrid)
        solids = _moving(t, centre, reach)
        got = a.collide_solids(S.to_ws(ws, solids))
        want = _host_collide(b, solids, params)
        _same_reaction(got, want, t)
        seen += int(got[0].sum())
        a.run(1)
        b.run(1)
        assert same_bits(a.read_positions(), b.read_positions()), t
        assert same_bits(a.read_velocities(), b.read_velocities()), t
    assert seen > 20 * 20 and a.steps_done() == 20
    a.close()
    b.close()


# ---- 3. nothing touched changes nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_a_call_that_touches_nothing_changes_nothing(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    outside = [ws.fluid.solid("sphere", (100.0, 100.0, 100.0), 1.0, margin=0.5, restitution=1.0),
               ws.fluid.solid("box", (0.0, 0.0, 0.0), (50.0, 50.0, 50.0), hollow=True, margin=0.25)]
    plain = ws.FluidWorker(pos, params, graph=graph)
    called = ws.FluidWorker(pos, params, graph=graph)
    replayed = []
    for t in range(50):
        got = called.collide_solids(outside, reaction=(t % 2 == 0))
        assert got is None or (not got[0].any() and not got[1].any() and not got[2].any())
        called.run(1)
        plain.run(1)
        if graph:
            replayed.append(called.stats()["graph_steps"])
    want, got = plain.read_vec("particles"), called.read_vec("particles")
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if graph:  # the captured step was neither dropped nor bypassed: one replay per step from the second step on
        assert all(replayed[t] - replayed[t - 1] == 1 for t in range(1, 50)), replayed
        assert plain.stats()["graph_steps"] > 0
    plain.close()
    called.close()


# ---- 4. views ---------------------------------------------------------------------------------------------------------------------
def _flat_solids(dx):
    """Three solids in the plane of the C1 container (16 x 18 x 0.2), shifted by dx."""
    return [S.solid(S.SPHERE, (1.0 + dx, 0.0, 0.0), 1.5, restitution=0.5, friction=0.1, velocity=(1.0, 0.0, 0.0), margin=0.05),
            S.solid(S.BOX, (-3.0 + dx, -2.0, 0.0), (1.0, 0.75, 0.5), rot=S.rotation((0.0, 0.0, 1.0), 0.5), angular_velocity=(0.0, 0.0, 2.0),
                    restitution=0.2, friction=0.5, margin=0.02),
            S.solid(S.CAPSULE, (3.0 + dx, 4.0, 0.0), (0.6, 1.5), rot=S.rotation((0.0, 0.0, 1.0), -0.7), margin=0.0)]


def test_the_views_of_the_last_step_stay_and_the_readers_see_the_new_positions(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    w.run(12)
    before = w.read_vec("particles")
    solids = _flat_solids(0.0)
    got = w.collide_solids(S.to_ws(ws, solids))
    after = w.read_vec("particles")
    want = S.collide(_xyz(before, "position"), _xyz(before, "velocity"), solids, *_ext(params))
    _same_reaction(got, want, "views")
    assert got[0].min() > 0 and before["density"].any() and before["acceleration"].any()
    for field in ("density", "pressure", "acceleration"):
        assert same_bits(after[field], before[field]), field
    for field, key in (("position", "pos"), ("velocity", "vel"), ("predicted_position", "pred")):
        assert same_bits(_xyz(after, field), want[key]), field
    assert not same_bits(want["pos"], _xyz(before, "position")) and w.steps_done() == 12
    assert same_bits(w.read_positions(), want["pos"]) and same_bits(w.read_velocities(), want["vel"])
    # the density field sums over the new positions: the bits of a handle that was loaded with them
    q = _xyz(before, "position")[::16] + F32(0.01)
    other = ws.FluidWorker(pos, params)
    _load(other, before, want["pos"], want["vel"], want["pred"])
    assert same_bits(w.sample_density_points(q), other.sample_density_points(q)) and w.sample_density_points(q).any()
    # a call between the two halves of an asynchronous readback leaves the captured positions alone
    buf = np.empty((w.n, 3), F32)
    w.read_positions_begin(buf)
    w.collide_solids(S.to_ws(ws, _flat_solids(2.5)), reaction=False)
    w.read_positions_end()
    assert same_bits(buf, want["pos"]) and not same_bits(w.read_positions(), want["pos"])
    w.close()
    other.close()


# ---- 5. water stays out -----------------------------------------------------------------------------------------------------------
def test_water_stays_out_of_a_sphere_and_inside_a_hollow_box(ws):
    """The C1 cloud in a container deep enough in z for the sphere's whole margin shell to lie inside it (a push-out that
    the container rule cuts short would end nearer than the margin by design), the hollow box strictly inside the
    container with margin 0 (tests/test_solids_reference.py says why) and the sphere more than its reach from the walls."""
    pos, _ = ws.workloads.make_workload("c1", "cloud")
    params = ws.make_params(container_size=(16.0, 18.0, 3.0))
    glass = S.solid(S.BOX, (0.0, 0.0, 0.0), (7.0, 8.0, 1.4), hollow=True, restitution=0.2, friction=0.1, margin=0.0)
    ball = S.solid(S.SPHERE, (0.5, -5.0, 0.0), 1.2, restitution=0.3, friction=0.2, margin=0.05)
    solids = [glass, ball]
    arr = S.to_ws(ws, solids)
    w = ws.FluidWorker(pos, params)
    contacts = np.zeros(2, np.int64)
    for t in range(200):
        w.run(1)
        contacts += w.collide_solids(arr)[0]
    assert contacts.min() > 0, contacts
    x, v = w.read_positions(), w.read_velocities()
    for e, s in enumerate(solids):
        sd, _ = S.distance(x, s, np.float64)
        _, _, E_p, _, _ = bounds(x, v, s, 2.0)
        short = float(s["margin"]) - sd
        print("kind %d: contacts %d, worst shortfall %.3e, bound there %.3e" % (s["kind"], contacts[e], short.max(),
                                                                                 E_p[np.argmax(short)]))
        assert np.all(short <= E_p), (s["kind"], float((short / E_p).max()))
    w.close()


# ---- 6. slabs ---------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 10


def _slab_solids(t):
    # the cuts of 2 and 3 slabs of the 16-wide container lie at x = 0 and near +-2.7: every solid straddles one
    return [S.solid(S.SPHERE, (0.3 * np.cos(t), -2.5, 0.0), 2.0, restitution=0.5, friction=0.2, velocity=(1.0, 0.0, 0.0), margin=0.05),
            S.solid(S.BOX, (-2.5, -3.0, 0.5), (1.5, 1.0, 2.0), rot=S.rotation((0.0, 1.0, 0.2), 0.4), angular_velocity=(0.0, 1.0, 0.0),
                    margin=0.02, friction=0.5),
            S.solid(S.CAPSULE, (2.7, 0.0, 0.0), (1.0, 2.0), rot=QUARTER, restitution=1.0, margin=0.0)]


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_and_the_same_global_sums_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    w = ws.FluidWorker(pos, params)
    want = []
    for t in range(SLAB_STEPS):
        out = w.collide_solids(S.to_ws(ws, _slab_solids(t))) if t % 2 == 0 else None
        w.run(1)
        if t in (2, SLAB_STEPS - 1):
            want.append((w.read_positions(), w.read_velocities()))
        if out is not None:
            want.append(list(out))
    assert min(int(c[0].min()) for c in want if isinstance(c, list)) > 100
    assert all(np.abs(c[1]).max() > 0 and np.abs(c[2]).max() > 0 for c in want if isinstance(c, list))
    w.close()

    def program(s, r):
        out = []
        for t in range(SLAB_STEPS):
            good = S.to_ws(ws, _slab_solids(t))
            got = None
            if t % 2 == 0:
                got = s.collide_solids(good, reaction=(r != 1))  # rank 1 passes every output NULL and still applies
            elif t == 3:
                # one rank passes an invalid solid: every rank refuses, nothing changes
                bad = S.to_ws(ws, _slab_solids(t))
                if r == 0:
                    bad[1].size[2] = -1.0
                arr = (ws.fluid.WsSolid * 3)(*bad)
                assert s._L.ws_collide_solids(s._h, C.byref(arr), 3, None, None, None) == 1, (r, t)
            elif t == 5:
                # one rank passes a different, valid solid: every rank refuses, nothing changes
                other = S.to_ws(ws, _slab_solids(t))
                if r == world - 1:
                    other[0].restitution = 0.75
                arr = (ws.fluid.WsSolid * 3)(*other)
                n, imp = np.full(3, 7, np.uint32), np.full((3, 3), 7.0)
                assert s._L.ws_collide_solids(s._h, C.byref(arr), 3, n.ctypes.data, imp.ctypes.data, None) == 1, (r, t)
                assert np.all(n == 7) and np.all(imp == 7.0)
            s.run(1)
            if t in (2, SLAB_STEPS - 1):
                out.append((s.read_positions(), s.read_velocities()))
            if t % 2 == 0:
                out.append(got)
        return out

    got = _slab_run(ws, params, pos, world, 0, program)
    for r in range(world):
        assert len(got[r]) == len(want)
        for a, b in zip(got[r], want):
            if isinstance(b, tuple):
                assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), r
            elif r == 1:
                assert a is None
            else:
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (r, a, b)


# ---- 7. two edits between the same two steps ------------------------------------------------------------------------------------
ORDERS = {"forces-then-solids": ("forces", "solids"), "solids-then-forces": ("solids", "forces")}
STATE = ("position", "velocity", "predicted_position")


def _host_two_edits(order, forces, solids, dt, params, host):
    """Both edits in `order` on `host` with no step between them, each one the host's route: a read, the restatement, a
    write back.  Returns the particles that both edits changed, the restatements' outputs per edit and the state."""
    both, outputs = np.ones(host.n, bool), []
    for what in order:
        rec = host.read_vec("particles")
        if what == "forces":
            both &= F.accelerate(_xyz(rec, "position"), _xyz(rec, "velocity"), forces)[1]
            outputs.append(_host_apply(host, forces, dt))
        else:
            outputs.append(_host_collide(host, solids, params))
            both &= outputs[-1]["touched"]
    return both, outputs, host.read_vec("particles")


def _call_two_edits(ws, w, order, forces, solids, dt, outputs):
    """The two calls on `w`, counts and reaction on: the restatements' outputs, and the state they leave."""
    for what, want in zip(order, outputs):
        if what == "forces":
            got = w.apply_forces(F.to_ws(ws, forces), dt)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (order, got, want)
        else:
            _same_reaction(w.collide_solids(S.to_ws(ws, solids)), want, order)
    return w.read_vec("particles")


def _same_state(got, want, fields, what):
    for f in fields:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f)


@pytest.mark.parametrize("order", list(ORDERS))
def test_two_edits_between_two_steps_are_two_host_edits(ws, order):
    n = BLOCK + 1  # two workgroups, the second with one lane
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(n)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    forces, solids = _emitter_sets()["mixed16"], _solid_sets()["mixed16"]
    a, b = ws.FluidWorker(pos, params), ws.FluidWorker(pos, params)
    for w in (a, b):
        _load(w, w.read_vec("particles"), vel=vel)
    dt = F32(1.0 / 60.0)
    both, outputs, want = _host_two_edits(ORDERS[order], forces, solids, dt, params, b)
    assert both.any()  # some particle is seen by an emitter AND touched by a solid
    got = _call_two_edits(ws, a, ORDERS[order], forces, solids, dt, outputs)
    _same_state(got, want, STATE, order)
    assert not same_bits(_xyz(want, "position"), pos) and not same_bits(_xyz(want, "velocity"), vel)
    a.run(1)
    b.run(1)
    _same_state(a.read_vec("particles"), b.read_vec("particles"), want.dtype.names, order)
    assert a.steps_done() == 1
    a.close()
    b.close()


@pytest.mark.parametrize("order", list(ORDERS))
def test_two_edits_between_two_steps_on_slabs(ws, order):
    pos, params, _, centre, reach = _scene(ws, "merged-4096")
    forces = _moving_forces(2, centre, reach, float(params.smoothing_radius))
    solids = _moving(2, centre, reach)
    host = ws.FluidWorker(pos, params)
    dt = F32(params.delta_time)
    both, outputs, want = _host_two_edits(ORDERS[order], forces, solids, dt, params, host)
    assert both.any()
    host.run(1)
    want_stepped = host.read_vec("particles")
    host.close()

    def program(s, r):
        got = _call_two_edits(ws, s, ORDERS[order], forces, solids, dt, outputs)  # (global outputs on every rank)
        s.run(1)
        return got, s.read_vec("particles")

    for r, (got, stepped) in enumerate(_slab_run(ws, params, pos, 2, 0, program)):
        _same_state(got, want, STATE, (order, r))
        _same_state(stepped, want_stepped, want.dtype.names, (order, r))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    steps = 0

    def call(edit=None, k=1, null=False, at=0, kind="box"):
        size = {"box": (1.0, 2.0, 0.5), "sphere": 1.0, "capsule": (1.0, 2.0)}[kind]
        s = [ws.fluid.solid(kind, (0.0, 0.0, 0.0), size, restitution=0.5, friction=0.5, margin=0.1, velocity=(1.0, 0.0, 0.0),
                            angular_velocity=(0.0, 1.0, 0.0)) for _ in range(max(k, 2))]
        if edit:
            edit(s[at])
        arr = (ws.fluid.WsSolid * len(s))(*s)
        n, imp, ang = np.full(17, 7, np.uint32), np.full((17, 3), 7.0), np.full((17, 3), 7.0)
        st = L.ws_collide_solids(h, None if null else C.byref(arr), k, n.ctypes.data, imp.ctypes.data, ang.ctypes.data)
        assert st != 0 and np.all(n == 7) and np.all(imp == 7.0) and np.all(ang == 7.0) or st == 0
        return st

    def set_(name, value, index=None):
        def edit(s):
            if index is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[index] = value
        return edit

    cases = [("NULL s", dict(null=True)), ("k 0", dict(k=0)), ("k 17", dict(k=17)), ("kind 3", dict(edit=set_("kind", 3))),
             ("flags 2", dict(edit=set_("flags", 2))), ("flags 3", dict(edit=set_("flags", 3))),
             ("reserved 0", dict(edit=set_("reserved", 1, 0))), ("reserved 1", dict(edit=set_("reserved", 9, 1))),
             ("second solid", dict(edit=set_("margin", -1.0), k=2, at=1)), ("margin < 0", dict(edit=set_("margin", -0.01))),
             ("capsule length < 0", dict(edit=set_("size", -0.5, 1), kind="capsule"))]
    for name in ("restitution", "friction"):
        cases += [("%s %r" % (name, val), dict(edit=set_(name, val))) for val in (-0.01, 1.01, np.nan, np.inf)]
    for kind, used in (("sphere", 1), ("box", 3), ("capsule", 1)):
        for i in range(used):
            cases += [("%s size[%d] %r" % (kind, i, val), dict(edit=set_("size", val, i), kind=kind)) for val in (0.0, -1.0)]
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        cases += [("centre %r" % val, dict(edit=set_("centre", val, 1))), ("rot %r" % val, dict(edit=set_("rot", val, 7))),
                  ("size %r" % val, dict(edit=set_("size", val, 2))), ("velocity %r" % val, dict(edit=set_("velocity", val, 0))),
                  ("angular %r" % val, dict(edit=set_("angular_velocity", val, 2))), ("margin %r" % val, dict(edit=set_("margin", val))),
                  ("unused size %r" % val, dict(edit=set_("size", val, 2), kind="sphere")),
                  ("unused rot %r" % val, dict(edit=set_("rot", val, 0), kind="sphere"))]
    for what, kw in cases:
        assert call(**kw) == 1, what
        w.run(2)  # ... followed by two good steps
        steps += 2
    fresh.run(steps)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # allowed: the largest magnitudes, a capsule of length 0, zero unused sizes, the limits of the ranges, sixteen solids
    assert call(edit=set_("centre", 1e15, 0)) == 0 and call(edit=set_("size", 0.0, 1), kind="capsule") == 0
    assert call(edit=set_("size", 0.0, 2), kind="sphere") == 0 and call(edit=set_("restitution", 1.0)) == 0
    assert call(edit=set_("friction", 0.0)) == 0 and call(edit=set_("margin", 0.0)) == 0 and call(k=16) == 0
    assert call(edit=set_("flags", 1)) == 0
    w.run(2)
    w.close()
    fresh.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    with pytest.raises(ws.WsError) as e:
        w.collide_solids(ws.fluid.solid("sphere", (0, 0, 0), 1.0))
    assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_the_call(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    s = ws.fluid.solid("sphere", (0, 0, 0), 4.0)
    assert w.collide_solids(s)[0][0] > 0
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    with pytest.raises(ws.WsError) as e:
        w.collide_solids(s)
    assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()
