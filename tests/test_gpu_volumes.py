"""ws_volume_upload / ws_collide_volumes on the GPU: bit for bit against the numpy restatement (tests/volumes_ref.py) at
every launch shape -- positions, velocities, predicted positions, contact counts and both reaction sums -- the step picking
the edit up exactly as it picks up a host edit through ws_write_particles, a call that touches nothing changing nothing (a
captured step included), the views the call must leave alone, water that stays above a tilted plane, slabs, this call with
ws_apply_forces and ws_collide_solids between the same two steps, lifetimes and refusals."""
import ctypes as C
import threading

import numpy as np
import pytest

import forces_ref as F
import solids_ref as S
import volumes_ref as V
from test_gpu_aniso_surface import _slab_run, same_bits
from test_gpu_forces import _emitter_sets, _host_apply, _scene, _xyz
from test_gpu_handle_lifetimes import _leak_over_eight_cycles
from test_gpu_solids import _ext, _load, _same_reaction, _solid_sets
from test_gpu_solids import _host_collide as _host_collide_solids
from test_volumes_reference import bounds, node_rounding, plane_volume, sphere_volume, terrain_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
BLOCK = 256  # threads per workgroup of k_edit_current (WS_BLOCK)
QUARTER = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]  # a quarter turn about z: exact entries


def _host_collide(w, volumes, poses, params):
    """ws_read_particles, the restatement on the host, ws_write_particles: what a host without the call has to do."""
    rec = w.read_vec("particles")
    a = V.collide(_xyz(rec, "position"), _xyz(rec, "velocity"), volumes, poses, *_ext(params))
    _load(w, rec, a["pos"], a["vel"], a["pred"])
    return a


# ---- 1. bits against the restatement ------------------------------------------------------------------------------------------
def _cell():
    """One cell over [0, 1]^3 with s = y - 0.25 in binary fractions: (uint32_t)g is clamped to 0 on the far faces."""
    xyz = V.nodes((2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    return V.volume(xyz[..., 1] - 0.25, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


CELL_POSE = dict(restitution=0.5, friction=0.25, margin=0.125)


def _volume_sets():
    """name -> (the volumes of slots 0 .. , the poses)."""
    rng = np.random.default_rng(42)
    R = S.rotation((1.0, 2.0, -0.5), 0.7)
    rough = V.volume(rng.uniform(-0.5, 0.5, (3, 4, 5)), (-1.0, -0.375, -0.125), (0.5, 0.25, 0.125))
    ball, land = sphere_volume(17), terrain_volume()
    flat = V.volume(np.full((2, 2, 2), -0.5), (-0.5, -0.5, -0.5), (1.0, 1.0, 1.0))
    sets = {
        "cell": ([_cell()], [V.pose(0, **CELL_POSE)]),
        "rough": ([rough], [V.pose(0, (0.0, 0.1, 0.0), rot=R, velocity=(0.5, 0.0, -0.25), angular_velocity=(0.0, 2.0, 0.5),
                                   restitution=0.25, friction=0.3, margin=0.04)]),
        "sphere": ([ball], [V.pose(0, (0.25, 0.5, -0.25), rot=QUARTER, velocity=(0.5, 0.0, 0.0), restitution=0.5, friction=0.2,
                                   margin=0.125)]),
        "terrain": ([land], [V.pose(0, (0.05, 0.0, -0.1), rot=R, angular_velocity=(0.5, 3.0, -1.0), restitution=1.0, friction=1.0,
                                    margin=0.03)]),
        # no gradient anywhere: every particle in the domain leaves along local up, R_1 = (-1, 0, 0)
        "flat": ([flat], [V.pose(0, (0.0, 0.0, 0.0), rot=QUARTER, restitution=0.5, margin=0.25)]),
        # rot is the host's: all zeros puts every particle at l = 0, the origin node, with a zero normal -- touched, neither
        # moved nor kicked
        "zero-rot": ([_cell()], [V.pose(0, rot=np.zeros((3, 3)), margin=0.125, restitution=1.0)]),
    }
    mixed = [V.pose(0, **CELL_POSE), V.pose(2, (0.25, 0.5, -0.25), rot=QUARTER, restitution=0.5, friction=0.2, margin=0.0625),
             V.pose(1, (0.0, 0.1, 0.0), rot=R, margin=0.01, restitution=0.5),
             V.pose(3, (0.0, -0.6, 0.0), margin=0.03, friction=1.0)]
    for e in range(4, 15):
        mixed.append(V.pose((2, 2, 1, 3, 2, 0)[e % 6], rng.uniform(-0.8, 0.8, 3), rot=(0.4 if e % 2 else 1.0) * S.rotation(rng.normal(0, 1, 3), rng.uniform(0, 3)),
                            velocity=rng.normal(0, 1, 3), angular_velocity=rng.normal(0, 2, 3) if e % 2 else (0, 0, 0),
                            restitution=rng.uniform(0, 1), friction=rng.uniform(0, 1), margin=rng.uniform(0, 0.05)))
    mixed.append(V.pose(3, (50.0, 50.0, 50.0)))  # touches nothing
    sets["mixed16"] = ([_cell(), rough, ball, land], mixed)
    return sets


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000, 4097])
def test_the_call_gives_the_restatements_bits(ws, n):
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(n)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    pos[0] = (1.0, 0.25, 1.0)                                       # on two far faces of the cell: in the domain, f == 1
    if n > 3:
        pos[1] = (np.nextafter(F32(1.0), F32(2.0)), 0.25, 1.0)      # one step beyond the far face: outside
        pos[2] = (0.0, 0.0, 0.0)                                    # exactly at a node
        pos[3] = (0.5, 0.375, 0.5)                                  # s == margin exactly: not a contact
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    vel[::5, 0] = F32(-0.0)
    vel[3::7] = F32(-0.0)
    w = ws.FluidWorker(pos, params)
    rec = w.read_vec("particles")
    for name, (volumes, poses) in _volume_sets().items():
        V.upload(w, volumes)
        _load(w, rec, vel=vel)
        got = w.collide_volumes(V.to_ws(ws, poses))
        state = w.read_vec("particles")
        want = V.collide(pos, vel, volumes, poses, *_ext(params))
        _same_reaction(got, want, name)
        assert same_bits(_xyz(state, "position"), want["pos"]), name
        assert same_bits(_xyz(state, "velocity"), want["vel"]), name
        assert same_bits(_xyz(state, "predicted_position"), want["pred"]), name
        assert same_bits(w.read_positions(), want["pos"]) and w.steps_done() == 0, name
        if name in ("cell", "mixed16"):
            assert want["hit"][0][0] and (n <= 3 or list(want["hit"][0][1:4]) == [False, True, False]), name
        if name == "cell":
            assert want["pos"][0][1] == F32(0.375) and (n <= 3 or same_bits(want["pos"][[1, 3]], pos[[1, 3]])), name
        if name == "mixed16":
            assert got[0][-1] == 0 and len(got[0]) == 16 and not got[1][-1].any() and not got[2][-1].any()
            assert n < 1000 or (got[0][:15] > 0).all(), got[0]
        if name == "zero-rot":
            assert got[0][0] == n and not got[1][0].any() and same_bits(want["pos"], pos) and same_bits(want["vel"], vel)
        if name == "flat" and n >= 63:
            moved = want["hit"][0]
            assert moved.any() and np.all(want["pos"][moved, 0] < pos[moved, 0]) and same_bits(want["pos"][moved, 1:], pos[moved, 1:])
        if n >= 63 and name in ("cell", "rough", "sphere", "terrain"):  # most particles are untouched, some with -0 components: kept
            out = ~want["touched"]
            assert 0 < out.sum() < n, name
            v_out = _xyz(state, "velocity")[out]
            assert np.any(np.signbit(v_out) & (v_out == 0)), name
            assert n < 1000 or np.abs(got[1][0]).max() > 0 and np.abs(got[2][0]).max() > 0, name
        # without the reaction: the same state
        _load(w, rec, vel=vel)
        assert w.collide_volumes(V.to_ws(ws, poses), reaction=False) is None
        state = w.read_vec("particles")
        assert same_bits(_xyz(state, "position"), want["pos"]) and same_bits(_xyz(state, "velocity"), want["vel"]), name
        assert same_bits(_xyz(state, "predicted_position"), want["pred"]), name
    w.close()


# ---- 2. the step picks it up exactly as a host edit ---------------------------------------------------------------------------
def _moving_volumes(reach):
    return [sphere_volume(17, 0.2 * reach, 0.4 * reach), terrain_volume(0.4 * reach)]


def _moving(t, centre, reach):
    """A ball that circles and spins and a terrain patch that rises with the step number t."""
    c = np.asarray(centre, np.float64)
    s = 0.3 * reach
    return [V.pose(0, c + s * np.array([np.cos(0.3 * t), 0.1, np.sin(0.3 * t)]), rot=S.rotation((0.2, 1.0, 0.1), 0.15 * t),
                   velocity=(-0.09 * s * np.sin(0.3 * t) * 50, 0.0, 0.09 * s * np.cos(0.3 * t) * 50), angular_velocity=(1.0, 5.0, 0.5),
                   restitution=0.5, friction=0.1, margin=0.01 * reach),
            V.pose(1, c + s * np.array([-0.3, -0.6 + 0.02 * t, 0.2]), rot=S.rotation((1.0, 0.0, 0.0), 0.3),
                   velocity=(0.0, 0.02 * s * 50, 0.0), restitution=0.2, friction=0.5, margin=0.005 * reach)]


@pytest.mark.parametrize("which", ["merged-4096", "regrid-31646"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_step_picks_the_call_up_exactly_as_a_host_edit(ws, which, ieee):
    pos, params, regrid, centre, reach = _scene(ws, which)
    a = ws.FluidWorker(pos, params, ieee_division=ieee)
    b = ws.FluidWorker(pos, params, ieee_division=ieee)
    volumes = _moving_volumes(reach)
    V.upload(a, volumes)
    seen = 0
    for t in range(20):
        if regrid is not None and t == 10:
            a.set_params(regrid)  # (the volumes survive the re-grid)
            b.set_params(regrid)
        poses = _moving(t, centre, reach)
        got = a.collide_volumes(V.to_ws(ws, poses))
        want = _host_collide(b, volumes, poses, params)
        _same_reaction(got, want, t)
        seen += int(got[0].sum())
        a.run(1)
        b.run(1)
        assert same_bits(a.read_positions(), b.read_positions()), t
        assert same_bits(a.read_velocities(), b.read_velocities()), t
    assert seen > 20 * 20 and a.steps_done() == 20, seen
    a.close()
    b.close()


# ---- 3. nothing touched changes nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_a_call_that_touches_nothing_changes_nothing(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    # the whole container lies in the domain of a volume that is positive everywhere (the padding a host gives its
    # volumes); a second pose of it is far away
    far = V.volume(np.full((3, 3, 3), 5.0), (-20.0, -20.0, -20.0), (20.0, 20.0, 20.0))
    outside = [ws.fluid.volume_pose(0, margin=0.5, restitution=1.0), ws.fluid.volume_pose(0, (100.0, 100.0, 100.0), margin=0.25)]
    plain = ws.FluidWorker(pos, params, graph=graph)
    called = ws.FluidWorker(pos, params, graph=graph)
    V.upload(called, [far])
    replayed = []
    for t in range(50):
        got = called.collide_volumes(outside, reaction=(t % 2 == 0))
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
FLAT_VOLUMES = [sphere_volume(17, 1.5, 2.0), terrain_volume(4.0)]


def _flat_poses(dx):
    """Two volumes in the plane of the C1 container (16 x 18 x 0.2), shifted by dx."""
    return [V.pose(0, (1.0 + dx, 0.0, 0.0), restitution=0.5, friction=0.1, velocity=(1.0, 0.0, 0.0), margin=0.05),
            V.pose(1, (-3.0 + dx, -4.0, 0.0), rot=S.rotation((0.0, 0.0, 1.0), 0.5), angular_velocity=(0.0, 0.0, 2.0), restitution=0.2,
                   friction=0.5, margin=0.02)]


def test_the_views_of_the_last_step_stay_and_the_readers_see_the_new_positions(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    V.upload(w, FLAT_VOLUMES)
    w.run(12)
    before = w.read_vec("particles")
    poses = _flat_poses(0.0)
    got = w.collide_volumes(V.to_ws(ws, poses))
    after = w.read_vec("particles")
    want = V.collide(_xyz(before, "position"), _xyz(before, "velocity"), FLAT_VOLUMES, poses, *_ext(params))
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
    w.collide_volumes(V.to_ws(ws, _flat_poses(2.5)), reaction=False)
    w.read_positions_end()
    assert same_bits(buf, want["pos"]) and not same_bits(w.read_positions(), want["pos"])
    w.close()
    other.close()


# ---- 5. water stays above a tilted plane ------------------------------------------------------------------------------------------
def test_water_stays_above_a_tilted_plane_terrain(ws):
    """The C1 cloud over a ramp that fills the lower left corner of the container (0.6 x + 0.8 y = -9: from (-8, -5.25) to
    (-3, -9)): the push-out goes up and to the right, away from the two walls the ramp meets, so the container rule never
    cuts one short.  Trilinear interpolation is exact for a plane: after a call no particle in the domain lies deeper than
    the restatement's counted-rounding bound -- E_p at the position it was pushed from if the call touched it, E_s if the
    call decided not to -- plus the rounding of the nodes themselves (tests/test_volumes_reference.py)."""
    pos, params = ws.workloads.make_workload("c1", "cloud")
    nrm, c = np.array([0.6, 0.8, 0.0]), -9.0
    ramp = plane_volume(nrm, c, dims=(5, 5, 3), origin=(-8.5, -9.5, -2.0), spacing=(4.25, 4.75, 2.0))
    ps = V.pose(0, restitution=0.2, friction=0.1, margin=0.05)
    arr = V.to_ws(ws, [ps])
    w = ws.FluidWorker(pos, params)
    V.upload(w, [ramp])
    contacts = 0
    for t in range(199):
        w.run(1)
        contacts += int(w.collide_volumes(arr)[0][0])
    w.run(1)
    x0, v0 = w.read_positions(), w.read_velocities()
    contacts += int(w.collide_volumes(arr)[0][0])
    x = w.read_positions()
    want = V.collide(x0, v0, [ramp], [ps], *_ext(params))
    assert contacts > 0 and want["hit"][0].any() and same_bits(x, want["pos"]), contacts
    E_g, E_s, E_n, E_p, _, _, _ = bounds(x0, v0, ps, ramp, 2.0)
    node_s, node_g = node_rounding(ramp)
    s0 = x0.astype(np.float64) @ nrm - c
    _, inside = V.grid_coordinate(x, ps, ramp)
    assert inside.all()
    tol = np.where(want["hit"][0], E_p + np.abs(float(ps["margin"]) - s0) * (node_g + 8 * 2.0 ** -24), E_s) + node_s
    short = float(ps["margin"]) - (x.astype(np.float64) @ nrm - c)
    print("contacts %d (%d in the last call), worst shortfall %.3e, bound there %.3e" %
          (contacts, want["hit"][0].sum(), short.max(), tol[np.argmax(short)]))
    assert np.all(short <= tol), float((short / tol).max())
    w.close()


# ---- 6. slabs ---------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 10
SLAB_VOLUMES = [sphere_volume(17, 2.0, 3.0), terrain_volume(3.0)]


def _slab_poses(t):
    # the cuts of 2 and 3 slabs of the 16-wide container lie at x = 0 and near +-2.7: every pose straddles one
    return [V.pose(0, (0.3 * np.cos(t), -2.5, 0.0), restitution=0.5, friction=0.2, velocity=(1.0, 0.0, 0.0), margin=0.05),
            V.pose(1, (-2.5, -3.0, 0.5), rot=S.rotation((0.0, 1.0, 0.2), 0.4), angular_velocity=(0.0, 1.0, 0.0), margin=0.02, friction=0.5),
            V.pose(0, (2.7, 2.0, 0.0), rot=QUARTER, restitution=1.0, margin=0.0)]


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_same_bits_and_the_same_global_sums_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    w = ws.FluidWorker(pos, params)
    V.upload(w, SLAB_VOLUMES)
    want = []
    for t in range(SLAB_STEPS):
        out = w.collide_volumes(V.to_ws(ws, _slab_poses(t))) if t % 2 == 0 else None
        w.run(1)
        if t in (2, SLAB_STEPS - 1):
            want.append((w.read_positions(), w.read_velocities()))
        if out is not None:
            want.append(list(out))
    assert min(int(c[0].min()) for c in want if isinstance(c, list)) > 20
    assert all(np.abs(c[1]).max() > 0 and np.abs(c[2]).max() > 0 for c in want if isinstance(c, list))
    w.close()
    # an upload frees and allocates device memory, which waits for the whole device: with every rank a thread of this
    # process on one GPU, a rank uploads only while no peer is inside a collective (the barrier), as hosts on their own
    # devices never have to
    together = threading.Barrier(world)

    def alone(s, r, who, slot, vol):
        """Rank `who` replaces its slot (vol = None: releases it) while the others wait."""
        together.wait(120)
        if r == who:
            if vol is None:
                s.upload_volume(slot, None, None, None)
            else:
                s.upload_volume(slot, [float(x) for x in vol["origin"]], [float(x) for x in vol["spacing"]], vol["sdf"])
        together.wait(120)

    def refused(s, r, t, poses, k=3):
        arr = (ws.fluid.WsVolumePose * 3)(*poses)
        n, imp = np.full(3, 7, np.uint32), np.full((3, 3), 7.0)
        assert s._L.ws_collide_volumes(s._h, C.byref(arr), k, n.ctypes.data, imp.ctypes.data, None) == 1, (r, t)
        assert np.all(n == 7) and np.all(imp == 7.0)

    def program(s, r):
        out = []
        together.wait(120)
        V.upload(s, SLAB_VOLUMES)  # LOCAL: every rank its own copy
        together.wait(120)
        for t in range(SLAB_STEPS):
            good = V.to_ws(ws, _slab_poses(t))
            got = None
            if t % 2 == 0:
                got = s.collide_volumes(good, reaction=(r != 1))  # rank 1 passes every output NULL and still applies
            elif t == 3:
                # one rank holds a different array in the slot (one node differs): every rank refuses, nothing changes
                other = dict(SLAB_VOLUMES[1], sdf=SLAB_VOLUMES[1]["sdf"].copy())
                other["sdf"][1, 1, 4] += F32(0.125)
                alone(s, r, 0, 1, other)
                refused(s, r, t, good)
                alone(s, r, 0, 1, SLAB_VOLUMES[1])
            elif t == 5:
                # one rank's slot is empty: every rank refuses, nothing changes
                alone(s, r, world - 1, 0, None)
                refused(s, r, t, good)
                alone(s, r, world - 1, 0, SLAB_VOLUMES[0])
            elif t == 7:
                # one rank passes a different, valid pose: every rank refuses, nothing changes
                if r == world - 1:
                    good[0].restitution = 0.75
                refused(s, r, t, good)
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


# ---- 7. three edits between the same two steps ------------------------------------------------------------------------------------
STATE = ("position", "velocity", "predicted_position")


def test_three_edits_between_two_steps_are_three_host_edits(ws):
    n = BLOCK + 1  # two workgroups, the second with one lane
    params = ws.make_params(container_size=(4.0, 4.0, 4.0))
    rng = np.random.default_rng(n)
    pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    vel = rng.normal(0.0, 2.0, (n, 3)).astype(F32)
    forces, solids = _emitter_sets()["mixed16"], _solid_sets()["mixed16"]
    volumes, poses = _volume_sets()["mixed16"]
    a, b = ws.FluidWorker(pos, params), ws.FluidWorker(pos, params)
    V.upload(a, volumes)
    for w in (a, b):
        _load(w, w.read_vec("particles"), vel=vel)
    dt = F32(1.0 / 60.0)
    # the host's route on b, one read and one write per edit ...
    rec = b.read_vec("particles")
    seen = F.accelerate(_xyz(rec, "position"), _xyz(rec, "velocity"), forces)[1]
    counts = _host_apply(b, forces, dt)
    by_volumes = _host_collide(b, volumes, poses, params)
    by_solids = _host_collide_solids(b, solids, params)
    want = b.read_vec("particles")
    assert (seen & by_volumes["touched"] & by_solids["touched"]).any()  # some particle is changed by all three
    # ... and the three calls on a
    got = a.apply_forces(F.to_ws(ws, forces), dt)
    assert got.dtype == np.uint32 and np.array_equal(got, counts)
    _same_reaction(a.collide_volumes(V.to_ws(ws, poses)), by_volumes, "volumes")
    _same_reaction(a.collide_solids(S.to_ws(ws, solids)), by_solids, "solids")
    got = a.read_vec("particles")
    for f in STATE:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    a.run(1)
    b.run(1)
    got, want = a.read_vec("particles"), b.read_vec("particles")
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert a.steps_done() == 1
    a.close()
    b.close()


# ---- 8. lifetimes and refusals ----------------------------------------------------------------------------------------------------
def _raw_upload(w, slot, origin, spacing, dims, sdf):
    three = lambda x, T: None if x is None else (T * 3)(*x)  # noqa: E731
    return w._L.ws_volume_upload(w._h, slot, three(origin, C.c_float), three(spacing, C.c_float), three(dims, C.c_uint32),
                                 None if sdf is None else sdf.ctypes.data)


def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params)
    fresh = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    ball = sphere_volume(9, 1.5, 2.0)
    V.upload(w, [ball])
    at_the_floor = V.pose(0, (0.0, -8.0, 0.0), margin=0.05, restitution=0.5)  # where the water is after the steps below
    steps = 0

    def stepped_on(what, status):
        nonlocal steps
        assert status == 1, what
        w.run(2)  # ... followed by two good steps
        steps += 2

    # ---- uploads into the slot that holds the ball
    good = dict(origin=(-2.0, -2.0, -2.0), spacing=(0.5, 0.5, 0.5), dims=(9, 9, 9), sdf=np.ones((9, 9, 9), F32))
    small = np.ones(8, F32)
    uploads = [("slot 4", dict(slot=4)), ("NULL origin", dict(origin=None)), ("NULL spacing", dict(spacing=None)),
               ("NULL dims", dict(dims=None)), ("dims 1", dict(dims=(9, 1, 9))), ("dims 0", dict(dims=(0, 9, 9))),
               ("dims 1025", dict(dims=(9, 9, 1025), sdf=small)), ("2^26 + nodes", dict(dims=(1024, 1024, 65), sdf=small)),
               ("extent", dict(dims=(1024, 2, 2), spacing=(1e13, 0.5, 0.5), sdf=small))]
    for val in (0.0, -0.5, np.nan, np.inf, 2e15):
        uploads.append(("spacing %r" % val, dict(spacing=(0.5, val, 0.5))))
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        uploads.append(("origin %r" % val, dict(origin=(-2.0, -2.0, val))))
        bad = np.ones((9, 9, 9), F32)
        bad[8, 8, 8] = val  # the last value of the array
        uploads.append(("sdf %r" % val, dict(sdf=bad)))
    for what, kw in uploads:
        args = dict(good, slot=0)
        args.update(kw)
        stepped_on(what, _raw_upload(w, args["slot"], args["origin"], args["spacing"], args["dims"], args["sdf"]))

    # ---- collides
    def call(edit=None, k=1, null=False, at=0):
        v = [ws.fluid.volume_pose(0, (1.0, 0.0, 0.0), restitution=0.5, friction=0.5, margin=0.1, velocity=(1.0, 0.0, 0.0),
                                  angular_velocity=(0.0, 1.0, 0.0)) for _ in range(max(k, 2))]
        if edit:
            edit(v[at])
        arr = (ws.fluid.WsVolumePose * len(v))(*v)
        n, imp, ang = np.full(17, 7, np.uint32), np.full((17, 3), 7.0), np.full((17, 3), 7.0)
        st = L.ws_collide_volumes(h, None if null else C.byref(arr), k, n.ctypes.data, imp.ctypes.data, ang.ctypes.data)
        assert st != 0 and np.all(n == 7) and np.all(imp == 7.0) and np.all(ang == 7.0) or st == 0
        return st

    def set_(name, value, index=None):
        def edit(s):
            if index is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[index] = value
        return edit

    cases = [("NULL v", dict(null=True)), ("k 0", dict(k=0)), ("k 17", dict(k=17)), ("slot 4", dict(edit=set_("slot", 4))),
             ("an empty slot", dict(edit=set_("slot", 3))), ("flags 1", dict(edit=set_("flags", 1))),
             ("reserved 1", dict(edit=set_("reserved", 1))), ("second pose", dict(edit=set_("margin", -1.0), k=2, at=1)),
             ("margin < 0", dict(edit=set_("margin", -0.01)))]
    for name in ("restitution", "friction"):
        cases += [("%s %r" % (name, val), dict(edit=set_(name, val))) for val in (-0.01, 1.01, np.nan, np.inf)]
    for val in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        cases += [("centre %r" % val, dict(edit=set_("centre", val, 1))), ("rot %r" % val, dict(edit=set_("rot", val, 7))),
                  ("velocity %r" % val, dict(edit=set_("velocity", val, 0))),
                  ("angular %r" % val, dict(edit=set_("angular_velocity", val, 2))), ("margin %r" % val, dict(edit=set_("margin", val)))]
    for what, kw in cases:
        stepped_on(what, call(**kw))
    fresh.run(steps)
    assert np.array_equal(w.read_vec("particles").view(np.uint8), fresh.read_vec("particles").view(np.uint8))
    # every refused upload left the ball where it was: the call gives what the restatement gives with it
    rec = w.read_vec("particles")
    want = V.collide(_xyz(rec, "position"), _xyz(rec, "velocity"), [ball], [at_the_floor], *_ext(params))
    _same_reaction(w.collide_volumes(V.to_ws(ws, [at_the_floor])), want, "the old volume")
    assert want["contacts"][0] > 0 and same_bits(w.read_positions(), want["pos"])
    # allowed: the largest magnitudes, the limits of the ranges, sixteen poses, the smallest and a 1024-long volume
    assert call(edit=set_("centre", 1e15, 0)) == 0 and call(edit=set_("restitution", 1.0)) == 0
    assert call(edit=set_("friction", 0.0)) == 0 and call(edit=set_("margin", 0.0)) == 0 and call(k=16) == 0
    assert _raw_upload(w, 3, (1e15, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), np.ones(8, F32)) == 0
    assert _raw_upload(w, 2, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1024, 2, 2), np.ones(4096, F32)) == 0
    assert call(edit=set_("slot", 3)) == 0 and call(edit=set_("slot", 2)) == 0
    w.run(2)
    w.close()
    fresh.close()


def test_a_volume_is_replaced_released_and_survives_reset_and_regrid(ws):
    pos, params, regrid, centre, reach = _scene(ws, "regrid-31646")
    w = ws.FluidWorker(pos, params)
    ball, land = sphere_volume(17, 0.6, 1.0), terrain_volume(1.5)
    arr = None

    def check(vol, what, shift):
        """The call against the restatement, the pose `shift` further along x each time: into water no earlier check moved."""
        nonlocal arr
        ps = V.pose(0, (-1.5 + shift, -0.5, 0.1), rot=S.rotation((0.2, 1.0, 0.1), 0.4), restitution=0.5, friction=0.1, margin=0.02)
        arr = V.to_ws(ws, [ps])
        rec = w.read_vec("particles")
        want = V.collide(_xyz(rec, "position"), _xyz(rec, "velocity"), [vol], [ps], *_ext(params))
        _same_reaction(w.collide_volumes(arr), want, what)
        assert want["contacts"][0] > 20 and same_bits(w.read_positions(), want["pos"]), what

    V.upload(w, [ball])
    w.run(2)
    check(ball, "uploaded", 0.0)
    V.upload(w, [land])  # other dims in the same slot: replaced
    check(land, "replaced", 0.75)
    w.reset(pos)
    check(land, "after ws_reset", 1.5)
    w.set_params(regrid)
    w.run(2)
    check(land, "after a re-grid", 2.25)
    w.write_slice("particles", w.read_vec("particles"))
    check(land, "after ws_write_particles", 3.0)
    w.upload_volume(0, None, None, None)  # released: the slot is empty
    with pytest.raises(ws.WsError) as e:
        w.collide_volumes(arr)
    assert e.value.status == 1 and "holds no volume" in str(e.value)
    w.upload_volume(0, None, None, None)  # releasing an empty slot is not an error
    w.run(2)
    w.close()


def test_a_reference_order_handle_is_unsupported(ws, refcheck):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, reference_order=True, library=refcheck)
    ball = sphere_volume(9)
    with pytest.raises(ws.WsError) as e:
        V.upload(w, [ball])
    assert e.value.status == 6
    with pytest.raises(ws.WsError) as e:
        w.collide_volumes(ws.fluid.volume_pose(0))
    assert e.value.status == 6
    w.run(2)
    w.close()


def test_a_dead_handle_refuses_both_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    ball = sphere_volume(9, 4.0, 6.0)
    V.upload(w, [ball])
    p = ws.fluid.volume_pose(0)
    assert w.collide_volumes(p)[0][0] > 0
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    with pytest.raises(ws.WsError) as e:
        w.collide_volumes(p)
    assert e.value.status == 4 and "unusable" in str(e.value)
    with pytest.raises(ws.WsError) as e:
        V.upload(w, [ball])
    assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()


def test_destroy_gives_the_volumes_memory_back(ws):
    """Four resident 64^3 volumes (1 MiB each) per handle: less than one of them may be missing after eight cycles."""
    pos, params = ws.workloads.make_workload("c1", "cloud")
    big = sphere_volume(64, 3.0, 4.0)
    poses = [ws.fluid.volume_pose(s, (float(s), 0.0, 0.0), margin=0.05) for s in range(4)]

    def cycle():
        w = ws.FluidWorker(pos, params)
        V.upload(w, [big] * 4)
        w.run(1)
        assert w.collide_volumes(poses)[0].min() > 0
        V.upload(w, [big])  # replaced: the old array is freed here, the new one by ws_destroy
        w.upload_volume(1, None, None, None)
        w.sync()
        w.close()

    assert _leak_over_eight_cycles(cycle) < big["sdf"].nbytes
