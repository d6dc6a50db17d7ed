"""The density field sampler (ws_sample_density_grid / ws_sample_density_points) on the GPU: against a float64 brute
force, tied to the step's own K4 density, grid == points bit for bit, no effect on the simulation, slabs, errors and
lifetime."""
import threading

import numpy as np
import pytest

from util import PARITY_REPORT

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


def _accept(h):
    """Largest f32 T with sqrtf(T) <= h (the library's d2_accept)."""
    h = np.float32(h)
    t = np.float32(h * h)
    while np.sqrt(t) > h:
        t = np.nextafter(t, np.float32(0))
    while np.sqrt(np.nextafter(t, np.float32(np.inf))) <= h:
        t = np.nextafter(t, np.float32(np.inf))
    return t


def _pairs(q, pos, h):
    """(query index, particle index) of every pair within one cell of each other (cells of edge h, float64 cell list),
    and the f32 acceptance test the library applies."""
    hq = np.float64(h)
    pc = np.floor(pos.astype(np.float64) / hq).astype(np.int64)
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
                e = np.searchsorted(sk, k, "right")
                cnt = e - b
                qi = np.repeat(np.arange(len(q)), cnt)
                off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                qi_all.append(qi)
                pj_all.append(order[np.repeat(b, cnt) + off])
    qi = np.concatenate(qi_all)
    pj = np.concatenate(pj_all)
    e = pos[pj] - q[qi]  # f32, as the kernel forms it
    d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
    ok = ~(d2 > _accept(h))
    qi, pj = qi[ok], pj[ok]
    s = np.lexsort((pj, qi))
    return qi[s], pj[s]


def brute_force(q, pos, params, ws):
    """float64 density and gradient at q, and f32 forward / reversed sums (the noise the tolerance is built from)."""
    k = ws.get_smoothing_kernel(params)
    h = np.float64(params.smoothing_radius)
    qi, pj = _pairs(q, pos, params.smoothing_radius)
    diff = q[qi].astype(np.float64) - pos[pj].astype(np.float64)
    d = np.sqrt((diff * diff).sum(1))
    w = (h - d) ** 2 * np.float64(k.pow2)
    slope = (d - h) * np.float64(k.pow2_der)
    g = np.where(d[:, None] > 0, diff * (slope / np.where(d > 0, d, 1.0))[:, None], 0.0)
    m = len(q)
    rho = np.bincount(qi, w, minlength=m)
    grad = np.stack([np.bincount(qi, g[:, c], minlength=m) for c in range(3)], 1)
    # f32 sums in the canonical direction and reversed, per query
    starts = np.searchsorted(qi, np.arange(m))
    has = np.bincount(qi, minlength=m) > 0
    terms = np.concatenate([w[:, None], g], 1).astype(np.float32)
    rev = np.empty_like(terms)
    cnt = np.bincount(qi, minlength=m)
    # reversed order inside each query's group
    idx = np.arange(len(qi))
    first = np.repeat(starts, cnt)
    last = first + np.repeat(cnt, cnt) - 1
    rev[:] = terms[first + last - idx]
    fw = np.zeros((m, 4), np.float32)
    rv = np.zeros((m, 4), np.float32)
    for i in np.flatnonzero(has):  # sequential f32 sums (np.add.reduce would sum pairwise)
        a, e = starts[i], starts[i] + cnt[i]
        fw[i] = np.cumsum(terms[a:e], axis=0, dtype=np.float32)[-1]
        rv[i] = np.cumsum(rev[a:e], axis=0, dtype=np.float32)[-1]
    # noise unit: f32 summation noise of these terms -- forward against reversed, and either against the float64 sum (a
    # long sum of same-signed terms drifts alike in both directions: dense piles sum ~2000 terms into 10^5)
    exact = np.concatenate([rho[:, None], grad], 1)
    noise = (np.maximum(np.abs(fw.astype(np.float64) - rv), np.maximum(np.abs(fw - exact), np.abs(rv - exact))).max(0)
             if m else np.zeros(4))
    return rho, grad, noise, cnt


def check_field(case, arithmetic, q, rho, grad, pos, params, ws):
    want_rho, want_grad, noise, cnt = brute_force(q, pos, params, ws)
    for field, got, want, nz in (("density", rho, want_rho, noise[0]), ("gradient", grad, want_grad, noise[1:].max())):
        got = got.astype(np.float64).reshape(want.shape)
        err = float(np.max(np.abs(got - want))) if got.size else 0.0
        tol = 4.0 * float(nz) + 4.0 * EPS32 * float(np.max(np.abs(want)) if want.size else 0.0)
        PARITY_REPORT.append({"case": case, "arithmetic": arithmetic, "field": field, "n": int(len(q)), "linf_error": err,
                              "noise_unit": float(nz), "tolerance": tol,
                              "error_over_tolerance": err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))})
        assert err <= tol, "%s %s: L-inf error %.3e > tolerance %.3e" % (case, field, err, tol)
    far = cnt == 0
    assert np.all(rho.reshape(-1)[far] == 0) and np.all(grad.reshape(-1, 3)[far] == 0), case
    return cnt  # contributing particles per query, of the brute force alone


def nodes(origin, spacing, dims):
    """The grid's nodes as the header specifies them, x fastest: fl(origin + fl(i * spacing))."""
    o = np.asarray(origin, np.float32)
    s = np.asarray(spacing, np.float32)
    ax = [o[a] + np.arange(dims[a], dtype=np.float32) * s[a] for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


def cover(params, dims, margin):
    mn = np.asarray(params.ext_min[:3], np.float32) - np.float32(margin)
    mx = np.asarray(params.ext_max[:3], np.float32) + np.float32(margin)
    spacing = ((mx - mn) / (np.asarray(dims, np.float32) - 1)).astype(np.float32)
    return mn, spacing


@pytest.mark.parametrize("dist", ["cloud", "lattice"])
@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_c1_grid_against_float64_brute_force(ws, dist, ieee):
    pos, params = ws.workloads.make_workload("c1", dist)
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    dims = (48, 27, 27)
    origin, spacing = cover(params, dims, 0.5)
    q = nodes(origin, spacing, dims)
    done = 0
    for steps in (0, 50, 400):
        w.run(steps - done)
        done = steps
        cur = w.read_positions()
        rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
        assert rho.shape == (27, 27, 48) and grad.shape == (27, 27, 48, 3)
        check_field("field c1 %s grid step %d" % (dist, steps), "ieee" if ieee else "hw", q, rho, grad, cur, params, ws)
    w.close()


def test_c3_settled_points_and_small_grid_against_float64_brute_force(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    w.run(400)
    cur = w.read_positions()
    rng = np.random.default_rng(5)
    mn = np.asarray(params.ext_min[:3], np.float32)
    mx = np.asarray(params.ext_max[:3], np.float32)
    q = (mn + rng.random((20000, 3)).astype(np.float32) * (mx - mn)).astype(np.float32)
    q[:10000] = cur[rng.choice(len(cur), 10000, replace=False)] + rng.normal(0, 0.05, (10000, 3)).astype(np.float32)
    rho, grad = w.sample_density_points(q, gradient=True)
    check_field("field c3 settled points", "hw", q, rho, grad, cur, params, ws)
    # the same kind of nodes embedded in a small grid around the fluid's densest point
    c = cur[np.argmax(rho[:10000])]
    dims = (24, 20, 16)
    spacing = np.full(3, np.float32(params.smoothing_radius) / np.float32(3), np.float32)
    origin = (c - spacing * np.asarray(dims, np.float32) / 2).astype(np.float32)
    rg, gg = w.sample_density_grid(origin, spacing, dims, gradient=True)
    check_field("field c3 settled grid", "hw", nodes(origin, spacing, dims), rg, gg, cur, params, ws)
    assert rg.max() > 0
    w.close()


def test_points_at_the_particles_match_the_first_steps_density(ws):
    # 4096 particles: hash_n is a power of two whose 27-stencil does not alias (K4 takes its non-ALIAS path)
    pos, params = ws.workloads.make_workload("c1", "cloud")
    for ieee in (False, True):
        w = ws.FluidWorker(pos, params, ieee_division=ieee)
        rho = w.sample_density_points(pos)
        w.run(1)
        k4 = w.read_vec("particles")["density"][:, 0]
        w.close()
        # before the first step pred == pos: K4 sums the same pairs in the same order (+ DENSITY_PADDING)
        assert np.array_equal(k4, (rho + np.float32(0.00001)).astype(np.float32)), ieee


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
@pytest.mark.parametrize("per_cell", [2.0, 0.6])
def test_grid_equals_points_bit_for_bit(ws, ieee, per_cell):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, ieee_division=ieee)
    w.run(60)
    h = np.float32(params.smoothing_radius)
    spacing = np.full(3, h / np.float32(per_cell), np.float32)
    mn = np.asarray(params.ext_min[:3], np.float32) - h
    mx = np.asarray(params.ext_max[:3], np.float32) + h
    dims = tuple(int(v) for v in np.minimum(np.ceil((mx - mn) / spacing) + 1, 160))
    rg, gg = w.sample_density_grid(mn, spacing, dims, gradient=True)
    rp, gp = w.sample_density_points(nodes(mn, spacing, dims), gradient=True)
    assert rg.max() > 0
    assert np.array_equal(rg.reshape(-1).view(np.uint32), rp.view(np.uint32))
    assert np.array_equal(gg.reshape(-1, 3).view(np.uint32), gp.view(np.uint32))
    # the density alone is the same as with the gradient
    assert np.array_equal(w.sample_density_grid(mn, spacing, dims).view(np.uint32), rg.view(np.uint32))
    w.close()


def _trajectory(ws, pos, params, steps, sample, graph=False, regrid_at=None, small=None):
    w = ws.FluidWorker(pos, params, graph=graph)
    dims = (32, 24, 8)
    origin, spacing = cover(params, dims, 0.2)
    for t in range(steps):
        if regrid_at is not None and t == regrid_at:
            w.set_params(small)
        w.run(1)
        if sample:
            w.sample_density_grid(origin, spacing, dims, gradient=(t % 2 == 0))
    out = w.read_vec("particles")
    stats = w.stats()
    w.close()
    return out, stats


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_sampling_every_step_leaves_the_trajectory_bitwise_unchanged(ws, graph):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _ = _trajectory(ws, pos, params, 200, False, graph)
    got, stats = _trajectory(ws, pos, params, 200, True, graph)
    if graph:
        assert stats["graph_steps"] > 0
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


def test_sampling_across_a_regrid_leaves_the_trajectory_bitwise_unchanged(ws):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    small = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.2))
    want, _ = _trajectory(ws, pos, params, 80, False, regrid_at=40, small=small)
    got, _ = _trajectory(ws, pos, params, 80, True, regrid_at=40, small=small)
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_sample_the_same_bits_as_a_single_handle(ws, world):
    params = ws.make_params(container_size=(16.0, 9.0, 9.0), gravity=(6.0, -9.8, 0.0, 0.0))
    pos = ws.workloads.uniform_cloud(65536, 1234, list(params.ext_min), list(params.ext_max))
    steps = 30
    dims = (40, 24, 24)
    origin, spacing = cover(params, dims, 0.3)
    q = nodes(origin, spacing, dims)[::7].copy()
    w = ws.FluidWorker(pos, params)
    w.run(steps)
    want_g = w.sample_density_grid(origin, spacing, dims, gradient=True)
    want_p = w.sample_density_points(q, gradient=True)
    w.close()
    owner = ws.slab.assign(params, pos, world)
    hub = ws.slab.LoopbackHub(world)
    got = [None] * world
    errors = []

    def body(r):
        try:
            sel = np.flatnonzero(owner == r).astype(np.uint32)
            s = ws.slab.SlabWorker(pos[sel], sel, pos.shape[0], params, r, world, hub.transport(r))
            s.run(steps)
            want = r != 1  # rank 1 only contributes
            g = s.sample_density_grid(origin, spacing, dims, gradient=True, want=want)
            p = s.sample_density_points(q, gradient=True, want=want)
            got[r] = (g, p)
            s.close()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not errors, errors
    for r in range(world):
        g, p = got[r]
        if r == 1:
            assert g == (None, None) and p == (None, None)
            continue
        for a, b in zip(g + p, want_g + want_p):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), r


def test_invalid_arguments_are_refused_and_the_handle_steps_on(ws):
    import ctypes as C

    pos, params = ws.workloads.make_workload("c1", "cloud")
    want, _ = _trajectory(ws, pos, params, 20, False)
    w = ws.FluidWorker(pos, params)
    L, h = w._L, w._h
    o = np.zeros(3, np.float32)
    s = np.full(3, 0.1, np.float32)
    d = np.full(3, 4, np.uint32)
    out = np.empty(4096 * 3, np.float32)

    def grid(o=o, s=s, d=d, rho=out, grad=None):
        return L.ws_sample_density_grid(h, o.ctypes.data, s.ctypes.data, d.ctypes.data,
                                        None if rho is None else rho.ctypes.data, None if grad is None else grad.ctypes.data)

    def bad(v, i, x):
        v = v.copy()
        v[i] = x
        return v

    assert grid() == 0
    assert grid(rho=None) == 1
    assert grid(d=bad(d, 1, 0)) == 1
    assert grid(o=bad(o, 2, np.nan)) == 1 and grid(o=bad(o, 0, np.inf)) == 1
    assert grid(s=bad(s, 0, 0.0)) == 1 and grid(s=bad(s, 1, -0.1)) == 1 and grid(s=bad(s, 2, np.inf)) == 1
    assert grid(d=np.array([2048, 2048, 1024], np.uint32)) == 1  # 2^32 nodes
    pts = np.zeros((4, 3), np.float32)
    assert L.ws_sample_density_points(h, pts.ctypes.data, 0, out.ctypes.data, None) == 1
    assert L.ws_sample_density_points(h, pts.ctypes.data, 4, None, None) == 1
    assert L.ws_sample_density_points(h, bad(pts, (1, 1), np.nan).ctypes.data, 4, out.ctypes.data, None) == 1
    assert L.ws_sample_density_points(h, pts.ctypes.data, 4, out.ctypes.data, None) == 0
    w.run(20)
    got = w.read_vec("particles")
    w.close()
    for f in want.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


def test_a_dead_handle_refuses_both_calls(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(3)
    w.sample_density_points(pos[:16])
    smaller = ws.make_params(container_size=ws.workloads.CONFIGS["c1"][1], smoothing_radius=np.float32(0.15))
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError):
        w.set_params(smaller)
    monkeypatch.delenv("WS_FAIL_REGRID")
    for call in (lambda: w.sample_density_points(pos[:16]), lambda: w.sample_density_grid((0, 0, 0), (0.1, 0.1, 0.1), (4, 4, 4))):
        with pytest.raises(ws.WsError) as e:
            call()
        assert e.value.status == 4 and "unusable" in str(e.value)
    w.close()


def test_repeated_sampling_then_destroy_leaks_nothing_visible(ws):
    pos, params = ws.workloads.make_workload("c3", "lattice")
    w = ws.FluidWorker(pos, params)
    dims = (256, 144, 144)
    origin = np.asarray(params.ext_min[:3], np.float32)
    spacing = np.full(3, np.float32(params.smoothing_radius), np.float32)
    for _ in range(3):
        rho, grad = w.sample_density_grid(origin, spacing, dims, gradient=True)
        w.run(2)
    assert rho.max() > 0
    w.close()
    w2 = ws.FluidWorker(pos, params)
    w2.run(2)
    assert w2.sample_density_points(pos[:64]).max() > 0
    w2.close()
