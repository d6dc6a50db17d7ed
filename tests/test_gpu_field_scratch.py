"""Every derived-field call kind against every other on ONE handle: the calls share a handle's scratch (grow-only
buffers, buffers that carry another call's results, per-cell tables rebuilt after a re-grid), so a call must give the
bits it gives on a fresh handle whatever ran before it and at whatever size.

Scene: tests/test_gpu_whitewater.py's dam break without the hand-placed extras -- 16^3 lattice particles (spacing 0.12) in
the lowest corner of a (6, 4, 3) container at h = 0.25, stepped 20 times, the state read back once.  The expected value of
a call is the same call on a fresh handle loaded with that state, computed once per (arithmetic, parameters, call, size).
Everything is compared bit for bit (same_bits; the step's uint8 classes byte for byte): no tolerances."""
import numpy as np
import pytest

from test_gpu_aniso_surface import _slab_run, padded, same_bits
from test_gpu_whitewater import load_state

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS = 20
SIZES = (65, 4097, 1)  # one per pass: grow, grow again, reuse while larger than needed
KINDS = ("density_grid", "density_points", "aniso_grid", "aniso_points", "anisotropy", "surface", "aniso_surface", "cast_rays",
         "cast_camera", "velocity_grid", "velocity_points", "advect_points", "read_whitewater", "emit_whitewater",
         "step_whitewater", "read_velocities", "read_cohesion", "body_forces")
ORDER = tuple(KINDS[i] for i in np.random.default_rng(16).permutation(len(KINDS)))
# the passes of the mixed run: the shuffled list, the same list reversed, the shuffled list again
PASSES = tuple((kind, size) for order, size in zip((ORDER, ORDER[::-1], ORDER), SIZES) for kind in order)


def flat(out):
    """A call's results as a list of arrays."""
    if out is None:
        return None
    if isinstance(out, dict):
        return [np.asarray(out[k]) for k in sorted(out)]
    if isinstance(out, tuple):
        return [np.asarray(a) for a in out if a is not None] or None  # (a contributing slab rank gets a tuple of None)
    return [out]


def same(got, want):
    return len(got) == len(want) and all(
        same_bits(a, b) if a.dtype.itemsize == 4 else a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        for a, b in zip(got, want))


class _Scene:
    def __init__(self, ws):
        self.ws = ws
        self.params = ws.make_params(container_size=(6.0, 4.0, 3.0))
        self.regrid = ws.make_params(container_size=(6.0, 4.0, 3.0), smoothing_radius=F32(0.2))
        lo = np.asarray(self.params.ext_min[:3], np.float64)
        block = ws.cube_fluid(16, 16, 16, 0.06).astype(np.float64)
        self.start = (block + (lo + 0.05 - block.min(0))).astype(F32)
        w = ws.FluidWorker(self.start, self.params)
        w.run(STEPS)
        self.pos, self.vel = w.read_positions(), w.read_velocities()
        w.close()
        self.n = len(self.pos)
        assert self.n == 4096 and float(self.params.smoothing_radius) == 0.25
        for a in (self.start, self.pos, self.vel):
            a.setflags(write=False)
        self.inputs = {m: self._inputs(m) for m in SIZES}
        self.want = {}

    def _inputs(self, m):
        """The m query points, rays and diffuse particles of a pass: near the fluid, in the air and outside the box."""
        rng = np.random.default_rng(m)
        hi = np.asarray(self.params.ext_max[:3], np.float64)
        pts = self.pos[rng.choice(self.n, m)] + rng.normal(0.0, 0.1, (m, 3))
        pts[::5] += rng.normal(0.0, 2.0, pts[::5].shape)
        eye = hi + 1.0 + rng.random((m, 3))
        return dict(pts=pts.astype(F32), eye=eye.astype(F32), dir=(pts - eye).astype(F32),
                    vel=rng.normal(0.0, 2.0, (m, 3)).astype(F32), life=rng.uniform(-0.01, 0.06, m).astype(F32))

    def fresh(self, ieee, params):
        w = self.ws.FluidWorker(self.pos, params, ieee_division=ieee)
        load_state(w, self.pos, self.vel)
        return w

    def call(self, x, params, kind, m, **kw):
        """One call of `kind` at size m on x (a FluidWorker, or a SlabWorker with want=...), its results as arrays."""
        ws, q = self.ws, self.inputs[m]
        h = F32(params.smoothing_radius)
        rho0 = F32(params.target_density)
        fine = padded(params, h / F32(2), h)  # one node per cell and more: the brick path
        grid = padded(params, {65: h, 4097: h / F32(2), 1: h * F32(0.75)}[m], h)
        a = ws.fluid.aniso_params()
        march = ws.fluid.ray_params(0.0, float(h / F32(2)), 160, 6, float(rho0 / F32(2)))
        if kind == "density_grid":
            return flat(x.sample_density_grid(*fine, gradient=True, **kw))
        if kind == "density_points":
            return flat(x.sample_density_points(q["pts"], gradient=True, **kw))
        if kind == "aniso_grid":
            return flat(x.sample_aniso_grid(*grid, gradient=True, aniso=a, **kw))
        if kind == "aniso_points":
            return flat(x.sample_aniso_points(q["pts"], gradient=True, aniso=a, **kw))
        if kind == "anisotropy":
            return flat(x.anisotropy(a, **kw))
        if kind == "surface":
            return flat(x.extract_surface(*grid, rho0 / F32(2), **kw))
        if kind == "aniso_surface":
            return flat(x.extract_aniso_surface(*grid, rho0 / F32(2), aniso=a, **kw))
        if kind == "cast_rays":
            return flat(x.cast_rays(march, q["eye"], q["dir"], **kw))
        if kind == "cast_camera":
            centre = (np.asarray(params.ext_min[:3], F32) + np.asarray(params.ext_max[:3], F32)) / F32(2)
            eye = np.asarray(params.ext_max[:3], F32) + F32(2)
            cam = ws.fluid.camera(eye, centre - eye, (0.5, 0.0, -0.5), (0.0, 0.5, 0.0))
            return flat(x.cast_camera(march, cam, (8, 8), aniso=a, **kw))
        if kind == "velocity_grid":
            return flat(x.sample_velocity_grid(*grid, density=True, **kw))
        if kind == "velocity_points":
            return flat(x.sample_velocity_points(q["pts"], **kw))
        if kind == "advect_points":
            return flat(x.advect_points(ws.fluid.advect_params(0.05, 2), q["pts"], field=True, **kw))
        if kind == "read_whitewater":
            return flat(x.read_whitewater(**kw))
        if kind == "emit_whitewater":
            e = ws.fluid.whitewater_emit_params(tau_trapped=(0.0, 2.0), tau_crest=(0.0, 2.0), tau_energy=(0.0, 2.0), seed=3)
            out = x.emit_whitewater(e, cap=8 * self.n, **kw)
            if out is None:
                return None
            assert 0 < out.pop("count") == len(out["xyz"]) < 8 * self.n
            return flat(out)
        if kind == "step_whitewater":
            return flat(x.step_whitewater(ws.fluid.whitewater_step_params(), q["pts"], q["vel"], q["life"], **kw))
        if kind == "read_velocities":
            return flat(x.read_velocities(**kw))
        if kind == "read_cohesion":
            return flat(x.read_cohesion(ws.fluid.cohesion_params(), F32(1.0 / 60.0), **kw))
        assert kind == "body_forces"
        # the m samples as three bodies, each about the mean of its samples (an empty body about the origin)
        start = np.array([0, m // 3, 2 * m // 3, m], np.uint32)
        centres = np.array([q["pts"][a:b].mean(0) if b > a else np.zeros(3) for a, b in zip(start[:-1], start[1:])], F32)
        return flat(x.body_forces(ws.fluid.body_params(), q["pts"], q["vel"], F32(0.001) + np.abs(q["life"]), start, centres,
                                  samples=True, **kw))

    def expected(self, ieee, regridded, kind, m):
        key = (ieee, regridded, kind, m)
        if key not in self.want:
            params = self.regrid if regridded else self.params
            w = self.fresh(ieee, params)
            self.want[key] = self.call(w, params, kind, m)
            w.close()
            for a in self.want[key]:
                a.setflags(write=False)
        return self.want[key]


@pytest.fixture(scope="module")
def scene(ws):
    return _Scene(ws)


def test_the_scene_exercises_every_call(ws, scene):
    """What the mixed runs rely on: meshes, hits and misses, spawns, a moving fluid."""
    assert len(set(KINDS)) == len(KINDS) == 18 and set(ORDER) == set(KINDS) and ORDER != KINDS
    assert np.abs(scene.pos - scene.start).max() > 0.1 and scene.vel.any()
    for kind in ("surface", "aniso_surface"):
        xyz, nrm, tri = scene.expected(False, False, kind, 4097)
        assert len(xyz) > 0 and len(tri) > 0 and nrm.shape == xyz.shape
    t, n = scene.expected(False, False, "cast_rays", 4097)
    assert np.isfinite(t).any() and np.isinf(t).any()
    assert np.isfinite(scene.expected(False, False, "cast_camera", 65)[0]).any()
    rho, grad = scene.expected(False, False, "density_grid", 65)
    assert rho.any() and grad.any()


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_mixed_calls_on_one_handle_give_a_fresh_handles_bits(ws, scene, ieee):
    w = scene.fresh(ieee, scene.params)
    for k, (kind, m) in enumerate(PASSES):
        assert same(scene.call(w, scene.params, kind, m), scene.expected(ieee, False, kind, m)), (k, kind, m)
    w.close()


def test_a_regrid_between_the_calls(ws, scene):
    """The first half of the list, ws_set_params to a smaller radius (another cell grid: the per-cell tables are
    rebuilt, the per-particle arrays and the grow-only buffers stay), the second half at the new parameters."""
    w = scene.fresh(False, scene.params)
    dims = w.grid_dims()
    half = len(ORDER) // 2
    for kind in ORDER[:half]:
        assert same(scene.call(w, scene.params, kind, 4097), scene.expected(False, False, kind, 4097)), kind
    w.set_params(scene.regrid)
    assert tuple(w.grid_dims()) != tuple(dims)
    for kind in ORDER[half:]:
        assert same(scene.call(w, scene.regrid, kind, 65), scene.expected(False, True, kind, 65)), kind
    w.close()


def test_two_slabs_give_the_single_handles_bits(ws, scene):
    """Two loopback slabs stepped from the scene's start: the same mixed passes, rank 1 only contributing to every second
    call.  Every wanted result is the single handle's."""
    def calls(s, r):
        return [scene.call(s, scene.params, kind, m, want=(r == 0 or k % 2 == 0)) for k, (kind, m) in enumerate(PASSES)]

    got = _slab_run(ws, scene.params, scene.start, 2, STEPS, calls)
    for r in range(2):
        for k, (kind, m) in enumerate(PASSES):
            if r == 1 and k % 2:
                assert got[r][k] is None, (k, kind)
            else:
                assert same(got[r][k], scene.expected(False, False, kind, m)), (r, k, kind, m)
