"""The brick kernel's chunk loop: bricks whose support holds more candidates than one staged chunk (512 for the density
field, 256 for the velocity field), so that the grid calls cross one and several chunk boundaries with a remainder.

Scene: a (4.5, 1.5, 1.5) container, nothing stepped.  Three clusters of particles written directly, each strictly inside one
sampler cell (a cube of edge 0.6 h about the cell's centre), the cells seven apart along x: 300, 700 and 1300 particles --
more than one velocity chunk and less than a density chunk; one density chunk and a remainder; two density chunks (five
velocity chunks) and a remainder.  Elsewhere there is nothing: most bricks are air.  Every particle has its own non-zero
velocity.  The grid has spacing h / 2 (the brick form), dims that are no multiples of 4, and covers the container.

The grid calls are compared with the points calls on the same nodes bit for bit, in both arithmetics, and on the IEEE
handle with the numpy restatements (tests/velocity_ref.py, tests/aniso_ref.py) at 512 nodes or fewer.  What makes the
comparison mean something -- the cell loads, a node that accepts more than 1024 candidates, a node in the air -- is
asserted from numpy alone."""
import numpy as np
import pytest

import aniso_ref as A
import velocity_ref as V
from test_gpu_aniso_surface import padded, same_bits
from test_gpu_whitewater import load_state

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = (300, 700, 1300)  # clusters A, B, C
FIRST_CELL, CELL_STEP = -8, 7  # floor(x / h) of the clusters' cells along x
NEAR, AIR = 120, 100  # restated nodes: the nearest to each cluster's centre, and nodes far from every particle


class _Scene:
    def __init__(self, ws):
        self.ws = ws
        self.params = ws.make_params(container_size=(4.5, 1.5, 1.5))
        h = F32(self.params.smoothing_radius)
        rng = np.random.default_rng(20)
        self.centres = np.array([[(FIRST_CELL + CELL_STEP * k + 0.5) * float(h), 0.5 * float(h), 0.5 * float(h)]
                                 for k in range(3)])
        self.pos = np.concatenate([c + rng.uniform(-0.3, 0.3, (m, 3)) * float(h)
                                   for c, m in zip(self.centres, COUNTS)]).astype(F32)
        n = len(self.pos)
        self.vel = (rng.uniform(0.25, 2.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F32)
        origin, spacing, dims = padded(self.params, h / F32(2), h)
        self.grid = (origin, spacing, tuple(d + 1 if d % 4 == 0 else d for d in dims))
        self.nodes = A.grid_nodes(*self.grid)
        # the restated nodes: around each cluster, and in the air
        d = np.stack([np.linalg.norm(self.nodes.astype(np.float64) - c, axis=1) for c in self.centres], 1)
        near = [np.argsort(d[:, k], kind="stable")[:NEAR] for k in range(3)]
        air = np.flatnonzero(d.min(1) > 3.0 * float(h))
        self.sel = np.unique(np.concatenate(near + [air[:: max(1, len(air) // AIR)][:AIR]]))
        for a in (self.pos, self.vel, self.nodes, self.sel):
            a.setflags(write=False)
        self.workers = {}
        self.restated = None

    def worker(self, ieee):
        if ieee not in self.workers:
            w = self.ws.FluidWorker(self.pos, self.params, ieee_division=ieee)
            load_state(w, self.pos, self.vel)
            self.workers[ieee] = w
        return self.workers[ieee]

    def restatement(self):
        """(u, rho of velocity_ref, rho of the density restatement, accepted candidates) at the selected nodes, once."""
        if self.restated is None:
            merged = self.worker(True).stats()["cells_merged"]
            q = self.nodes[self.sel]
            u, rho, _ = V.field32(self.params, self.pos, self.vel, q, merged)
            accepted = A.accepted_counts(self.params, self.pos, q, merged)
            self.restated = (u, rho, A.iso_field32(self.params, self.pos, q, merged), accepted)
        return self.restated

    def close(self):
        for w in self.workers.values():
            w.close()


@pytest.fixture(scope="module")
def scene(ws):
    s = _Scene(ws)
    yield s
    s.close()


def test_the_scene_crosses_the_chunk_boundaries(scene):
    """From numpy alone: the cell loads, the cells' distances, the velocities, the grid and the restated nodes."""
    grid = A.Grid(scene.params, scene.worker(True).stats()["cells_merged"])
    cells, load = np.unique(grid.cells(scene.pos), axis=0, return_counts=True)
    print("cells %s loads %s, grid dims %s, %d restated nodes" % (cells.tolist(), load.tolist(), scene.grid[2], len(scene.sel)))
    assert len(cells) == 3 and sorted(load) == sorted(COUNTS)
    a, b, c = sorted(int(v) for v in load)
    assert 257 <= a <= 511
    assert 513 <= b <= 1023 and b % 256
    assert c >= 1025 and c % 256
    for i in range(3):
        for j in range(i):
            assert np.abs(cells[i] - cells[j]).max() >= 6
    # strictly inside the cells: no particle within 0.1 h of a cell wall
    frac = scene.pos.astype(np.float64) / float(grid.h)
    assert np.all(np.abs(frac - np.round(frac)) > 0.1)
    assert (scene.vel != 0).all() and len(np.unique(scene.vel, axis=0)) == len(scene.vel)
    origin, spacing, dims = scene.grid
    assert all(d % 4 for d in dims) and np.all(spacing == grid.h / F32(2))
    assert np.all(scene.nodes.min(0) < scene.pos.min(0)) and np.all(scene.nodes.max(0) > scene.pos.max(0))
    _, rho, _, accepted = scene.restatement()
    assert len(scene.sel) <= 512
    assert accepted.max() >= 1025 and np.count_nonzero(accepted == 0) >= 32
    assert np.count_nonzero(rho == 0) >= 32 and np.count_nonzero(rho) >= 3 * NEAR // 2


@pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])
def test_the_grid_calls_give_the_points_calls_bits(scene, ieee):
    w = scene.worker(ieee)
    origin, spacing, dims = scene.grid
    nodes = dims[0] * dims[1] * dims[2]
    rho_g, grad_g = w.sample_density_grid(origin, spacing, dims, gradient=True)
    rho_p, grad_p = w.sample_density_points(scene.nodes, gradient=True)
    assert rho_p.any() and grad_p.any() and np.count_nonzero(rho_p == 0) > nodes // 2
    assert same_bits(rho_g.reshape(-1), rho_p) and same_bits(grad_g.reshape(-1, 3), grad_p)
    u_g, vrho_g = w.sample_velocity_grid(origin, spacing, dims, density=True)
    u_p, vrho_p = w.sample_velocity_points(scene.nodes, density=True)
    assert u_p.any()
    assert same_bits(u_g.reshape(-1, 3), u_p) and same_bits(vrho_g.reshape(-1), vrho_p)
    assert same_bits(vrho_g, rho_g)
    # out_density alone (the velocity pointer NULL)
    only = np.full(dims[::-1], np.nan, F32)
    o, sp, d = np.ascontiguousarray(origin, F32), np.ascontiguousarray(spacing, F32), np.asarray(dims, np.uint32)
    assert w._L.ws_sample_velocity_grid(w._h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, None, only.ctypes.data) == 0
    assert same_bits(only, rho_g)
    if ieee:
        want_u, want_rho, want_iso, _ = scene.restatement()
        assert same_bits(u_g.reshape(-1, 3)[scene.sel], want_u) and same_bits(vrho_g.reshape(-1)[scene.sel], want_rho)
        assert same_bits(rho_g.reshape(-1)[scene.sel], want_iso)
