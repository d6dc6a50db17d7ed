"""The accept-mask rows are addressed through running pointers (K4: one stride further each time a lane's 32-bit
accumulator fills; K5's per-lane iterator: one stride per mask word fetched).  The product library equals the developer
build's one-thread-per-particle kernels bit for bit, in both arithmetics,

 * on 8 192-particle clouds at three densities whose candidates per particle cover every residue mod 32 (every phase of
   K4's word crossing) and every mask-word count from 1 to 20 (every advance of K5's iterator; waves below
   and above the in-step walk's limit of 4 words at this size);
 * on constructed positions in which the 27 cells of the particles of one cell hold exactly 2 047, 2 048, 2 049 and
   2 080 candidates -- the last mask row (63) partly filled, exactly filled, and one / 32 candidates past it, where a
   running pointer could run one row too far.  The overflow counter equals the number of particles with more than
   2 048 candidates, counted on the host.

`simple` comes from the developer build's WS_VARIANT hook, `listed` is the product library as it ships."""
import numpy as np
import pytest

import f64_step as F
from test_gpu_launch_shapes import _cloud, _same, _worker

BOTH_ARITHMETICS = pytest.mark.parametrize("ieee", [False, True], ids=["hw-rcp-sqrt", "ieee-division"])

N = 8192
# particles per cell.  The walls of so small a container leave corner particles with 8 of their 27 cells, so each cloud
# spans a wide band of mask words per particle (candidates / 32, rounded up): 1-3, 2-14 and 4-21
CLOUDS = {"sparse": 1.6, "middle": 14.0, "dense": 23.0}
MASK_CANDIDATES = 2048  # 32 * ND_MASK_WORDS
EDGE_COUNTS = [2047, 2048, 2049, 2080]
FREE_STEPS = 3


def cloud(ws, name):
    pos, params = _cloud(ws, N, CLOUDS[name], 0x6A5)
    return pos, params, F.CellList(pos, params.smoothing_radius).candidates(np.arange(N))


def edge_positions(ws, count):
    """N particles: `count` of them in the 27 cells around cell (0, 0, 0), at least 64 (a whole wave of the sorted order)
    in that cell itself, each well inside its cell (a step's prediction moves a particle at rest by gravity * dt / 50, far
    less than the margin); the others sparse and more than two cells away from all of them."""
    params = ws.make_params(container_size=(6.0, 6.0, 6.0))
    h = np.float32(params.smoothing_radius)
    rng = np.random.default_rng(count)
    cell = rng.integers(-1, 2, (count, 3))
    cell[:96] = 0
    clump = (cell + rng.uniform(0.2, 0.8, (count, 3))) * h
    lo, hi = np.array(list(params.ext_min)[:3]), np.array(list(params.ext_max)[:3])
    lo[0] = 1.0  # (the clump ends at x = 2 h = 0.5)
    back = rng.uniform(lo + 0.01, hi - 0.01, (N - count, 3))
    pos = np.concatenate([clump, back]).astype(np.float32)
    return pos[rng.permutation(N)], params


def test_the_inputs_cover_what_they_are_meant_to(ws):
    """Host side only: no aliasing (an aliasing count takes the hashed kernels, not the listed ones), every residue of
    the candidate count mod 32, every word count from 1 to 20, and the four edge counts exactly."""
    assert not F.stencil_aliases(N)
    residues, words = set(), set()
    for name in CLOUDS:
        cand = cloud(ws, name)[2]
        assert 0 < cand.min() and cand.max() <= MASK_CANDIDATES
        words |= set(((cand + 31) // 32).tolist())
        residues |= set((cand % 32).tolist())
    assert residues == set(range(32))
    assert set(range(1, 21)) <= words, sorted(words)
    for count in EDGE_COUNTS:
        pos, params = edge_positions(ws, count)
        cand = F.CellList(pos, params.smoothing_radius).candidates(np.arange(N))
        assert cand.max() == count and int((cand == count).sum()) >= 96, (count, cand.max())
        assert int((cand > MASK_CANDIDATES).sum()) == (0 if count <= MASK_CANDIDATES else int((cand == count).sum()))


def one_step_each(ws, devlib, pos, params, ieee, what, free_steps=0):
    simple = _worker(ws, "simple", pos, params, ieee, devlib)
    listed = _worker(ws, "listed", pos, params, ieee, devlib)
    try:
        state = listed.read_vec("particles")
        for w in (simple, listed):  # one teacher-forced step from the same records
            w.write_slice("particles", state)
            w.run()
        got = listed.read_vec("particles")
        overflow = listed.stats()["mask_overflow"]
        _same(simple.read_vec("particles"), got, what + " step 1")
        if free_steps:
            simple.run(free_steps)
            listed.run(free_steps)
            _same(simple.read_vec("particles"), listed.read_vec("particles"), what + " free step %d" % (1 + free_steps))
        return state, overflow
    finally:
        simple.close()
        listed.close()


@pytest.mark.gpu
@BOTH_ARITHMETICS
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_listed_equals_simple_at_every_word_phase(ws, devlib, name, ieee):
    pos, params, _ = cloud(ws, name)
    _, overflow = one_step_each(ws, devlib, pos, params, ieee, "cloud %s %s" % (name, "ieee" if ieee else "hw"), FREE_STEPS)
    assert overflow == 0


@pytest.mark.gpu
@BOTH_ARITHMETICS
@pytest.mark.parametrize("count", EDGE_COUNTS)
def test_listed_equals_simple_around_the_last_mask_row(ws, devlib, count, ieee):
    pos, params = edge_positions(ws, count)
    _, overflow = one_step_each(ws, devlib, pos, params, ieee, "%d candidates %s" % (count, "ieee" if ieee else "hw"))
    # the step bins by the predicted positions: pred = position + velocity * (1 / 50) after gravity, cells unchanged
    cand = F.CellList(pos, params.smoothing_radius).candidates(np.arange(N))
    assert cand.max() == count
    assert overflow == int((cand > MASK_CANDIDATES).sum())
