"""A plain restatement of k_schedule (csrc/ws_kernels.hip "tile schedule"): from a cost per tile to the eight cut points
`split` and the tile order `perm` of one neighbour kernel.  Exact integers throughout (Python ints and numpy uint64, no
floats), written from the kernel's comment block and text; tests/test_gpu_schedule_kernel.py compares the kernel with
it word for word.  `check_schedule` knows nothing of costs: it states what the scheduled K4 / K5 need of ANY schedule in
order to run every tile exactly once.

The shared input matrix (tile counts, cost shapes, groupings) of the CPU and GPU tests lives here too."""
import numpy as np

BLOCK = 1024          # WS_SCHED_BLOCK: threads of a k_schedule workgroup, each owning one slice of the tiles
MAX_CLASSES = 8       # WS_SCHED_CLASSES
SHIFT = 10            # per-thread sums are scaled down by 2^10 before the 32-bit block scans
COST_CLAMP = 1 << 24  # the largest cost K4 / K5 write: min(ticks, 0xFFFFFF) + 1
M32 = 0xFFFFFFFF


def limits(T):
    """(nmin, nmax): the fewest and the most tiles one XCD's range may hold."""
    return T // 16, T // 8 + T // 16 + 1


def sched_grid_rows(T):
    """Rows per XCD of a scheduled launch (wsk_sched_grid(T) / 8): a range longer than this loses tiles."""
    return T // 8 + T // 16 + 2


class Cuts:
    """What the first half of the kernel derives: the cuts, the cost an unmeasured tile counts as, and how it got there."""

    def __init__(self, split, fill, total_s, filled):
        self.split, self.fill, self.total_s, self.filled = split, fill, total_s, filled


def cuts(cost):
    """split[9] of cost[T] (T >= 1)."""
    cost = np.asarray(cost, dtype=np.uint64)
    T = int(cost.size)
    assert T >= 1
    per = (T + BLOCK - 1) // BLOCK
    padded = np.zeros(BLOCK * per, dtype=np.uint64)
    padded[:T] = cost
    slices = padded.reshape(BLOCK, per)  # thread tid owns tiles [min(tid * per, T), min(tid * per + per, T))
    # ---- fill: what an unmeasured tile (cost 0) counts as -- the average of the measured ones
    tot_known = int(np.count_nonzero(cost))
    sum32 = slices.sum(axis=1) & np.uint64(M32)  # (the kernel's per-thread sum is 32 bits wide)
    tot_sum = int((sum32 >> np.uint64(SHIFT)).sum()) & M32
    fill = min(max((tot_sum << SHIFT) // tot_known, 1), 0xFFFFFF) if tot_known else 1
    # ---- scaled scan of the FILLED costs
    filled = np.where(cost == 0, np.uint64(fill), cost)
    padded[:T] = filled
    mine = padded.reshape(BLOCK, per).sum(axis=1)  # 64-bit
    mine_s = [int(v) & M32 for v in (mine >> np.uint64(SHIFT))]
    before_s, acc = [], 0
    for v in mine_s:
        before_s.append(acc)
        acc = (acc + v) & M32
    total_s = acc
    cut = [0] * 8 + [T]
    if total_s >= 8:
        # the thread whose slice contains the k-th eighth of the total looks for the exact tile
        for tid in range(BLOCK):
            a = min(tid * per, T)
            b = min(a + per, T)
            for k in range(1, 8):
                target = total_s * k // 8
                if before_s[tid] <= target < before_s[tid] + mine_s[tid]:
                    run, want = before_s[tid] << SHIFT, target << SHIFT
                    t = a
                    while t < b:
                        run += int(filled[t])
                        if run > want:
                            break
                        t += 1
                    cut[k] = min(t + 1, T)
    else:
        for k in range(1, 8):
            cut[k] = T * k // 8
    # ---- every XCD keeps between nmin and nmax tiles, and the rest must stay coverable by the XCDs still to come
    nmin, nmax = limits(T)
    prev = 0
    for k in range(1, 8):
        left = 8 - k
        lo, hi = prev + nmin, prev + nmax
        lo = max(lo, T - left * nmax if T > left * nmax else 0)
        hi = min(hi, T - min(T, left * nmin))
        c = min(max(cut[k], lo), max(hi, lo))
        c = min(c, T)
        cut[k] = c
        prev = c
    cut[0], cut[8] = 0, T
    return Cuts(cut, fill, total_s, filled)


def order(c, nclasses, G):
    """perm[T] for the cuts `c`: inside each range the groups of G tiles (clipped to the range) in ascending class, class 0
    the heaviest; group order kept inside a class, tile order inside a group."""
    nclasses = min(max(int(nclasses), 1), MAX_CLASSES)  # wsk_schedule
    G = max(int(G), 1)
    T = c.split[8]
    perm = np.empty(T, dtype=np.uint32)
    for x in range(8):
        r0, r1 = c.split[x], c.split[x + 1]
        if r1 == r0:
            continue
        starts = np.array([r0] + list(range((r0 // G + 1) * G, r1, G)), dtype=np.int64)  # first tile of every clipped group
        lens = np.diff(np.append(starts, r1)).astype(np.uint64)
        mean = np.add.reduceat(c.filled[r0:r1], starts - r0) // lens
        cmax = int(mean.max()) + 1
        cls = ((np.uint64(cmax - 1) - mean) * np.uint64(nclasses)) // np.uint64(cmax)
        at = r0
        for g in np.argsort(cls, kind="stable"):
            n = int(lens[g])
            perm[at:at + n] = np.arange(starts[g], starts[g] + n, dtype=np.uint32)
            at += n
    return perm


def schedule(cost, nclasses=8, G=1):
    """(split[9] as a list of ints, perm[T] as uint32) -- what k_schedule writes for one kernel."""
    c = cuts(cost)
    return c.split, order(c, nclasses, G)


# ---------------------------------------------------------------------------------------------------------------------
# the invariant checker
# ---------------------------------------------------------------------------------------------------------------------
class ScheduleFault(AssertionError):
    """`fault` names what is wrong: one of FAULTS."""

    def __init__(self, fault, detail):
        super().__init__("%s: %s" % (fault, detail))
        self.fault = fault


FAULTS = ("first cut is not 0", "last cut is not T", "split is not monotone", "range longer than nmax", "range shorter than nmin",
          "perm has the wrong length", "tile outside its range", "tile duplicated")


def check_schedule(split, perm, T):
    """What the scheduled k_density_listed / k_force_listed need in order to run every tile exactly once: workgroup
    (x, j) runs tile perm[split[x] + j] for j < split[x + 1] - split[x], on a grid with sched_grid_rows(T) rows per x."""
    split = [int(v) for v in split]
    perm = np.asarray(perm, dtype=np.int64)
    nmin, nmax = limits(T)
    assert nmax < sched_grid_rows(T)
    if len(split) != 9 or split[0] != 0:
        raise ScheduleFault("first cut is not 0", str(split))
    if split[8] != T:
        raise ScheduleFault("last cut is not T", "%s, T = %d" % (split, T))
    for x in range(8):
        if split[x + 1] < split[x]:
            raise ScheduleFault("split is not monotone", "%s at range %d" % (split, x))
    for x in range(8):
        n = split[x + 1] - split[x]
        if n > nmax:
            raise ScheduleFault("range longer than nmax", "range %d of %s has %d tiles, nmax = %d" % (x, split, n, nmax))
        if n < nmin:
            raise ScheduleFault("range shorter than nmin", "range %d of %s has %d tiles, nmin = %d" % (x, split, n, nmin))
    if perm.size != T:
        raise ScheduleFault("perm has the wrong length", "%d entries for %d tiles" % (perm.size, T))
    for x in range(8):
        r0, r1 = split[x], split[x + 1]
        part = perm[r0:r1]
        out = part[(part < r0) | (part >= r1)]
        if out.size:
            raise ScheduleFault("tile outside its range", "range %d = [%d, %d) lists tile %d" % (x, r0, r1, out[0]))
        if not np.array_equal(np.sort(part), np.arange(r0, r1)):
            seen = np.bincount(part - r0, minlength=r1 - r0)
            raise ScheduleFault("tile duplicated", "range %d = [%d, %d) lists tile %d %d times and misses tile %d"
                                % (x, r0, r1, r0 + int(seen.argmax()), int(seen.max()), r0 + int(seen.argmin())))


# ---------------------------------------------------------------------------------------------------------------------
# the inputs both test files run over
# ---------------------------------------------------------------------------------------------------------------------
TILE_COUNTS = (1, 2, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 313, 1023, 1024, 1025, 4096)
BIG_TILE_COUNTS = (4099, 16384, 23438)  # C2's K4, the schedule window's upper end, 1.5 M particles: G = 1, 8 classes only
GROUPS = (1, 3, 8, 1024)                # 1024: more than nmax of every T in TILE_COUNTS -- one group covers a whole range
CLASSES = (1, 2, 8)


def _hot(T, where):
    c = np.ones(T, dtype=np.uint32)
    c[where] = COST_CLAMP
    return c


def _eighth(T, first):
    c = np.ones(T, dtype=np.uint32)
    n = max(T // 8, 1)
    if first:
        c[:n] = COST_CLAMP
    else:
        c[T - n:] = COST_CLAMP
    return c


def _ramp(T):
    return (1 + np.arange(T, dtype=np.uint64) * np.uint64(COST_CLAMP - 1) // np.uint64(max(T - 1, 1))).astype(np.uint32)


def _lognormal(T, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.exp(rng.normal(9.0, 2.5, T)), 1, COST_CLAMP).astype(np.uint32)


def _half_zero(T, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(1, COST_CLAMP + 1, T, dtype=np.uint32)
    c[rng.permutation(T)[:(T + 1) // 2]] = 0
    return c


def _single(T):
    c = np.zeros(T, dtype=np.uint32)
    c[T // 3] = 5000
    return c


def _scaled_total(T, k):
    """Every slice sums to less than 2^10 (scaled: 0) but k units of 2^10 spread over the tiles: total_s == k exactly."""
    c = np.ones(T, dtype=np.uint32)
    for j in range(k):
        c[j * T // k] += 1 << SHIFT
    return c


SHAPES = {
    "all-zero": lambda T: np.zeros(T, dtype=np.uint32),
    "all-one": lambda T: np.ones(T, dtype=np.uint32),
    "all-clamped": lambda T: np.full(T, COST_CLAMP, dtype=np.uint32),
    "hot-first": lambda T: _hot(T, 0),
    "hot-last": lambda T: _hot(T, T - 1),
    "hot-middle": lambda T: _hot(T, T // 2),
    "first-eighth-hot": lambda T: _eighth(T, True),
    "last-eighth-hot": lambda T: _eighth(T, False),
    "ramp-up": _ramp,
    "ramp-down": lambda T: _ramp(T)[::-1].copy(),
    "lognormal": lambda T: _lognormal(T, 1000 + T),
    "half-zero": lambda T: _half_zero(T, 2000 + T),
    "single-measured": _single,
    "total-7": lambda T: _scaled_total(T, 7),
    "total-8": lambda T: _scaled_total(T, 8),
}


def _random(T, seed):
    """Uniform in magnitude rather than in value: shifted right by 0 .. 24 bits, so zeros and clamped costs both occur."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, COST_CLAMP + 1, T, dtype=np.uint32) >> rng.integers(0, 25, T, dtype=np.uint32)


# what the consumer test plants before five consecutive steps (K4 gets the array, K5 the same array reversed)
PLANTED = ("hot-first", "hot-last", "last-eighth-hot", "all-zero", "random")


def planted(kind, T):
    return _random(T, 3000 + T) if kind == "random" else SHAPES[kind](T)


def matrix():
    """[(T, shape name, cost[T])]: every tile count with every cost shape."""
    return [(T, name, make(T)) for T in TILE_COUNTS + BIG_TILE_COUNTS for name, make in SHAPES.items()]


def groupings(T):
    """[(G, nclasses)] a tile count is ordered with."""
    return [(1, 8)] if T in BIG_TILE_COUNTS else [(G, k) for G in GROUPS for k in CLASSES]
