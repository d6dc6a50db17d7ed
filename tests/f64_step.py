"""A float64 restatement of one fluid step, with an error bound for every particle.

Written from assets/simulation.wgsl (the passes the oracle cites: K1 hash_particles :130-141, K4 update_density
:143-195, K5 update_pressure_force :197-269, K6 integrate :271-310), not from the oracle's loops.  It is a plain helper
module of the suite, imported by tests/test_f64_step_reference.py (the CPU oracle) and tests/test_gpu_f64_step.py /
tests/test_gpu_launch_shapes.py (the HIP step).  Input is one float32 particle state and the params (teacher forcing).

Pairs.  A particle's cell is floorf(pred / h) in float32.  The pairs of particle i are every j whose cell lies in the
27-cell stencil of i's cell and whose float32 `d2 = ex*ex + ey*ey + ez*ez` is <= d2_accept, the largest float32 T with
sqrtf(T) <= h (the reference's `dst > h` test).  Each pair carries the reference's multiplicity
m_ij = #{o in stencil : hash(c_i + o) % N == hash(c_j) % N} (u32 wrap, simulation.wgsl:125-128): the reference walks one
bucket per stencil offset and meets j once per offset whose bucket is j's.  No special case for aliasing sizes.

Density, near density (K4) and acceleration (K5) are float64 sums over the pairs.  K5's inputs are the densities and
pressures the step under test produced (read back), so a density error does not leak into the force check; self is
excluded by index; at d == 0 the direction is (0, 1, 0).

Per-particle bound, one formula and one constant for every field, case and arithmetic:

    tol_i = c * u * [ (n_i + 8) * sum_j m_ij |t_ij|  +  sum_j m_ij |dt_ij/dd| * h ],    u = 2^-24

t_ij are the pair terms of that field component (for the acceleration: pressure, near-pressure and viscosity term of
the pair, each with its final 1/rho_i or viscosity_strength factor), n_i the number of pairs counted with their
multiplicity.  The first part is the recursive-summation bound for n_i terms that each carry a few roundings (the +8
covers the per-term roundings, the padding and the final scaling of a short sum).  The second part covers the rounding
of the distance: a float32 d (or d*d) is off by about u * d <= u * h, and the kernel terms are steep where h - d
cancels.  dt/dd is taken over the kernel factor only (the 1/d of the direction is a relative error, in the first part).

c = 4 (the starting value of the calibration, kept).  Measured use of the bound (worst err_i / tol_i over every
particle and component): the f32 oracle -- a forward sum with correctly rounded sqrt and division -- 0.28 for the
acceleration and 0.06 for the density over the cases of tests/test_f64_step_reference.py, which asserts < 0.5 so that
another summation order fits under the same c; the HIP step 0.33 / 0.07 with hardware rcp / sqrt and 0.31 / 0.07 with
IEEE division over tests/test_gpu_f64_step.py.  A smaller c buys little: the per-particle bound is already far below the
global tolerance for the quiet particles where the global check is blind (tests/test_f64_step_reference.py, sensitivity).

K6 is restated in numpy float32 in the WGSL order; it takes the acceleration of the step under test, so position,
velocity and predicted position are compared bit for bit for every particle.

Results are recorded into util.PARITY_REPORT with the usual keys: `tolerance` is the largest per-particle bound used
and `error_over_tolerance` the worst err_i / tol_i."""
import numpy as np

from util import PARITY_REPORT

C_BOUND = 4.0
U = 2.0 ** -24
P1, P2, P3 = np.uint32(15823), np.uint32(9737333), np.uint32(440817757)  # simulation.wgsl:38-40
INF = 999999999
DENSITY_PADDING = np.float32(0.00001)  # simulation.wgsl:4
LOOKAHEAD = np.float32(1.0 / 50.0)  # simulation.wgsl:3
# simulation.wgsl:6-34: x slowest, z fastest
OFFSETS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int64)
CHUNK_PAIRS = 1 << 22  # candidates per numpy chunk (a few hundred MB of temporaries)


def accept(h):
    """Largest f32 T with sqrtf(T) <= h (the library's d2_accept)."""
    h = np.float32(h)
    t = np.float32(h * h)
    while np.sqrt(t) > h:
        t = np.nextafter(t, np.float32(0))
    while np.sqrt(np.nextafter(t, np.float32(np.inf))) <= h:
        t = np.nextafter(t, np.float32(np.inf))
    return t


def _linear(cx, cy, cz):
    """hash_cell before its `% N`: vec3<u32>(cell) reinterprets the bits, products and sums wrap mod 2^32."""
    with np.errstate(over="ignore"):
        return (np.asarray(cx, np.int64).astype(np.uint32) * P1 + np.asarray(cy, np.int64).astype(np.uint32) * P2
                + np.asarray(cz, np.int64).astype(np.uint32) * P3)


def stencil_aliases(n):
    """Host-side replica of the library's upload_mult predicate: can two cells of one 27-stencil share a bucket of the
    reference's N-bucket table?  Power-of-two N: hash_cell is linear mod N, compare the 27 offsets' buckets.  Any other N:
    two stencil cells whose linear forms differ by delta can alias iff delta or delta -+ 2^32 is a multiple of N."""
    n = int(n)
    lin = [int(_linear(x, y, z)) for x, y, z in OFFSETS]
    if n & (n - 1) == 0:
        return len({v % n for v in lin}) < 27
    for a in range(27):
        for b in range(27):
            if a != b and any((lin[a] - lin[b] + k * (1 << 32)) % n == 0 for k in (-1, 0, 1)):
                return True
    return False


def cells_of(pred, h):
    """floorf(pred / h) per axis in float32 (simulation.wgsl:121-123), as int64."""
    return np.floor(np.ascontiguousarray(pred[:, :3], np.float32) / np.float32(h)).astype(np.int32).astype(np.int64)


def hash_keys(cell, n):
    return (_linear(cell[:, 0], cell[:, 1], cell[:, 2]) % np.uint32(n)).astype(np.uint32)


class CellList:
    """Particles grouped by their float32 cell; lookups of a cell's [start, start + count) range in `order`."""

    def __init__(self, pred, h):
        self.cell = cells_of(pred, h)
        lo = self.cell.min(axis=0) - 1
        self.dims = self.cell.max(axis=0) - lo + 2
        self.shift = lo
        self.key = self._key(self.cell)
        self.order = np.argsort(self.key, kind="stable")
        ukey, ustart, ucount = np.unique(self.key[self.order], return_index=True, return_counts=True)
        ncell = int(np.prod(self.dims))
        if ncell <= (1 << 26):  # a dense table: one gather per lookup
            self.start = np.zeros(ncell, np.int64)
            self.count = np.zeros(ncell, np.int64)
            self.start[ukey] = ustart
            self.count[ukey] = ucount
            self.ukey = None
        else:  # particles far outside the container: search the occupied cells
            self.ukey, self.ustart, self.ucount = ukey, ustart, ucount

    def _key(self, cell):
        c = cell - self.shift
        return (c[:, 0] * self.dims[1] + c[:, 1]) * self.dims[2] + c[:, 2]

    def delta(self, o):
        return (int(o[0]) * int(self.dims[1]) + int(o[1])) * int(self.dims[2]) + int(o[2])

    def lookup(self, key):
        if self.ukey is None:
            return self.start[key], self.count[key]
        pos = np.minimum(np.searchsorted(self.ukey, key), len(self.ukey) - 1)
        hit = self.ukey[pos] == key
        return self.ustart[pos], np.where(hit, self.ucount[pos], 0)

    def candidates(self, queries):
        """Per query particle: the number of particles in its 27 stencil cells (the kernels' candidate count)."""
        total = np.zeros(len(queries), np.int64)
        kq = self.key[queries]
        for o in OFFSETS:
            total += self.lookup(kq + self.delta(o))[1]
        return total


def _pairs(cl, pred32, queries, accept_d2, mult_hash):
    """Yield (query slice, local query index, j, m) for the queries in chunks of about CHUNK_PAIRS candidates."""
    cand = cl.candidates(queries)
    ends = np.cumsum(cand)
    s = 0
    while s < len(queries):
        e = int(np.searchsorted(ends, (ends[s - 1] if s else 0) + CHUNK_PAIRS, side="right"))
        e = max(e, s + 1)
        q = queries[s:e]
        kq = cl.key[q]
        il, jl = [], []
        for o in OFFSETS:
            st, cnt = cl.lookup(kq + cl.delta(o))
            tot = int(cnt.sum())
            if not tot:
                continue
            loc = np.repeat(np.arange(len(q)), cnt)
            first = np.repeat(np.cumsum(cnt) - cnt, cnt)
            il.append(loc)
            jl.append(cl.order[np.repeat(st, cnt) + (np.arange(tot) - first)])
        if il:
            i_loc, j = np.concatenate(il), np.concatenate(jl)
            e32 = pred32[j] - pred32[q[i_loc]]
            d2 = e32[:, 0] * e32[:, 0] + e32[:, 1] * e32[:, 1] + e32[:, 2] * e32[:, 2]
            ok = ~(d2 > accept_d2)
            i_loc, j = i_loc[ok], j[ok]
            if mult_hash is None:
                m = np.ones(len(j), np.float64)
            else:
                n, keys = mult_hash
                cq = cl.cell[q]
                hq = np.stack([(_linear(cq[:, 0] + o[0], cq[:, 1] + o[1], cq[:, 2] + o[2]) % np.uint32(n)) for o in OFFSETS], 1)
                m = (hq[i_loc] == keys[j][:, None]).sum(1).astype(np.float64)
                assert m.min() >= 1
        else:
            i_loc, j, m = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
        yield slice(s, e), q, i_loc, j, m
        s = e


class StepReference:
    """Float64 K4 / K5 of one step from `state` (f32 particle records) for the particles `queries` (default: all).
    `produced`: the step's output records -- their densities and pressures are K5's inputs.  keep_pairs: also keep every
    pair's (i, j, m, d, density terms, acceleration terms) in self.pair_terms (small cases only)."""

    def __init__(self, state, params, kernel, produced, queries=None, keep_pairs=False):
        n = len(state)
        self.n = n
        self.queries = np.arange(n, dtype=np.int64) if queries is None else np.asarray(queries, np.int64)
        h32 = np.float32(params.smoothing_radius)
        h = float(h32)
        pow2, pow3 = float(np.float32(kernel.pow2)), float(np.float32(kernel.pow3))
        pow2d, pow3d, spk = float(np.float32(kernel.pow2_der)), float(np.float32(kernel.pow3_der)), float(np.float32(kernel.spikey_pow3))
        vs = float(np.float32(params.viscosity_strength))
        pred32 = np.ascontiguousarray(state["predicted_position"][:, :3], np.float32)
        pred = pred32.astype(np.float64)
        vel = state["velocity"][:, :3].astype(np.float64)
        rho = produced["density"].astype(np.float64)
        prs = produced["pressure"].astype(np.float64)
        cl = CellList(pred32, h32)
        keys = hash_keys(cl.cell, n)
        self.keys = keys
        mult_hash = (n, keys) if stencil_aliases(n) else None
        Q = len(self.queries)
        self.candidates = cl.candidates(self.queries)
        dens = np.zeros((Q, 2))
        dsum = np.zeros((Q, 2))
        dder = np.zeros((Q, 2))
        npair = np.zeros(Q)
        acc = np.zeros((Q, 3))
        asum = np.zeros((Q, 3))
        ader = np.zeros((Q, 3))
        nacc = np.zeros(Q)
        kept = []
        for sl, q, il, j, m in _pairs(cl, pred32, self.queries, accept(h32), mult_hash):
            nq = len(q)
            i = q[il]
            e = pred[j] - pred[i]
            d = np.sqrt((e * e).sum(1))
            hd = h - d
            t2, t3 = hd * hd * pow2, hd * hd * hd * pow3
            bc = lambda w: np.bincount(il, weights=w, minlength=nq)  # noqa: E731
            dens[sl, 0] += bc(m * t2)
            dens[sl, 1] += bc(m * t3)
            dsum[sl, 0] += bc(m * np.abs(t2))
            dsum[sl, 1] += bc(m * np.abs(t3))
            dder[sl, 0] += bc(m * 2 * np.abs(hd) * pow2 * h)
            dder[sl, 1] += bc(m * 3 * hd * hd * pow3 * h)
            npair[sl] += bc(m)
            # K5: self excluded by index, before the distance test (simulation.wgsl:232)
            k = j != i
            il5, i5, j5, m5, e5, d5 = il[k], i[k], j[k], m[k], e[k], d[k]
            dirv = np.where(d5[:, None] > 0, e5 / np.where(d5 > 0, d5, 1.0)[:, None], np.array([0.0, 1.0, 0.0]))
            sp = (prs[i5, 0] + prs[j5, 0]) / 2
            spn = (prs[i5, 1] + prs[j5, 1]) / 2
            dh = d5 - h
            a = sp * dh * pow2d / rho[j5, 0] / rho[i5, 0]
            b = spn * dh * dh * pow3d / rho[j5, 1] / rho[i5, 0]
            w = h * h - d5 * d5
            visc = w * w * w * spk * vs
            da = np.abs(sp) * pow2d / rho[j5, 0] / rho[i5, 0]
            db = np.abs(spn) * 2 * np.abs(dh) * pow3d / rho[j5, 1] / rho[i5, 0]
            dv = 6 * d5 * w * w * spk * vs
            bc5 = lambda w_: np.bincount(il5, weights=w_, minlength=nq)  # noqa: E731
            nacc[sl] += bc5(m5)
            for c in range(3):
                pt, nt, vt = dirv[:, c] * a, dirv[:, c] * b, (vel[j5, c] - vel[i5, c]) * visc
                acc[sl, c] += bc5(m5 * (pt + nt + vt))
                asum[sl, c] += bc5(m5 * (np.abs(pt) + np.abs(nt) + np.abs(vt)))
                ader[sl, c] += bc5(m5 * (np.abs(dirv[:, c]) * (da + db) + np.abs(vel[j5, c] - vel[i5, c]) * dv) * h)
            if keep_pairs:
                tacc = np.zeros((len(j), 3))
                tacc[k] = dirv * (a + b)[:, None] + (vel[j5] - vel[i5]) * visc[:, None]
                kept.append((i, j, m, d, np.stack([t2, t3], 1), tacc))
        pad = float(DENSITY_PADDING)
        self.density = dens + pad
        self.density_tol = C_BOUND * U * ((npair[:, None] + 8) * (dsum + pad) + dder)
        self.acceleration = acc
        self.acceleration_tol = C_BOUND * U * ((nacc[:, None] + 8) * asum + ader)
        self.pairs = npair
        if keep_pairs:
            self.pair_terms = tuple(np.concatenate(x) for x in zip(*kept))

    def errors(self, got):
        """|got - float64| of the queries: (density (Q, 2), acceleration (Q, 3))."""
        q = self.queries
        return (np.abs(got["density"][q].astype(np.float64) - self.density),
                np.abs(got["acceleration"][q, :3].astype(np.float64) - self.acceleration))

    def ratios(self, got):
        """err_i / tol_i of the queries: (density (Q, 2), acceleration (Q, 3))."""
        ed, ea = self.errors(got)
        return _ratio(ed, self.density_tol), _ratio(ea, self.acceleration_tol)


def integrate_f32(state, acceleration, params):
    """K6 (simulation.wgsl:271-310) in numpy float32, in the WGSL order, with the given acceleration.
    Returns (position, velocity, predicted_position), each (n, 4)."""
    dt = np.float32(params.delta_time)
    damp = np.float32(-1.0) * np.float32(params.collision_damping)
    g = np.array([params.gravity[k] for k in range(4)], np.float32)
    mn = np.array([params.ext_min[k] for k in range(3)], np.float32)
    mx = np.array([params.ext_max[k] for k in range(3)], np.float32)
    v = state["velocity"] + (g + acceleration.astype(np.float32)) * dt
    p = state["position"] + v * dt
    for k in range(3):
        lo = p[:, k] < mn[k]
        hi = ~lo & (p[:, k] > mx[k])
        v[lo | hi, k] *= damp
        p[lo, k] = mn[k]
        p[hi, k] = mx[k]
    return p, v, p + v * LOOKAHEAD


def sort_view(state, h):
    """K1 / sort / K3 of the step recomputed: (per-particle keys, sorted key sequence, cell offsets)."""
    n = len(state)
    keys = hash_keys(cells_of(state["predicted_position"], h), n)
    srt = np.sort(keys)
    off = np.full(n, INF, np.uint32)
    head = np.r_[True, srt[1:] != srt[:-1]]
    off[srt[head]] = np.flatnonzero(head).astype(np.uint32)
    return keys, srt, off


def _ratio(err, tol):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))


def _record(what, arithmetic, field, err, tol):
    ratio = _ratio(err, tol)
    PARITY_REPORT.append({"case": what, "arithmetic": arithmetic, "field": field, "n": int(err.shape[0]),
                          "linf_error": float(err.max()) if err.size else 0.0, "noise_unit": None,
                          "tolerance": float(tol.max()) if tol.size else 0.0,
                          "error_over_tolerance": float(ratio.max()) if ratio.size else 0.0, "per_particle": True})
    return ratio


def check_step(state, got, params, kernel, what="", arithmetic=None, queries=None, check_sort=None):
    """Compare the step `got` (output records of one step from `state`) with the float64 restatement, particle by
    particle: density and near density within their bound, pressures as float32 functions of the step's densities bit
    for bit, acceleration within its bound, K6 bit for bit.  check_sort: (keys, perm, offsets) of the step to compare
    with the recomputed sort view.  Returns {field: worst err/tol} (the reference object under "ref")."""
    ref = StepReference(state, params, kernel, got, queries)
    q = ref.queries
    out = {"ref": ref}
    fails = []
    ed, ea = ref.errors(got)
    rd = _record(what, arithmetic, "density", ed, ref.density_tol)
    ra = _record(what, arithmetic, "acceleration", ea, ref.acceleration_tol)
    for name, r in (("density", rd), ("acceleration", ra)):
        out[name] = float(r.max()) if r.size else 0.0
        if not out[name] <= 1.0:
            bad = np.unravel_index(np.argmax(r), r.shape)
            p = int(q[bad[0]])
            fails.append("%s: %s of particle %d (component %d, %d pairs, %d candidates) is %.3f x its bound: got %r, float64 %r"
                         % (what, name, p, bad[1], ref.pairs[bad[0]], ref.candidates[bad[0]], out[name],
                            (got["density"] if name == "density" else got["acceleration"])[p, bad[1]],
                            (ref.density if name == "density" else ref.acceleration)[bad]))
    dens = got["density"]
    press = np.stack([np.float32(params.pressure_scalar) * (dens[:, 0] - np.float32(params.target_density)),
                      np.float32(params.near_pressure_scalar) * dens[:, 1]], 1)
    if not np.array_equal(press.view(np.uint32), got["pressure"].view(np.uint32)):
        fails.append("%s: pressures are not the float32 functions of the step's own densities" % what)
    # K6 has no reduction: every particle, also outside `queries`
    pos, vel, pred = integrate_f32(state, got["acceleration"], params)
    for name, want in (("position", pos), ("velocity", vel), ("predicted_position", pred)):
        same = np.all(got[name].view(np.uint32) == want.view(np.uint32), axis=1)
        PARITY_REPORT.append({"case": what, "arithmetic": arithmetic, "field": name, "n": int(len(state)), "linf_error":
                              0.0 if same.all() else float(np.max(np.abs(got[name] - want))), "noise_unit": 0.0,
                              "tolerance": 0.0, "error_over_tolerance": 0.0 if same.all() else float("inf"),
                              "bitwise": True, "per_particle": True})
        if not same.all():
            p = int(np.argmin(same))
            fails.append("%s: K6 %s of %d particles differs from the float32 restatement (first: particle %d, got %r, want %r)"
                         % (what, name, int((~same).sum()), p, got[name][p], want[p]))
    if check_sort is not None:
        keys, perm, off = check_sort
        want_keys, want_sorted, want_off = sort_view(state, params.smoothing_radius)
        if not np.array_equal(keys, want_keys):
            fails.append("%s: hash keys differ from the recomputation" % what)
        elif not (np.array_equal(np.sort(perm), np.arange(len(state), dtype=np.uint32)) and np.array_equal(keys[perm], want_sorted)):
            fails.append("%s: the permutation does not sort the keys" % what)
        elif not np.array_equal(off, want_off):
            fails.append("%s: cell offsets differ from the recomputation" % what)
    assert not fails, "; ".join(fails)
    return out
