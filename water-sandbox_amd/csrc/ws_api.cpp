// ws_api.cpp -- the C ABI of include/wsfluid.h: handle lifetime, device buffers, the
// per-step launch sequence and the readback paths.  Host-only logic; all device work is
// in the .hip files.  The role played here is the one bevy_app_compute's
// AppComputeWorker plays in the reference (src/fluid_compute.rs:277-366,:393-397).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <new>

#include "ws_internal.h"

namespace {

constexpr int kGridPad = 2;                     // empty cell layers around the container
constexpr uint64_t kMaxCells = 1ull << 29;      // hard cap of the cell tables (3 x u32 per cell -> 6 GiB); see derive_dev

thread_local std::string g_create_error;

// ws_slab.inc
void slab_free(ws_handle *h);
void slab_drop_graphs(WsSlab *S);
ws_status slab_step(ws_handle *h);
ws_status slab_settle(ws_handle *h);
ws_status slab_read_by_id(ws_handle *h, int kind, void *out);
ws_status slab_gather_by_id(ws_handle *h, int kind);
ws_status slab_reset(ws_handle *h, const float *pos_xyz);
ws_status slab_write_particles(ws_handle *h, const ws_particle80 *in);
ws_status slab_regrid(ws_handle *h, const ws_params *params, bool rebalance);
ws_status slab_field_positions(ws_handle *h, const float **xyz, WsDev *global, bool with_vel);
// 32-bit FNV-1a over bytes: a collective call's arguments in the slabs' agreement (slab_verdict)
struct ArgHash {
    uint32_t word = 2166136261u;
    void operator()(const void *p, size_t bytes)
    {
        for (size_t b = 0; b < bytes; b++) word = (word ^ static_cast<const uint8_t *>(p)[b]) * 16777619u;
    }
};
struct VerdictText {
    const char *tag, *things;  // "<tag>: the slabs were given different <things>"
    bool mutates;              // the call changes state: its refusals end in "; nothing was changed"
};
ws_status slab_verdict(ws_handle *h, const VerdictText &text, const char *why, ws_status mine, uint32_t hash);
template <class Call>
ws_status slab_edit_gathered(ws_handle *h, Call &call);
ws_status global_grid(const ws_params *params, uint32_t n_global, WsDev *out);
// ws_field.inc
void free_field(ws_handle *h);
const char *cohesion_refusal(const ws_cohesion_params *p, float dt);
ws_status attr_ensure(ws_handle *h);
ws_status cohesion_prepare(ws_handle *h, const WsGathered *g, const ws_cohesion_params *p, float dt, WsCohesionArgs *args);

ws_status fail(ws_handle *h, ws_status st, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    if (h)
        h->err = buf;
    else
        g_create_error = buf;
    return st;
}

// (ws_hip_failed, below: the status a HIP error stands for, `what` and the error in ws_last_error)
#define HIP_TRY(h, expr)                                          \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) return ws_hip_failed(h, #expr, e_); \
    } while (0)

// The same inside ws_create / ws_slab_create, where a failure gives the half-built handle up through the function's `bail`.
#define CREATE_TRY(expr)                  \
    do {                                  \
        ws_status s_ = (expr);            \
        if (s_) return bail(s_);          \
    } while (0)
#define CREATE_HIP(expr)                                                \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) return bail(ws_hip_failed(h, #expr, e_)); \
    } while (0)

// A host <-> device copy on the HANDLE'S OWN stream, complete on return.  Never the legacy (null) stream: it
// synchronises implicitly with streams that are none of this handle's business, and it fails outright
// (hipErrorStreamCaptureImplicit) while any other thread of the host is capturing a hipGraph -- another handle with
// WS_FLAG_GRAPH, the host's own graphs.  Ordered behind whatever the handle has enqueued.
hipError_t copy_now(ws_handle *h, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// `bytes` of a call's output scratch: grown if need be, and zeroed on the handle's stream
template <class T>
ws_status scratch_zeroed(ws_handle *h, WsScratch<T> &buf, size_t bytes, const char *what)
{
    const ws_status st = buf.grow(h, bytes, what);
    if (st) return st;
    HIP_TRY(h, hipMemsetAsync(buf.p, 0, bytes, h->stream));
    return WS_OK;
}

// Rust f32::powi -> llvm.powi -> compiler-rt __powisf2 (square-and-multiply).
float powi_f32(float a, int b)
{
    float r = 1.0f;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return r;
}

// Largest float T with sqrtf(T) <= h, so that (d2 > T) == (sqrtf(d2) > h) for every d2.
float accept_threshold(float h)
{
    float t = h * h;
    while (sqrtf(t) > h) t = nextafterf(t, 0.0f);
    for (;;) {
        const float up = nextafterf(t, INFINITY);
        if (sqrtf(up) <= h)
            t = up;
        else
            break;
    }
    return t;
}

}  // namespace

// A HIP call that failed, as the entry point's return value (HIP_TRY, and the two owner forms of ws_internal.h when HIP
// refuses them memory): the sticky error cleared, the status, `what` and the error's name in ws_last_error.
ws_status ws_hip_failed(ws_handle *h, const char *what, hipError_t e)
{
    (void)hipGetLastError();
    return fail(h, e == hipErrorOutOfMemory ? WS_ERR_OUT_OF_MEMORY : WS_ERR_HIP, what, e);
}

namespace {

bool is_pow2(uint32_t n) { return n && !(n & (n - 1)); }

// hash_cell before its `% N`, assets/simulation.wgsl:125-128 (u32 wrap arithmetic)
uint32_t ref_linear(int x, int y, int z)
{
    return (uint32_t)x * 15823u + (uint32_t)y * 9737333u + (uint32_t)z * 440817757u;
}

uint32_t ref_hash_delta(int x, int y, int z, uint32_t n) { return ref_linear(x, y, z) % n; }

ws_status validate_params(ws_handle *h, const ws_params *p)
{
    if (!p) return fail(h, WS_ERR_INVALID_ARG, "params is NULL");
    if (!(p->smoothing_radius > 0.0f) || !isfinite(p->smoothing_radius))
        return fail(h, WS_ERR_INVALID_ARG, "smoothing_radius must be finite and > 0");
    for (int c = 0; c < 3; c++) {
        if (!isfinite(p->ext_min[c]) || !isfinite(p->ext_max[c]) || p->ext_min[c] > p->ext_max[c])
            return fail(h, WS_ERR_INVALID_ARG, "container ext_min/ext_max must be finite with ext_min <= ext_max");
    }
    return WS_OK;
}

// Fill the by-value kernel parameter block from the ABI params.
ws_status derive_dev(ws_handle *h, const ws_params &p, uint32_t n, WsDev *out)
{
    WsDev d{};
    d.dt = p.delta_time;
    d.damping = p.collision_damping;
    d.h = p.smoothing_radius;
    d.target_density = p.target_density;
    d.pressure_scalar = p.pressure_scalar;
    d.near_pressure_scalar = p.near_pressure_scalar;
    d.viscosity = p.viscosity_strength;
    ws_smoothing_kernel sk;
    ws_get_smoothing_kernel(&p, &sk);
    d.k_pow2 = sk.pow2;
    d.k_pow2_der = sk.pow2_der;
    d.k_pow3 = sk.pow3;
    d.k_pow3_der = sk.pow3_der;
    d.k_spikey = sk.spikey_pow3;
    for (int c = 0; c < 3; c++) {
        d.grav[c] = p.gravity[c];
        d.ext_min[c] = p.ext_min[c];
        d.ext_max[c] = p.ext_max[c];
    }
    d.d2_accept = accept_threshold(d.h);
    // Reference-sized cells (edge h) over the container padded by kGridPad cells.  Cell coordinates are carried as
    // f32 in the kernels (floorf(x / h) - org): keep them exactly representable.
    uint64_t cells = 1;
    for (int c = 0; c < 3; c++) {
        const double lo = floor((double)floorf(p.ext_min[c] / d.h)) - kGridPad;
        const double hi = floor((double)floorf(p.ext_max[c] / d.h)) + kGridPad;
        const double dim = hi - lo + 1.0;
        if (!(fabs(lo) < 8388608.0) || !(fabs(hi) < 8388608.0))
            return fail(h, WS_ERR_INVALID_ARG, "container / smoothing_radius out of range (more than 2^23 cells along an axis)");
        d.org[c] = (int32_t)lo;
        d.fdim[c] = d.dim[c] = (int32_t)dim;
        d.cm[c] = 1;
        cells *= (uint64_t)d.dim[c];  // < 2^69 / overflow-free: three factors below 2^24
    }
    // The cell budget.  The reference's N-bucket hashed table (simulation.wgsl:125-128) costs the same whatever the
    // smoothing radius; a dense grid of reference-sized cells does not (two HUD key presses take h from 0.25 to 0.05,
    // src/hud.rs:135-138: 125 x the cells).  When the reference-sized grid exceeds the budget, grid cells are MERGED
    // along z first (a (dx, dy) column stays one contiguous particle run, only longer), then y, then x, until it
    // fits: every cell edge stays >= h, so the 27-cell search still sees every neighbour, the order inside the
    // runs stays canonical (multi-GPU bit-identity), and the only cost is more candidates for the distance test.
    // No smoothing radius the reference accepts runs out of table memory.
    uint64_t budget = std::max<uint64_t>(16ull * n, 1ull << 24);
    if (const char *v = WS_DEV_ENV("WS_CELL_BUDGET")) budget = std::max<uint64_t>(strtoull(v, nullptr, 10), 64);  // developer builds: force the merge on small domains
    budget = std::min<uint64_t>(budget, kMaxCells);
    for (int c = 2; c >= 0 && cells > budget; c--) {
        const uint64_t others = cells / (uint64_t)d.dim[c];
        // smallest merge factor that brings this axis (and with it the grid) under the budget, at most the whole axis
        uint64_t want = std::max<uint64_t>(budget / std::max<uint64_t>(others, 1), 1);  // grid cells this axis may keep
        uint64_t m = ((uint64_t)d.fdim[c] + want - 1) / want;
        // y and z keep at least three grid cells: the nine runs of a particle are spans [cc - 1, cc + 1] of the
        // LINEAR cell index around cc = c + dx * rowy + dy * rowz, which are disjoint only if dim2 >= 3 and dim1 >= 3
        // (fewer, and z + 1 of one (dx, dy) column IS z - 1 of the next: neighbours would be counted twice)
        const uint64_t m_max = c == 0 ? (uint64_t)d.fdim[c] : (uint64_t)d.fdim[c] / 3;
        m = std::min<uint64_t>(std::max<uint64_t>(m, 1), std::max<uint64_t>(m_max, 1));
        d.cm[c] = (int32_t)m;
        d.dim[c] = (int32_t)(((uint64_t)d.fdim[c] + m - 1) / m);
        cells = others * (uint64_t)d.dim[c];
    }
    d.coarse = (d.cm[0] != 1 || d.cm[1] != 1 || d.cm[2] != 1) ? 1u : 0u;
    if (cells > kMaxCells) return fail(h, WS_ERR_OUT_OF_MEMORY, "cell grid too large even with merged cells");
    d.ncells = (uint32_t)cells;
    d.guard = d.dim[1] * d.dim[2] + d.dim[2] + 1;
    d.n = n;
    d.base = 0;
    d.gdim_x = d.dim[0];
    d.xoff = 0;
    d.hash_n = n;
    h->sk = sk;
    *out = d;
    return WS_OK;
}

void free_grid(ws_handle *h)
{
    h->cells.release();
    h->starts.release();
    h->start = nullptr;  // (the shifted alias of start_alloc)
    h->grid_alloc_cells = 0;
}

ws_status alloc_grid(ws_handle *h)
{
    const WsDev &d = h->dev;
    // (developer builds: WS_FAIL_REGRID=1 makes a RE-grid's allocation fail -- the tests' way to a dead handle)
    if (h->steps > 0 && WS_DEV_ENV("WS_FAIL_REGRID")) return fail(h, WS_ERR_OUT_OF_MEMORY, "cell tables: allocation failure forced by WS_FAIL_REGRID");
    ws_status st = WS_OK;
    if (h->grid_alloc_cells < d.ncells) {
        free_grid(h);
        if ((st = h->cells.alloc(h, &h->count, (size_t)d.ncells * 4, "cell counts"))) return st;
        if ((st = h->cells.alloc(h, &h->cursor, (size_t)d.ncells * 4, "cell cursors"))) return st;
        h->grid_alloc_cells = d.ncells;
    }
    // start is sized by the guard too, which depends on the dims: always (re)build it
    h->starts.release();
    h->start = nullptr;
    const size_t nstart = (size_t)d.ncells + 2 * (size_t)d.guard + 2;
    // the scan writes start's body (from entry `guard`) 16 B at a time: shift the array so that entry is aligned
    if ((st = h->starts.alloc(h, &h->start_alloc, (nstart + 4) * 4, "cell starts"))) return st;
    h->start = h->start_alloc + (4u - (uint32_t)d.guard % 4u) % 4u;
    // (zeroed on the same stream as its users)
    if ((st = h->starts.alloc(h, &h->bsum, (size_t)wsk_scan_state_words(d.ncells) * 4, "cell scan state", true))) return st;
    // constant parts of cell_start: front guard = 0, [ncells] and the back guard = n
    HIP_TRY(h, hipMemsetAsync(h->start, 0, (size_t)d.guard * 4, h->stream));
    std::vector<uint32_t> tail((size_t)d.guard + 2, d.n);
    HIP_TRY(h, hipMemcpyAsync(h->start + d.guard + d.ncells, tail.data(), tail.size() * 4, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemsetAsync(h->count, 0, (size_t)d.ncells * 4, h->stream));
    return WS_OK;
}

// Does the reference's N-bucket table put two cells of one 27-stencil into the same bucket?  Then a neighbour
// is visited once per aliasing stencil cell (the reference counts it that often) and the kernels take the
// multiplicity path (`alias`).  Power-of-two N: hash_cell is linear mod N, the multiplicity depends on the
// cell difference only and is tabulated here.  Any other N: `% N` follows a wrap mod 2^32, so two stencil cells
// whose linear forms differ by delta can alias iff delta, delta - 2^32 or delta + 2^32 is a multiple of N (which
// of them applies depends on the cell); if none of the 27 x 26 differences qualifies no particle can ever see an
// aliased bucket, otherwise the kernels count the aliasing offsets per pair (alias_mult).
ws_status upload_mult(ws_handle *h)
{
    uint8_t m[27];
    bool alias = false;
    const uint32_t n = h->dev.hash_n;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dz = -1; dz <= 1; dz++) {
                uint32_t cnt = 0;
                for (int ox = -1; ox <= 1; ox++)
                    for (int oy = -1; oy <= 1; oy++)
                        for (int oz = -1; oz <= 1; oz++) {
                            if (is_pow2(n)) {
                                if (ref_hash_delta(ox, oy, oz, n) == ref_hash_delta(dx, dy, dz, n)) cnt++;
                                continue;
                            }
                            if (ox == dx && oy == dy && oz == dz) {
                                cnt++;
                                continue;
                            }
                            const int64_t delta = (int64_t)ref_linear(ox, oy, oz) - (int64_t)ref_linear(dx, dy, dz);
                            for (int64_t k = -1; k <= 1; k++)
                                if ((delta + k * ((int64_t)1 << 32)) % (int64_t)n == 0) alias = true;
                        }
                if (cnt > 1) alias = true;
                m[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] = (uint8_t)(cnt ? cnt : 1);
            }
    h->alias = alias;
    if (!h->mult) {
        const ws_status st = h->fixed.alloc(h, &h->mult, 32, "stencil multiplicities");
        if (st) return st;
    }
    HIP_TRY(h, copy_now(h, h->mult, m, 27, hipMemcpyHostToDevice));
    return WS_OK;
}

// kernel family and pair arithmetic of a new handle (flags already set)
void configure_kernels(ws_handle *h)
{
    if (const char *v = WS_DEV_ENV("WS_VARIANT")) h->variant = strcmp(v, "simple") == 0 ? WS_VARIANT_SIMPLE : WS_VARIANT_LISTED;
    h->ieee = (h->flags & WS_FLAG_IEEE_DIVISION) != 0;
}

// The staging buffer of uploads and readbacks, at least `bytes` large.  ws_handle::stage is what the calls read and write:
// the alias of stage_mem.p, refreshed here, the one place that grows it.
ws_status ensure_stage(ws_handle *h, size_t bytes)
{
    const ws_status st = h->stage_mem.grow(h, bytes, "staging buffer");
    h->stage = h->stage_mem.p;
    return st;
}

// A handle whose re-grid failed after the old tables were given up (h->dead; ws_set_params, slab_regrid): its cell
// tables, sorted arrays or -- on a slab -- its particle set are missing or half rebuilt.  EVERY entry point that would
// launch over them, or enter a collective its peers may skip, refuses with the reason instead (only ws_step
// did; a frame loop reads before it steps).  What still works: ws_destroy, ws_last_error, ws_ready, the profile and
// statistics getters, and ws_read_positions_end / _view of a readback that had completed.
#define WS_DEAD_CHECK(h)                                               \
    do {                                                               \
        if ((h)->dead) return fail((h), WS_ERR_HIP, (h)->err.c_str()); \
    } while (0)

// the refusal of the reference-order validation mode, by the calls that have no literal six-pass form (`tag` leads it)
ws_status reference_order_refused(ws_handle *h, const char *tag)
{
    return fail(h, WS_ERR_UNSUPPORTED, (std::string(tag) + ": not in the reference-order validation mode").c_str());
}

// What a call between two steps refuses before it looks at its arguments, in this order: a NULL handle, a dead one, the
// reference-order validation mode; then the handle's device is made current.
ws_status enter(ws_handle *h, const char *tag)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    if (h->flags & WS_FLAG_REFERENCE_ORDER) return reference_order_refused(h, tag);
    HIP_TRY(h, hipSetDevice(h->device));
    return WS_OK;
}

// The test-only build also contains a validation mode that runs the reference's six passes literally
// (tests/refcheck/): its handles are handed over at the top of every entry point.  Nothing of it exists in the product.
#ifdef WS_WITH_REFCHECK
#include "ws_refcheck_host.inc"
#define WS_REF_DISPATCH(h, call)       \
    do {                               \
        if ((h)->refmode) return call; \
    } while (0)
#else
#define WS_REF_DISPATCH(h, call) ((void)0)
#endif

// ---- profiling ---------------------------------------------------------------------
hipEvent_t get_event(ws_handle *h)
{
    if (!h->pool.empty()) {
        hipEvent_t e = h->pool.back();
        h->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;  // the bracket is then skipped, the step is not
    return e;
}

struct Prof {
    ws_handle *h;
    bool on;
    WsEventPair p{};
    Prof(ws_handle *h_, uint32_t k) : h(h_), on((h_->flags & WS_FLAG_PROFILE) != 0 && ((h_->prof_mask >> k) & 1u))
    {
        if (!on) return;
        p.kernel = k;
        p.a = get_event(h);
        p.b = get_event(h);
        if (!p.a || !p.b || hipEventRecord(p.a, h->stream) != hipSuccess) {  // out of events: time nothing, run everything
            if (p.a) h->pool.push_back(p.a);
            if (p.b) h->pool.push_back(p.b);
            on = false;
        }
    }
    ~Prof()
    {
        if (!on) return;
        if (hipEventRecord(p.b, h->stream) == hipSuccess) {
            h->pending.push_back(p);
        } else {
            h->pool.push_back(p.a);
            h->pool.push_back(p.b);
        }
    }
};

// The same for ONE kernel launch: the pair goes to the launch (hipExtLaunchKernelGGL start / stop events) instead of
// being recorded around it.  The pair is queued for reading only if a launch actually took it (events()); otherwise
// it goes back to the pool -- a pair no launch has stamped would read as the elapsed time of an earlier use.
struct ProfLaunch {
    ws_handle *h;
    bool on, taken = false;
    WsEventPair p{};
    ProfLaunch(ws_handle *h_, uint32_t k, bool counts = true)
        : h(h_), on((h_->flags & WS_FLAG_PROFILE) != 0 && ((h_->prof_mask >> k) & 1u))
    {
        if (!on) return;
        p.kernel = k;
        p.counts = counts;
        p.a = get_event(h);
        p.b = get_event(h);
        if (!p.a || !p.b) {
            if (p.a) h->pool.push_back(p.a);
            if (p.b) h->pool.push_back(p.b);
            on = false;
        }
    }
    // called by the launcher at the moment it launches
    const WsEventPair *events()
    {
        if (!on) return nullptr;
        taken = true;
        return &p;
    }
    ~ProfLaunch()
    {
        if (!on) return;
        if (taken) {
            h->pending.push_back(p);
        } else {
            h->pool.push_back(p.a);
            h->pool.push_back(p.b);
        }
    }
};

void drain_profile(ws_handle *h)
{
    for (auto &p : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            h->prof_ms[p.kernel] += ms;
            h->prof_cnt[p.kernel] += p.counts ? 1 : 0;
        }
        h->pool.push_back(p.a);
        h->pool.push_back(p.b);
    }
    h->pending.clear();
}

// WS_FLAG_PROFILE with a host that never calls ws_sync: read the event pairs back before the list (and the event
// pool behind it) grows without bound.  Profile mode only; costs one stream synchronisation per 4096 pairs.
void bound_pending(ws_handle *h)
{
    if (h->pending.size() < 4096) return;
    if (hipStreamSynchronize(h->stream) == hipSuccess) drain_profile(h);
}

// The tile schedule of a single-GPU handle's K4 / K5 (WsSched, ws_internal.h): split / perm / cost per kernel in two
// sets, a stream and two events for k_schedule.  Built once here with no costs known: equal shares, tiles in their own
// order.  Only handles of WS_SCHED_MIN_PARTICLES <= n < WS_SCHED_END_PARTICLES take it (profiles/r05/sched/; the
// range re-measured on the round's final kernels: sched_range_final_kernels.log):
//   * there (C2: 262 144 particles; 2^19) a neighbour kernel is one or two rounds of workgroups -- most of the grid is
//     resident at once -- so it lasts as long as its slowest workgroup lives, and starting the expensive tiles first is
//     worth 10-19 % of K4 and 5-15 % of K5 (step -7.6 % settled at C2, -7 % at 2^19, -5 % sparse);
//   * below (the reference's own 65 536 particles: +12 %; 2^17: K4 -8 %, K5 -3 %, step +4 %) the step is launch-bound and
//     the extra launch with its two cross-stream events costs 5-8 us of a 75-110 us step;
//   * above (2^20 settled: K5 +8 %, step +3.8 %; 2^21: +6 %; C3, C4) an XCD works through many rounds, the equal static
//     shares are within 4 % of balanced, and every reordering of the tiles costs more in L2 locality than the shorter
//     drain returns (K5 +4 ... +13 %).  (2^20 in the sparse state would still gain 4 %: the settled state decides.)
#define WS_SCHED_MIN_PARTICLES (1u << 18)
#define WS_SCHED_END_PARTICLES (1u << 20)

void free_schedule(ws_handle *h)
{
    if (h->sched_stream) {
        hipStreamSynchronize(h->sched_stream);
        hipStreamDestroy(h->sched_stream);
    }
    if (h->ev_sched_in) hipEventDestroy(h->ev_sched_in);
    if (h->ev_sched_out) hipEventDestroy(h->ev_sched_out);
    h->sched.release();
    h->sched4[1].cost = nullptr;  // (the alias of sched4[0].cost)
    h->sched_stream = nullptr;
    h->ev_sched_in = h->ev_sched_out = nullptr;
    h->sched_on = false;
}

ws_status alloc_schedule(ws_handle *h)
{
    if (h->variant != WS_VARIANT_LISTED || h->slab) return WS_OK;
    uint32_t min_n = WS_SCHED_MIN_PARTICLES, max_n = WS_SCHED_END_PARTICLES - 1u;
    if (const char *v = WS_DEV_ENV("WS_TILE_SCHEDULE")) {  // developer builds: 0 = never, 1 = at every size (A/B runs)
        min_n = 0;
        max_n = atoi(v) ? 0xFFFFFFFFu : 0u;
    }
    if (h->n > max_n || h->n < min_n) return WS_OK;
    if (const char *v = WS_DEV_ENV("WS_SCHED_CLASSES")) h->sched_classes = (uint32_t)atoi(v);
    if (const char *v = WS_DEV_ENV("WS_SCHED_GROUP")) h->sched_group = (uint32_t)atoi(v);
    h->sched_tiles4 = (h->n + wsk_density_tile() - 1u) / wsk_density_tile();
    h->sched_tiles5 = (h->n + wsk_force_tile(h->n) - 1u) / wsk_force_tile(h->n);
    const size_t t4 = (size_t)h->sched_tiles4 * 4, t5 = (size_t)h->sched_tiles5 * 4;
    WsGroup &G = h->sched;
    // K4's two sets share one cost array, owned once (through set 0); the costs start at zero
    ws_status st = G.alloc(h, &h->sched4[0].cost, t4, "tile costs", true);
    h->sched4[1].cost = h->sched4[0].cost;
    for (int k = 0; k < 2 && !st; k++) {
        st = G.alloc(h, &h->sched4[k].split, 16 * 4, "tile schedule");
        if (!st) st = G.alloc(h, &h->sched4[k].perm, t4, "tile schedule");
        if (!st) st = G.alloc(h, &h->sched5[k].split, 16 * 4, "tile schedule");
        if (!st) st = G.alloc(h, &h->sched5[k].perm, t5, "tile schedule");
        if (!st) st = G.alloc(h, &h->sched5[k].cost, t5, "tile costs", true);
    }
    if (st) return st;
    HIP_TRY(h, hipStreamCreateWithFlags(&h->sched_stream, hipStreamNonBlocking));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sched_in, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sched_out, hipEventDisableTiming));
    for (int k = 0; k < 2; k++)  // (costs all unknown: both sets come out as the equal shares)
        wsk_schedule(h->stream, h->sched4[k], h->sched_tiles4, h->sched5[k], h->sched5[k], h->sched_tiles5, h->sched_classes, h->sched_group,
                     wsk_force_tile(h->n));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sched_parity = 0;
    h->sched_on = true;
    return WS_OK;
}

// The single-GPU step: scan -> scatter -> reorder -> K4 -> K5+K6+K1'.  Enqueued directly or captured.
void enqueue_step(ws_handle *h)
{
    const WsDev &d = h->dev;
    hipStream_t s = h->stream;
    // (not in a captured step: k_schedule joins the NEXT step, and the two sets alternate -- a replayed graph has one baked in)
    const bool sched = h->sched_on && !h->alias && h->variant == WS_VARIANT_LISTED && !(h->flags & WS_FLAG_GRAPH);
    const uint32_t par = h->sched_parity;
    {
        Prof p(h, WS_K_SCAN);
        // no fill cursors: particles are placed by the ranks they drew when they were binned
        wsk_scan(s, h->count, h->start + d.guard, nullptr, h->bsum, d.ncells, true, 0);
    }
    {
        Prof p(h, WS_K_SCATTER);
        wsk_place(s, d, h->cid_cur, h->cur.rank, h->start, h->slot_tmp);
    }
    {
        Prof p(h, WS_K_REORDER);
        wsk_reorder(s, d, h->slot_tmp, h->cid_cur, h->start, h->cur, h->srt, h->cid_srt, h->sxyz, h->pred_stale);
    }
    if (sched) hipStreamWaitEvent(s, h->ev_sched_out, 0);  // (the previous step's k_schedule: long done; nothing before the first)
    {
        // one launch each: timed by events the launch itself carries (no event packets between the kernels)
        ProfLaunch p(h, WS_K_DENSITY);
        wsk_density(s, d, h->start, h->cid_srt, h->srt, h->mult, h->alias, h->variant, h->ieee, h->stats, h->mask, h->sxyz,
                    p.events(), sched ? h->sched4[par] : WsSched{});
    }
    if (sched) {
        // next step's schedule, beside this step's K5 (16 workgroups; K5 is not bound by what they need): from the costs
        // K4 has just measured and the ones the PREVIOUS step's K5 left in the other set
        hipEventRecord(h->ev_sched_in, s);
        hipStreamWaitEvent(h->sched_stream, h->ev_sched_in, 0);
        wsk_schedule(h->sched_stream, h->sched4[par ^ 1u], h->sched_tiles4, h->sched5[par ^ 1u], h->sched5[par ^ 1u], h->sched_tiles5,
                     h->sched_classes, h->sched_group, wsk_force_tile(h->n));
        hipEventRecord(h->ev_sched_out, h->sched_stream);
        h->sched_parity = par ^ 1u;
    }
    {
        ProfLaunch p(h, WS_K_FORCE);
        wsk_force(s, d, h->start, h->cid_srt, h->srt, h->cur, h->accel, h->cid_cur, h->count, h->mult, h->alias,
                  h->variant, h->ieee, h->mask, false, p.events(), sched ? h->sched5[par] : WsSched{});
    }
    h->pred_stale = true;   // the epilogue stores position and velocity only (k_reorder)
    h->accel_stale = true;  // ... and no accelerations (refresh_accel)
}

// The record views report pressure = f(density) (simulation.wgsl:192-193) without storing it: what f was when the step
// about to be enqueued computes its densities.  ws_set_params between that step and a read must not leak into the view.
void note_step_params(ws_handle *h)
{
    h->last_pressure = {h->dev.pressure_scalar, h->dev.target_density, h->dev.near_pressure_scalar};
}

// cur.pred is not maintained by the step loop (k_reorder recomputes it): bring it up to date for a reader off the loop
void refresh_pred(ws_handle *h, const WsDev &d)
{
    if (!h->pred_stale) return;
    wsk_refresh_pred(h->stream, d, h->cur);
    h->pred_stale = false;
}

// The accelerations of the last step, for the 80-byte record views: the force kernel once more over the sorted state
// that step left behind (cell table, sorted records with densities, accept masks: all intact until the next step
// starts), storing nothing but accel[].  Not profiled: it is not part of a step.
ws_status refresh_accel(ws_handle *h)
{
    if (!h->accel_stale) return WS_OK;
    WsDev d = h->dev;
    auto pass = [&](const WsDev &dd) {
        if (dd.n)
            wsk_force(h->stream, dd, h->start, h->cid_srt, h->srt, h->cur, h->accel, h->cid_cur, h->count, h->mult, h->alias,
                      h->variant, h->ieee, h->mask, true);
    };
    if (h->slab) {
        const WsSlab *S = h->slab;
        d.dyn = S->dyn;
        d.n = S->cap;  // upper bound; the kernel reads the owned count from the device
        if (S->last_split) {
            // the step ran K4 / K5 as an early and a late launch, and the early ones number their candidates on runs cut
            // to the owned range (ws_kernels.hip ws_cut): walk the same masks the same way
            d.range_sel = WS_RANGE_EARLY;
            pass(d);
            d.range_sel = d.has_left && d.has_right ? WS_RANGE_LATE_BOTH : d.has_left ? WS_RANGE_LATE_LEFT : WS_RANGE_LATE_RIGHT;
            d.n = (uint32_t)std::min<uint64_t>(S->cap, 2ull * S->halo_cap);
            pass(d);
        } else {
            d.range_sel = WS_RANGE_ALL;
            pass(d);
        }
    } else {
        pass(d);
    }
    HIP_TRY(h, hipGetLastError());
    h->accel_stale = false;
    return WS_OK;
}

// Put `cur` (freshly uploaded, or the current state after a re-grid) into the "binned" state every ws_step starts from.
ws_status bin_current(ws_handle *h)
{
    refresh_pred(h, h->dev);
    HIP_TRY(h, hipMemsetAsync(h->count, 0, (size_t)h->dev.ncells * 4, h->stream));
    {
        Prof pr(h, WS_K_BIN);
        wsk_bin(h->stream, h->dev, h->cur, h->cid_cur, h->count);
    }
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

ws_status upload_positions(ws_handle *h, const float *pos_xyz)
{
    const size_t bytes = (size_t)h->n * 12;
    ws_status st = ensure_stage(h, bytes);
    if (st) return st;
    HIP_TRY(h, hipMemcpyAsync(h->stage, pos_xyz, bytes, hipMemcpyHostToDevice, h->stream));
    wsk_upload_positions(h->stream, (const float *)h->stage, h->cur, h->n);
    HIP_TRY(h, hipGetLastError());
    h->pred_stale = false;
    h->accel_stale = false;  // no step yet: the views report zero acceleration
    st = bin_current(h);
    if (st) return st;
    // the caller's buffer must not be referenced after return
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->steps = 0;
    h->have_step = false;
    h->last_pressure = {};
    return WS_OK;
}

// captured steps hold kernel arguments by value (WsDev) and array pointers: anything that changes either drops them
void drop_graphs(ws_handle *h)
{
    if (h->graph_exec) hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
    if (h->slab) slab_drop_graphs(h->slab);
}

// The particle arrays of a handle: `slots` particle slots (n on a single handle; ghosts | capacity | ghosts on a slab), and
// accept masks of `mask_particles` particles per row (n; on a slab the owned capacity: ghosts have no masks).
ws_status alloc_particle_arrays(ws_handle *h, size_t slots, uint32_t mask_particles)
{
    // +16 entries: phase 1 trips read up to U-1 slots past a run's end (masked, but must be mapped)
    const size_t n16 = (slots + 16) * 16, n4 = slots * 4;
    WsGroup &G = h->particles;
    ws_status st = G.alloc(h, &h->cur.pv, 2 * n16, "particle records");
    if (!st) st = G.alloc(h, &h->cur.pred, n16, "predicted positions");
    if (!st) st = G.alloc(h, &h->cur.rank, n4, "cell ranks");
    if (!st) st = G.alloc(h, &h->srt.pos, n16, "sorted positions");
    if (!st) st = G.alloc(h, &h->srt.pv, 2 * n16, "sorted records");
    for (float **plane : {&h->sxyz.x, &h->sxyz.y, &h->sxyz.z})
        if (!st) st = G.alloc(h, plane, n16 / 4, "sorted position planes", true);
    if (!st) st = G.alloc(h, &h->cid_cur, n4, "cell ids");
    if (!st) st = G.alloc(h, &h->cid_srt, n4, "sorted cell ids");
    if (!st) st = G.alloc(h, &h->accel, n16, "accelerations");
    if (!st) st = G.alloc(h, &h->slot_tmp, n4, "sort slots");
    if (!st && h->variant == WS_VARIANT_LISTED) {
        h->mask.stride = mask_particles;
        st = G.alloc(h, &h->mask.words, (size_t)wsk_mask_words() * mask_particles * 4, "accept masks");
    }
    return st;
}

void free_particle_arrays(ws_handle *h)
{
    drop_graphs(h);
    h->particles.release();
    h->mask.stride = 0;
}

// A single-GPU handle's particle arrays at a larger capacity, every byte of the old ones carried over: the state, the
// binned state and the last step's sorted copy, masks and accelerations all stay what they were (ws_reserve_particles, an
// addition beyond the capacity).  The new arrays are allocated FIRST: a failure leaves the handle as it was.  The copies
// go by the order in which alloc_particle_arrays allocates (WsGroup::fields keeps it); the accept masks are rows of
// `stride` words and move row by row.  Captured steps hold the old pointers and are dropped.
ws_status grow_particle_arrays(ws_handle *h, uint32_t cap)
{
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->sched_stream) HIP_TRY(h, hipStreamSynchronize(h->sched_stream));
    const uint32_t old_stride = h->mask.stride;
    const size_t o16 = ((size_t)h->cap + 16) * 16, o4 = (size_t)h->cap * 4;
    // (alloc_particle_arrays' sizes, in its order; the masks follow)
    const size_t old_bytes[12] = {2 * o16, o16, o4, o16, 2 * o16, o16 / 4, o16 / 4, o16 / 4, o4, o4, o16, o4};
    const bool masks = h->variant == WS_VARIANT_LISTED;
    if (h->particles.fields.size() != 12u + (masks ? 1u : 0u)) return fail(h, WS_ERR_HIP, "particle arrays: unexpected layout");
    WsGroup::Held held = h->particles.take();
    ws_status st = alloc_particle_arrays(h, cap, cap);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < 12 && !st && e == hipSuccess; i++)
        e = hipMemcpyAsync(*held.fields[i], held.bufs[i], old_bytes[i], hipMemcpyDeviceToDevice, h->stream);
    if (!st && e == hipSuccess && masks)
        e = hipMemcpy2DAsync(h->mask.words, (size_t)cap * 4, held.bufs[12], (size_t)old_stride * 4, (size_t)old_stride * 4,
                             wsk_mask_words(), hipMemcpyDeviceToDevice, h->stream);
    if (!st && e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (!st && e != hipSuccess) st = fail(h, WS_ERR_HIP, "particle arrays: copy into the larger arrays", e);
    if (st) {  // the new arrays go, the old ones are the handle's again
        h->particles.restore(held);
        h->mask.stride = old_stride;
        return st;
    }
    drop_graphs(h);
    WsGroup::drop(held);
    h->cap = cap;
    return WS_OK;
}

void free_all(ws_handle *h)
{
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->copy_stream) {
        hipStreamSynchronize(h->copy_stream);
        hipStreamDestroy(h->copy_stream);
    }
    free_schedule(h);
    if (h->rb_gathered) hipEventDestroy(h->rb_gathered);
    if (h->rb_done) hipEventDestroy(h->rb_done);
    release_all(h->rb_stage, h->rb_host[0], h->rb_host[1]);
    drain_profile(h);
    for (auto e : h->pool) hipEventDestroy(e);
    free_grid(h);
    free_particle_arrays(h);
    release_all(h->fixed, h->stage_mem, h->force_cnt, h->solid_sums, h->v_keys, h->v_perm, h->v_tmp, h->v_count, h->v_cursor, h->v_start, h->v_bsum,
                h->v_off, h->pop_words, h->gauge_out, h->gauge_ids);
    for (auto &volume : h->volume) release_all(volume);
    release_all(h->attr);
    free_field(h);
#ifdef WS_WITH_REFCHECK
    ref_free(h);
#endif
    slab_free(h);
    if (h->done) hipEventDestroy(h->done);
    if (h->stream && h->own_stream) hipStreamDestroy(h->stream);
}

}  // namespace

// ======================================================================================
// host-side functions of the path
// ======================================================================================
extern "C" {

uint32_t ws_abi_version(void) { return WS_ABI_VERSION; }

const char *ws_status_string(ws_status s)
{
    switch (s) {
        case WS_OK: return "ok";
        case WS_ERR_INVALID_ARG: return "invalid argument";
        case WS_ERR_NO_DEVICE: return "no usable gfx950 device";
        case WS_ERR_OUT_OF_MEMORY: return "out of device memory";
        case WS_ERR_HIP: return "HIP runtime error";
        case WS_ERR_COMM: return "RCCL communication error";
        case WS_ERR_UNSUPPORTED: return "unsupported";
        case WS_ERR_NOT_READY: return "not ready";
    }
    return "unknown status";
}

const char *ws_kernel_name(uint32_t k)
{
    static const char *names[WS_K_COUNT] = {"cell_scan", "cell_scatter", "reorder", "density", "force_integrate_bin",
                                            "bin"};
    return k < WS_K_COUNT ? names[k] : "?";
}

// src/fluid_compute.rs:20-27,:67-79; src/gravity.rs:6,:29-33; src/fluid_container.rs:8-9
ws_status ws_default_params(ws_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->delta_time = 1.0f / 60.0f;
    out->collision_damping = 0.95f;
    out->smoothing_radius = 0.25f;
    out->target_density = 10.0f;
    out->pressure_scalar = 22.0f;
    out->near_pressure_scalar = 2.0f;
    out->viscosity_strength = 0.1f;
    out->gravity[1] = -9.8f;
    const float position[3] = {0.f, 0.f, 0.f}, size[3] = {16.f, 9.f, 9.f};
    return ws_get_ext(position, size, 0.1f, out->ext_min, out->ext_max);
}

// src/fluid_compute.rs:55-63
ws_status ws_get_smoothing_kernel(const ws_params *p, ws_smoothing_kernel *out)
{
    if (!p || !out) return WS_ERR_INVALID_ARG;
    const float PI = 3.14159265358979323846f;  // std::f32::consts::PI
    const float h = p->smoothing_radius;
    out->pow2 = 15.0f / (2.0f * PI * powi_f32(h, 5));
    out->pow2_der = 15.0f / (PI * powi_f32(h, 5));
    out->pow3 = 15.0f / (PI * powi_f32(h, 6));
    out->pow3_der = 45.0f / (PI * powi_f32(h, 6));
    out->spikey_pow3 = 315.0f / (64.0f * PI * powi_f32(h, 9));
    return WS_OK;
}

// src/helpers.rs:3-20
ws_status ws_cube_fluid(uint32_t ni, uint32_t nj, uint32_t nk, float r, float *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    const float ox = r - (float)ni * r, oy = r - (float)nj * r, oz = r - (float)nk * r;
    const float diam = r * 2.0f;
    size_t o = 0;
    for (uint32_t i = 0; i < ni; i++)
        for (uint32_t j = 0; j < nj; j++)
            for (uint32_t k = 0; k < nk; k++) {
                out[o++] = (float)i * diam + ox;
                out[o++] = (float)j * diam + oy;
                out[o++] = (float)k * diam + oz;
            }
    return WS_OK;
}

// src/fluid_container.rs:42-50
ws_status ws_get_ext(const float position[3], const float size[3], float padding, float ext_min[4], float ext_max[4])
{
    if (!position || !size || !ext_min || !ext_max) return WS_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++) {
        const float half = size[c] / 2.0f;
        ext_min[c] = (position[c] - half) + padding;
        ext_max[c] = (position[c] + half) - padding;
    }
    ext_min[3] = ext_max[3] = 0.0f;
    return WS_OK;
}

// src/fluid_compute.rs:251-273
uint32_t ws_bit_sorter_stage_count(uint32_t data_length)
{
    uint32_t k = 0;
    uint64_t p = 1;
    while (p < data_length) {
        p <<= 1;
        k++;
    }
    return k * (k + 1) / 2;
}

// ======================================================================================
// lifetime
// ======================================================================================
ws_status ws_create(const ws_params *params, const float *pos_xyz, uint32_t n, const ws_device_cfg *cfg,
                    ws_handle **out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    *out = nullptr;
    if (!pos_xyz || n == 0) return fail(nullptr, WS_ERR_INVALID_ARG, "pos_xyz is NULL or n == 0");
    if (n > WS_MAX_SLOTS - 16u) return fail(nullptr, WS_ERR_INVALID_ARG, "more than 2^27 particles on one device");
    ws_status st = validate_params(nullptr, params);
    if (st) return st;
    if (cfg && cfg->world_size > 1) return fail(nullptr, WS_ERR_UNSUPPORTED, "multi-GPU slabs are created with ws_slab_create");
#ifndef WS_WITH_REFCHECK
    if (cfg && (cfg->flags & WS_FLAG_REFERENCE_ORDER))
        return fail(nullptr, WS_ERR_UNSUPPORTED,
                    "WS_FLAG_REFERENCE_ORDER is a validation mode of the test-only build (tests/libwsfluid_refcheck.so)");
#endif

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, WS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    const int device = cfg ? cfg->device : 0;
    if (device < 0 || device >= ndev) return fail(nullptr, WS_ERR_NO_DEVICE, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, WS_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, WS_ERR_NO_DEVICE, "device is not gfx950 (kernels are built for MI355X only)");

    ws_handle *h = new (std::nothrow) ws_handle();
    if (!h) return fail(nullptr, WS_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->device = device;
    h->flags = cfg ? cfg->flags : 0;
    h->n = n;
    h->cap = n;
    h->params = *params;
    configure_kernels(h);
    if (h->flags & WS_FLAG_GRAPH) h->flags &= ~(uint32_t)WS_FLAG_PROFILE;  // event brackets are not part of a captured step

    auto bail = [&](ws_status s) {
        g_create_error = h->err;
        free_all(h);
        delete h;
        return s;
    };

    CREATE_HIP(hipSetDevice(device));
    CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CREATE_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
    CREATE_TRY(derive_dev(h, *params, n, &h->dev));
#ifdef WS_WITH_REFCHECK
    if (h->flags & WS_FLAG_REFERENCE_ORDER) {
        CREATE_TRY(ref_alloc(h));
        CREATE_TRY(ref_upload_positions(h, pos_xyz));
        *out = h;
        return WS_OK;
    }
#endif
    CREATE_TRY(alloc_particle_arrays(h, n, n));
    CREATE_TRY(h->fixed.alloc(h, &h->stats, 64, "device counters", true));
    CREATE_TRY(alloc_grid(h));
    CREATE_TRY(upload_mult(h));
    CREATE_TRY(upload_positions(h, pos_xyz));
    CREATE_TRY(alloc_schedule(h));
    *out = h;
    return WS_OK;
}

ws_status ws_destroy(ws_handle *h)
{
    if (!h) return WS_OK;
    hipSetDevice(h->device);
    free_all(h);
    delete h;
    return WS_OK;
}

const char *ws_last_error(ws_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }
uint32_t ws_num_particles(ws_handle *h) { return h ? h->n : 0; }
uint64_t ws_steps_done(ws_handle *h) { return h ? h->steps : 0; }

// ======================================================================================
// per frame
// ======================================================================================
ws_status ws_step(ws_handle *h)
{
    if (!h) return WS_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) return slab_step(h);
    WS_REF_DISPATCH(h, ref_step(h));
    if (h->dead) return fail(h, WS_ERR_HIP, h->err.c_str());
    hipStream_t s = h->stream;
    bound_pending(h);
    note_step_params(h);
    // WS_FLAG_GRAPH: the five launches as one captured graph (the reference replays its pass graph the same way,
    // src/fluid_compute.rs:309-363,:396).  Off by default: measured no faster than the direct launches, which already
    // pipeline on the stream (round 1: C1 0.061 vs 0.055 ms/step, C2 0.107 vs 0.100, C3 equal; round 3: DESIGN.md).
    // The first step after an upload takes the caller's predicted positions (k_reorder<false>) and is launched directly.
    if ((h->flags & WS_FLAG_GRAPH) && !h->graph_failed && h->pred_stale) {
        if (!h->graph_exec) {
            hipGraph_t gr = nullptr;
            // (relaxed mode: a host may drive several handles from several threads -- in-process slabs, or simply two fluids --
            // and in the other modes one thread's capture makes ANOTHER thread's legacy-stream hipMemcpy fail with
            // hipErrorStreamCaptureImplicit; this thread itself issues nothing but launches, events and async copies here)
            hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
            if (e == hipSuccess) {
                enqueue_step(h);
                e = hipStreamEndCapture(s, &gr);
                if (e == hipSuccess) e = hipGraphInstantiate(&h->graph_exec, gr, nullptr, nullptr, 0);
                if (gr) hipGraphDestroy(gr);
            }
            if (e != hipSuccess || !h->graph_exec) {
                (void)hipGetLastError();
                h->graph_failed = true;
                h->graph_exec = nullptr;
                h->err = std::string("WS_FLAG_GRAPH: capture failed (") + hipGetErrorName(e) + "), using direct launches";
            }
        }
        if (h->graph_exec) {
            HIP_TRY(h, hipGraphLaunch(h->graph_exec, s));
            h->pred_stale = true;
            h->accel_stale = true;
            h->graph_steps++;
            HIP_TRY(h, hipEventRecord(h->done, s));
            h->done_recorded = true;
            h->steps++;
            h->have_step = true;
            return WS_OK;
        }
    }
    enqueue_step(h);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->done, s));
    h->done_recorded = true;
    h->steps++;
    h->have_step = true;
    return WS_OK;
}

ws_status ws_ready(ws_handle *h, int *ready)
{
    if (!h || !ready) return WS_ERR_INVALID_ARG;
    if (!h->done_recorded) {
        *ready = 1;
        return WS_OK;
    }
    const hipError_t e = hipEventQuery(h->done);
    if (e == hipSuccess)
        *ready = 1;
    else if (e == hipErrorNotReady)
        *ready = 0;
    else
        return fail(h, WS_ERR_HIP, "hipEventQuery", e);
    return WS_OK;
}

ws_status ws_sync(ws_handle *h)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) {  // also the communication stream, and the device-side error bits of every rank seen so far
        const ws_status st = slab_settle(h);
        drain_profile(h);
        return st;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

ws_status ws_set_params(ws_handle *h, const ws_params *params)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    ws_status st = validate_params(h, params);
    if (st) return st;
    HIP_TRY(h, hipSetDevice(h->device));
    WsDev nd;
    st = derive_dev(h, *params, h->slab ? h->slab->n_global : h->n, &nd);  // (the cell budget follows the GLOBAL count)
    if (st) return st;
    const WsDev &od = h->dev;
    bool regrid = memcmp(nd.org, od.org, sizeof nd.org) || memcmp(nd.dim, od.dim, sizeof nd.dim) || nd.h != od.h;
    if (h->slab) {
        // keep the slab's local grid; only the global y/z extents and the radius can be compared
        regrid = nd.h != od.h || nd.dim[1] != od.dim[1] || nd.dim[2] != od.dim[2] || nd.dim[0] != od.gdim_x ||
                 memcmp(nd.org, od.org, sizeof nd.org);
        nd.dim[0] = od.dim[0]; nd.gdim_x = od.gdim_x; nd.xoff = od.xoff; nd.ncells = od.ncells; nd.guard = od.guard;
        nd.base = od.base; nd.n = od.n; nd.hash_n = od.hash_n;
        nd.has_left = od.has_left; nd.has_right = od.has_right; nd.mig = od.mig;
        memcpy(nd.lidx, od.lidx, sizeof nd.lidx);
    }
    WS_REF_DISPATCH(h, ref_set_params(h, params, nd));
    // (slab handles: COLLECTIVE when the cell size or the container changes -- every rank must make the same call)
    if (h->slab && regrid) return slab_regrid(h, params, false);
    // The last step's accelerations are computed on demand from the state and the parameters that step used: if a
    // parameter they depend on changes (or the grid goes away), compute them now.  (A host that pushes unchanged
    // parameters every frame, as the reference's update() does, pays nothing.)
    const bool accel_params_changed =
        nd.h != od.h || nd.target_density != od.target_density || nd.pressure_scalar != od.pressure_scalar ||
        nd.near_pressure_scalar != od.near_pressure_scalar || nd.viscosity != od.viscosity || nd.k_pow2_der != od.k_pow2_der ||
        nd.k_pow3_der != od.k_pow3_der || nd.k_spikey != od.k_spikey || nd.d2_accept != od.d2_accept;
    if (regrid || accel_params_changed) {
        st = refresh_accel(h);
        if (st) return st;
    }
    h->params = *params;
    if (!regrid) {
        // (update() pushes the same parameters every frame, src/fluid_compute.rs:479-481: a captured step survives that)
        if (memcmp(&h->dev, &nd, sizeof nd) != 0) {
            drop_graphs(h);
            // new dynamics (a gravity flip can set the whole fluid in motion within a few steps): a slab's messages
            // travel at full capacity until the counts of the new regime have come round (every rank makes this call)
            if (h->slab) h->slab->limit_hold = 8;
        }
        h->dev = nd;  // by-value kernel argument: picked up by the next ws_step
        return WS_OK;
    }
    drop_graphs(h);
    // cell size or container changed: rebuild the grid tables and re-bin the current state
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->dev = nd;
    st = alloc_grid(h);
    if (!st) st = bin_current(h);
    if (st) {
        // the old cell tables are gone and the new ones are not there: no ws_step may launch on this handle again
        h->dead = true;
        h->err = "re-grid failed after the old cell tables were given up (" + h->err + "); the handle is unusable";
    }
    return st;
}

ws_status ws_read_positions(ws_handle *h, float *out_xyz)
{
    if (!h || (!out_xyz && !h->slab)) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) return slab_read_by_id(h, WS_PACK_POS_H, out_xyz);  // collective: all n_global positions, by id
    WS_REF_DISPATCH(h, ref_read_positions(h, out_xyz));
    const size_t bytes = (size_t)h->n * 12;
    ws_status st = ensure_stage(h, bytes);
    if (st) return st;
    wsk_gather_positions(h->stream, h->cur, (float *)h->stage, h->n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_xyz, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

// The frame loop's readback, overlapped with the next step: `begin` enqueues the id-order gather behind the steps
// enqueued so far (a ~65 us kernel on the library's stream) and starts the device->host copy on a separate copy
// stream; steps enqueued after `begin` run while the copy is in flight; `end` waits for the copy alone.
// out_xyz == NULL: into one of two page-locked buffers the library owns, alternately (ws_read_positions_view).
ws_status ws_read_positions_begin(ws_handle *h, float *out_xyz)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    WS_REF_DISPATCH(h, fail(h, WS_ERR_UNSUPPORTED, "no asynchronous readback in the reference-order validation mode"));
    if (h->rb_inflight) return fail(h, WS_ERR_INVALID_ARG, "a readback is already in flight (call ws_read_positions_end)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)(h->slab ? h->slab->n_global : h->n) * 12;
    if (!h->copy_stream) {
        // A stream of another PRIORITY than the step's: the runtime multiplexes the streams of one priority onto a few
        // hardware queues (round-robin, 4 by default), and a copy stream that lands on the step stream's queue puts its
        // wait-for-the-copy barrier in front of the next step's kernels -- copy and step then run in series.  Queues
        // are pooled per priority, so this stream can never share one with the step.
        int lo = 0, hi = 0;
        const char *pr = WS_DEV_ENV("WS_COPY_STREAM_PRIORITY");  // "default" = same priority as the step's stream (A/B runs)
        if (pr && strcmp(pr, "default") == 0) {
            HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        } else {
            HIP_TRY(h, hipDeviceGetStreamPriorityRange(&lo, &hi));  // (numerically lowest = highest priority)
            HIP_TRY(h, hipStreamCreateWithPriority(&h->copy_stream, hipStreamNonBlocking, hi));
        }
        HIP_TRY(h, hipEventCreateWithFlags(&h->rb_gathered, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&h->rb_done, hipEventDisableTiming));
    }
    const bool owned = out_xyz == nullptr;
    if (owned) {
        if (h->rb_host[1].bytes < bytes) {  // (the pair has one size: [1] is allocated last)
            release_all(h->rb_host[0], h->rb_host[1]);
            h->rb_last = -1;
            for (auto &b : h->rb_host) {
                const ws_status st = b.alloc(h, bytes, "page-locked readback buffer");
                if (st) return st;
            }
        }
        h->rb_fill = h->rb_last == 0 ? 1 : 0;  // never the buffer the host may still be reading
        out_xyz = h->rb_host[h->rb_fill].p;
    }
    const float *src;
    if (h->slab) {
        // the collective gather (it settles the enqueued steps: the counts travel through the host), then the copy of
        // the id-ordered result overlaps with the steps enqueued after this call, as on a single handle
        const ws_status st = slab_gather_by_id(h, WS_PACK_POS_H);
        if (st) return st;
        src = reinterpret_cast<const float *>(h->slab->g_out.p);
    } else {
        const ws_status st = h->rb_stage.grow(h, bytes, "readback staging buffer");
        if (st) return st;
        wsk_gather_positions(h->stream, h->cur, h->rb_stage.p, h->n);
        HIP_TRY(h, hipGetLastError());
        src = h->rb_stage.p;
    }
    HIP_TRY(h, hipEventRecord(h->rb_gathered, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, h->rb_gathered, 0));
    // hipMemcpyAsync, i.e. an SDMA engine: it reads HBM and writes PCIe beside the shader's memory path.  (Measured in
    // round 4, profiles/r04/readback: a copy KERNEL storing into the mapped host buffer -- even one of only 64 workgroups
    // -- slows the step's short bandwidth-bound kernels while it runs, k_scan 21 -> 170-560 us, k_place 31 -> 220-590 us;
    // the runtime's own blit kernel, which it substitutes for SDMA whenever a profiler is attached, does the same.)
    HIP_TRY(h, hipMemcpyAsync(out_xyz, src, bytes, hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(h, hipEventRecord(h->rb_done, h->copy_stream));
    h->rb_inflight = true;
    h->rb_owned = owned;
    return WS_OK;
}

ws_status ws_read_positions_end(ws_handle *h)
{
    if (!h) return WS_ERR_INVALID_ARG;
    if (!h->rb_inflight) return fail(h, WS_ERR_INVALID_ARG, "no readback in flight");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(h->rb_done));
    h->rb_inflight = false;
    if (h->rb_owned) h->rb_last = h->rb_fill;
    return WS_OK;
}

ws_status ws_read_positions_view(ws_handle *h, const float **out_xyz)
{
    if (!h || !out_xyz) return WS_ERR_INVALID_ARG;
    *out_xyz = nullptr;
    if (h->rb_last < 0) return fail(h, WS_ERR_INVALID_ARG, "no finished readback into the library's buffers (ws_read_positions_begin(h, NULL) / _end)");
    *out_xyz = h->rb_host[h->rb_last].p;
    return WS_OK;
}

ws_status ws_read_speeds(ws_handle *h, float *out_speed)
{
    if (!h || (!out_speed && !h->slab)) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) return slab_read_by_id(h, WS_PACK_SPEED_H, out_speed);
    WS_REF_DISPATCH(h, ref_read_speeds(h, out_speed));
    const size_t bytes = (size_t)h->n * 4;
    ws_status st = ensure_stage(h, bytes);
    if (st) return st;
    wsk_gather_speeds(h->stream, h->cur, (float *)h->stage, h->n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_speed, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

// The velocities by id, ws_read_positions' companion.  A slab gathers {position, velocity} records (the velocity field's
// one collective) and keeps the velocity half.
ws_status ws_read_velocities(ws_handle *h, float *out_xyz)
{
    if (!h || (!out_xyz && !h->slab)) return WS_ERR_INVALID_ARG;
    ws_status st = enter(h, "velocities");
    if (st) return st;
    const uint32_t n = h->slab ? h->slab->n_global : h->n;
    const size_t bytes = (size_t)n * 12;
    if (h->slab) {
        if ((st = slab_gather_by_id(h, WS_PACK_POSVEL_H))) return st;
        if (out_xyz) {
            if ((st = ensure_stage(h, bytes))) return st;
            wsk_field_split(h->stream, reinterpret_cast<const float *>(h->slab->g_out.p), nullptr, (float *)h->stage, n);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(out_xyz, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return WS_OK;
    }
    if ((st = ensure_stage(h, bytes))) return st;
    wsk_gather_velocities(h->stream, h->cur, (float *)h->stage, n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_xyz, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

// Page-lock / release a host buffer the caller owns and keeps alive (e.g. the Vec update() reads positions
// into every frame): a device->host copy into pinned memory runs at PCIe rate (C3: 0.97 ms for 50 MB) instead
// of through the runtime's pageable staging (9.8 ms).  Explicit on purpose: pinning caller memory behind its
// back is unsafe -- the caller may free it while it is still registered.
ws_status ws_pin_host_buffer(ws_handle *h, void *ptr, uint64_t bytes)
{
    if (!h || !ptr || !bytes) return WS_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
    return WS_OK;
}

ws_status ws_unpin_host_buffer(ws_handle *h, void *ptr)
{
    if (!h || !ptr) return WS_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipHostUnregister(ptr));
    return WS_OK;
}

ws_status ws_read_particles(ws_handle *h, ws_particle80 *out)
{
    if (!h || (!out && !h->slab)) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) return slab_read_by_id(h, WS_PACK_RECORD_H, out);  // collective: all n_global records, by id
    WS_REF_DISPATCH(h, ref_read_particles(h, out));
    const size_t bytes = (size_t)h->n * sizeof(ws_particle80);
    ws_status st = ensure_stage(h, bytes);
    if (st) return st;
    refresh_pred(h, h->dev);
    st = refresh_accel(h);
    if (st) return st;
    wsk_gather_particles(h->stream, h->cur, h->srt, h->accel, h->have_step, h->last_pressure, (ws_particle80 *)h->stage, h->n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

ws_status ws_reset(ws_handle *h, const float *pos_xyz)
{
    if (!h || !pos_xyz) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    // the attributes return to +0 (include/wsfluid.h; an array that was never allocated is all +0 already)
    if (h->attr.p) HIP_TRY(h, hipMemsetAsync(h->attr.p, 0, h->attr.bytes, h->stream));
    if (h->slab) return slab_reset(h, pos_xyz);  // pos_xyz: ALL n_global positions, on every rank
    WS_REF_DISPATCH(h, ref_upload_positions(h, pos_xyz));
    return upload_positions(h, pos_xyz);
}

ws_status ws_write_particles(ws_handle *h, const ws_particle80 *in)
{
    if (!h || !in) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->slab) return slab_write_particles(h, in);  // in: ALL n_global records, on every rank
    WS_REF_DISPATCH(h, ref_load(h, in, false));  // write_slice("particles") leaves the index buffers alone
    const size_t bytes = (size_t)h->n * sizeof(ws_particle80);
    ws_status st = ensure_stage(h, bytes);
    if (st) return st;
    HIP_TRY(h, hipMemcpyAsync(h->stage, in, bytes, hipMemcpyHostToDevice, h->stream));
    wsk_upload_particles(h->stream, (const ws_particle80 *)h->stage, h->cur, h->n);
    HIP_TRY(h, hipGetLastError());
    h->pred_stale = false;  // the caller's predicted positions, as they are
    h->accel_stale = false;
    st = bin_current(h);
    if (st) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->steps = 0;
    h->have_step = false;
    h->last_pressure = {};
    return WS_OK;
}

// ======================================================================================
// acting on the fluid
// ======================================================================================
}  // extern "C"

namespace {

// ws_apply_forces, ws_collide_solids and ws_collide_volumes are one route around three descriptions.  A description
// (ForcesCall, SolidsCall, VolumesCall) carries
//   tag, things     the call and its objects in ws_last_error;
//   refuse()        the argument error, or nullptr; nothing is touched before it has passed;
//   prepare(h, g)   after that: `args`, the kernel's argument, built once, and the output scratch it points to, grown
//                   and zeroed on the handle's stream; an edit that looks at neighbours (CohesionCall) runs its stage
//                   here, on `cur` (g == nullptr) or on the state records a slab handle has gathered (g);
//   mix(m, valid)   the arguments hashed with m(pointer, bytes) for the slabs' agreement -- the objects' bytes only if
//                   `valid`;
//   fetch(h)        the kernel's sums, complete on return.
// The route: a single handle validates, then one streaming pass over `cur` behind the steps enqueued so far leaves the
// edited records and the binned state every ws_step starts from (bin_current's pair: the counts zeroed, then the kernel
// that draws cell ids, counts and ranks).  srt, the accept masks and accel[] are not touched -- the 80-byte view keeps
// the last step's density, pressure and acceleration -- and no array moves, so a captured step is replayed as it is.
// Slab handles gather first and validate in common (slab_edit_gathered, ws_slab.inc).
template <class Call>
ws_status edit_fluid(ws_handle *h, Call &call)
{
    ws_status st = enter(h, call.tag);
    if (st) return st;
    if (h->slab) return slab_edit_gathered(h, call);  // collective: validated after the gather
    if (const char *why = call.refuse()) return fail(h, WS_ERR_INVALID_ARG, why);
    if ((st = call.prepare(h, nullptr))) return st;
    HIP_TRY(h, hipMemsetAsync(h->count, 0, (size_t)h->dev.ncells * 4, h->stream));
    wsk_edit_current(h->stream, h->dev, h->cur, h->cid_cur, h->count, call.args);
    HIP_TRY(h, hipGetLastError());
    h->pred_stale = true;  // cur.pred is behind the edited records: k_reorder<true> / refresh_pred recompute it
    HIP_TRY(h, call.fetch(h));
    return WS_OK;
}

// the argument errors of ws_apply_forces (nullptr = acceptable)
const char *forces_refusal(const ws_force *f, uint32_t k, float dt)
{
    if (!f) return "forces: f is NULL";
    if (k < 1u || k > WS_MAX_FORCES) return "forces: k outside 1 .. WS_MAX_FORCES";
    if (ws_bad_float(dt) || !(dt > 0.f)) return "forces: dt must be finite, > 0 and at most 1e15";
    for (uint32_t e = 0; e < k; e++) {
        if (f[e].kind > WS_FORCE_VORTEX) return "forces: unknown kind";
        if (f[e].reserved[0] || f[e].reserved[1]) return "forces: reserved words must be 0";
        for (int c = 0; c < 3; c++)
            if (ws_bad_float(f[e].centre[c]) || ws_bad_float(f[e].axis[c])) return "forces: centre and axis must be finite and at most 1e15 in magnitude";
        if (ws_bad_float(f[e].strength) || ws_bad_float(f[e].damping)) return "forces: strength and damping must be finite and at most 1e15 in magnitude";
        if (f[e].damping < 0.f) return "forces: damping must be >= 0";
        if (ws_bad_float(f[e].radius) || !(f[e].radius > 0.f)) return "forces: radius must be finite, > 0 and at most 1e15";
    }
    return nullptr;
}

struct ForcesCall {
    const ws_force *f;
    uint32_t k;
    float dt;
    uint32_t *out_affected;
    const char *tag = "forces", *things = "emitters";
    WsForceArgs args{};
    const char *refuse() const { return forces_refusal(f, k, dt); }
    ws_status prepare(ws_handle *h, const WsGathered *)  // (the k per-emitter counters only if the caller asks for them)
    {
        memcpy(args.fs.e, f, (size_t)k * sizeof(ws_force));
        args.k = k;
        args.dt = dt;
        if (!out_affected) return WS_OK;
        const ws_status st = scratch_zeroed(h, h->force_cnt, WS_MAX_FORCES * 4, "force counters");
        args.affected = h->force_cnt.p;
        return st;
    }
    template <class M>
    void mix(M m, bool valid) const
    {
        m(&k, 4);
        m(&dt, 4);
        if (valid) m(f, (size_t)k * sizeof(ws_force));
    }
    hipError_t fetch(ws_handle *h) const
    {
        return out_affected ? copy_now(h, out_affected, h->force_cnt.p, (size_t)k * 4, hipMemcpyDeviceToHost) : hipSuccess;
    }
};

}  // namespace

extern "C" {

ws_status ws_apply_forces(ws_handle *h, const ws_force *f, uint32_t k, float dt, uint32_t *out_affected)
{
    ForcesCall call{f, k, dt, out_affected};
    return edit_fluid(h, call);
}

// ======================================================================================
// surface tension and XSPH: the edit that looks at neighbours (the stage: ws_field.inc)
// ======================================================================================
}  // extern "C"

namespace {

struct CohesionCall {
    const ws_cohesion_params *p;
    float dt;
    uint32_t *out_affected;
    const char *tag = "cohesion", *things = "parameters";
    WsCohesionArgs args{};
    const char *refuse() const { return cohesion_refusal(p, dt); }
    uint32_t partial[WS_COHESION_SLOTS * WS_COHESION_SLOT_WORDS];
    ws_status prepare(ws_handle *h, const WsGathered *g)  // the stage, then the partial counters if the caller asks for the count
    {
        ws_status st = cohesion_prepare(h, g, p, dt, &args);
        if (st || !out_affected) return st;
        st = scratch_zeroed(h, h->force_cnt, sizeof partial, "cohesion counters");  // (the emitters' scratch, grown)
        args.affected = h->force_cnt.p;
        return st;
    }
    template <class M>
    void mix(M m, bool valid) const
    {
        m(&dt, 4);
        if (valid) m(p, sizeof *p);
    }
    hipError_t fetch(ws_handle *h)
    {
        if (!out_affected) return hipSuccess;
        const hipError_t e = copy_now(h, partial, h->force_cnt.p, sizeof partial, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        uint32_t total = 0;
        for (uint32_t s = 0; s < WS_COHESION_SLOTS; s++) total += partial[s * WS_COHESION_SLOT_WORDS];
        *out_affected = total;
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

ws_status ws_apply_cohesion(ws_handle *h, const ws_cohesion_params *p, float dt, uint32_t *out_affected)
{
    CohesionCall call{p, dt, out_affected};
    return edit_fluid(h, call);
}

// ======================================================================================
// solid things in the water
// ======================================================================================
}  // extern "C"

namespace {

// the argument errors of ws_collide_solids (nullptr = acceptable); nothing is touched before this has passed
const char *solids_refusal(const ws_solid *s, uint32_t k)
{
    if (!s) return "solids: s is NULL";
    if (k < 1u || k > WS_MAX_SOLIDS) return "solids: k outside 1 .. WS_MAX_SOLIDS";
    for (uint32_t e = 0; e < k; e++) {
        const ws_solid &o = s[e];
        if (o.kind > WS_SOLID_CAPSULE) return "solids: unknown kind";
        if (o.flags & ~WS_SOLID_HOLLOW) return "solids: unknown flag bits";
        if (o.reserved[0] || o.reserved[1]) return "solids: reserved words must be 0";
        for (int c = 0; c < 9; c++)
            if (ws_bad_float(o.rot[c])) return "solids: rot must be finite and at most 1e15 in magnitude";
        for (int c = 0; c < 3; c++)
            if (ws_bad_float(o.centre[c]) || ws_bad_float(o.size[c]) || ws_bad_float(o.velocity[c]) || ws_bad_float(o.angular_velocity[c]))
                return "solids: centre, size, velocity and angular_velocity must be finite and at most 1e15 in magnitude";
        if (ws_bad_float(o.restitution) || ws_bad_float(o.friction) || ws_bad_float(o.margin)) return "solids: restitution, friction and margin must be finite";
        const int used = o.kind == WS_SOLID_BOX ? 3 : 1;
        for (int c = 0; c < used; c++)
            if (!(o.size[c] > 0.f)) return "solids: a radius or half extent must be > 0";
        if (o.kind == WS_SOLID_CAPSULE && o.size[1] < 0.f) return "solids: a capsule's half length must be >= 0";
        if (o.restitution < 0.f || o.restitution > 1.f || o.friction < 0.f || o.friction > 1.f) return "solids: restitution and friction must lie in [0, 1]";
        if (o.margin < 0.f) return "solids: margin must be >= 0";
    }
    return nullptr;
}

// A lower bound of sigma_min(R)^2 that is safe to divide by, or a value that is not > 0 where R is too near singular for
// one.  sigma_min(R)^2 = the smallest eigenvalue of the symmetric G = R R^T, from the characteristic cubic's trigonometric
// solution (G is 3 x 3 positive semi-definite).
double rot_sigma_min2(const float *rot)
{
    double G[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            G[i][j] = (double)rot[3 * i] * rot[3 * j] + (double)rot[3 * i + 1] * rot[3 * j + 1] + (double)rot[3 * i + 2] * rot[3 * j + 2];
    const double tr = G[0][0] + G[1][1] + G[2][2], mean = tr / 3.0;
    const double off = G[0][1] * G[0][1] + G[0][2] * G[0][2] + G[1][2] * G[1][2];
    double dev = 2.0 * off;
    for (int i = 0; i < 3; i++) dev += (G[i][i] - mean) * (G[i][i] - mean);
    const double pp = sqrt(dev / 6.0);
    double lam_min = mean;  // (a multiple of the identity)
    if (pp > 0.0) {
        double B[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) B[i][j] = (G[i][j] - (i == j ? mean : 0.0)) / pp;
        const double det = B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0]) +
                           B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]);
        const double phi = acos(std::min(1.0, std::max(-1.0, det / 2.0))) / 3.0;
        lam_min = mean + 2.0 * pp * cos(phi + 2.0 * 3.14159265358979323846 / 3.0);
    }
    // (the eigenvalue carries an absolute error of a few 1e-16 tr: taken off, with the kernel's roundings, as 1e-3 tr)
    return lam_min - 1e-3 * tr;
}

// a reach as the squared float the kernels compare |q|^2 with: (reach + 0.1 %)^2, rounded up; +inf where it has no float
float reach2_of(double reach)
{
    const double r2 = reach * reach * 1.002001;
    return r2 < 3e38 ? (float)r2 * 1.000001f : INFINITY;
}

// The squared distance from a solid's centre beyond which no particle can be in contact with it, whatever `rot` holds:
// what lets a wave skip the solid without changing a bit.  A contact needs s < margin, and
//   SPHERE:  s = fl(d - r) < margin                                   =>  d <= r + margin (up to roundings);
//   CAPSULE: the same for d = |q - t R_1| with |t| <= L               =>  |q| <= r + margin + L |R_1|;
//   BOX:     every |l_i| < b_i + margin, l = R q                      =>  |q| <= |b + margin| / sigma_min(R),
// sigma_min = the smallest singular value of R (1 for a rotation; near 0 the bound is useless and the solid is never
// skipped).  The float roundings of the kernel's q, dot products and differences are relative errors of a few 2^-24 at
// the magnitudes |q| and |R_i| |q|: the 1e-3 margins below cover them a thousand times over.  HOLLOW solids touch
// everything outside them: never skipped.
float solids_reach2(const ws_solid &o)
{
    if (o.flags & WS_SOLID_HOLLOW) return INFINITY;
    const double m = o.margin;
    double reach;
    if (o.kind == WS_SOLID_SPHERE) {
        reach = o.size[0] + m;
    } else if (o.kind == WS_SOLID_CAPSULE) {
        reach = o.size[0] + m + (double)o.size[1] * sqrt((double)o.rot[3] * o.rot[3] + (double)o.rot[4] * o.rot[4] + (double)o.rot[5] * o.rot[5]);
    } else {
        const double safe = rot_sigma_min2(o.rot);
        if (!(safe > 0.0)) return INFINITY;
        const double b0 = o.size[0] + m, b1 = o.size[1] + m, b2 = o.size[2] + m;
        reach = sqrt((b0 * b0 + b1 * b1 + b2 * b2) / safe);
    }
    return reach2_of(reach);
}

// The reaction of ws_collide_solids and ws_collide_volumes, one part for both: the caller's three outputs, the device
// accumulator words (the handle's solid_sums) and the host's copy of them.
struct Reaction {
    uint32_t *out_contacts;
    double *out_impulse, *out_angular;
    static_assert(WS_MAX_SOLIDS == WS_MAX_VOLUME_POSES, "one array of sums serves the solids and the poses");
    unsigned long long sums[WS_MAX_SOLIDS * WS_SOLID_WORDS];  // fetch()'s copy of the accumulator words
    bool react() const { return out_contacts || out_impulse || out_angular; }
    // the kernel's `sums` argument: nullptr if nobody asks, else the scratch grown and zeroed on the handle's stream
    // (`what` names it in an allocation error)
    ws_status prepare(ws_handle *h, const char *what, unsigned long long **args_sums)
    {
        if (!react()) return WS_OK;
        const ws_status st = scratch_zeroed(h, h->solid_sums, sizeof sums, what);
        *args_sums = h->solid_sums.p;
        return st;
    }
    hipError_t fetch(ws_handle *h) { return react() ? copy_now(h, sums, h->solid_sums.p, sizeof sums, hipMemcpyDeviceToHost) : hipSuccess; }
    // the accumulator words as the caller's outputs: counts, and the fixed-point sums as (double)sum * 2^-24.  Only after
    // the whole call has succeeded -- on slab handles after the edit has been agreed on: a refused call writes nothing.
    void outputs(uint32_t k) const
    {
        for (uint32_t e = 0; react() && e < k; e++) {
            const unsigned long long *w = sums + (size_t)e * WS_SOLID_WORDS;
            if (out_contacts) out_contacts[e] = (uint32_t)w[0];
            for (int c = 0; c < 3; c++) {
                if (out_impulse) out_impulse[3 * e + c] = (double)(long long)w[1 + c] * 0x1p-24;
                if (out_angular) out_angular[3 * e + c] = (double)(long long)w[4 + c] * 0x1p-24;
            }
        }
    }
};

struct SolidsCall {
    const ws_solid *s;
    uint32_t k;
    Reaction reaction;
    const char *tag = "solids", *things = "solids";
    WsSolidArgs args{};
    const char *refuse() const { return solids_refusal(s, k); }
    ws_status prepare(ws_handle *h, const WsGathered *)  // the solids' bytes as given, and each one's reach
    {
        memcpy(args.ss.e, s, (size_t)k * sizeof(ws_solid));
        for (uint32_t e = 0; e < k; e++) args.ss.reach2[e] = solids_reach2(s[e]);
        args.k = k;
        return reaction.prepare(h, "solid reaction sums", &args.sums);
    }
    template <class M>
    void mix(M m, bool valid) const
    {
        m(&k, 4);
        if (valid) m(s, (size_t)k * sizeof(ws_solid));
    }
    hipError_t fetch(ws_handle *h) { return reaction.fetch(h); }
    void outputs() const { reaction.outputs(k); }
};

}  // namespace

extern "C" {

ws_status ws_collide_solids(ws_handle *h, const ws_solid *s, uint32_t k, uint32_t *out_contacts, double *out_impulse,
                            double *out_angular)
{
    SolidsCall call{s, k, {out_contacts, out_impulse, out_angular}};
    const ws_status st = edit_fluid(h, call);
    if (!st) call.outputs();
    return st;
}

// ======================================================================================
// solids given as signed-distance volumes
// ======================================================================================
}  // extern "C"

namespace {

// 64-bit FNV-1a over 32-bit words: what a slot remembers of its volume for the slabs' agreement
uint64_t volume_mix(uint64_t hash, const void *p, size_t words)
{
    const uint32_t *w = static_cast<const uint32_t *>(p);
    for (size_t t = 0; t < words; t++) hash = (hash ^ w[t]) * 1099511628211ull;
    return hash;
}

// the argument errors of ws_volume_upload with an array (nullptr = acceptable)
const char *volume_refusal(const float *origin, const float *spacing, const uint32_t *dims, const float *sdf)
{
    if (!origin || !spacing || !dims) return "volume: origin, spacing or dims is NULL";
    uint64_t nodes = 1;
    for (int c = 0; c < 3; c++) {
        if (dims[c] < 2u || dims[c] > 1024u) return "volume: every dims entry must lie in 2 .. 1024";
        nodes *= dims[c];
        if (ws_bad_float(origin[c])) return "volume: origin must be finite and at most 1e15 in magnitude";
        if (ws_bad_float(spacing[c]) || !(spacing[c] > 0.f)) return "volume: spacing must be finite, > 0 and at most 1e15";
        if ((double)(dims[c] - 1u) * spacing[c] > 1e15) return "volume: an extent (dims - 1) * spacing is above 1e15";
    }
    if (nodes > (1ull << 26)) return "volume: more than 2^26 nodes";
    for (uint64_t t = 0; t < nodes; t++)
        if (ws_bad_float(sdf[t])) return "volume: every sdf value must be finite and at most 1e15 in magnitude";
    return nullptr;
}

void volume_clear(ws_handle *h, uint32_t slot)
{
    h->volume[slot].release();
    h->volume_desc[slot] = WsVolumeDesc{};
    h->volume_hash[slot] = 0;
}

// the argument errors of ws_collide_volumes (nullptr = acceptable); nothing is touched before this has passed
const char *volumes_refusal(const ws_handle *h, const ws_volume_pose *v, uint32_t k)
{
    if (!v) return "volumes: v is NULL";
    if (k < 1u || k > WS_MAX_VOLUME_POSES) return "volumes: k outside 1 .. WS_MAX_VOLUME_POSES";
    for (uint32_t e = 0; e < k; e++) {
        const ws_volume_pose &o = v[e];
        if (o.slot >= WS_MAX_VOLUMES) return "volumes: slot must be below WS_MAX_VOLUMES";
        if (!h->volume[o.slot].p) return "volumes: the slot holds no volume (ws_volume_upload)";
        if (o.flags) return "volumes: flags must be 0";
        if (o.reserved) return "volumes: the reserved word must be 0";
        for (int c = 0; c < 9; c++)
            if (ws_bad_float(o.rot[c])) return "volumes: rot must be finite and at most 1e15 in magnitude";
        for (int c = 0; c < 3; c++)
            if (ws_bad_float(o.centre[c]) || ws_bad_float(o.velocity[c]) || ws_bad_float(o.angular_velocity[c]))
                return "volumes: centre, velocity and angular_velocity must be finite and at most 1e15 in magnitude";
        if (ws_bad_float(o.restitution) || ws_bad_float(o.friction) || ws_bad_float(o.margin)) return "volumes: restitution, friction and margin must be finite";
        if (o.restitution < 0.f || o.restitution > 1.f || o.friction < 0.f || o.friction > 1.f) return "volumes: restitution and friction must lie in [0, 1]";
        if (o.margin < 0.f) return "volumes: margin must be >= 0";
    }
    return nullptr;
}

// The squared distance from a pose's centre beyond which no particle can be in the volume's domain -- outside the domain
// there is no contact, so the margin does not enter.  In the domain every l_a lies between origin_a and origin_a + (dims_a
// - 1) spacing_a, so |l| is at most the largest |l| over the box's eight corners, and |q| <= |l| / sigma_min(R) (solids_reach2
// has the roundings' allowance; a near-singular rot gives +inf: never skipped).
float volumes_reach2(const ws_volume_pose &o, const WsVolumeDesc &D)
{
    const double safe = rot_sigma_min2(o.rot);
    if (!(safe > 0.0)) return INFINITY;
    double far2 = 0.0;
    for (int c = 0; c < 3; c++) {
        const double lo = D.origin[c], hi = lo + (double)(D.dims[c] - 1u) * D.spacing[c];
        const double a = std::max(fabs(lo), fabs(hi));
        far2 += a * a;
    }
    return reach2_of(sqrt(far2 / safe));
}

struct VolumesCall {
    const ws_handle *owner;  // whose slots the poses name
    const ws_volume_pose *v;
    uint32_t k;
    Reaction reaction;
    const char *tag = "volumes", *things = "poses or volumes";
    WsVolumeArgs args{};
    const char *refuse() const { return volumes_refusal(owner, v, k); }
    ws_status prepare(ws_handle *h, const WsGathered *)  // the slots as they are now, the poses' bytes as given, and each one's reach
    {
        memcpy(args.vs.vol, h->volume_desc, sizeof args.vs.vol);
        memcpy(args.vs.e, v, (size_t)k * sizeof(ws_volume_pose));
        for (uint32_t e = 0; e < k; e++) args.vs.reach2[e] = volumes_reach2(v[e], h->volume_desc[v[e].slot]);
        args.k = k;
        return reaction.prepare(h, "volume reaction sums", &args.sums);
    }
    // (valid: every slot the poses name is below WS_MAX_VOLUMES and holds a volume)
    template <class M>
    void mix(M m, bool valid) const
    {
        m(&k, 4);
        if (!valid) return;
        m(v, (size_t)k * sizeof(ws_volume_pose));
        for (uint32_t s = 0; s < WS_MAX_VOLUMES; s++) {
            bool used = false;
            for (uint32_t e = 0; e < k; e++) used = used || v[e].slot == s;
            if (used) m(&owner->volume_hash[s], 8);  // (covers dims, origin, spacing and the array: ws_volume_upload)
        }
    }
    hipError_t fetch(ws_handle *h) { return reaction.fetch(h); }
    void outputs() const { reaction.outputs(k); }  // (Reaction::outputs: only after the whole call has succeeded)
};

}  // namespace

extern "C" {

ws_status ws_volume_upload(ws_handle *h, uint32_t slot, const float origin[3], const float spacing[3], const uint32_t dims[3],
                           const float *sdf)
{
    ws_status st = enter(h, "volume");
    if (st) return st;
    if (slot >= WS_MAX_VOLUMES) return fail(h, WS_ERR_INVALID_ARG, "volume: slot must be below WS_MAX_VOLUMES");
    if (sdf)
        if (const char *why = volume_refusal(origin, spacing, dims, sdf)) return fail(h, WS_ERR_INVALID_ARG, why);
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // an enqueued edit may still be reading the old array
    volume_clear(h, slot);
    if (!sdf) return WS_OK;
    const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
    if ((st = h->volume[slot].alloc(h, nodes * 4, "signed-distance volume"))) return st;
    const hipError_t e = copy_now(h, h->volume[slot].p, sdf, nodes * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        volume_clear(h, slot);
        return ws_hip_failed(h, "volume: the copy to the device", e);
    }
    WsVolumeDesc &D = h->volume_desc[slot];
    D.sdf = h->volume[slot].p;
    for (int c = 0; c < 3; c++) {
        D.dims[c] = dims[c];
        D.origin[c] = origin[c];
        D.spacing[c] = spacing[c];
    }
    uint64_t hash = volume_mix(14695981039346656037ull, D.dims, 3);
    hash = volume_mix(hash, D.origin, 3);
    hash = volume_mix(hash, D.spacing, 3);
    h->volume_hash[slot] = volume_mix(hash, sdf, nodes);
    return WS_OK;
}

ws_status ws_collide_volumes(ws_handle *h, const ws_volume_pose *v, uint32_t k, uint32_t *out_contacts, double *out_impulse,
                             double *out_angular)
{
    VolumesCall call{h, v, k, {out_contacts, out_impulse, out_angular}};
    const ws_status st = edit_fluid(h, call);
    if (!st) call.outputs();
    return st;
}

// ======================================================================================
// pouring water in and draining it: the particle count as a variable (kernels: ws_population.hip)
// ======================================================================================
}  // extern "C"

namespace {

constexpr uint32_t kMaxParticles = WS_MAX_SLOTS - 16u;  // ws_create's limit

// What the three count-changing calls and ws_reserve_particles refuse before they look at their arguments.
ws_status population_enter(ws_handle *h, const char *tag)
{
    const ws_status st = enter(h, tag);  // (a slab handle is never in the reference-order mode: ws_slab_create)
    if (st) return st;
    if (h->slab)
        return fail(h, WS_ERR_UNSUPPORTED, (std::string(tag) + ": slab handles keep their particle count (ids and attributes are replicated on every rank: the change would be collective)").c_str());
    if (h->rb_inflight)
        return fail(h, WS_ERR_INVALID_ARG, (std::string(tag) + ": a position readback is in flight (call ws_read_positions_end first)").c_str());
    return WS_OK;
}

// The attribute array at a larger capacity (it exists): the new one first, all +0 behind the n attributes carried over.
ws_status grow_attributes(ws_handle *h, uint32_t cap)
{
    WsScratch<float4> bigger;
    const ws_status st = bigger.alloc(h, (size_t)cap * 16, "attribute array");
    if (st) return st;
    hipError_t e = hipMemsetAsync(bigger.p, 0, (size_t)cap * 16, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(bigger.p, h->attr.p, (size_t)h->n * 16, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        bigger.release();
        return ws_hip_failed(h, "attribute array", e);
    }
    h->attr.release();
    h->attr = bigger;  // (the one owner again: `bigger` is a plain pair of pointer and size)
    return WS_OK;
}

// A single-GPU handle at capacity `cap` > h->cap: attributes first, then the particle arrays (either failure leaves the
// handle as it was, but for an attribute array that may already be the larger one -- it holds the same n attributes).
ws_status grow_capacity(ws_handle *h, uint32_t cap)
{
    if (h->attr.p) {
        const ws_status st = grow_attributes(h, cap);
        if (st) return st;
    }
    return grow_particle_arrays(h, cap);
}

// "The count is now n_new": what every count change ends in, after `cur` holds the n_new records of the new set (in any
// order, ids dense).  Modelled on the re-grid of ws_set_params: nd = derive_dev(params, n_new), made by the caller BEFORE
// it touched anything (the cell budget follows n).  The cell tables are rebuilt (start's tail holds n), the alias
// multiplicities follow the new hash_n, the tile schedule exists only for 2^18 <= n < 2^20, the sort view's scratch is
// keyed by n; then the set is binned.  A failure once the old tables have been given up leaves a dead handle.
ws_status population_commit(ws_handle *h, uint32_t n_new, const WsDev &nd)
{
    drop_graphs(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->dev = nd;
    h->n = n_new;
    ws_status st = alloc_grid(h);
    if (!st) st = upload_mult(h);
    if (!st) {
        free_schedule(h);
        st = alloc_schedule(h);
    }
    release_all(h->v_keys, h->v_perm, h->v_tmp, h->v_count, h->v_cursor, h->v_start, h->v_bsum, h->v_off);
    // an edit: every predicted position from the library's own rule; the last step's fields describe another set
    h->pred_stale = true;
    h->accel_stale = false;
    h->have_step = false;
    h->last_pressure = {};
    if (!st) st = bin_current(h);
    if (!st && hipStreamSynchronize(h->stream) != hipSuccess) st = fail(h, WS_ERR_HIP, "count change: binning");
    if (st) {
        h->dead = true;
        h->err = "count change failed after the old cell tables were given up (" + h->err + "); the handle is unusable";
        return st;
    }
    h->pred_stale = true;  // (cur.pred is the rule's, and the next step recomputes it: a captured step replays from here)
    return WS_OK;
}

// the argument errors of ws_remove_particles (nullptr = acceptable)
const char *sinks_refusal(const ws_sink *s, uint32_t k)
{
    if (!s) return "sinks: s is NULL";
    if (k < 1u || k > WS_MAX_SINKS) return "sinks: k outside 1 .. WS_MAX_SINKS";
    for (uint32_t e = 0; e < k; e++) {
        if (s[e].kind > WS_SINK_BOX) return "sinks: unknown kind";
        if (s[e].reserved) return "sinks: reserved must be 0";
        for (int c = 0; c < 3; c++)
            if (ws_bad_float(s[e].centre[c]) || ws_bad_float(s[e].half[c])) return "sinks: centre and half must be finite and at most 1e15 in magnitude";
        if (s[e].kind == WS_SINK_BOX) {
            for (int c = 0; c < 3; c++)
                if (!(s[e].half[c] > 0.f)) return "sinks: a box's half extents must be > 0";
        } else {
            if (!(s[e].half[0] > 0.f)) return "sinks: a sphere's radius half[0] must be > 0";
            if (s[e].half[1] != 0.f || s[e].half[2] != 0.f) return "sinks: a sphere's half[1] and half[2] must be 0";
        }
    }
    return nullptr;
}

// words of ws_handle::pop_words: the per-sink counts, the survivor count, the scan's tile sums
constexpr uint32_t kPopTotal = WS_MAX_SINKS, kPopSums = WS_MAX_SINKS + 1u;

// Both removals.  ids == nullptr: the sinks of `sinks` mark; else the m ids (validated).  The marks live in slot_tmp,
// which only a step's own sort phase reads and writes, so until the survivor count is known nothing of the handle has
// changed.
ws_status remove_marked(ws_handle *h, const WsSinkArgs *sinks, const uint32_t *ids, uint32_t m, uint32_t *out_removed,
                        uint32_t *out_new_id)
{
    const uint32_t n = h->n, k = sinks ? sinks->k : 0u;
    hipStream_t s = h->stream;
    ws_status st = h->pop_words.grow(h, ((size_t)kPopSums + wsk_pop_tiles(n)) * 4, "count change scratch");
    if (!st && (ids || out_new_id)) st = ensure_stage(h, (size_t)std::max(n, m) * 4);
    if (st) return st;
    uint32_t *const map = h->slot_tmp, *const words = h->pop_words.p;
    HIP_TRY(h, hipMemsetAsync(words, 0, (size_t)kPopSums * 4, s));
    if (ids) {
        HIP_TRY(h, hipMemcpyAsync(h->stage, ids, (size_t)m * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(map), 1, n, s));
        wsk_pop_clear_ids(s, (const uint32_t *)h->stage, m, map);
    } else {
        WsSinkArgs a = *sinks;
        a.removed = words;
        wsk_pop_mark_sinks(s, h->cur, n, a, map);
    }
    wsk_pop_scan(s, map, n, words + kPopSums, words + kPopTotal);
    HIP_TRY(h, hipGetLastError());
    uint32_t got[kPopSums];
    HIP_TRY(h, copy_now(h, got, words, sizeof got, hipMemcpyDeviceToHost));  // (the one wait of a removal)
    const uint32_t left = got[kPopTotal];
    if (left > n) return fail(h, WS_ERR_HIP, "count change: the scan counted more survivors than particles");
    if (left == 0u) return fail(h, WS_ERR_INVALID_ARG, "count change: the removal would leave no particle");
    if (left == n) {  // nothing claimed: the handle stays exactly as it was
        if (out_removed) memset(out_removed, 0, (size_t)k * 4);
        if (out_new_id)
            for (uint32_t i = 0; i < n; i++) out_new_id[i] = i;
        return WS_OK;
    }
    WsDev nd;
    if ((st = derive_dev(h, h->params, left, &nd))) return st;
    if (out_new_id) wsk_pop_new_ids(s, map, n, (uint32_t *)h->stage);
    // survivors to slot `new id` of the sorted copy's records -- the last step's views are given up anyway -- which then
    // becomes `cur`; the attributes through the sorted positions and back
    wsk_pop_compact(s, h->cur.pv, n, map, h->srt.pv);
    if (h->attr.p) {
        wsk_pop_compact_attr(s, h->attr.p, n, map, h->srt.pos);
        HIP_TRY(h, hipMemcpyAsync(h->attr.p, h->srt.pos, (size_t)left * 16, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(h, hipGetLastError());
    std::swap(h->cur.pv, h->srt.pv);  // (both belong to the `particles` group, which frees whatever the two fields hold)
    if ((st = population_commit(h, left, nd))) return st;
    if (out_new_id) HIP_TRY(h, copy_now(h, out_new_id, h->stage, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (out_removed) memcpy(out_removed, got, (size_t)k * 4);
    drain_profile(h);
    return WS_OK;
}

}  // namespace

extern "C" {

uint32_t ws_particle_capacity(ws_handle *h)
{
    if (!h) return 0;
    if (h->slab) return h->slab->cap;
    return (h->flags & WS_FLAG_REFERENCE_ORDER) ? h->n : h->cap;
}

ws_status ws_reserve_particles(ws_handle *h, uint32_t capacity)
{
    const ws_status st = population_enter(h, "reserve");
    if (st) return st;
    if (capacity > kMaxParticles) return fail(h, WS_ERR_INVALID_ARG, "reserve: more than 2^27 - 16 particles on one device");
    if (capacity <= h->cap) return WS_OK;
    return grow_capacity(h, capacity);
}

ws_status ws_remove_particles(ws_handle *h, const ws_sink *s, uint32_t k, uint32_t *out_removed, uint32_t *out_new_id)
{
    const ws_status st = population_enter(h, "sinks");
    if (st) return st;
    if (const char *why = sinks_refusal(s, k)) return fail(h, WS_ERR_INVALID_ARG, why);
    WsSinkArgs a{};
    memcpy(a.ss.e, s, (size_t)k * sizeof(ws_sink));
    a.k = k;
    return remove_marked(h, &a, nullptr, 0, out_removed, out_new_id);
}

ws_status ws_remove_particle_ids(ws_handle *h, const uint32_t *ids, uint32_t m, uint32_t *out_new_id)
{
    const ws_status st = population_enter(h, "remove ids");
    if (st) return st;
    if (m == 0u) {  // a no-op: the id map is the identity
        if (out_new_id)
            for (uint32_t i = 0; i < h->n; i++) out_new_id[i] = i;
        return WS_OK;
    }
    if (!ids) return fail(h, WS_ERR_INVALID_ARG, "remove ids: ids is NULL");
    for (uint32_t j = 0; j < m; j++)
        if (ids[j] >= h->n) return fail(h, WS_ERR_INVALID_ARG, "remove ids: an id is not below the particle count");
    return remove_marked(h, nullptr, ids, m, nullptr, out_new_id);
}

ws_status ws_add_particles(ws_handle *h, const float *pos_xyz, const float *vel_xyz, const float *attr, uint32_t m)
{
    ws_status st = population_enter(h, "add");
    if (st) return st;
    if (m == 0u) return WS_OK;
    if (!pos_xyz) return fail(h, WS_ERR_INVALID_ARG, "add: pos_xyz is NULL");
    if ((uint64_t)h->n + m > kMaxParticles) return fail(h, WS_ERR_INVALID_ARG, "add: more than 2^27 - 16 particles on one device");
    for (size_t t = 0; t < (size_t)m * 3; t++)
        if (ws_bad_float(pos_xyz[t]) || (vel_xyz && ws_bad_float(vel_xyz[t])))
            return fail(h, WS_ERR_INVALID_ARG, "add: positions and velocities must be finite and at most 1e15 in magnitude");
    for (size_t t = 0; attr && t < (size_t)m * 4; t++)
        if (ws_bad_float(attr[t])) return fail(h, WS_ERR_INVALID_ARG, "add: attributes must be finite and at most 1e15 in magnitude");
    const uint32_t n0 = h->n, n1 = n0 + m;
    WsDev nd;
    if ((st = derive_dev(h, h->params, n1, &nd))) return st;
    // everything that allocates, before anything is written: the staging (positions | velocities | attributes), the
    // capacity, the attribute array if the new particles are the first to carry any
    const size_t off_vel = (size_t)m * 12, off_attr = (2 * off_vel + 15) & ~(size_t)15;  // (the attributes are read 16 bytes at a time)
    if ((st = ensure_stage(h, off_attr + (size_t)m * 16))) return st;
    if (n1 > h->cap && (st = grow_capacity(h, (uint32_t)std::min<uint64_t>((uint64_t)n1 + n1 / 2u, kMaxParticles)))) return st;
    if (attr && (st = attr_ensure(h))) return st;
    hipStream_t s = h->stream;
    char *const stage = (char *)h->stage;
    HIP_TRY(h, hipMemcpyAsync(stage, pos_xyz, (size_t)m * 12, hipMemcpyHostToDevice, s));
    if (vel_xyz) HIP_TRY(h, hipMemcpyAsync(stage + off_vel, vel_xyz, (size_t)m * 12, hipMemcpyHostToDevice, s));
    if (attr) HIP_TRY(h, hipMemcpyAsync(stage + off_attr, attr, (size_t)m * 16, hipMemcpyHostToDevice, s));
    wsk_pop_append(s, (const float *)stage, vel_xyz ? (const float *)(stage + off_vel) : nullptr,
                   attr ? (const float4 *)(stage + off_attr) : nullptr, m, n0, h->cur, h->attr.p);
    HIP_TRY(h, hipGetLastError());
    if ((st = population_commit(h, n1, nd))) return st;  // (it waits: the caller's arrays are not referenced after return)
    drain_profile(h);
    return WS_OK;
}

// ======================================================================================
// gauges: measure and select the fluid inside regions (kernels: ws_gauges.hip)
// ======================================================================================
}  // extern "C"

namespace {

// the argument errors both gauge calls share (nullptr = acceptable); a region is a ws_sink, refused for what a sink is
const char *regions_refusal(const ws_region *r, uint32_t k, uint32_t flags)
{
    if (!r) return "regions: r is NULL";
    if (k < 1u || k > WS_MAX_REGIONS) return "regions: k outside 1 .. WS_MAX_REGIONS";
    if (flags & ~WS_GAUGE_ATTRIBUTES) return "regions: unknown flag bits";
    return sinks_refusal(r, k);
}

// the device's words (wsk_gauge_measure's layout) as the caller's k gauges
struct GaugeWords {
    unsigned long long sums[WS_MAX_REGIONS][WS_GAUGE_SUMS];
    uint32_t keys[WS_MAX_REGIONS][WS_GAUGE_KEYS];
    static float unkey(uint32_t key)
    {
        const uint32_t bits = key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu);
        float x;
        memcpy(&x, &bits, 4);
        return x;
    }
    void outputs(ws_gauge *out, uint32_t k) const
    {
        for (uint32_t e = 0; e < k; e++) {
            ws_gauge &g = out[e];
            const unsigned long long *w = sums[e];
            g.count = w[0];
            for (int c = 0; c < 3; c++) {
                g.sum_pos[c] = (int64_t)w[1 + c];
                g.sum_vel[c] = (int64_t)w[4 + c];
                g.sum_ang[c] = (int64_t)w[7 + c];
                g.min_pos[c] = unkey(keys[e][c]);
                g.max_pos[c] = unkey(keys[e][3 + c]);
            }
            g.sum_speed2 = (int64_t)w[10];
            for (int c = 0; c < 4; c++) g.sum_attr[c] = (int64_t)w[11 + c];
            g.max_speed2 = unkey(keys[e][6]);
            g.reserved = 0u;
        }
    }
};
static_assert(sizeof(GaugeWords) == WS_GAUGE_OUT_BYTES, "the host's view of the gauge words is the kernel's layout");
static_assert(sizeof(ws_gauge) == 152, "ws_gauge is 152 bytes (include/wsfluid.h)");

}  // namespace

extern "C" {

// One streaming pass over `cur` behind the steps enqueued so far, and one wait for the gauges' words.  Nothing of the
// handle is written but the call's own scratch: no array moves, nothing is binned, pred_stale and the last step's views
// stay, a captured step is replayed as it is, and no profiling event is recorded.
// Slab handles (COLLECTIVE): the velocity field's gather first, the arguments validated in common after it
// (slab_verdict), and every rank measures the global set by id; out == NULL: this rank only contributes.
ws_status ws_measure(ws_handle *h, const ws_region *r, uint32_t k, uint32_t flags, ws_gauge *out)
{
    ws_status st = enter(h, "measure");
    if (st) return st;
    const WsSlab *S = h->slab;
    if (!S && !out) return fail(h, WS_ERR_INVALID_ARG, "measure: out is NULL");
    if (S && (st = slab_gather_by_id(h, WS_PACK_POSVEL_H))) return st;
    const char *why = regions_refusal(r, k, flags);
    const ws_status mine = why ? WS_OK : h->gauge_out.grow(h, WS_GAUGE_OUT_BYTES, "gauge words");
    ArgHash hash;
    hash(&k, 4);
    hash(&flags, 4);
    if (!why) hash(r, (size_t)k * sizeof(ws_region));
    if ((st = slab_verdict(h, {"measure", "regions or flags", false}, why, mine, hash.word))) return st;
    WsRegionSet rs{};
    memcpy(rs.e, r, (size_t)k * sizeof(ws_region));
    wsk_gauge_measure(h->stream, S ? nullptr : h->cur.pv, S ? reinterpret_cast<const float *>(S->g_out.p) : nullptr,
                      (flags & WS_GAUGE_ATTRIBUTES) ? h->attr.p : nullptr, S ? S->n_global : h->n, rs, k, h->gauge_out.p);
    HIP_TRY(h, hipGetLastError());
    GaugeWords words;
    HIP_TRY(h, copy_now(h, &words, h->gauge_out.p, sizeof words, hipMemcpyDeviceToHost));
    if (!S) drain_profile(h);
    if (out) words.outputs(out, k);
    return WS_OK;
}

// The removal's route with the mark turned round: the selected ids marked in the id map (the step's sort slots, which
// nothing reads between two steps), wsk_pop_scan, the first `cap` of them written in id order, and the readback.
ws_status ws_select_particles(ws_handle *h, const ws_region *r, uint32_t k, uint32_t cap, uint32_t *out_ids, uint32_t *out_total)
{
    ws_status st = enter(h, "select");
    if (st) return st;
    if (h->slab) return fail(h, WS_ERR_UNSUPPORTED, "select: not on slab handles (every rank holds its own slab's records: the list would be collective)");
    if (!out_total) return fail(h, WS_ERR_INVALID_ARG, "select: out_total is NULL");
    if (!out_ids && cap) return fail(h, WS_ERR_INVALID_ARG, "select: out_ids is NULL with cap > 0");
    if (const char *why = regions_refusal(r, k, 0u)) return fail(h, WS_ERR_INVALID_ARG, why);
    const uint32_t n = h->n, room = std::min(cap, n);
    if ((st = h->pop_words.grow(h, ((size_t)kPopSums + wsk_pop_tiles(n)) * 4, "selection scratch"))) return st;
    if (room && (st = h->gauge_ids.grow(h, (size_t)room * 4, "selected ids"))) return st;
    hipStream_t s = h->stream;
    uint32_t *const map = h->slot_tmp, *const words = h->pop_words.p;
    WsRegionSet rs{};
    memcpy(rs.e, r, (size_t)k * sizeof(ws_region));
    wsk_gauge_mark(s, h->cur, n, rs, k, map);
    wsk_pop_scan(s, map, n, words + kPopSums, words + kPopTotal);
    if (room) wsk_gauge_list(s, map, n, room, h->gauge_ids.p);
    HIP_TRY(h, hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(h, copy_now(h, &total, words + kPopTotal, 4, hipMemcpyDeviceToHost));
    if (total > n) return fail(h, WS_ERR_HIP, "select: the scan counted more particles than there are");
    const uint32_t wrote = std::min(total, room);
    if (wrote) HIP_TRY(h, copy_now(h, out_ids, h->gauge_ids.p, (size_t)wrote * 4, hipMemcpyDeviceToHost));
    drain_profile(h);
    *out_total = total;
    return WS_OK;
}

// ======================================================================================
// reference-layout sort view
// ======================================================================================
ws_status ws_read_sort_view(ws_handle *h, uint32_t *keys_by_id, uint32_t *perm, uint32_t *cell_offsets)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    // a slab handle answers for the WHOLE domain (collective: the keys of every rank's particles are gathered by id)
    const uint32_t n = h->slab ? h->slab->n_global : h->n;
    const bool stepped = h->slab ? h->steps > h->slab->t0 : h->have_step;
    hipStream_t s = h->stream;
    WS_REF_DISPATCH(h, ref_read_sort_view(h, keys_by_id, perm, cell_offsets));
    if (!h->v_bsum.p) {  // (allocated last: it is there only if all eight are)
        ws_status st = WS_OK;
        for (auto *v : {&h->v_keys, &h->v_perm, &h->v_tmp, &h->v_count, &h->v_cursor, &h->v_off})
            if ((st = v->alloc(h, (size_t)n * 4, "sort view"))) return st;
        if ((st = h->v_start.alloc(h, ((size_t)n + 1) * 4, "sort view"))) return st;
        if ((st = h->v_bsum.alloc(h, (size_t)wsk_scan_state_words(n) * 4, "sort view"))) return st;
        HIP_TRY(h, hipMemsetAsync(h->v_bsum.p, 0, (size_t)wsk_scan_state_words(n) * 4, h->stream));
        HIP_TRY(h, copy_now(h, h->v_start.p + n, &n, 4, hipMemcpyHostToDevice));
    }
    if (!stepped) {
        // src/fluid_compute.rs:306-308: all three buffers start as the identity
        if (h->slab) HIP_TRY(h, hipStreamSynchronize(s));
        wsk_iota(s, h->v_keys.p, n);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(s));
        for (uint32_t *dst : {keys_by_id, perm, cell_offsets})
            if (dst) HIP_TRY(h, copy_now(h, dst, h->v_keys.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return WS_OK;
    }
    HIP_TRY(h, hipMemsetAsync(h->v_count.p, 0, (size_t)n * 4, s));
    const uint32_t *keys = h->v_keys.p;
    if (h->slab) {
        const ws_status st = slab_gather_by_id(h, WS_PACK_KEY_H);
        if (st) return st;
        keys = h->slab->g_out.p;
        wsk_view_count(s, keys, h->v_count.p, n);
    } else {
        // the predicted positions the last step started from live in the sorted copy
        wsk_view_keys(s, h->dev, h->srt, h->v_keys.p, h->v_count.p);
    }
    wsk_scan(s, h->v_count.p, h->v_start.p, h->v_cursor.p, h->v_bsum.p, n, false, 0);
    wsk_scatter(s, keys, h->v_cursor.p, h->v_tmp.p, n, nullptr);
    wsk_view_fix(s, h->v_tmp.p, keys, h->v_start.p, h->v_perm.p, n);
    wsk_view_offsets(s, h->v_start.p, h->v_off.p, n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    if (keys_by_id) HIP_TRY(h, copy_now(h, keys_by_id, keys, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (perm) HIP_TRY(h, copy_now(h, perm, h->v_perm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (cell_offsets) HIP_TRY(h, copy_now(h, cell_offsets, h->v_off.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return WS_OK;
}

// ======================================================================================
// introspection
// ======================================================================================
ws_status ws_profile_read(ws_handle *h, uint32_t k, double *total_ms, uint64_t *launches)
{
    if (!h || k >= WS_K_COUNT) return WS_ERR_INVALID_ARG;
    ws_status st = ws_sync(h);
    if (st) return st;
    if (total_ms) *total_ms = h->prof_ms[k];
    if (launches) *launches = h->prof_cnt[k];
    return WS_OK;
}

ws_status ws_profile_reset(ws_handle *h)
{
    if (!h) return WS_ERR_INVALID_ARG;
    ws_status st = ws_sync(h);
    if (st) return st;
    for (int k = 0; k < WS_K_COUNT; k++) {
        h->prof_ms[k] = 0;
        h->prof_cnt[k] = 0;
    }
    return WS_OK;
}

ws_status ws_profile_select(ws_handle *h, uint32_t kernel_mask)
{
    if (!h) return WS_ERR_INVALID_ARG;
    h->prof_mask = kernel_mask;
    return WS_OK;
}

ws_status ws_read_stats(ws_handle *h, uint32_t out[16])
{
    if (!h || !out) return WS_ERR_INVALID_ARG;
    ws_status st = ws_sync(h);
    if (st) return st;
    HIP_TRY(h, copy_now(h, out, h->stats, 64, hipMemcpyDeviceToHost));
    for (int c = 0; c < 3; c++) out[1 + c] = (uint32_t)h->dev.cm[c];  // reference cells merged per grid cell (host-side)
    out[4] = (uint32_t)(h->slab ? h->slab->graph_steps : h->graph_steps);  // steps replayed from a captured graph
    out[15] = (h->sched_on && !h->alias && !(h->flags & WS_FLAG_GRAPH)) ? 1u : 0u;  // the cost-guided tile schedule drives K4 / K5
    if (h->slab) {  // how close the fixed message capacities came to overrunning, since the last load
        uint32_t dyn[WS_DYN_WORDS];
        HIP_TRY(h, copy_now(h, dyn, h->slab->dyn, sizeof dyn, hipMemcpyDeviceToHost));
        out[5] = dyn[DY_PEAK_HALO];
        out[6] = h->slab->halo_cap;
        out[7] = dyn[DY_PEAK_MIG];
        out[8] = h->slab->mig_cap;
        out[9] = dyn[DY_PEAK_FAR];
        out[10] = h->slab->far_cap;
        out[11] = h->slab->mig_limit_next;   // what the next step's messages will carry (they follow the fluid)
        out[12] = h->slab->halo_limit_next;
        out[13] = h->slab->far_limit_next;
        out[14] = h->slab->size_waits;
        if (h->slab->world == 1) {
            out[11] = out[12] = out[13] = 0;  // no peers, no messages
        } else if (h->slab->exact_messages) {  // ... what the last step's messages carried
            out[11] = h->slab->exact_now[0];
            out[12] = h->slab->exact_now[1];
            out[13] = h->slab->exact_now[2];
        }
    }
    return WS_OK;
}

ws_status ws_grid_dims(ws_handle *h, uint32_t dims[3])
{
    if (!h || !dims) return WS_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++) dims[c] = (uint32_t)h->dev.dim[c];
    return WS_OK;
}

}  // extern "C"

#ifdef WS_DEV_HOOKS
// ======================================================================================
// developer build only: k_schedule on tile costs the CALLER chooses (tests/test_gpu_schedule_kernel.py).  In a step the
// costs are whatever the clock measured; these three calls let a test hand the kernel the arrays its arithmetic is
// delicate at, and see which tiles the scheduled K4 / K5 then ran.  Not declared in include/wsfluid.h.
// ======================================================================================
namespace {

// the arrays of one call, released before it returns (hipFree waits for the device: these calls are not on a hot path)
struct DevSchedArrays {
    WsScratch<uint32_t> cost4, cost5, split4, split5, perm4, perm5;
    void release() { release_all(cost4, cost5, split4, split5, perm4, perm5); }
};

ws_status dev_upload_costs(ws_handle *h, WsScratch<uint32_t> &buf, const uint32_t *cost, uint32_t nt)
{
    const ws_status st = buf.alloc(h, (size_t)nt * 4, "planted tile costs");
    if (st) return st;
    if (nt) HIP_TRY(h, hipMemcpyAsync(buf.p, cost, (size_t)nt * 4, hipMemcpyHostToDevice, h->stream));
    return WS_OK;
}

// split (16 words, as alloc_schedule makes it) and perm of one kernel, all bits set: what k_schedule leaves unwritten shows
ws_status dev_schedule_outputs(ws_handle *h, WsScratch<uint32_t> &split, WsScratch<uint32_t> &perm, uint32_t nt)
{
    ws_status st = split.alloc(h, 16 * 4, "tile schedule");
    if (!st) st = perm.alloc(h, (size_t)nt * 4, "tile schedule");
    if (st) return st;
    HIP_TRY(h, hipMemsetAsync(split.p, 0xFF, 16 * 4, h->stream));
    if (nt) HIP_TRY(h, hipMemsetAsync(perm.p, 0xFF, (size_t)nt * 4, h->stream));
    return WS_OK;
}

ws_status dev_drain(ws_handle *h)
{
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->sched_stream) HIP_TRY(h, hipStreamSynchronize(h->sched_stream));
    return WS_OK;
}

}  // namespace

extern "C" {

// k_schedule once, on cost arrays of the caller's: nt4 / nt5 tiles (any counts, whatever the handle's n; 0 = that half
// of the launch returns at once and its outputs stay all-ones), group_particles / tile5 as wsk_schedule takes them
// (K4's groups are group_particles / 64 tiles, K5's group_particles / tile5).  Waits; split4 / split5: 9 words each.
ws_status ws_dev_schedule(ws_handle *h, const uint32_t *cost4, uint32_t nt4, const uint32_t *cost5, uint32_t nt5, uint32_t nclasses,
                          uint32_t group_particles, uint32_t tile5, uint32_t *split4, uint32_t *perm4, uint32_t *split5, uint32_t *perm5)
{
    if (!h || !split4 || !split5 || (nt4 && (!cost4 || !perm4)) || (nt5 && (!cost5 || !perm5)) || !tile5) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    DevSchedArrays a;
    const ws_status st = [&]() -> ws_status {
        ws_status s = dev_upload_costs(h, a.cost4, cost4, nt4);
        if (!s) s = dev_upload_costs(h, a.cost5, cost5, nt5);
        if (!s) s = dev_schedule_outputs(h, a.split4, a.perm4, nt4);
        if (!s) s = dev_schedule_outputs(h, a.split5, a.perm5, nt5);
        if (s) return s;
        WsSched s4, s5;
        s4.split = a.split4.p, s4.perm = a.perm4.p, s4.cost = a.cost4.p;
        s5.split = a.split5.p, s5.perm = a.perm5.p, s5.cost = a.cost5.p;
        wsk_schedule(h->stream, s4, nt4, s5, s5, nt5, nclasses, group_particles, tile5);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(split4, a.split4.p, 9 * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(split5, a.split5.p, 9 * 4, hipMemcpyDeviceToHost, h->stream));
        if (nt4) HIP_TRY(h, hipMemcpyAsync(perm4, a.perm4.p, (size_t)nt4 * 4, hipMemcpyDeviceToHost, h->stream));
        if (nt5) HIP_TRY(h, hipMemcpyAsync(perm5, a.perm5.p, (size_t)nt5 * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return WS_OK;
    }();
    (void)hipStreamSynchronize(h->stream);  // (a failure half way: nothing of `a` is still in flight when it is freed)
    a.release();
    return st;
}

// A handle whose schedule is on: the NEXT ws_step's K4 and K5 run the split / perm k_schedule makes of cost4
// [sched_tiles4] and cost5 [sched_tiles5], and the cost arrays those two kernels write start at zero, so that
// ws_dev_read_tile_costs shows afterwards which tiles ran.  The step after that is scheduled from measured costs again.
ws_status ws_dev_plant_schedule(ws_handle *h, const uint32_t *cost4, const uint32_t *cost5)
{
    if (!h || !cost4 || !cost5) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->sched_on) return fail(h, WS_ERR_INVALID_ARG, "ws_dev_plant_schedule: the handle has no tile schedule");
    DevSchedArrays a;
    const ws_status st = [&]() -> ws_status {
        ws_status s = dev_drain(h);
        if (!s) s = dev_upload_costs(h, a.cost4, cost4, h->sched_tiles4);
        if (!s) s = dev_upload_costs(h, a.cost5, cost5, h->sched_tiles5);
        if (s) return s;
        const uint32_t par = h->sched_parity;  // the set the next step's kernels read
        WsSched s4 = h->sched4[par], from5;
        s4.cost = a.cost4.p;
        from5.cost = a.cost5.p;
        wsk_schedule(h->stream, s4, h->sched_tiles4, h->sched5[par], from5, h->sched_tiles5, h->sched_classes, h->sched_group,
                     wsk_force_tile(h->n));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemsetAsync(h->sched4[par].cost, 0, (size_t)h->sched_tiles4 * 4, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->sched5[par].cost, 0, (size_t)h->sched_tiles5 * 4, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return WS_OK;
    }();
    (void)hipStreamSynchronize(h->stream);
    a.release();
    return st;
}

// The costs K4 and K5 of the last step wrote (cost4 [sched_tiles4], cost5 [sched_tiles5]; either may be NULL), and the
// two tile counts (ntiles[2]; may be NULL).
ws_status ws_dev_read_tile_costs(ws_handle *h, uint32_t *cost4, uint32_t *cost5, uint32_t *ntiles)
{
    if (!h) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->sched_on) return fail(h, WS_ERR_INVALID_ARG, "ws_dev_read_tile_costs: the handle has no tile schedule");
    const ws_status st = dev_drain(h);
    if (st) return st;
    if (ntiles) ntiles[0] = h->sched_tiles4, ntiles[1] = h->sched_tiles5;
    const uint32_t ran = h->sched_parity ^ 1u;  // the set the last step's kernels read, and whose costs its K5 wrote
    if (cost4) HIP_TRY(h, copy_now(h, cost4, h->sched4[ran].cost, (size_t)h->sched_tiles4 * 4, hipMemcpyDeviceToHost));
    if (cost5) HIP_TRY(h, copy_now(h, cost5, h->sched5[ran].cost, (size_t)h->sched_tiles5 * 4, hipMemcpyDeviceToHost));
    return WS_OK;
}

}  // extern "C"
#endif  // WS_DEV_HOOKS

#include "ws_field.inc"
#include "ws_slab.inc"
