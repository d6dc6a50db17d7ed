// ws_device.h -- what more than one of the .hip files needs on the device side, and nothing else: the block size, the
// XCD tile map, the cell of a position, the wave scans, the smoothing kernels, the two sqrt / division forms and the
// bool-to-template dispatch.  Included by the .hip files only (ws_kernels.hip: the step; ws_edits.hip: the between-step
// edits; ws_population.hip: the count changes; ws_gauges.hip: the gauges; ws_views.hip: read-backs and id-ordered views; ws_fields.hip: the field calls); a helper that one file uses
// stays in that file.  The arithmetic contract is the one stated at the top of ws_kernels.hip.
#pragma once

#include <type_traits>

#include "ws_internal.h"

#pragma clang fp contract(off)

#define WS_BLOCK 256

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Workgroup -> tile map of the reorder pass and the two neighbour kernels.  Blocks are dealt round-robin over the 8 XCDs
// (b and b + 8 share one), each with its own L2: tile = f(b) gives every XCD one CONTIGUOUS eighth of the sorted order (an
// x-slab of the domain), so a tile's neighbour records are fetched into one L2 instead of into all eight (round 2) --
// and the SAME eighth in k_reorder, K4 and K5 (round 5), walked in alternating directions: k_reorder ascending, K4
// DESCENDING (`reverse`), K5 ascending.  So every kernel starts on what the kernel before it wrote LAST on this very
// XCD -- the end of the range k_reorder has just filled is still in this XCD's L2 when K4 begins there, the accept masks
// and densities K4 wrote last are where K5 begins (C3: K4 -9 % sparse, K5 -4 % settled; steps -3.2 % / -2.5 %; C2, the
// reference's 65 536: -2.5 %; C4 settled -1.5 %; profiles/r05/ab/ab_zigzag_*.log).  Speed / traffic only: any
// placement and any order compute the same thing.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t nt, bool reverse = false)
{
    const uint32_t xcd = b & 7u, q = nt >> 3, r = nt & 7u;
    const uint32_t first = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q, mine = q + (xcd < r ? 1u : 0u);
    const uint32_t j = b >> 3;
    return first + (reverse ? mine - 1u - j : j);
}

// ---------------------------------------------------------------------------------
// cell helpers
// ---------------------------------------------------------------------------------

// get_cell, assets/simulation.wgsl:121-123: vec3<i32>(floor(position / h)) with an
// IEEE divide (not a reciprocal multiply), then clamped into the padded dense grid.
// Clamping is monotone per axis, so two particles whose true cells are adjacent stay
// in adjacent-or-equal grid cells: the 27-cell search over grid cells visits a superset
// of the reference's candidates and the exact distance test decides, as it does there.
// Global x layer (grid cells along x of the whole domain) of a position: the slab cuts are expressed in these.
__device__ __forceinline__ int grid_layer_x(const WsDev &d, float x)
{
    const float fx = floorf(x / d.h) - (float)d.org[0];
    int gxg = (int)fminf(fmaxf(fx, 0.0f), (float)(d.fdim[0] - 1));  // fmaxf/fminf also squash NaN to the low border
    if (d.coarse) gxg /= d.cm[0];
    return gxg;
}

__device__ __forceinline__ uint32_t grid_cell(const WsDev &d, float x, float y, float z)
{
    const float fy = floorf(y / d.h) - (float)d.org[1];
    const float fz = floorf(z / d.h) - (float)d.org[2];
    // x: clamped in GLOBAL grid coordinates, then shifted into this handle's local (slab) grid and
    // clamped again so a particle that left the slab still bins inside the local tables
    const int gxg = grid_layer_x(d, x);
    int gy = (int)fminf(fmaxf(fy, 0.0f), (float)(d.fdim[1] - 1));
    int gz = (int)fminf(fmaxf(fz, 0.0f), (float)(d.fdim[2] - 1));
    if (d.coarse) {  // (wave-uniform; integer division only on the rare handles whose grid cells are merged)
        gy /= d.cm[1];
        gz /= d.cm[2];
    }
    const int gx = min(max(gxg - d.xoff, 0), d.dim[0] - 1);
    return (uint32_t)((gx * d.dim[1] + gy) * d.dim[2] + gz);
}

// hash_cell(get_cell(p)), assets/simulation.wgsl:121-128 (u32 wrap arithmetic).
__device__ __forceinline__ uint32_t ref_hash_key(const WsDev &d, float x, float y, float z)
{
    const uint32_t cx = (uint32_t)(int32_t)floorf(x / d.h);
    const uint32_t cy = (uint32_t)(int32_t)floorf(y / d.h);
    const uint32_t cz = (uint32_t)(int32_t)floorf(z / d.h);
    return (cx * 15823u + cy * 9737333u + cz * 440817757u) % d.hash_n;
}

// the owned particle count: slab handles keep it on the device (WsDev::dyn)
__device__ __forceinline__ uint32_t ws_n(const WsDev &d) { return d.dyn ? d.dyn[DY_N] : d.n; }

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// A float as the 64-bit fixed-point term of an order-free sum (ws_collide_solids step 6, ws_measure): clamped to
// +-2^31 -- a NaN comes out of fmaxf as -2^31 --, times 2^24, rounded to nearest even; and such terms summed across a wave.
__device__ __forceinline__ long long solids_fixed(float x)
{
    return llrintf(fminf(fmaxf(x, -2147483648.f), 2147483648.f) * 16777216.f);
}

__device__ __forceinline__ long long wave_sum_i64(long long x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// Wave-level aggregation of `atomicAdd(&table[key], 1)`: consecutive lanes with the same key form a
// run; the run's first lane adds the run length once and every member gets base + its offset in the run.
// Particles are processed in (previous) cell order, so in a dense fluid runs are ~7 lanes long and the
// atomic traffic on the per-cell counters drops accordingly.  Returns this lane's value of the counter
// (what its own atomicAdd(.., 1) would have returned in SOME serialisation).  `active` lanes only.
__device__ __forceinline__ uint32_t wave_run_atomic_inc(uint32_t *__restrict__ table, uint32_t key, bool active)
{
    // May be called from divergent code: lanes that are not executing simply do not appear in `act`
    // (their shuffled key is never trusted: a lane whose predecessor is not in `act` starts a run).
    const int lane = threadIdx.x & 63;
    const unsigned long long act = __ballot(active);
    const uint32_t prev = __shfl_up(key, 1, 64);
    const bool prev_active = lane > 0 && ((act >> (lane - 1)) & 1ull);
    const bool head = active && (!prev_active || key != prev);
    const unsigned long long heads = __ballot(head);
    if (!active) return 0u;
    const unsigned long long upto = heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    const int hl = 63 - __builtin_clzll(upto);                      // my run's head lane
    const unsigned long long above = (hl == 63) ? 0ull : (~((2ull << hl) - 1ull));
    // the run ends at the next head or at the first inactive lane above the head
    const unsigned long long stop = (heads | ~act) & above;
    const int end = stop ? __builtin_ctzll(stop) : 64;
    uint32_t base = 0;
    if (lane == hl) base = atomicAdd(&table[key], (uint32_t)(end - hl));
    base = __shfl(base, hl, 64);
    return base + (uint32_t)(lane - hl);
}

#define WS_LOOKAHEAD 0.02f  // 1. / 50., simulation.wgsl:3

// Run-time bools as template bools: f is called once, with a std::true_type or std::false_type for every bool given.
template <class F>
void ws_dispatch(F &&f)
{
    f();
}
template <class F, class... Bools>
void ws_dispatch(F &&f, bool first, Bools... rest)
{
    if (first) ws_dispatch([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else ws_dispatch([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// ---------------------------------------------------------------------------------
// smoothing kernels, assets/simulation.wgsl:93-117 (evaluation order as written)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float sk_density(const WsDev &d, float dst)
{
    const float v = d.h - dst;
    return v * v * d.k_pow2;
}
__device__ __forceinline__ float sk_near(const WsDev &d, float dst)
{
    const float v = d.h - dst;
    return v * v * v * d.k_pow3;
}
__device__ __forceinline__ float sk_der(const WsDev &d, float dst) { return (dst - d.h) * d.k_pow2_der; }
__device__ __forceinline__ float sk_der_near(const WsDev &d, float dst)
{
    const float v = dst - d.h;
    return v * v * d.k_pow3_der;
}
__device__ __forceinline__ float sk_visc(const WsDev &d, float dst)
{
    const float v = d.h * d.h - dst * dst;
    return v * v * v * d.k_spikey;
}

// sqrt and division of the pair terms.  IEEE = true: correctly rounded, in the reference's operation order -- the
// arithmetic of a CPU restatement (and always of the reference-order validation mode).  IEEE = false (default of
// the production kernels): the hardware's v_sqrt_f32 / v_rcp_f32 (1 ULP each), x / y evaluated as x * rcp(y) --
// within the accuracy the reference's shading language itself grants its GPU (WGSL: x / y 2.5 ULP, sqrt as
// 1 / inverseSqrt at 2 ULP) -- and, in the force pair, the scalar factors collected first (force_pair).  ~9
// correctly rounded divisions and a square root cost ~110 of the ~180 instructions of one IEEE force pair.
template <bool IEEE>
__device__ __forceinline__ float ws_sqrt(float x)
{
    if constexpr (IEEE) return sqrtf(x);
    else return __builtin_amdgcn_sqrtf(x);
}

template <bool IEEE>
struct WsDivisor {
    float v;
    __device__ __forceinline__ explicit WsDivisor(float den) : v(IEEE ? den : __builtin_amdgcn_rcpf(den)) {}
    __device__ __forceinline__ float operator()(float num) const { return IEEE ? num / v : num * v; }
};
