// ws_population.hip -- gfx950 (CDNA4) kernels of the calls that change the particle count: ws_remove_particles,
// ws_remove_particle_ids and ws_add_particles.  Never inside ws_step; each runs once per call, streaming over the particle
// records.  Compiled with the flags and under the arithmetic contract of ws_kernels.hip.
//
// A removal is mark -> scan -> compact over ONE word per particle id, the MAP (ws_api.cpp lends it the step's sort slots,
// which nothing reads between two steps):
//   mark     map[id] = 1 (the particle stays) or 0 (a sink claimed it / its id was named);
//   scan     map[id] = rank among the survivors by id << 1 | stays -- three launches: the sum of every tile, one workgroup
//            over the tile sums, every tile again.  A tile needs nothing but the finished launch before it: no workgroup
//            waits for another, and the result is a function of the marks alone;
//   compact  every surviving record to slot `new id` of another array with its id word rewritten, the attributes likewise.
// The survivor count is the scan's grand total, which the host reads before anything is moved.
#include "ws_device.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// mark
// ---------------------------------------------------------------------------------

// Does sink S contain position p?  include/wsfluid.h pins every operation; the sphere's distance is step 1 of
// ws_apply_forces (forces_eval, ws_edits.hip) operation for operation.  A NaN coordinate fails every comparison.
__device__ __forceinline__ bool sink_contains(const ws_sink &S, const float4 &p)
{
    const float qx = p.x - S.centre[0], qy = p.y - S.centre[1], qz = p.z - S.centre[2];
    if (S.kind == WS_SINK_SPHERE) {
        const float dst = sqrtf(qx * qx + qy * qy + qz * qz);
        return dst < S.half[0];
    }
    return fabsf(qx) <= S.half[0] && fabsf(qy) <= S.half[1] && fabsf(qz) <= S.half[2];
}

// One lane per record of `cur` (one 16-byte load: the half with position and id).  The sinks are a by-value kernel
// argument (512 B): the loop over them is wave-uniform and reads them through scalar loads.  The first sink that contains
// a particle claims it; the per-sink counts are one ballot per sink and wave and one atomic per wave that claimed anything
// (the emitters' counters, forces_eval).
__global__ void __launch_bounds__(WS_BLOCK) k_pop_mark_sinks(WsSoA cur, uint32_t n, WsSinkArgs a, uint32_t *__restrict__ map)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    const bool active = i < n;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) p = cur.pos(i);
    bool claimed = false;
    for (uint32_t e = 0; e < a.k; e++) {
        const bool in = active && !claimed && sink_contains(a.ss.e[e], p);
        const uint32_t c = (uint32_t)__popcll(__ballot(in));
        if (c && (threadIdx.x & 63u) == 0u) atomicAdd(&a.removed[e], c);
        claimed = claimed || in;
    }
    if (active) map[__float_as_uint(p.w)] = claimed ? 0u : 1u;
}

// the id form: the host has set every word of the map to 1 (a fill); the named ids are cleared (duplicates store the same 0)
__global__ void __launch_bounds__(WS_BLOCK) k_pop_clear_ids(const uint32_t *__restrict__ ids, uint32_t m, uint32_t *__restrict__ map)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j < m) map[ids[j]] = 0u;
}

// ---------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------
#define POP_ITEMS 8u                        // consecutive map words per thread
#define POP_TILE (WS_BLOCK * POP_ITEMS)     // map words per workgroup
#define POP_SUMS_BLOCK 1024                 // the one workgroup over the tile sums

// the 8 marks of this thread (0 beyond n), and how many of them are set
__device__ __forceinline__ uint32_t pop_load(const uint32_t *__restrict__ map, uint32_t n, uint32_t first, uint32_t (&v)[POP_ITEMS])
{
    if (first + POP_ITEMS <= n) {  // (the map is 16-byte aligned and `first` a multiple of 8)
        const uint4 lo = *reinterpret_cast<const uint4 *>(map + first), hi = *reinterpret_cast<const uint4 *>(map + first + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < POP_ITEMS; j++) v[j] = first + j < n ? map[first + j] : 0u;
    }
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < POP_ITEMS; j++) sum += v[j];
    return sum;
}

// exclusive prefix of `v` over the workgroup's threads (any multiple of 64 up to 1024), and the workgroup's total
__device__ __forceinline__ uint32_t pop_block_excl(uint32_t v, uint32_t *s_wave, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < nwaves; w++) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    total = all;
    return before + incl - v;
}

__global__ void __launch_bounds__(WS_BLOCK) k_pop_tile_sums(const uint32_t *__restrict__ map, uint32_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s_wave[WS_BLOCK / 64];
    uint32_t v[POP_ITEMS], total;
    const uint32_t mine = pop_load(map, n, blockIdx.x * POP_TILE + threadIdx.x * POP_ITEMS, v);
    (void)pop_block_excl(mine, s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[t] becomes the survivors in front of tile t; *total the survivors in all (ntiles <= 2^27 / POP_TILE = 65 536: at
// most 64 sums per thread)
__global__ void __launch_bounds__(POP_SUMS_BLOCK) k_pop_scan_sums(uint32_t *__restrict__ sums, uint32_t ntiles, uint32_t *__restrict__ total)
{
    __shared__ uint32_t s_wave[POP_SUMS_BLOCK / 64];
    const uint32_t per = (ntiles + POP_SUMS_BLOCK - 1u) / POP_SUMS_BLOCK, first = threadIdx.x * per;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < per; j++) mine += first + j < ntiles ? sums[first + j] : 0u;
    uint32_t all;
    uint32_t run = pop_block_excl(mine, s_wave, all);
    for (uint32_t j = 0; j < per; j++) {
        if (first + j >= ntiles) break;
        const uint32_t t = sums[first + j];
        sums[first + j] = run;
        run += t;
    }
    if (threadIdx.x == 0) *total = all;
}

__global__ void __launch_bounds__(WS_BLOCK) k_pop_apply(uint32_t *__restrict__ map, uint32_t n, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s_wave[WS_BLOCK / 64];
    uint32_t v[POP_ITEMS], total;
    const uint32_t first = blockIdx.x * POP_TILE + threadIdx.x * POP_ITEMS;
    const uint32_t mine = pop_load(map, n, first, v);
    uint32_t run = sums[blockIdx.x] + pop_block_excl(mine, s_wave, total);
#pragma unroll
    for (uint32_t j = 0; j < POP_ITEMS; j++) {
        const uint32_t keep = v[j];
        v[j] = run << 1 | keep;
        run += keep;
    }
    if (first + POP_ITEMS <= n) {
        *reinterpret_cast<uint4 *>(map + first) = make_uint4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<uint4 *>(map + first + 4) = make_uint4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < POP_ITEMS; j++)
            if (first + j < n) map[first + j] = v[j];
    }
}

// ---------------------------------------------------------------------------------
// compact, the id map, append
// ---------------------------------------------------------------------------------

// src / dst: 32-byte records {position, id | velocity, cell id} (WsSoA::pv).  The cell id is whatever: the count change
// ends in a re-binning, which writes it.
__global__ void __launch_bounds__(WS_BLOCK) k_pop_compact(const float4 *__restrict__ src, uint32_t n, const uint32_t *__restrict__ map,
                                                          float4 *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4 p = src[2 * (size_t)i];
    const float4 v = src[2 * (size_t)i + 1];
    const uint32_t w = map[__float_as_uint(p.w)];
    if (!(w & 1u)) return;
    const size_t to = w >> 1;
    p.w = __uint_as_float((uint32_t)to);
    dst[2 * to] = p;
    dst[2 * to + 1] = make_float4(v.x, v.y, v.z, 0.f);
}

__global__ void __launch_bounds__(WS_BLOCK) k_pop_compact_attr(const float4 *__restrict__ attr, uint32_t n, const uint32_t *__restrict__ map,
                                                               float4 *__restrict__ out)
{
    const uint32_t id = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (id >= n) return;
    const uint32_t w = map[id];
    if (w & 1u) out[w >> 1] = attr[id];
}

__global__ void __launch_bounds__(WS_BLOCK) k_pop_new_ids(const uint32_t *__restrict__ map, uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t id = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (id >= n) return;
    const uint32_t w = map[id];
    out[id] = (w & 1u) ? w >> 1 : 0xFFFFFFFFu;
}

// m staged particles into the slots n0 .. n0 + m - 1 with those ids; vel == nullptr: at rest; attr == nullptr: the handle
// has no attribute array; attr_in == nullptr: +0
__global__ void __launch_bounds__(WS_BLOCK) k_pop_append(const float *__restrict__ pos, const float *__restrict__ vel,
                                                         const float4 *__restrict__ attr_in, uint32_t m, uint32_t n0, WsSoA cur,
                                                         float4 *__restrict__ attr)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = n0 + j;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (vel) {
        vx = vel[3 * (size_t)j];
        vy = vel[3 * (size_t)j + 1];
        vz = vel[3 * (size_t)j + 2];
    }
    cur.pos(i) = make_float4(pos[3 * (size_t)j], pos[3 * (size_t)j + 1], pos[3 * (size_t)j + 2], __uint_as_float(i));
    cur.vel(i) = make_float4(vx, vy, vz, 0.f);
    if (attr) attr[i] = attr_in ? attr_in[j] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
uint32_t wsk_pop_tiles(uint32_t n) { return cdiv(n, POP_TILE); }

void wsk_pop_mark_sinks(hipStream_t s, WsSoA cur, uint32_t n, const WsSinkArgs &a, uint32_t *map)
{
    hipLaunchKernelGGL(k_pop_mark_sinks, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, n, a, map);
}

void wsk_pop_clear_ids(hipStream_t s, const uint32_t *ids, uint32_t m, uint32_t *map)
{
    hipLaunchKernelGGL(k_pop_clear_ids, dim3(cdiv(m, WS_BLOCK)), dim3(WS_BLOCK), 0, s, ids, m, map);
}

void wsk_pop_scan(hipStream_t s, uint32_t *map, uint32_t n, uint32_t *sums, uint32_t *total)
{
    const uint32_t nt = wsk_pop_tiles(n);
    hipLaunchKernelGGL(k_pop_tile_sums, dim3(nt), dim3(WS_BLOCK), 0, s, map, n, sums);
    hipLaunchKernelGGL(k_pop_scan_sums, dim3(1), dim3(POP_SUMS_BLOCK), 0, s, sums, nt, total);
    hipLaunchKernelGGL(k_pop_apply, dim3(nt), dim3(WS_BLOCK), 0, s, map, n, sums);
}

void wsk_pop_compact(hipStream_t s, const float4 *src, uint32_t n, const uint32_t *map, float4 *dst)
{
    hipLaunchKernelGGL(k_pop_compact, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, src, n, map, dst);
}

void wsk_pop_compact_attr(hipStream_t s, const float4 *attr, uint32_t n, const uint32_t *map, float4 *out)
{
    hipLaunchKernelGGL(k_pop_compact_attr, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, attr, n, map, out);
}

void wsk_pop_new_ids(hipStream_t s, const uint32_t *map, uint32_t n, uint32_t *out)
{
    hipLaunchKernelGGL(k_pop_new_ids, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, map, n, out);
}

void wsk_pop_append(hipStream_t s, const float *pos, const float *vel, const float4 *attr_in, uint32_t m, uint32_t n0, WsSoA cur,
                    float4 *attr)
{
    hipLaunchKernelGGL(k_pop_append, dim3(cdiv(m, WS_BLOCK)), dim3(WS_BLOCK), 0, s, pos, vel, attr_in, m, n0, cur, attr);
}
