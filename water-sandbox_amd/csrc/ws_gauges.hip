// ws_gauges.hip -- gfx950 (CDNA4) kernels of the gauges: ws_measure and ws_select_particles.  Never inside ws_step; each
// runs once per call, streaming over the particle records, and writes none of them.  Compiled with the flags and under the
// arithmetic contract of ws_kernels.hip.
//
// ws_measure is ONE reduction pass: every output is an integer sum that wraps, or a float chosen by a total order on its
// bits, so lanes, waves and workgroups may meet in any order and the result is a function of the particle set alone.
// ws_select_particles is the removal's route with the mark turned round (ws_population.hip): mark the selected ids in the
// map, wsk_pop_scan, write id to out[rank].
#include "ws_device.h"

#pragma clang fp contract(off)

// Particles per lane.  A lane holds them in registers with the region loop OUTSIDE, so that a region costs one reduction
// per wave and 64 * GAUGE_ITEMS particles, not one per 64 (the choice: DESIGN.md 9.13).
#define GAUGE_ITEMS 4u
#define GAUGE_TILE (WS_BLOCK * GAUGE_ITEMS)  // particles per workgroup

// the total order of the extremes: a float's bits as an unsigned key (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
__device__ __forceinline__ uint32_t gauge_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the identity of key slot c of a region: min_pos[3] from +inf, max_pos[3] from -inf, max_speed2 from +0
__device__ __forceinline__ uint32_t gauge_identity(uint32_t c) { return c < 3u ? 0xFF800000u : c < 6u ? 0x007FFFFFu : 0x80000000u; }

// Does region S contain position p?  ws_remove_particles step 1 operation for operation (sink_contains, ws_population.hip);
// q = p - centre comes back for the angular sums.  A NaN coordinate fails every comparison.
__device__ __forceinline__ bool region_contains(const ws_region &S, float px, float py, float pz, float &qx, float &qy, float &qz)
{
    qx = px - S.centre[0];
    qy = py - S.centre[1];
    qz = pz - S.centre[2];
    if (S.kind == WS_SINK_SPHERE) {
        const float dst = sqrtf(qx * qx + qy * qy + qz * qz);
        return dst < S.half[0];
    }
    return fabsf(qx) <= S.half[0] && fabsf(qy) <= S.half[1] && fabsf(qz) <= S.half[2];
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor(x, o, 64));
    return x;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor(x, o, 64));
    return x;
}

// ---------------------------------------------------------------------------------
// ws_measure
//
// out: WS_MAX_REGIONS rows of WS_GAUGE_SUMS 64-bit words {count, sum_pos[3], sum_vel[3], sum_ang[3], sum_speed2,
// sum_attr[4]}, then WS_MAX_REGIONS rows of WS_GAUGE_KEYS 32-bit keys {min_pos[3], max_pos[3], max_speed2}; k_gauge_init
// sets the identities on the stream before the pass.
// A workgroup takes GAUGE_TILE consecutive records: lane t the records t, t + 256, ... of the tile, each as one pair of
// 16-byte loads (BYID: a slab's gathered {position, velocity} by id, three 8-byte loads), all of them in registers before
// the first region is looked at.  The regions are a by-value kernel argument (512 B): the loop over them is wave-uniform,
// reads them through scalar loads and skips a region that no lane's ballot is in.  For a region somebody is in: the count
// is the ballots' popcount; every lane sums its own particles' fixed-point terms privately; ONE shuffle reduction per wave,
// region and word; the wave's first lane adds the non-zero words to the workgroup's row in LDS (64-bit LDS adds, 32-bit LDS
// min / max on the keys).  After a barrier one thread per region and word issues at most one global atomic, and none for a
// region the workgroup never touched or a word that is zero.  No float atomics anywhere.
// ATTR: the four attribute floats by id (one scattered 16-byte gather per particle; BYID: in order) -- an instance of its
// own, so that the unflagged kernel carries none of its code or registers.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(WS_BLOCK) k_gauge_init(unsigned long long *__restrict__ out)
{
    const uint32_t t = threadIdx.x;
    uint32_t *const keys = reinterpret_cast<uint32_t *>(out + WS_MAX_REGIONS * WS_GAUGE_SUMS);
    if (t < WS_MAX_REGIONS * WS_GAUGE_SUMS) out[t] = 0ull;
    if (t < WS_MAX_REGIONS * WS_GAUGE_KEYS) keys[t] = gauge_identity(t % WS_GAUGE_KEYS);
}

template <bool ATTR, bool BYID>
__global__ void __launch_bounds__(WS_BLOCK) k_gauge_measure(const float4 *__restrict__ pv, const float *__restrict__ posvel,
                                                            const float4 *__restrict__ attr, uint32_t n, WsRegionSet rs, uint32_t k,
                                                            unsigned long long *__restrict__ out)
{
    static_assert(WS_MAX_REGIONS * WS_GAUGE_SUMS <= (uint32_t)WS_BLOCK, "one thread zeroes and flushes one word");
    constexpr uint32_t NW = ATTR ? WS_GAUGE_SUMS - 1u : WS_GAUGE_SUMS - 5u;  // fixed-point words per region: 14 or 10
    __shared__ unsigned long long acc[WS_MAX_REGIONS * WS_GAUGE_SUMS];
    __shared__ uint32_t ext[WS_MAX_REGIONS * WS_GAUGE_KEYS];
    const uint32_t t = threadIdx.x;
    if (t < WS_MAX_REGIONS * WS_GAUGE_SUMS) acc[t] = 0ull;
    if (t < WS_MAX_REGIONS * WS_GAUGE_KEYS) ext[t] = gauge_identity(t % WS_GAUGE_KEYS);
    __syncthreads();

    float px[GAUGE_ITEMS], py[GAUGE_ITEMS], pz[GAUGE_ITEMS], vx[GAUGE_ITEMS], vy[GAUGE_ITEMS], vz[GAUGE_ITEMS];
    float4 at[GAUGE_ITEMS];
    bool active[GAUGE_ITEMS];
#pragma unroll
    for (uint32_t j = 0; j < GAUGE_ITEMS; j++) {
        const uint32_t i = blockIdx.x * GAUGE_TILE + j * WS_BLOCK + t;  // (n <= 2^27)
        active[j] = i < n;
        px[j] = py[j] = pz[j] = vx[j] = vy[j] = vz[j] = 0.f;
        at[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active[j]) {
            uint32_t id = i;
            if constexpr (BYID) {
                const float2 *const r = reinterpret_cast<const float2 *>(posvel) + 3 * (size_t)i;
                const float2 a = r[0], b = r[1], c = r[2];
                px[j] = a.x; py[j] = a.y; pz[j] = b.x;
                vx[j] = b.y; vy[j] = c.x; vz[j] = c.y;
            } else {
                const float4 p = pv[2 * (size_t)i], v = pv[2 * (size_t)i + 1];
                px[j] = p.x; py[j] = p.y; pz[j] = p.z;
                vx[j] = v.x; vy[j] = v.y; vz[j] = v.z;
                id = __float_as_uint(p.w);
            }
            if constexpr (ATTR) at[j] = attr[id];
        }
    }

    const bool lead = (t & 63u) == 0u;
    for (uint32_t e = 0; e < k; e++) {
        const ws_region &S = rs.e[e];
        bool in[GAUGE_ITEMS];
        float qx[GAUGE_ITEMS], qy[GAUGE_ITEMS], qz[GAUGE_ITEMS];
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < GAUGE_ITEMS; j++) {
            in[j] = active[j] && region_contains(S, px[j], py[j], pz[j], qx[j], qy[j], qz[j]);
            cnt += (uint32_t)__popcll(__ballot(in[j]));
        }
        if (!cnt) continue;  // wave-uniform: nobody of this wave is in the region
        long long w[NW];
#pragma unroll
        for (uint32_t c = 0; c < NW; c++) w[c] = 0;
        uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, fast = 0x80000000u;
#pragma unroll
        for (uint32_t j = 0; j < GAUGE_ITEMS; j++) {
            if (!in[j]) continue;
            const float s2 = vx[j] * vx[j] + vy[j] * vy[j] + vz[j] * vz[j];
            w[0] += solids_fixed(px[j]);
            w[1] += solids_fixed(py[j]);
            w[2] += solids_fixed(pz[j]);
            w[3] += solids_fixed(vx[j]);
            w[4] += solids_fixed(vy[j]);
            w[5] += solids_fixed(vz[j]);
            w[6] += solids_fixed(qy[j] * vz[j] - qz[j] * vy[j]);
            w[7] += solids_fixed(qz[j] * vx[j] - qx[j] * vz[j]);
            w[8] += solids_fixed(qx[j] * vy[j] - qy[j] * vx[j]);
            w[9] += solids_fixed(s2);
            if constexpr (ATTR) {
                w[10] += solids_fixed(at[j].x);
                w[11] += solids_fixed(at[j].y);
                w[12] += solids_fixed(at[j].z);
                w[13] += solids_fixed(at[j].w);
            }
            const uint32_t kx = gauge_key(px[j]), ky = gauge_key(py[j]), kz = gauge_key(pz[j]);
            lo[0] = min(lo[0], kx); lo[1] = min(lo[1], ky); lo[2] = min(lo[2], kz);
            hi[0] = max(hi[0], kx); hi[1] = max(hi[1], ky); hi[2] = max(hi[2], kz);
            if (s2 == s2) fast = max(fast, gauge_key(s2));  // (a NaN is skipped, as fmaxf skips it)
        }
        unsigned long long *const a = acc + e * WS_GAUGE_SUMS;
        uint32_t *const x = ext + e * WS_GAUGE_KEYS;
        if (lead) atomicAdd(&a[0], (unsigned long long)cnt);
#pragma unroll
        for (uint32_t c = 0; c < NW; c++) {
            const long long sum = wave_sum_i64(w[c]);
            if (lead && sum) atomicAdd(&a[1u + c], (unsigned long long)sum);
        }
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const uint32_t l = wave_min_u32(lo[c]), h = wave_max_u32(hi[c]);
            if (lead) {
                atomicMin(&x[c], l);
                atomicMax(&x[3u + c], h);
            }
        }
        fast = wave_max_u32(fast);
        if (lead) atomicMax(&x[6], fast);
    }
    __syncthreads();

    // the workgroup's rows on their way out: only for the regions it touched (word 0, the count, is non-zero exactly then)
    uint32_t *const keys = reinterpret_cast<uint32_t *>(out + WS_MAX_REGIONS * WS_GAUGE_SUMS);
    if (t < k * WS_GAUGE_SUMS && acc[t - t % WS_GAUGE_SUMS] != 0ull && acc[t] != 0ull) atomicAdd(&out[t], acc[t]);
    if (t < k * WS_GAUGE_KEYS && acc[(t / WS_GAUGE_KEYS) * WS_GAUGE_SUMS] != 0ull) {
        const uint32_t c = t % WS_GAUGE_KEYS;
        if (c < 3u) atomicMin(&keys[t], ext[t]);
        else atomicMax(&keys[t], ext[t]);
    }
}

// ---------------------------------------------------------------------------------
// ws_select_particles
// ---------------------------------------------------------------------------------

// map[id] = 1 if at least one region contains the particle, else 0: k_pop_mark_sinks with the mark turned round and no
// counters.  One lane per record of `cur` (one 16-byte load: the half with position and id).
__global__ void __launch_bounds__(WS_BLOCK) k_gauge_mark(WsSoA cur, uint32_t n, WsRegionSet rs, uint32_t k, uint32_t *__restrict__ map)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = cur.pos(i);
    bool in = false;
    float qx, qy, qz;
    for (uint32_t e = 0; e < k; e++) in = in || region_contains(rs.e[e], p.x, p.y, p.z, qx, qy, qz);
    map[__float_as_uint(p.w)] = in ? 1u : 0u;
}

// after wsk_pop_scan: map[id] = rank among the selected << 1 | selected; the first `cap` selected ids, ascending
__global__ void __launch_bounds__(WS_BLOCK) k_gauge_list(const uint32_t *__restrict__ map, uint32_t n, uint32_t cap, uint32_t *__restrict__ out)
{
    const uint32_t id = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (id >= n) return;
    const uint32_t w = map[id];
    if ((w & 1u) && (w >> 1) < cap) out[w >> 1] = id;
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void wsk_gauge_measure(hipStream_t s, const float4 *pv, const float *posvel, const float4 *attr, uint32_t n, const WsRegionSet &rs,
                       uint32_t k, unsigned long long *out)
{
    hipLaunchKernelGGL(k_gauge_init, dim3(1), dim3(WS_BLOCK), 0, s, out);
    if (!n) return;
    ws_dispatch([&](auto with_attr, auto by_id) {
        hipLaunchKernelGGL((k_gauge_measure<decltype(with_attr)::value, decltype(by_id)::value>), dim3(cdiv(n, GAUGE_TILE)), dim3(WS_BLOCK),
                           0, s, pv, posvel, attr, n, rs, k, out);
    }, attr != nullptr, posvel != nullptr);
}

void wsk_gauge_mark(hipStream_t s, WsSoA cur, uint32_t n, const WsRegionSet &rs, uint32_t k, uint32_t *map)
{
    hipLaunchKernelGGL(k_gauge_mark, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, n, rs, k, map);
}

void wsk_gauge_list(hipStream_t s, const uint32_t *map, uint32_t n, uint32_t cap, uint32_t *out)
{
    hipLaunchKernelGGL(k_gauge_list, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, map, n, cap, out);
}
