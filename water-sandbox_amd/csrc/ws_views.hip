// ws_views.hip -- gfx950 (CDNA4) kernels of the read-backs, the reference-layout sort view and the id-ordered global
// views and loads of slab handles: what the C ABI launches around the step, never inside it.  Compiled with the flags and
// under the arithmetic contract of ws_kernels.hip.
#include "ws_device.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// readback in original-id order (update(), src/fluid_compute.rs:478-485)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(WS_BLOCK) k_gather_positions(WsSoA cur, float *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = cur.pos(i);
    const size_t id = __float_as_uint(p.w);
    out[3 * id] = p.x;
    out[3 * id + 1] = p.y;
    out[3 * id + 2] = p.z;
}

void wsk_gather_positions(hipStream_t s, WsSoA cur, float *out_xyz, uint32_t n)
{
    hipLaunchKernelGGL(k_gather_positions, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, out_xyz, n);
}

// `velocity.length()` per particle, the quantity of the reference's (commented-out) speed colouring,
// src/fluid_compute.rs:489-502; same left-to-right sum as the WGSL length() restatement
__global__ void __launch_bounds__(WS_BLOCK) k_gather_speeds(WsSoA cur, float *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 v = cur.vel(i);
    out[__float_as_uint(cur.pos(i).w)] = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
}

void wsk_gather_speeds(hipStream_t s, WsSoA cur, float *out, uint32_t n)
{
    hipLaunchKernelGGL(k_gather_speeds, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, out, n);
}

// the velocities by id (ws_read_velocities; the velocity field's input)
__global__ void __launch_bounds__(WS_BLOCK) k_gather_velocities(WsSoA cur, float *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 v = cur.vel(i);
    const size_t id = __float_as_uint(cur.pos(i).w);
    out[3 * id] = v.x;
    out[3 * id + 1] = v.y;
    out[3 * id + 2] = v.z;
}

void wsk_gather_velocities(hipStream_t s, WsSoA cur, float *out_xyz, uint32_t n)
{
    hipLaunchKernelGGL(k_gather_velocities, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, out_xyz, n);
}

__global__ void __launch_bounds__(WS_BLOCK) k_gather_particles(WsSoA cur, WsSorted srt, const float4 *__restrict__ accel,
                                                               int have_step, WsPressureParams pp,
                                                               ws_particle80 *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = cur.pos(i), v = cur.vel(i), q = cur.pred[i];
    const size_t id = __float_as_uint(p.w);
    float4 dp = make_float4(0.f, 0.f, 0.f, 0.f), a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (have_step) {
        dp.x = srt.pred(i).w;  // density / near density ride in the sorted copy's w lanes
        dp.y = srt.vel(i).w;
        // simulation.wgsl:192-193, with the parameters of the step that computed the densities (ws_handle::last_pressure)
        dp.z = pp.pressure_scalar * (dp.x - pp.target_density);
        dp.w = pp.near_pressure_scalar * dp.y;
        a = accel[i];
    }
    float4 *rec = reinterpret_cast<float4 *>(out + id);
    rec[0] = make_float4(p.x, p.y, p.z, 0.f);
    rec[1] = dp;
    rec[2] = make_float4(v.x, v.y, v.z, 0.f);
    rec[3] = make_float4(a.x, a.y, a.z, 0.f);
    rec[4] = make_float4(q.x, q.y, q.z, 0.f);
}

void wsk_gather_particles(hipStream_t s, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                          const WsPressureParams &pp, ws_particle80 *out, uint32_t n)
{
    hipLaunchKernelGGL(k_gather_particles, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, cur, srt, accel,
                       have_step ? 1 : 0, pp, out, n);
}

// ---------------------------------------------------------------------------------
// reference-layout sort view (diagnostic, on demand; never part of ws_step)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(WS_BLOCK) k_view_keys(WsDev d, WsSorted srt,
                                                        uint32_t *__restrict__ keys_by_id, uint32_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= d.n) return;
    const float4 p = srt.pred(i);
    const uint32_t id = __float_as_uint(srt.pos[i].w);
    const uint32_t key = ref_hash_key(d, p.x, p.y, p.z);
    keys_by_id[id] = key;
    atomicAdd(&count[key], 1u);
}

void wsk_view_keys(hipStream_t s, const WsDev &d, WsSorted srt, uint32_t *keys_by_id, uint32_t *count)
{
    hipLaunchKernelGGL(k_view_keys, dim3(cdiv(d.n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, srt, keys_by_id, count);
}

// the histogram alone, for keys that are already there (slab handles: gathered by id)
__global__ void __launch_bounds__(WS_BLOCK) k_view_count(const uint32_t *__restrict__ keys, uint32_t *__restrict__ count, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i < n) atomicAdd(&count[keys[i]], 1u);
}

void wsk_view_count(hipStream_t s, const uint32_t *keys, uint32_t *count, uint32_t n)
{
    hipLaunchKernelGGL(k_view_count, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, keys, count, n);
}

// stable order inside each bucket: ascending particle id
__global__ void __launch_bounds__(WS_BLOCK) k_view_fix(const uint32_t *__restrict__ tmp, const uint32_t *__restrict__ keys,
                                                       const uint32_t *__restrict__ start, uint32_t *__restrict__ perm,
                                                       uint32_t n)
{
    const uint32_t s = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t id = tmp[s];
    const uint32_t k = keys[id];
    const uint32_t b = start[k], e = start[k + 1];
    uint32_t rank = 0;
    for (uint32_t t = b; t < e; t++) rank += (tmp[t] < id) ? 1u : 0u;
    perm[b + rank] = id;
}

void wsk_view_fix(hipStream_t s, const uint32_t *tmp, const uint32_t *keys, const uint32_t *start, uint32_t *perm,
                  uint32_t n)
{
    hipLaunchKernelGGL(k_view_fix, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, tmp, keys, start, perm, n);
}

// cell_offsets[k] = first slot of key k, or INF (bitonic_sort.wgsl:48-59, simulation.wgsl:36)
__global__ void __launch_bounds__(WS_BLOCK) k_view_offsets(const uint32_t *__restrict__ start, uint32_t *__restrict__ off,
                                                           uint32_t n)
{
    const uint32_t k = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t b = start[k], e = start[k + 1];
    off[k] = (e > b) ? b : 999999999u;
}

void wsk_view_offsets(hipStream_t s, const uint32_t *start, uint32_t *off, uint32_t n)
{
    hipLaunchKernelGGL(k_view_offsets, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, start, off, n);
}

// four words from the host into device memory BY A KERNEL (arguments, not a copy): what a transport then reads -- a
// kernel of RCCL's, on the same stream -- was written by the kernel in front of it, the one ordering every runtime fences.
// (A small host-to-device copy may go through the CPU's window into device memory; round 4's stand-in for librccl read
// the previous call's words out of the L2 behind it now and then.)
__global__ void k_set_words4(uint32_t *__restrict__ p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    p[0] = a;
    p[1] = b;
    p[2] = c;
    p[3] = d;
}
void wsk_set_words4(hipStream_t s, uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    hipLaunchKernelGGL(k_set_words4, dim3(1), dim3(1), 0, s, p, a, b, c, d);
}

__global__ void __launch_bounds__(WS_BLOCK) k_iota(uint32_t *__restrict__ p, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i < n) p[i] = i;
}

void wsk_iota(hipStream_t s, uint32_t *p, uint32_t n)
{
    hipLaunchKernelGGL(k_iota, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, p, n);
}

// Slab readback: owned particles (state of the last step, sorted order) with their ids.
__global__ void __launch_bounds__(WS_BLOCK) k_gather_slab(WsDev d, WsSoA cur, WsSorted srt, const float4 *__restrict__ accel,
                                                          int have_step, WsPressureParams pp,
                                                          ws_particle80 *__restrict__ out, uint32_t *__restrict__ ids)
{
    const uint32_t k = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (k >= ws_n(d)) return;
    const uint32_t i = d.base + k;
    const float4 p = cur.pos(i), v = cur.vel(i), q = cur.pred[i];
    float4 dp = make_float4(0.f, 0.f, 0.f, 0.f), a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (have_step) {
        dp.x = srt.pred(i).w;
        dp.y = srt.vel(i).w;
        dp.z = pp.pressure_scalar * (dp.x - pp.target_density);  // (the last step's: k_gather_particles)
        dp.w = pp.near_pressure_scalar * dp.y;
        a = accel[i];
    }
    float4 *rec = reinterpret_cast<float4 *>(out + k);
    rec[0] = make_float4(p.x, p.y, p.z, 0.f);
    rec[1] = dp;
    rec[2] = make_float4(v.x, v.y, v.z, 0.f);
    rec[3] = make_float4(a.x, a.y, a.z, 0.f);
    rec[4] = make_float4(q.x, q.y, q.z, 0.f);
    ids[k] = __float_as_uint(p.w);
}

void wsk_gather_slab(hipStream_t s, const WsDev &d, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                     const WsPressureParams &pp, ws_particle80 *out, uint32_t *ids)
{
    if (d.n == 0) return;
    hipLaunchKernelGGL(k_gather_slab, dim3(cdiv(d.n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, cur, srt, accel,
                       have_step ? 1 : 0, pp, out, ids);
}

// upload of a slab's initial particles: ids are given explicitly
__global__ void __launch_bounds__(WS_BLOCK) k_upload_positions_ids(const float *__restrict__ xyz,
                                                                   const uint32_t *__restrict__ ids, WsSoA cur, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    cur.pos(i) = make_float4(x, y, z, __uint_as_float(ids[i]));
    cur.vel(i) = make_float4(0.f, 0.f, 0.f, 0.f);
    cur.pred[i] = make_float4(x, y, z, 0.f);
}

void wsk_upload_positions_ids(hipStream_t s, const float *xyz_dev, const uint32_t *ids_dev, WsSoA cur, uint32_t n)
{
    if (!n) return;
    hipLaunchKernelGGL(k_upload_positions_ids, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, xyz_dev, ids_dev, cur, n);
}

// ---------------------------------------------------------------------------------
// slab handles: the id-ordered GLOBAL views and loads of the C ABI (ws_read_positions / ws_read_speeds /
// ws_read_particles / ws_reset / ws_write_particles / a re-grid on ws_set_params), which the reference's host uses every
// frame (update(), src/fluid_compute.rs:478-485) and on Space (despawn_liquid, :505-525).  Reads: every slab packs
// {id, payload} records of the particles it owns, the records are all-gathered, and every rank scatters them by id.
// Loads: every rank is handed the same global array and keeps the particles whose x layer falls into its cuts.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t slab_owner(const WsDev &d, const uint32_t *__restrict__ cuts, uint32_t world, float x)
{
    const uint32_t gxg = (uint32_t)grid_layer_x(d, x);
    uint32_t dest = 0;
    while (dest + 1 < world && gxg >= cuts[dest + 1]) dest++;
    return dest;
}

// payload of one gathered record (after its id word)
enum { WS_PACK_POS = 0, WS_PACK_SPEED = 1, WS_PACK_RECORD = 2, WS_PACK_STATE = 3, WS_PACK_KEY = 4, WS_PACK_POSVEL = 5 };
__host__ __device__ constexpr uint32_t ws_pack_words(int kind)
{
    return kind == WS_PACK_POS ? 3u : kind == WS_PACK_SPEED ? 1u : kind == WS_PACK_RECORD ? 20u : kind == WS_PACK_STATE ? 9u :
           kind == WS_PACK_POSVEL ? 6u : 1u;
}
uint32_t wsk_pack_words(int kind) { return ws_pack_words(kind); }

template <int KIND>
__global__ void __launch_bounds__(WS_BLOCK) k_slab_pack(WsDev d, WsSoA cur, WsSorted srt, const float4 *__restrict__ accel,
                                                        int have_step, WsPressureParams pp, uint32_t *__restrict__ out)
{
    const uint32_t k = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (k >= d.n) return;
    const uint32_t i = d.base + k;
    constexpr uint32_t W = ws_pack_words(KIND) + 1u;
    uint32_t *rec = out + (size_t)k * W;
    float *f = reinterpret_cast<float *>(rec + 1);
    if constexpr (KIND == WS_PACK_KEY) {
        // the reference's particle_cell_indicies entry: hash of the cell of the predicted position the last step started from
        const float4 q = srt.pred(i);
        rec[0] = __float_as_uint(srt.pos[i].w);
        rec[1] = ref_hash_key(d, q.x, q.y, q.z);
        return;
    }
    const float4 p = cur.pos(i);
    rec[0] = __float_as_uint(p.w);
    if constexpr (KIND == WS_PACK_POS) {
        f[0] = p.x; f[1] = p.y; f[2] = p.z;
    } else if constexpr (KIND == WS_PACK_SPEED) {
        const float4 v = cur.vel(i);
        f[0] = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    } else if constexpr (KIND == WS_PACK_POSVEL) {  // the velocity field's input: one gather brings both
        const float4 v = cur.vel(i);
        f[0] = p.x; f[1] = p.y; f[2] = p.z;
        f[3] = v.x; f[4] = v.y; f[5] = v.z;
    } else if constexpr (KIND == WS_PACK_STATE) {
        const float4 v = cur.vel(i), q = cur.pred[i];
        f[0] = p.x; f[1] = p.y; f[2] = p.z;
        f[3] = v.x; f[4] = v.y; f[5] = v.z;
        f[6] = q.x; f[7] = q.y; f[8] = q.z;
    } else {  // the 80-byte record (k_gather_slab's fields)
        const float4 v = cur.vel(i), q = cur.pred[i];
        float4 dp = make_float4(0.f, 0.f, 0.f, 0.f), a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have_step) {
            dp.x = srt.pred(i).w;
            dp.y = srt.vel(i).w;
            dp.z = pp.pressure_scalar * (dp.x - pp.target_density);
            dp.w = pp.near_pressure_scalar * dp.y;
            a = accel[i];
        }
        f[0] = p.x; f[1] = p.y; f[2] = p.z; f[3] = 0.f;
        f[4] = dp.x; f[5] = dp.y; f[6] = dp.z; f[7] = dp.w;
        f[8] = v.x; f[9] = v.y; f[10] = v.z; f[11] = 0.f;
        f[12] = a.x; f[13] = a.y; f[14] = a.z; f[15] = 0.f;
        f[16] = q.x; f[17] = q.y; f[18] = q.z; f[19] = 0.f;
    }
}

void wsk_slab_pack(hipStream_t s, const WsDev &d, int kind, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                   const WsPressureParams &pp, uint32_t *out)
{
    if (!d.n) return;
    const dim3 g(cdiv(d.n, WS_BLOCK)), b(WS_BLOCK);
    const int hs = have_step ? 1 : 0;
    switch (kind) {
        case WS_PACK_POS: hipLaunchKernelGGL(k_slab_pack<WS_PACK_POS>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
        case WS_PACK_SPEED: hipLaunchKernelGGL(k_slab_pack<WS_PACK_SPEED>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
        case WS_PACK_RECORD: hipLaunchKernelGGL(k_slab_pack<WS_PACK_RECORD>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
        case WS_PACK_STATE: hipLaunchKernelGGL(k_slab_pack<WS_PACK_STATE>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
        case WS_PACK_POSVEL: hipLaunchKernelGGL(k_slab_pack<WS_PACK_POSVEL>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
        default: hipLaunchKernelGGL(k_slab_pack<WS_PACK_KEY>, g, b, 0, s, d, cur, srt, accel, hs, pp, out); break;
    }
}

// every rank's records (rank r: cnt[4 r] of them at all + r * stride_words) scattered by id: out[id * pw + j]
__global__ void __launch_bounds__(WS_BLOCK) k_slab_unpack_by_id(const uint32_t *__restrict__ all, const uint32_t *__restrict__ cnt,
                                                                uint32_t max_n, size_t stride_words, uint32_t pw,
                                                                uint32_t n_global, uint32_t *__restrict__ out)
{
    const uint32_t k = blockIdx.x * WS_BLOCK + threadIdx.x, r = blockIdx.y;
    if (k >= min(cnt[4 * r], max_n)) return;
    const uint32_t *rec = all + (size_t)r * stride_words + (size_t)k * (pw + 1u);
    const uint32_t id = rec[0];
    if (id >= n_global) return;
    for (uint32_t j = 0; j < pw; j++) out[(size_t)id * pw + j] = rec[1 + j];
}

void wsk_slab_unpack_by_id(hipStream_t s, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                           size_t stride_words, uint32_t pw, uint32_t n_global, uint32_t *out)
{
    if (!max_n) return;
    hipLaunchKernelGGL(k_slab_unpack_by_id, dim3(cdiv(max_n, WS_BLOCK), world), dim3(WS_BLOCK), 0, s, all, cnt, max_n,
                       stride_words, pw, n_global, out);
}

// x-layer histogram of ALL particles (gathered {id, pos, vel, pred} records of every rank): the input of a re-cut
// (ws_slab_rebalance).  Every rank computes the same histogram from the same gathered data, hence the same cuts.
__global__ void __launch_bounds__(WS_BLOCK) k_slab_layer_hist(WsDev d, const uint32_t *__restrict__ all, const uint32_t *__restrict__ cnt,
                                                              uint32_t max_n, size_t stride_words, uint32_t *__restrict__ hist)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x, r = blockIdx.y;
    if (t >= min(cnt[4 * r], max_n)) return;
    const float *f = reinterpret_cast<const float *>(all + (size_t)r * stride_words + (size_t)t * 10u + 1u);
    atomicAdd(&hist[grid_layer_x(d, f[6])], 1u);  // by PREDICTED x, what the step bins by
}

void wsk_slab_layer_hist(hipStream_t s, const WsDev &d, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                         size_t stride_words, uint32_t *hist)
{
    if (!max_n) return;
    hipLaunchKernelGGL(k_slab_layer_hist, dim3(cdiv(max_n, WS_BLOCK), world), dim3(WS_BLOCK), 0, s, d, all, cnt, max_n, stride_words,
                       hist);
}

// Loads.  One lane per record of a chunk of a GLOBAL array; the lanes whose particle this slab owns append it to the
// owned range (one atomic per wave; the order is free: the sort is canonical).  dyn[DY_N] is the fill counter.
//   SRC 0: positions at rest (float xyz; id = id0 + t)            -- ws_reset / FluidParticle::make_vec_from_positions
//   SRC 1: 80-byte records (id = id0 + t)                          -- ws_write_particles
//   SRC 2: gathered {id, pos, vel, pred} records of every rank     -- a re-grid (blockIdx.y = source rank)
template <int SRC>
__global__ void __launch_bounds__(WS_BLOCK) k_slab_select(WsDev d, const uint32_t *__restrict__ cuts, uint32_t world,
                                                          uint32_t me, const void *__restrict__ chunk, uint32_t id0, uint32_t m,
                                                          const uint32_t *__restrict__ cnt, size_t stride_words, WsSoA cur,
                                                          uint32_t cap, uint32_t *__restrict__ dyn)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x;
    bool mine = false;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p, q = p;
    uint32_t id = 0;
    if constexpr (SRC == 2) {
        const uint32_t r = blockIdx.y;
        if (t < min(cnt[4 * r], m)) {
            const uint32_t *rec = static_cast<const uint32_t *>(chunk) + (size_t)r * stride_words + (size_t)t * 10u;
            const float *f = reinterpret_cast<const float *>(rec + 1);
            id = rec[0];
            p = make_float4(f[0], f[1], f[2], 0.f);
            v = make_float4(f[3], f[4], f[5], 0.f);
            q = make_float4(f[6], f[7], f[8], 0.f);
            mine = true;
        }
    } else if (t < m) {
        id = id0 + t;
        if constexpr (SRC == 0) {
            const float *f = static_cast<const float *>(chunk) + 3 * (size_t)t;
            p = q = make_float4(f[0], f[1], f[2], 0.f);
        } else {
            const float4 *rec = reinterpret_cast<const float4 *>(static_cast<const ws_particle80 *>(chunk) + t);
            p = rec[0]; v = rec[2]; q = rec[4];
        }
        mine = true;
    }
    // ownership follows the PREDICTED position: it is what the step bins by (simulation.wgsl:139)
    mine = mine && slab_owner(d, cuts, world, q.x) == me;
    const unsigned long long sel = __ballot(mine);
    if (!sel) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)sel) - 1;
    uint32_t first = 0;
    if (lane == leader) first = atomicAdd(&dyn[DY_N], (uint32_t)__popcll(sel));
    first = __shfl(first, leader, 64);
    if (!mine) return;
    const uint32_t slot = first + (uint32_t)__popcll(sel & ((1ull << lane) - 1ull));
    if (slot >= cap) {  // counted, not stored: the host sees DY_N > cap and fails the load
        return;
    }
    const uint32_t i = d.base + slot;
    cur.pos(i) = make_float4(p.x, p.y, p.z, __uint_as_float(id));
    cur.vel(i) = make_float4(v.x, v.y, v.z, 0.f);
    cur.pred[i] = make_float4(q.x, q.y, q.z, 0.f);
}

void wsk_slab_select(hipStream_t s, const WsDev &d, int src, const uint32_t *cuts, uint32_t world, uint32_t me,
                     const void *chunk, uint32_t id0, uint32_t m, const uint32_t *cnt, size_t stride_words, WsSoA cur,
                     uint32_t cap, uint32_t *dyn)
{
    if (!m) return;
    const dim3 b(WS_BLOCK);
    if (src == 0)
        hipLaunchKernelGGL(k_slab_select<0>, dim3(cdiv(m, WS_BLOCK)), b, 0, s, d, cuts, world, me, chunk, id0, m, cnt, stride_words, cur, cap, dyn);
    else if (src == 1)
        hipLaunchKernelGGL(k_slab_select<1>, dim3(cdiv(m, WS_BLOCK)), b, 0, s, d, cuts, world, me, chunk, id0, m, cnt, stride_words, cur, cap, dyn);
    else
        hipLaunchKernelGGL(k_slab_select<2>, dim3(cdiv(m, WS_BLOCK), world), b, 0, s, d, cuts, world, me, chunk, id0, m, cnt, stride_words, cur, cap, dyn);
}
