// ws_fields.hip -- gfx950 (CDNA4) kernels of the call families built on field_sweep / field_launch: the density and
// velocity fields, advection, whitewater, the cohesion stage, attributes, bodies, rays, anisotropy and the iso-surface
// mesher.  Never inside ws_step.  Compiled with the flags and under the arithmetic contract of ws_kernels.hip.
#include <algorithm>

#include "ws_device.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// density field sampler (ws_sample_density_grid / _points; never inside ws_step)
//
// The field at a query point o is sum over particles p with !(d2 > d2_accept) of sk_density(|x_p - o|), and its gradient
// sum of sk_der(d) * (o - x_p) / d -- the reference's smoothing_kernel / smoothing_kernel_derivative
// (assets/simulation.wgsl:93-107) with d2 and d formed exactly as K4 forms them (e = x_p - o).  The particles are the
// CURRENT positions, binned by the sampler itself into arrays of its own (the step's sorted arrays describe the
// predicted positions the last step started from): keys = grid_cell(position) by id, then the sort view's count / scan /
// scatter / rank-by-id (k_view_count, k_scan, k_scatter, k_view_fix) and k_field_gather.  Candidates are visited in
// increasing linear cell id and, inside a cell, by particle id, whatever kernel visits them: the sums are a function of
// the particle set and the query point alone.  Neither the multiplicity path (ALIAS) nor the tile schedule applies.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(WS_BLOCK) k_field_keys(WsDev d, const float *__restrict__ xyz, uint32_t *__restrict__ keys,
                                                         uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = grid_cell(d, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
}

void wsk_field_keys(hipStream_t s, const WsDev &d, const float *xyz, uint32_t *keys, uint32_t n)
{
    hipLaunchKernelGGL(k_field_keys, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, xyz, keys, n);
}

// sorted copy: spos[j] = {position of particle perm[j], its id (bits)}
__global__ void __launch_bounds__(WS_BLOCK) k_field_gather(const uint32_t *__restrict__ perm, const float *__restrict__ xyz,
                                                           float4 *__restrict__ spos, uint32_t n)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t id = perm[j];
    spos[j] = make_float4(xyz[3 * id], xyz[3 * id + 1], xyz[3 * id + 2], __uint_as_float((uint32_t)id));
}

void wsk_field_gather(hipStream_t s, const uint32_t *perm, const float *xyz, float4 *spos, uint32_t n)
{
    hipLaunchKernelGGL(k_field_gather, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, perm, xyz, spos, n);
}

// Cell coordinate of x along axis a of a single-GPU (or gathered global) grid: the per-axis part of grid_cell.
__device__ __forceinline__ int field_axis_cell(const WsDev &d, int a, float x)
{
    const float f = floorf(x / d.h) - (float)d.org[a];
    int g = (int)fminf(fmaxf(f, 0.0f), (float)(d.fdim[a] - 1));
    if (d.coarse) g /= d.cm[a];
    return g;
}

// node (i, j, k) of the grid: fl(origin + fl((float)i * spacing)) per axis
struct WsFieldGrid {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz;
};
__device__ __forceinline__ float4 field_node(const WsFieldGrid &g, uint32_t i, uint32_t j, uint32_t k)
{
    return make_float4(g.ox + (float)i * g.sx, g.oy + (float)j * g.sy, g.oz + (float)k * g.sz, 0.f);
}

struct FieldAcc {
    float rho, gx, gy, gz;
};
// The sums the two field kernels keep per query: FieldAcc, unless the source names an accumulator of its own (Src::Acc).
template <class Src, class = void>
struct field_acc {
    using type = FieldAcc;
};
template <class Src>
struct field_acc<Src, std::void_t<typename Src::Acc>> {
    using type = typename Src::Acc;
};
template <class Src>
using field_acc_t = typename field_acc<Src>::type;

// One accepted pair.  (ex, ey, ez) = x_p - o (K4's e), d2 its squared length.  Gradient term (o - x_p) * W'(d) / d:
// IEEE = ((o - x_p) / d) * W'(d) with correctly rounded sqrt and division; default = (o - x_p) * (W'(d) * rcp(d)) with
// the hardware v_sqrt_f32 / v_rcp_f32 -- the two forms K5 uses for its direction.  d == 0 contributes no gradient.
template <bool IEEE, bool GRAD>
__device__ __forceinline__ void field_pair(const WsDev &d, float ex, float ey, float ez, float d2, FieldAcc &a)
{
    const float dst = ws_sqrt<IEEE>(d2);
    a.rho += sk_density(d, dst);
    if constexpr (GRAD) {
        const float slope = sk_der(d, dst);
        const bool apart = dst > 0.f;
        if constexpr (IEEE) {
            const WsDivisor<IEEE> by_dst(dst);
            a.gx += apart ? by_dst(-ex) * slope : 0.f;
            a.gy += apart ? by_dst(-ey) * slope : 0.f;
            a.gz += apart ? by_dst(-ez) * slope : 0.f;
        } else {
            const float s = slope * __builtin_amdgcn_rcpf(dst);
            a.gx += apart ? -ex * s : 0.f;
            a.gy += apart ? -ey * s : 0.f;
            a.gz += apart ? -ez * s : 0.f;
        }
    }
}

// The candidate source of a field kernel: FieldIso (the density sampler: sorted positions, K4's pair term), FieldVel (the
// velocity field, below) or FieldAniso (ws_sample_aniso_*: sorted centres and their ellipsoids).  at(j) = {position, id
// bits} of sorted candidate j; pair() adds candidate j, which passed the isotropic distance test.
//
// A source the brick kernel can stage says so with three more members: chunk, the candidates staged at a time; payload(j),
// what it stages of candidate j beside position and cell code (staged<GRAD> = whether it stages one at all); and term(),
// pair() with that payload in place of j.  FieldAniso has none of them: k_field_bricks does not compile over it.
struct FieldNone {};
struct FieldIso {
    const float4 *__restrict__ spos;
    static constexpr uint32_t chunk = 512;  // 8 KiB of LDS per wave
    using Payload = FieldNone;
    template <bool GRAD>
    static constexpr bool staged = false;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void term(const WsDev &d, float ex, float ey, float ez, float d2, FieldNone, FieldAcc &a) const
    {
        field_pair<IEEE, GRAD>(d, ex, ey, ez, d2, a);
    }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t, float ex, float ey, float ez, float d2, FieldAcc &a) const
    {
        term<IEEE, GRAD>(d, ex, ey, ez, d2, FieldNone{}, a);
    }
};

// ws_sample_aniso_*: candidates are the particles' CENTRES c_j binned like positions, each with its ellipsoid M_j (symmetric:
// xx yy zz xy xz yz) and f_j = det M_j in smf[2j] = {xx, yy, zz, xy}, smf[2j + 1] = {xz, yz, f, 0}.  A candidate that
// passed the isotropic test counts iff dM2 = |u|^2 <= d2_accept, u = M e; its terms are the isotropic ones with e -> v =
// M u and d -> dM, times f last (include/wsfluid.h).  M = I, f = 1 gives field_pair's bits.
struct FieldAniso {
    const float4 *__restrict__ srec;  // {c, id bits} in cell order
    const float4 *__restrict__ smf;
    __device__ __forceinline__ float4 at(uint32_t j) const { return srec[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float, FieldAcc &a) const
    {
        const float4 m0 = smf[2 * (size_t)j], m1 = smf[2 * (size_t)j + 1];
        const float mxx = m0.x, myy = m0.y, mzz = m0.z, mxy = m0.w, mxz = m1.x, myz = m1.y, f = m1.z;
        const float ux = (mxx * ex + mxy * ey) + mxz * ez;
        const float uy = (mxy * ex + myy * ey) + myz * ez;
        const float uz = (mxz * ex + myz * ey) + mzz * ez;
        const float dm2 = ux * ux + uy * uy + uz * uz;
        if (dm2 > d.d2_accept) return;
        const float dst = ws_sqrt<IEEE>(dm2);
        a.rho += sk_density(d, dst) * f;
        if constexpr (GRAD) {
            const float vx = (mxx * ux + mxy * uy) + mxz * uz;
            const float vy = (mxy * ux + myy * uy) + myz * uz;
            const float vz = (mxz * ux + myz * uy) + mzz * uz;
            const float slope = sk_der(d, dst);
            const bool apart = dst > 0.f;
            if constexpr (IEEE) {
                const WsDivisor<IEEE> by_dst(dst);
                a.gx += apart ? (by_dst(-vx) * slope) * f : 0.f;
                a.gy += apart ? (by_dst(-vy) * slope) * f : 0.f;
                a.gz += apart ? (by_dst(-vz) * slope) * f : 0.f;
            } else {
                const float s = slope * __builtin_amdgcn_rcpf(dst);
                a.gx += apart ? (-vx * s) * f : 0.f;
                a.gy += apart ? (-vy * s) * f : 0.f;
                a.gz += apart ? (-vz * s) * f : 0.f;
            }
        }
    }
};

// The definition: the 27 cells around the query's (clamped) cell, as 9 contiguous z-runs in increasing cell id.
// start has ncells + 1 entries (start[ncells] = n).
// Acc: the accumulator the source's pair() adds to (FieldAcc; the whitewater sources carry lanes of their own), zeroed here.
template <bool IEEE, bool GRAD, class Src, class Acc = FieldAcc>
__device__ __forceinline__ Acc field_sweep(const WsDev &d, const uint32_t *__restrict__ start, const Src &src, float4 o)
{
    Acc a = {};
    const int cx = field_axis_cell(d, 0, o.x), cy = field_axis_cell(d, 1, o.y), cz = field_axis_cell(d, 2, o.z);
    const int z0 = max(cz - 1, 0), z1 = min(cz + 1, d.dim[2] - 1);
    for (int x = max(cx - 1, 0); x <= min(cx + 1, d.dim[0] - 1); x++) {
        for (int y = max(cy - 1, 0); y <= min(cy + 1, d.dim[1] - 1); y++) {
            const uint32_t col = (uint32_t)(x * d.dim[1] + y) * (uint32_t)d.dim[2];
            const uint32_t b = start[col + z0], e = start[col + z1 + 1];
            for (uint32_t j = b; j < e; j++) {
                const float4 q = src.at(j);
                const float ex = q.x - o.x, ey = q.y - o.y, ez = q.z - o.z;
                const float d2 = ex * ex + ey * ey + ez * ez;
                if (d2 > d.d2_accept) continue;
                src.template pair<IEEE, GRAD>(d, j, ex, ey, ez, d2, a);
            }
        }
    }
    return a;
}

// ---------------------------------------------------------------------------------
// velocity field and tracer advection (ws_sample_velocity_grid / _points, ws_advect_points; never inside ws_step)
//
// include/wsfluid.h pins the field: per accepted candidate w = the density sampler's term, rho += w, M_a += w * v_a
// (product rounded, then the sum), u = M / rho correctly rounded where rho > 0 and +0 elsewhere.  The momentum sums
// ride in FieldAcc's gradient lanes through field_sweep (GRAD = the momentum is wanted), so rho is the density sampler's
// bits by construction: the same operations on the same candidates in the same order.
// ---------------------------------------------------------------------------------
// a slab's gathered {position, velocity} records by id (WS_PACK_POSVEL: 6 floats) as two arrays of 3 (pos may be nullptr)
__global__ void __launch_bounds__(WS_BLOCK) k_field_split(const float *__restrict__ pv, float *__restrict__ pos,
                                                          float *__restrict__ vel, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *r = pv + 6 * (size_t)i;
    if (pos) {
        pos[3 * (size_t)i] = r[0];
        pos[3 * (size_t)i + 1] = r[1];
        pos[3 * (size_t)i + 2] = r[2];
    }
    vel[3 * (size_t)i] = r[3];
    vel[3 * (size_t)i + 1] = r[4];
    vel[3 * (size_t)i + 2] = r[5];
}

void wsk_field_split(hipStream_t s, const float *pv, float *pos, float *vel, uint32_t n)
{
    hipLaunchKernelGGL(k_field_split, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, pv, pos, vel, n);
}

// k_field_gather's companion: svel[j] = velocity of particle perm[j], beside spos[j]
__global__ void __launch_bounds__(WS_BLOCK) k_field_gather_vel(const uint32_t *__restrict__ perm, const float *__restrict__ vxyz,
                                                               float4 *__restrict__ svel, uint32_t n)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t id = perm[j];
    svel[j] = make_float4(vxyz[3 * id], vxyz[3 * id + 1], vxyz[3 * id + 2], 0.f);
}

void wsk_field_gather_vel(hipStream_t s, const uint32_t *perm, const float *vxyz, float4 *svel, uint32_t n)
{
    hipLaunchKernelGGL(k_field_gather_vel, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, perm, vxyz, svel, n);
}

// The candidate source of the velocity field: FieldIso's positions and the velocities in the same order.  GRAD = the
// momentum sums are wanted; they take the accumulator's gradient lanes.  A staged candidate is then 32 B (position + cell
// code, and the velocity), so the chunk is 256 candidates: 8 KiB of LDS per wave, what the density brick stages, and with
// the run tables 18 one-wave workgroups per CU of 160 KiB -- the residency the density brick runs at.  Without GRAD the
// chunk stays 256 and no velocity is staged.
struct FieldVel {
    const float4 *__restrict__ spos;
    const float4 *__restrict__ svel;
    static constexpr uint32_t chunk = 256;
    using Payload = float4;
    template <bool GRAD>
    static constexpr bool staged = GRAD;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    __device__ __forceinline__ float4 payload(uint32_t j) const { return svel[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void term(const WsDev &d, float, float, float, float d2, const float4 &v, FieldAcc &a) const
    {
        const float w = sk_density(d, ws_sqrt<IEEE>(d2));
        a.rho += w;
        if constexpr (GRAD) {
            a.gx += w * v.x;
            a.gy += w * v.y;
            a.gz += w * v.z;
        }
    }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float d2, FieldAcc &a) const
    {
        term<IEEE, GRAD>(d, ex, ey, ez, d2, GRAD ? svel[j] : float4{}, a);
    }
};

// u = M / rho (correctly rounded whatever the handle's flags) where rho > 0, else (+0, +0, +0)
__device__ __forceinline__ float4 field_velocity(const FieldAcc &a)
{
    if (!(a.rho > 0.f)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(a.gx / a.rho, a.gy / a.rho, a.gz / a.rho, 0.f);
}

__device__ __forceinline__ void field_store3(float *__restrict__ out, size_t at, const float4 &v)
{
    out[3 * at] = v.x;
    out[3 * at + 1] = v.y;
    out[3 * at + 2] = v.z;
}

// the unit normal -g / sqrtf(g . g) of a gradient g (correctly rounded), (0, 0, 0) where g . g == 0
__device__ __forceinline__ float4 field_unit_normal(float gx, float gy, float gz)
{
    const float gg = gx * gx + gy * gy + gz * gz;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (gg != 0.f) {
        const float len = sqrtf(gg);
        nx = -gx / len;
        ny = -gy / len;
        nz = -gz / len;
    }
    return make_float4(nx, ny, nz, 0.f);
}

// ---------------------------------------------------------------------------------
// the two field kernels, over a candidate source, the queries and what is stored of a query's sums
// ---------------------------------------------------------------------------------
// The queries of the points form: the m points of xyz, or the nodes of g (node index = lane index, x fastest) -- the grid
// call's form below one node per cell.
struct QueryPoints {
    const float *__restrict__ xyz;
    uint32_t m;
    __device__ __forceinline__ uint32_t count() const { return m; }
    __device__ __forceinline__ float4 at(uint32_t t) const
    {
        return make_float4(xyz[3 * (size_t)t], xyz[3 * (size_t)t + 1], xyz[3 * (size_t)t + 2], 0.f);
    }
};
struct QueryNodes {
    WsFieldGrid g;
    __device__ __forceinline__ uint32_t count() const { return g.nx * g.ny * g.nz; }
    __device__ __forceinline__ float4 at(uint32_t t) const
    {
        const uint32_t i = t % g.nx, r = t / g.nx;
        return field_node(g, i, r % g.ny, r / g.ny);
    }
};

// What a query keeps of its sums, at slot `at`: the density and its gradient (either may be nullptr), or the velocity
// field's u = M / rho (GRAD: it is wanted, vel != nullptr) and density (may be nullptr).  plain: put() is stores alone, so
// the brick kernel's fallback makes its own and returns; a store that divides is not duplicated into the fallback but made
// once, at the kernel's end ("Grid kernel", has the measurement behind the two shapes).
struct StoreDensity {
    float *__restrict__ rho;
    float *__restrict__ grad;
    static constexpr bool plain = true;
    template <bool GRAD>
    __device__ __forceinline__ void put(const FieldAcc &a, size_t at) const
    {
        if (rho) rho[at] = a.rho;
        if (grad) field_store3(grad, at, make_float4(a.gx, a.gy, a.gz, 0.f));
    }
};
struct StoreVelocity {
    float *__restrict__ vel;
    float *__restrict__ rho;
    static constexpr bool plain = false;
    template <bool GRAD>
    __device__ __forceinline__ void put(const FieldAcc &a, size_t at) const
    {
        if (rho) rho[at] = a.rho;
        if constexpr (GRAD) field_store3(vel, at, field_velocity(a));
    }
};

// Points form (the definition): one lane per query, one field_sweep.
template <bool IEEE, bool GRAD, class Src, class Query, class Store>
__global__ void __launch_bounds__(WS_BLOCK) k_field_points(WsDev d, const uint32_t *__restrict__ start, Src src, Query query,
                                                           Store store)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (t >= query.count()) return;
    store.template put<GRAD>(field_sweep<IEEE, GRAD, Src, field_acc_t<Src>>(d, start, src, query.at(t)), t);
}

// Grid form (the hot path): one wave per brick of 4 x 4 x 4 nodes, lane l = node (l & 3, (l >> 2) & 3, l >> 4) of the
// brick.  The brick's support is the box of cells [first node's cell - 1, last node's cell + 1] per axis (clamped to
// the grid; cell coordinates are monotone in the node index), i.e. at most 64 z-runs (one per (x, y) column, x
// slower) when the node spacing is at most h.  The wave stages the runs' candidates into LDS in that order -- which
// is increasing cell id, then particle id -- Src::chunk at a time, the source's payload beside them, and every lane tests
// every staged candidate against its node.  A candidate counts for a node iff it passes the distance test AND lies in
// the node's own 27 cells (the points form never sees the others; the cell test is made on accepted candidates only),
// so each node sums the same terms in the same order as the points form: bit-identical.  A brick whose support holds no
// particle (air) writes zeros without a candidate loop.
#define FB_COLS 64  // z-runs a brick may span (6 x 6 = 36 at spacing h; more only through rounding at exactly h)

// staged candidate: xyz and the cell relative to the brick's first cell, one byte per axis + 1 (w lane)
__device__ __forceinline__ uint32_t field_pack_cell(int x, int y, int z) { return (uint32_t)((x + 1) << 16 | (y + 1) << 8 | (z + 1)); }

template <bool IEEE, bool GRAD, class Src, class Store>
__global__ void __launch_bounds__(64) k_field_bricks(WsDev d, const uint32_t *__restrict__ start, Src src, WsFieldGrid g,
                                                     uint32_t bx_n, uint32_t by_n, Store store)
{
    constexpr uint32_t CHUNK = Src::chunk;
    constexpr bool STAGED = Src::template staged<GRAD>;
    __shared__ float4 s_q[CHUNK];
    __shared__ typename Src::Payload s_v[STAGED ? CHUNK : 1];
    __shared__ uint32_t s_pre[FB_COLS + 1], s_b[FB_COLS];
    const uint32_t lane = threadIdx.x;
    const uint32_t bid = blockIdx.x;
    const uint32_t bi = bid % bx_n, bj = (bid / bx_n) % by_n, bk = bid / (bx_n * by_n);
    const uint32_t i0 = bi * 4u, j0 = bj * 4u, k0 = bk * 4u;
    const uint32_t i = i0 + (lane & 3u), j = j0 + ((lane >> 2) & 3u), k = k0 + (lane >> 4);
    const bool valid = i < g.nx && j < g.ny && k < g.nz;
    const float4 o = field_node(g, i, j, k);
    // the brick's cell box from its first and last VALID node (wave-uniform)
    const uint32_t il = min(i0 + 3u, g.nx - 1u), jl = min(j0 + 3u, g.ny - 1u), kl = min(k0 + 3u, g.nz - 1u);
    const float4 lo = field_node(g, i0, j0, k0), hi = field_node(g, il, jl, kl);
    const int x0 = max(field_axis_cell(d, 0, lo.x) - 1, 0), x1 = min(field_axis_cell(d, 0, hi.x) + 1, d.dim[0] - 1);
    const int y0 = max(field_axis_cell(d, 1, lo.y) - 1, 0), y1 = min(field_axis_cell(d, 1, hi.y) + 1, d.dim[1] - 1);
    const int z0 = max(field_axis_cell(d, 2, lo.z) - 1, 0), z1 = min(field_axis_cell(d, 2, hi.z) + 1, d.dim[2] - 1);
    const int ny_c = y1 - y0 + 1;
    const int ncol = (x1 - x0 + 1) * ny_c;
    const size_t at = ((size_t)k * g.ny + j) * g.nx + i;
    field_acc_t<Src> a = {};
    if (ncol > FB_COLS) {  // (a spacing the host would not send here: take the points form, lane by lane)
        if (valid) a = field_sweep<IEEE, GRAD, Src, field_acc_t<Src>>(d, start, src, o);
        if constexpr (Store::plain) {
            if (valid) store.template put<GRAD>(a, at);
            return;
        }
    } else {
        // the runs: lane c = column c (x slower), then an exclusive scan of their lengths
        uint32_t len = 0, b = 0;
        if ((int)lane < ncol) {
            const int x = x0 + (int)lane / ny_c, y = y0 + (int)lane % ny_c;
            const uint32_t col = (uint32_t)(x * d.dim[1] + y) * (uint32_t)d.dim[2];
            b = start[col + z0];
            len = start[col + z1 + 1] - b;
        }
        const uint32_t incl = wave_incl_scan(len);
        const uint32_t total = __shfl(incl, 63, 64);
        if (total != 0u) {
            s_pre[lane] = incl - len;
            s_b[lane] = b;
            if (lane == 0) s_pre[FB_COLS] = total;
            // this lane's node: its 27 cells, relative to the brick's box (fields >= 0; see field_pack_cell)
            const uint32_t own = (uint32_t)((field_axis_cell(d, 0, o.x) - x0) << 16 | (field_axis_cell(d, 1, o.y) - y0) << 8 |
                                            (field_axis_cell(d, 2, o.z) - z0));
            for (uint32_t base = 0; base < total; base += CHUNK) {
                const uint32_t cnt = min(CHUNK, total - base);
                __syncthreads();  // (the previous chunk has been consumed; s_pre / s_b are written)
                for (uint32_t t = lane; t < cnt; t += 64u) {
                    const uint32_t v = base + t;
                    int lo_c = 0, hi_c = ncol - 1;  // last column whose prefix is <= v (empty columns share a prefix)
                    while (lo_c < hi_c) {
                        const int mid = (lo_c + hi_c + 1) >> 1;
                        if (s_pre[mid] <= v) lo_c = mid;
                        else hi_c = mid - 1;
                    }
                    const uint32_t idx = s_b[lo_c] + (v - s_pre[lo_c]);
                    const float4 q = src.at(idx);
                    const uint32_t code = field_pack_cell(lo_c / ny_c, lo_c % ny_c, field_axis_cell(d, 2, q.z) - z0);
                    s_q[t] = make_float4(q.x, q.y, q.z, __uint_as_float(code));
                    if constexpr (STAGED) s_v[t] = src.payload(idx);
                }
                __syncthreads();
                for (uint32_t t = 0; t < cnt; t++) {
                    const float4 q = s_q[t];
                    const float ex = q.x - o.x, ey = q.y - o.y, ez = q.z - o.z;
                    const float d2 = ex * ex + ey * ey + ez * ez;
                    if (d2 > d.d2_accept) continue;
                    // in the node's 27 cells: every byte of code - own lies in [0, 2] (guard bit 7 keeps the bytes apart)
                    if ((((__float_as_uint(q.w) | 0x808080u) - own) & 0xFCFCFCu) != 0x808080u) continue;
                    src.template term<IEEE, GRAD>(d, ex, ey, ez, d2, s_v[STAGED ? t : 0u], a);
                }
            }
        }
    }
    if (valid) store.template put<GRAD>(a, at);
}

// Whether the brick kernel can stage a source: the source declares its chunk.
template <class Src, class = void>
constexpr bool field_stageable = false;
template <class Src>
constexpr bool field_stageable<Src, std::void_t<decltype(Src::chunk)>> = true;

// One field call: the m points of xyz (grid6 == nullptr), or the grid of grid6 = origin xyz, spacing xyz and dims (m its
// nodes) -- with the brick kernel where `bricks` (the host sends grids of spacing <= h on every axis there, DESIGN.md
// 9.4) and the source can be staged, else node by node in the points form.
template <class Src, class Store>
void field_launch(hipStream_t s, const WsDev &d, const uint32_t *start, Src src, Store store, bool ieee, bool grad_on,
                  const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks)
{
    const auto points = [&](auto query) {
        ws_dispatch([&](auto I, auto G) {
            hipLaunchKernelGGL((k_field_points<I(), G(), Src, decltype(query), Store>), dim3(cdiv(m, WS_BLOCK)),
                               dim3(WS_BLOCK), 0, s, d, start, src, query, store);
        }, ieee, grad_on);
    };
    if (!grid6) return points(QueryPoints{xyz, m});
    const WsFieldGrid g = {grid6[0], grid6[1], grid6[2], grid6[3], grid6[4], grid6[5], dims[0], dims[1], dims[2]};
    if constexpr (field_stageable<Src>) {
        if (bricks) {
            const uint32_t bx = cdiv(dims[0], 4u), by = cdiv(dims[1], 4u), bz = cdiv(dims[2], 4u);
            ws_dispatch([&](auto I, auto G) {
                hipLaunchKernelGGL((k_field_bricks<I(), G(), Src, Store>), dim3(bx * by * bz), dim3(64), 0, s, d, start,
                                   src, g, bx, by, store);
            }, ieee, grad_on);
            return;
        }
    }
    points(QueryNodes{g});
}

void wsk_field_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *smf, bool ieee,
                      bool grad_on, const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks,
                      float *rho, float *grad)
{
    // The anisotropic field takes the points form on grids too (FieldAniso declares no chunk): a brick form of it (the
    // staged candidates' sorted indices in LDS, M and f loaded for accepted pairs) lost to the points form on sparse C3 at
    // spacing h.
    const StoreDensity store = {rho, grad};
    if (smf) field_launch(s, d, start, FieldAniso{spos, smf}, store, ieee, grad_on, xyz, m, grid6, dims, bricks);
    else field_launch(s, d, start, FieldIso{spos}, store, ieee, grad_on, xyz, m, grid6, dims, bricks);
}

void wsk_velocity_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                         const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks, float *vel,
                         float *rho)
{
    field_launch(s, d, start, FieldVel{spos, svel}, StoreVelocity{vel, rho}, ieee, vel != nullptr, xyz, m, grid6, dims, bricks);
}

// k_advect, one lane per tracer: a plain loop of midpoint steps through the frozen field, each sample one field_sweep --
// the points sampler's own definition, so a host that marches with ws_sample_velocity_points gets the same bits
// (include/wsfluid.h pins every rounding).  pts holds the tracers on entry and the final positions on return; a lane
// reads and writes its own slot only.  A tracer can leave the container or, with large velocities, reach +-inf or NaN:
// field_axis_cell's fminf / fmaxf clamp maps any float (NaN to cell 0) into the grid, so every sweep stays in bounds.
template <bool IEEE, bool FIELD>
__global__ void __launch_bounds__(WS_BLOCK) k_advect(WsDev d, const uint32_t *__restrict__ start, FieldVel src, float *pts,
                                                     uint32_t m, float dt, float hdt, uint32_t substeps,
                                                     float *__restrict__ vel, float *__restrict__ rho)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (t >= m) return;
    float4 p = make_float4(pts[3 * (size_t)t], pts[3 * (size_t)t + 1], pts[3 * (size_t)t + 2], 0.f);
    for (uint32_t k = 0; k < substeps; k++) {
        const FieldAcc a1 = field_sweep<IEEE, true>(d, start, src, p);
        if (a1.rho == 0.f) break;  // in the air: the tracer stays, and would at every later substep
        const float4 u1 = field_velocity(a1);
        const float4 q = make_float4(p.x + hdt * u1.x, p.y + hdt * u1.y, p.z + hdt * u1.z, 0.f);
        const FieldAcc a2 = field_sweep<IEEE, true>(d, start, src, q);
        const float4 u2 = a2.rho == 0.f ? u1 : field_velocity(a2);  // the midpoint left the fluid: an Euler step
        p = make_float4(p.x + dt * u2.x, p.y + dt * u2.y, p.z + dt * u2.z, 0.f);
    }
    field_store3(pts, t, p);
    if constexpr (FIELD) {
        const FieldAcc a = field_sweep<IEEE, true>(d, start, src, p);
        if (rho) rho[t] = a.rho;
        if (vel) field_store3(vel, t, field_velocity(a));
    }
}

void wsk_advect(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                float *pts, uint32_t m, float dt, uint32_t substeps, float *vel, float *rho)
{
    const FieldVel src = {spos, svel};
    const float hdt = 0.5f * dt;
    ws_dispatch([&](auto I, auto F) {
        hipLaunchKernelGGL((k_advect<I(), F()>), dim3(cdiv(m, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, src, pts, m, dt,
                           hdt, substeps, vel, rho);
    }, ieee, vel || rho);
}

// ---------------------------------------------------------------------------------
// whitewater (ws_read_whitewater / ws_emit_whitewater / ws_step_whitewater; never inside ws_step)
//
// include/wsfluid.h pins every operation.  The per-particle stage is two kernels, one lane per particle in the sampler's
// cell order (neighbouring lanes share candidates), each one field_sweep: k_whitewater_normals (pass A: the density
// gradient at x_i, IEEE form, as a unit normal beside spos) and k_whitewater_stage (pass B, which needs every neighbour's
// normal: trapped air, crest, alignment, energy, count, scattered by id).  The stage is IEEE arithmetic whatever the
// handle's flags.  Emission: k_whitewater_count (m_i by id), k_scan over m_i, k_whitewater_spawn (one lane per emitter,
// its spawns at its scanned offset).  k_whitewater_step: one lane per diffuse particle, the velocity field's sweep with
// a count lane, in the handle's arithmetic.  No LDS: the candidates come through the caches, as in k_aniso / k_advect.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float ww_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return ax * bx + ay * by + az * bz;
}

__global__ void __launch_bounds__(WS_BLOCK) k_whitewater_normals(WsDev d, const uint32_t *__restrict__ start,
                                                                 const float4 *__restrict__ spos, float4 *__restrict__ snrm,
                                                                 uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const FieldAcc g = field_sweep<true, true>(d, start, FieldIso{spos}, spos[i]);
    snrm[i] = field_unit_normal(g.gx, g.gy, g.gz);
}

// Pass B's accumulator and candidate source: positions, velocities and normals in cell order, and the query particle's
// own velocity and normal.
struct WhiteAcc {
    float t, k;
    uint32_t c;
};
struct FieldWhite {
    const float4 *__restrict__ spos;
    const float4 *__restrict__ svel;
    const float4 *__restrict__ snrm;
    float4 vi, ni;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float d2, WhiteAcc &a) const
    {
        const float dst = sqrtf(d2);
        if (!(dst > 0.f)) return;  // i itself, a coincident particle
        const float xx = -ex / dst, xy = -ey / dst, xz = -ez / dst;
        const float w = 1.f - dst / d.h;
        const float4 vj = svel[j];
        const float rx = vi.x - vj.x, ry = vi.y - vj.y, rz = vi.z - vj.z;
        const float s = sqrtf(ww_dot(rx, ry, rz, rx, ry, rz));
        if (s > 0.f) a.t += (s * (1.f - ww_dot(rx / s, ry / s, rz / s, xx, xy, xz))) * w;
        if (ww_dot(-xx, -xy, -xz, ni.x, ni.y, ni.z) < 0.f) {
            const float4 nj = snrm[j];
            a.k += (1.f - ww_dot(ni.x, ni.y, ni.z, nj.x, nj.y, nj.z)) * w;
        }
        a.c++;
    }
};

// by id: trapped[n], crest[n], align[n], energy[n], normal[3 n], nb[n]
__global__ void __launch_bounds__(WS_BLOCK) k_whitewater_stage(WsDev d, const uint32_t *__restrict__ start,
                                                               const float4 *__restrict__ spos, const float4 *__restrict__ svel,
                                                               const float4 *__restrict__ snrm, float *__restrict__ trapped,
                                                               float *__restrict__ crest, float *__restrict__ align,
                                                               float *__restrict__ energy, float *__restrict__ normal,
                                                               uint32_t *__restrict__ nb, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 o = spos[i], v = svel[i], nh = snrm[i];
    const size_t id = __float_as_uint(o.w);
    const FieldWhite src = {spos, svel, snrm, v, nh};
    const WhiteAcc a = field_sweep<true, false, FieldWhite, WhiteAcc>(d, start, src, o);
    const float vv = ww_dot(v.x, v.y, v.z, v.x, v.y, v.z);
    const float sv = sqrtf(vv);
    trapped[id] = a.t;
    crest[id] = a.k;
    align[id] = sv > 0.f ? ww_dot(v.x / sv, v.y / sv, v.z / sv, nh.x, nh.y, nh.z) : 0.f;
    energy[id] = 0.5f * vv;
    nb[id] = a.c;
    field_store3(normal, id, nh);
}

void wsk_whitewater_stage(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel,
                          float4 *snrm, float *trapped, float *crest, float *align, float *energy, float *normal, uint32_t *nb,
                          uint32_t n)
{
    const dim3 grid(cdiv(n, WS_BLOCK)), block(WS_BLOCK);
    hipLaunchKernelGGL(k_whitewater_normals, grid, block, 0, s, d, start, spos, snrm, n);
    hipLaunchKernelGGL(k_whitewater_stage, grid, block, 0, s, d, start, spos, svel, snrm, trapped, crest, align, energy, normal,
                       nb, n);
}

// ---------------------------------------------------------------------------------
// surface tension and XSPH smoothing (ws_read_cohesion / ws_apply_cohesion; never inside ws_step)
//
// include/wsfluid.h pins every operation; IEEE arithmetic whatever the handle's flags.  The whitewater stage's shape: two
// kernels, one lane per particle in the sampler's cell order, each one field_sweep.  k_cohesion_normals (pass A): the
// density sampler's sums at x_i in their IEEE form, stored as ONE float4 {n_i = h g_i / rho_i, rho_i} beside spos, so that
// pass B fetches a candidate's normal and density with one 16-byte load.  k_cohesion_stage (pass B): per contributing
// candidate three 16-byte loads through the caches (position, velocity, {normal, density}), no LDS; the results scattered
// by id as 16-byte records -- {dv, count} (what the edit gathers, EditCohesion in ws_edits.hip) and, for ws_read_cohesion only,
// {normal, density} -- which k_cohesion_unpack, a streaming pass, splits into the call's four output arrays.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(WS_BLOCK) k_cohesion_normals(WsDev d, const uint32_t *__restrict__ start,
                                                               const float4 *__restrict__ spos, float4 *__restrict__ snd,
                                                               uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const FieldAcc g = field_sweep<true, true>(d, start, FieldIso{spos}, spos[i]);
    snd[i] = make_float4((d.h * g.gx) / g.rho, (d.h * g.gy) / g.rho, (d.h * g.gz) / g.rho, g.rho);  // (rho has i's own term: > 0)
}

// Pass B's accumulator and candidate source: positions, velocities and {normal, density} in cell order, the query
// particle's own velocity and {normal, density}, and the call's constants.
struct CohesionAcc {
    float ax, ay, az, xx, xy, xz;
    uint32_t c;
};
struct FieldCohesion {
    const float4 *__restrict__ spos;
    const float4 *__restrict__ svel;
    const float4 *__restrict__ snd;
    float4 vi, ni;
    WsCohesion k;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float d2, CohesionAcc &a) const
    {
        const float dst = sqrtf(d2);
        if (!(dst > 0.f)) return;  // i itself, a coincident particle
        const float xx = -ex / dst, xy = -ey / dst, xz = -ez / dst;
        const float4 nj = snd[j], vj = svel[j];
        const float q = 2.f / (ni.w + nj.w);
        const float K = k.rho0 * q;
        const float t = d.h - dst;
        const float pp = ((t * t) * t) * ((dst * dst) * dst);
        const float s = 2.f * dst > d.h ? pp : 2.f * pp - k.h664;
        const float fc = k.cohesion * (k.kc * s);
        a.ax = a.ax - K * (fc * xx + k.curvature * (ni.x - nj.x));
        a.ay = a.ay - K * (fc * xy + k.curvature * (ni.y - nj.y));
        a.az = a.az - K * (fc * xz + k.curvature * (ni.z - nj.z));
        const float w = sk_density(d, dst);
        a.xx = a.xx + ((vj.x - vi.x) * w) * q;
        a.xy = a.xy + ((vj.y - vi.y) * w) * q;
        a.xz = a.xz + ((vj.z - vi.z) * w) * q;
        a.c++;
    }
};

// by id: dvc[n] = {dv, c (bits)}, and if wanted nrho[n] = {n_i, rho_i}
__global__ void __launch_bounds__(WS_BLOCK) k_cohesion_stage(WsDev d, const uint32_t *__restrict__ start,
                                                             const float4 *__restrict__ spos, const float4 *__restrict__ svel,
                                                             const float4 *__restrict__ snd, WsCohesion k,
                                                             float4 *__restrict__ dvc, float4 *__restrict__ nrho, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 o = spos[i], v = svel[i], nd = snd[i];
    const size_t id = __float_as_uint(o.w);
    const FieldCohesion src = {spos, svel, snd, v, nd, k};
    const CohesionAcc a = field_sweep<true, false, FieldCohesion, CohesionAcc>(d, start, src, o);
    float4 out = make_float4(0.f, 0.f, 0.f, __uint_as_float(a.c));
    if (a.c) {
        out.x = k.dt * a.ax + k.xsph * a.xx;
        out.y = k.dt * a.ay + k.xsph * a.xy;
        out.z = k.dt * a.az + k.xsph * a.xz;
    }
    dvc[id] = out;
    if (nrho) nrho[id] = nd;
}

void wsk_cohesion_stage(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel,
                        float4 *snd, const WsCohesion &k, float4 *dvc, float4 *nrho, uint32_t n)
{
    const dim3 grid(cdiv(n, WS_BLOCK)), block(WS_BLOCK);
    hipLaunchKernelGGL(k_cohesion_normals, grid, block, 0, s, d, start, spos, snd, n);
    hipLaunchKernelGGL(k_cohesion_stage, grid, block, 0, s, d, start, spos, svel, snd, k, dvc, nrho, n);
}

// ws_read_cohesion's outputs from the stage's records, by id: normal[3 n], rho[n], dv[3 n], nb[n]
__global__ void __launch_bounds__(WS_BLOCK) k_cohesion_unpack(const float4 *__restrict__ dvc, const float4 *__restrict__ nrho,
                                                              float *__restrict__ normal, float *__restrict__ rho,
                                                              float *__restrict__ dv, uint32_t *__restrict__ nb, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 a = dvc[i], b = nrho[i];
    field_store3(normal, i, b);
    rho[i] = b.w;
    field_store3(dv, i, a);
    nb[i] = __float_as_uint(a.w);
}

void wsk_cohesion_unpack(hipStream_t s, const float4 *dvc, const float4 *nrho, float *normal, float *rho, float *dv, uint32_t *nb,
                         uint32_t n)
{
    hipLaunchKernelGGL(k_cohesion_unpack, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, dvc, nrho, normal, rho, dv, nb, n);
}

// ---------------------------------------------------------------------------------
// per-particle attributes (ws_paint_attributes / ws_diffuse_attributes / ws_sample_attribute_*; never inside ws_step)
//
// include/wsfluid.h pins every operation.  The attributes live BY ID, one float4 per particle (ws_handle::attr).  Paint is
// a streaming pass by id with the brushes as a by-value kernel argument (768 B, scalar loads in the wave-uniform loop, as
// ws_apply_forces carries its emitters).  Diffusion is the cohesion stage's shape: one lane per particle in the sampler's
// cell order, one field_sweep each, no LDS.  k_attr_density (pass A): the density sampler's IEEE sum at x_i, no gradient.
// k_attr_diffuse (pass B): positions, densities and attributes IN CELL ORDER, so that a wave's gathers stay inside its
// neighbourhood -- per contributing candidate two 16-byte loads (position, attribute) and one 4-byte load (density).  The
// iterations ping-pong between two cell-ordered arrays; one scatter by id follows the last.
// ---------------------------------------------------------------------------------
template <bool COUNTS>
__global__ void __launch_bounds__(WS_BLOCK) k_attr_paint(WsBrushArgs a, const float *__restrict__ xyz, float4 *__restrict__ attr,
                                                         uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    const bool active = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        px = xyz[3 * (size_t)i];
        py = xyz[3 * (size_t)i + 1];
        pz = xyz[3 * (size_t)i + 2];
        A = attr[i];
    }
    bool hit = false;
    for (uint32_t e = 0; e < a.k; e++) {
        const ws_brush &b = a.bs.e[e];
        const float qx = px - b.centre[0], qy = py - b.centre[1], qz = pz - b.centre[2];
        const float dst = sqrtf(qx * qx + qy * qy + qz * qz);
        const bool in = active && dst < b.radius;
        if constexpr (COUNTS) {
            const uint32_t c = (uint32_t)__popcll(__ballot(in));
            if (c && (threadIdx.x & 63u) == 0u) atomicAdd(&a.painted[e], c);
        }
        if (!in) continue;
        hit = true;
        const float t = dst / b.radius;
        const float w = 1.f - b.falloff * t;
        const float s = b.strength * w;
        const float keep = 1.f - s;
        const bool mix = b.kind == WS_BRUSH_MIX;
        const auto channel = [&](float &x, uint32_t c) {
            if (!((b.channels >> c) & 1u)) return;
            const float add = s * b.value[c];
            x = mix ? keep * x + add : x + add;
        };
        channel(A.x, 0u);
        channel(A.y, 1u);
        channel(A.z, 2u);
        channel(A.w, 3u);
    }
    if (hit) attr[i] = A;
}

void wsk_attr_paint(hipStream_t s, const WsBrushArgs &a, const float *xyz, float4 *attr, uint32_t n)
{
    if (!n) return;
    ws_dispatch([&](auto counts) {
        hipLaunchKernelGGL(k_attr_paint<counts()>, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, a, xyz, attr, n);
    }, a.painted != nullptr);
}

// sa[j] = the attribute of the particle at sorted slot j (its id rides in spos[j].w)
__global__ void __launch_bounds__(WS_BLOCK) k_attr_gather(const float4 *__restrict__ spos, const float4 *__restrict__ attr,
                                                          float4 *__restrict__ sa, uint32_t n)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= n) return;
    sa[j] = attr[__float_as_uint(spos[j].w)];
}

void wsk_attr_gather(hipStream_t s, const float4 *spos, const float4 *attr, float4 *sa, uint32_t n)
{
    hipLaunchKernelGGL(k_attr_gather, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, spos, attr, sa, n);
}

// ... and back: attr[id of slot j] = sa[j]
__global__ void __launch_bounds__(WS_BLOCK) k_attr_scatter(const float4 *__restrict__ spos, const float4 *__restrict__ sa,
                                                           float4 *__restrict__ attr, uint32_t n)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= n) return;
    attr[__float_as_uint(spos[j].w)] = sa[j];
}

void wsk_attr_scatter(hipStream_t s, const float4 *spos, const float4 *sa, float4 *attr, uint32_t n)
{
    hipLaunchKernelGGL(k_attr_scatter, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, spos, sa, attr, n);
}

// pass A: srho[i] = the density sampler's IEEE sum at x_i (i's own term included: > 0), in spos' order
__global__ void __launch_bounds__(WS_BLOCK) k_attr_density(WsDev d, const uint32_t *__restrict__ start,
                                                           const float4 *__restrict__ spos, float *__restrict__ srho, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    srho[i] = field_sweep<true, false>(d, start, FieldIso{spos}, spos[i]).rho;
}

void wsk_attr_density(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, float *srho, uint32_t n)
{
    hipLaunchKernelGGL(k_attr_density, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, spos, srho, n);
}

// Pass B's five-word accumulator and candidate source: the query particle's own attribute and density beside the arrays.
struct AttrAcc {
    float s0, s1, s2, s3;
    uint32_t c;
};
struct FieldAttr {
    const float4 *__restrict__ spos;
    const float *__restrict__ srho;
    const float4 *__restrict__ sa;
    float4 ai;
    float rhoi;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float, float, float, float d2, AttrAcc &a) const
    {
        const float dst = sqrtf(d2);
        if (!(dst > 0.f)) return;  // i itself, a coincident particle
        const float4 aj = sa[j];
        const float q = 2.f / (rhoi + srho[j]);
        const float g = sk_density(d, dst) * q;
        a.s0 = a.s0 + (aj.x - ai.x) * g;
        a.s1 = a.s1 + (aj.y - ai.y) * g;
        a.s2 = a.s2 + (aj.z - ai.z) * g;
        a.s3 = a.s3 + (aj.w - ai.w) * g;
        a.c++;
    }
};

// one iteration, cell order in and out; r = fl(rate * dt) per channel (0: the channel keeps its bits).  affected: the
// WS_COHESION_SLOTS partial counts the first iteration of a call adds to (c_i does not change between iterations), or nullptr.
__global__ void __launch_bounds__(WS_BLOCK) k_attr_diffuse(WsDev d, const uint32_t *__restrict__ start,
                                                           const float4 *__restrict__ spos, const float *__restrict__ srho,
                                                           const float4 *__restrict__ sa, float4 r, float4 *__restrict__ out,
                                                           uint32_t *__restrict__ affected, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    const bool active = i < n;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    AttrAcc a = {};
    if (active) {
        A = sa[i];
        const FieldAttr src = {spos, srho, sa, A, srho[i]};
        a = field_sweep<true, false, FieldAttr, AttrAcc>(d, start, src, spos[i]);
    }
    const bool hit = a.c > 0u;
    if (affected) {  // (kernel-uniform)
        const uint32_t k = (uint32_t)__popcll(__ballot(hit));
        const uint32_t slot = (i >> 6) % WS_COHESION_SLOTS;
        if (k && (threadIdx.x & 63u) == 0u) atomicAdd(affected + slot * WS_COHESION_SLOT_WORDS, k);
    }
    if (!active) return;
    if (hit) {
        if (r.x != 0.f) A.x = A.x + r.x * a.s0;
        if (r.y != 0.f) A.y = A.y + r.y * a.s1;
        if (r.z != 0.f) A.z = A.z + r.z * a.s2;
        if (r.w != 0.f) A.w = A.w + r.w * a.s3;
    }
    out[i] = A;
}

void wsk_attr_diffuse(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float *srho, const float4 *sa,
                      const float *r4, float4 *out, uint32_t *affected, uint32_t n)
{
    hipLaunchKernelGGL(k_attr_diffuse, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, spos, srho, sa,
                       make_float4(r4[0], r4[1], r4[2], r4[3]), out, affected, n);
}

// The attribute field's source and store: FieldVel's shape with four moment sums beside rho (an accumulator of its own,
// AttrFieldAcc) and a store of four quotients.  GRAD = the values are wanted.  A staged candidate is 32 B (position + cell
// code, and the attribute): FieldVel's chunk and residency.  rho takes the density sampler's operations on the same
// candidates in the same order: the same bits.
struct AttrFieldAcc {
    float rho, m0, m1, m2, m3;
};
struct FieldAttrValue {
    const float4 *__restrict__ spos;
    const float4 *__restrict__ sa;
    using Acc = AttrFieldAcc;
    static constexpr uint32_t chunk = 256;
    using Payload = float4;
    template <bool GRAD>
    static constexpr bool staged = GRAD;
    __device__ __forceinline__ float4 at(uint32_t j) const { return spos[j]; }
    __device__ __forceinline__ float4 payload(uint32_t j) const { return sa[j]; }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void term(const WsDev &d, float, float, float, float d2, const float4 &v, AttrFieldAcc &a) const
    {
        const float w = sk_density(d, ws_sqrt<IEEE>(d2));
        a.rho += w;
        if constexpr (GRAD) {
            a.m0 += w * v.x;
            a.m1 += w * v.y;
            a.m2 += w * v.z;
            a.m3 += w * v.w;
        }
    }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float d2, AttrFieldAcc &a) const
    {
        term<IEEE, GRAD>(d, ex, ey, ez, d2, GRAD ? sa[j] : float4{}, a);
    }
};
// value = M / rho (correctly rounded whatever the handle's flags) where rho > 0, else four +0: one 16-byte store
struct StoreAttr {
    float4 *__restrict__ value;
    float *__restrict__ rho;
    static constexpr bool plain = false;
    template <bool GRAD>
    __device__ __forceinline__ void put(const AttrFieldAcc &a, size_t at) const
    {
        if (rho) rho[at] = a.rho;
        if constexpr (GRAD) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.rho > 0.f) v = make_float4(a.m0 / a.rho, a.m1 / a.rho, a.m2 / a.rho, a.m3 / a.rho);
            value[at] = v;
        }
    }
};

void wsk_attr_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *sa, bool ieee,
                     const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks, float4 *value, float *rho)
{
    field_launch(s, d, start, FieldAttrValue{spos, sa}, StoreAttr{value, rho}, ieee, value != nullptr, xyz, m, grid6, dims, bricks);
}

// The gathered state records of slab handles (state_record) as positions and velocities by id: what field_source leaves
// on a single handle.  A record whose id is out of range is skipped.
__global__ void __launch_bounds__(WS_BLOCK) k_state_split(const uint32_t *__restrict__ all, const uint32_t *__restrict__ cnt,
                                                          uint32_t max_n, size_t stride_words, uint32_t n_global,
                                                          float *__restrict__ pos, float *__restrict__ vel)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x, r = blockIdx.y;
    if (t >= min(cnt[4 * r], max_n)) return;
    const uint32_t *rec = all + (size_t)r * stride_words + (size_t)t * 10u;
    const size_t id = rec[0];
    if (id >= n_global) return;
    const float *f = reinterpret_cast<const float *>(rec + 1);
    field_store3(pos, id, make_float4(f[0], f[1], f[2], 0.f));
    field_store3(vel, id, make_float4(f[3], f[4], f[5], 0.f));
}

void wsk_state_split(hipStream_t s, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n, size_t stride_words,
                     uint32_t n_global, float *pos, float *vel)
{
    if (!max_n) return;
    hipLaunchKernelGGL(k_state_split, dim3(cdiv(max_n, WS_BLOCK), world), dim3(WS_BLOCK), 0, s, all, cnt, max_n, stride_words,
                       n_global, pos, vel);
}

// the counter-based random numbers of the header: pure 32-bit integer arithmetic
__device__ __forceinline__ uint32_t ww_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float ww_uniform(uint32_t seed, uint32_t id, uint32_t c)
{
    const uint32_t word = ww_mix(ww_mix(seed + id * 0x9E3779B9u) + c);
    return (float)(word >> 8) * 0x1p-24f;
}
__device__ __forceinline__ float ww_clamp(float v, float lo, float hi) { return (fminf(v, hi) - fminf(v, lo)) / (hi - lo); }

// m_i by id: the stochastic rounding of the emission rate
__global__ void __launch_bounds__(WS_BLOCK) k_whitewater_count(WsWhiteEmit e, const float *__restrict__ vxyz,
                                                               const float *__restrict__ trapped, const float *__restrict__ crest,
                                                               const float *__restrict__ align, const float *__restrict__ energy,
                                                               uint32_t *__restrict__ cnt, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float vx = vxyz[3 * (size_t)i], vy = vxyz[3 * (size_t)i + 1], vz = vxyz[3 * (size_t)i + 2];
    const float sv = sqrtf(ww_dot(vx, vy, vz, vx, vy, vz));
    uint32_t m = 0;
    if (sv != 0.f) {
        const float c = align[i] >= e.align ? e.kc * ww_clamp(crest[i], e.tc0, e.tc1) : 0.f;
        const float rate = (ww_clamp(energy[i], e.te0, e.te1) * (e.kt * ww_clamp(trapped[i], e.tt0, e.tt1) + c)) * e.dt;
        const float f = floorf(rate + ww_uniform(e.seed, i, 0u));
        if (f >= (float)e.maxpp) m = e.maxpp;
        else if (f >= 1.f) m = (uint32_t)f;
    }
    cnt[i] = m;
}

// One lane per emitter: its cnt[i] spawns at off[i] .. (ids ascending, then k).  Outputs may be nullptr.
__global__ void __launch_bounds__(WS_BLOCK) k_whitewater_spawn(WsWhiteEmit e, const float *__restrict__ pxyz,
                                                               const float *__restrict__ vxyz, const uint32_t *__restrict__ cnt,
                                                               const uint32_t *__restrict__ off, float *__restrict__ out_xyz,
                                                               float *__restrict__ out_vel, float *__restrict__ out_life,
                                                               uint32_t *__restrict__ out_src, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = cnt[i];
    if (m == 0u) return;
    const float px = pxyz[3 * (size_t)i], py = pxyz[3 * (size_t)i + 1], pz = pxyz[3 * (size_t)i + 2];
    const float vx = vxyz[3 * (size_t)i], vy = vxyz[3 * (size_t)i + 1], vz = vxyz[3 * (size_t)i + 2];
    const float sv = sqrtf(ww_dot(vx, vy, vz, vx, vy, vz));
    const float hx = vx / sv, hy = vy / sv, hz = vz / sv;
    // e1 from the axis of the smallest |component| (lowest axis on a tie), e2 = vh x e1
    const float ax = fabsf(hx), ay = fabsf(hy), az = fabsf(hz);
    int q = 0;
    float least = ax;
    if (ay < least) { q = 1; least = ay; }
    if (az < least) q = 2;
    float cx, cy, cz;
    if (q == 0) { cx = 0.f; cy = -hz; cz = hy; }
    else if (q == 1) { cx = hz; cy = 0.f; cz = -hx; }
    else { cx = -hy; cy = hx; cz = 0.f; }
    const float cl = sqrtf(ww_dot(cx, cy, cz, cx, cy, cz));
    const float e1x = cx / cl, e1y = cy / cl, e1z = cz / cl;
    const float e2x = hy * e1z - hz * e1y, e2y = hz * e1x - hx * e1z, e2z = hx * e1y - hy * e1x;
    const float span = e.l1 - e.l0;
    const size_t first = off[i];
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t b = 1u + 18u * k;
        const float uh = ww_uniform(e.seed, i, b), ul = ww_uniform(e.seed, i, b + 1u);
        float da = 0.f, db = 0.f;
        for (uint32_t t = 0; t < 8u; t++) {
            const float a = 2.f * ww_uniform(e.seed, i, b + 2u + 2u * t) - 1.f;
            const float c = 2.f * ww_uniform(e.seed, i, b + 3u + 2u * t) - 1.f;
            if (a * a + c * c <= 1.f) {
                da = a;
                db = c;
                break;
            }
        }
        const float ox = e.radius * (da * e1x + db * e2x);
        const float oy = e.radius * (da * e1y + db * e2y);
        const float oz = e.radius * (da * e1z + db * e2z);
        const float along = uh * e.dt;
        const size_t at = first + k;
        if (out_xyz) field_store3(out_xyz, at, make_float4((px + ox) + along * vx, (py + oy) + along * vy, (pz + oz) + along * vz, 0.f));
        if (out_vel) field_store3(out_vel, at, make_float4(vx + ox, vy + oy, vz + oz, 0.f));
        if (out_life) out_life[at] = e.l0 + ul * span;
        if (out_src) out_src[at] = i;
    }
}

void wsk_whitewater_count(hipStream_t s, const WsWhiteEmit &e, const float *vxyz, const float *trapped, const float *crest,
                          const float *align, const float *energy, uint32_t *cnt, uint32_t n)
{
    hipLaunchKernelGGL(k_whitewater_count, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, e, vxyz, trapped, crest, align, energy,
                       cnt, n);
}

void wsk_whitewater_spawn(hipStream_t s, const WsWhiteEmit &e, const float *pxyz, const float *vxyz, const uint32_t *cnt,
                          const uint32_t *off, float *out_xyz, float *out_vel, float *out_life, uint32_t *out_src, uint32_t n)
{
    hipLaunchKernelGGL(k_whitewater_spawn, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, e, pxyz, vxyz, cnt, off, out_xyz,
                       out_vel, out_life, out_src, n);
}

// The velocity field's source with a count lane: FieldVel's terms, the same bits, and the number of accepted candidates.
// It holds a FieldVel rather than being one: it declares no chunk, so the brick kernel, whose sums have no count lane,
// does not compile over it.
struct FieldCountAcc : FieldAcc {
    uint32_t c;
};
struct FieldVelCount {
    FieldVel vel;
    __device__ __forceinline__ float4 at(uint32_t j) const { return vel.at(j); }
    template <bool IEEE, bool GRAD>
    __device__ __forceinline__ void pair(const WsDev &d, uint32_t j, float ex, float ey, float ez, float d2,
                                         FieldCountAcc &a) const
    {
        vel.pair<IEEE, GRAD>(d, j, ex, ey, ez, d2, a);
        a.c++;
    }
};

// One lane per diffuse particle; a lane reads and writes its own slots only (pts, vel, life in place).  A particle may
// lie anywhere: field_axis_cell clamps any float into the grid (k_advect).
template <bool IEEE>
__global__ void __launch_bounds__(WS_BLOCK) k_whitewater_step(WsDev d, const uint32_t *__restrict__ start, FieldVelCount src,
                                                              WsWhiteStep sp, float *pts, float *vel, float *life,
                                                              uint8_t *__restrict__ cls, uint32_t m)
{
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (t >= m) return;
    float p[3] = {pts[3 * (size_t)t], pts[3 * (size_t)t + 1], pts[3 * (size_t)t + 2]};
    float v[3] = {vel[3 * (size_t)t], vel[3 * (size_t)t + 1], vel[3 * (size_t)t + 2]};
    float l = life[t];
    const FieldCountAcc a =
        field_sweep<IEEE, true, FieldVelCount, FieldCountAcc>(d, start, src, make_float4(p[0], p[1], p[2], 0.f));
    const float4 u4 = field_velocity(a);
    const float u[3] = {u4.x, u4.y, u4.z};
    uint32_t kind;
    if (a.c < sp.spray_max) {
        kind = 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = v[k] + sp.dt * d.grav[k];
            p[k] = p[k] + sp.dt * v[k];
        }
    } else if (a.c > sp.bubble_min) {
        kind = 2u;
        const float nb = -sp.buoyancy;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = (v[k] + sp.dt * (nb * d.grav[k])) + sp.drag * (u[k] - v[k]);
            p[k] = p[k] + sp.dt * v[k];
        }
    } else {
        kind = 1u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = u[k];
            p[k] = p[k] + sp.dt * u[k];
        }
        l = l - sp.dt;
    }
    const float nd = -1.f * d.damping;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (p[k] < d.ext_min[k]) { v[k] *= nd; p[k] = d.ext_min[k]; } else if (p[k] > d.ext_max[k]) { v[k] *= nd; p[k] = d.ext_max[k]; }
    }
    if (l <= 0.f) kind = 3u;
    field_store3(pts, t, make_float4(p[0], p[1], p[2], 0.f));
    field_store3(vel, t, make_float4(v[0], v[1], v[2], 0.f));
    life[t] = l;
    cls[t] = (uint8_t)kind;
}

void wsk_whitewater_step(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                         const WsWhiteStep &sp, float *pts, float *vel, float *life, uint8_t *cls, uint32_t m)
{
    const FieldVelCount src = {{spos, svel}};
    ws_dispatch([&](auto I) {
        hipLaunchKernelGGL(k_whitewater_step<I()>, dim3(cdiv(m, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, src, sp, pts, vel,
                           life, cls, m);
    }, ieee);
}

// ---------------------------------------------------------------------------------
// buoyancy and drag on host-owned bodies (ws_body_forces; never inside ws_step)
//
// include/wsfluid.h pins every rounding of a sample's terms and the ORDER of a body's sums: a fixed binary tree over the
// body's samples in the order given, padded with +0 to a power of two above their number.  No float atomics anywhere: the
// tree is walked level by level, level L pairing slot i with slot i ^ (1 << L) of the body-relative sample index.
//
// k_body_forces, one workgroup per chunk = WS_BLOCK consecutive body-relative samples of ONE body (the host's chunk table
// says which): a lane sweeps the velocity field at its sample (field_sweep, the points sampler's own definition), forms the
// sample's F, T, vol and wet in registers, stores the per-sample outputs, then the workgroup sums the seven floats and the
// count over levels 0 .. 7 of the tree -- 0 .. 5 across the lanes of a wave, 6 and 7 across the four waves through LDS.
// A lane without a sample holds +0.  The chunk's partial is the tree's node at level 8.
// k_body_finish, one wave per body: the same tree continued over the body's chunk partials, 64 at a time across the lanes
// (6 more levels per block), the blocks' nodes merged like the carries of a binary counter (a stack of one node per level,
// in LDS, each lane owning one of the eight values), and what is left on the stack folded from the lowest level up into a
// carry that starts at +0 -- the padding: at least one +0 always enters, and further +0 change no bit.
// ---------------------------------------------------------------------------------
// levels 0 .. 5: every lane ends with the sum of its wave in tree order (a + b and b + a are the same bits)
__device__ __forceinline__ float body_wave_tree(float v)
{
#pragma unroll
    for (int sh = 1; sh <= 32; sh <<= 1) v = v + __shfl_xor(v, sh, 64);
    return v;
}
__device__ __forceinline__ uint32_t body_wave_count(uint32_t v)
{
#pragma unroll
    for (int sh = 1; sh <= 32; sh <<= 1) v += (uint32_t)__shfl_xor((int)v, sh, 64);
    return v;
}
// one node from two: values 0 .. 6 are floats, value 7 is the wet count (its bits travel in a float)
__device__ __forceinline__ float body_node(float lo, float hi, bool count)
{
    return count ? __uint_as_float(__float_as_uint(lo) + __float_as_uint(hi)) : lo + hi;
}

#define WS_BODY_LEVELS 16  // stack levels of the finishing tree: a call's 2^28 samples are at most 2^14 blocks of 64 chunks

template <bool IEEE>
__global__ void __launch_bounds__(WS_BLOCK) k_body_forces(WsDev d, const uint32_t *__restrict__ start, FieldVel src, WsBodyParams bp,
                                                          const uint4 *__restrict__ chunks, const float *__restrict__ xyz,
                                                          const float *__restrict__ wvel, const float *__restrict__ vol,
                                                          const float *__restrict__ centre, float *__restrict__ part,
                                                          float *__restrict__ sforce, float *__restrict__ sfrac)
{
    __shared__ float s_part[WS_BLOCK / 64][8];
    const uint4 ch = chunks[blockIdx.x];  // {body, first sample, samples, 0}
    const uint32_t lane = threadIdx.x;
    float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // F, T, vol
    uint32_t wet = 0u;
    if (lane < ch.z) {
        const size_t t = (size_t)ch.y + lane;
        const float p[3] = {xyz[3 * t], xyz[3 * t + 1], xyz[3 * t + 2]};
        const FieldAcc a = field_sweep<IEEE, true>(d, start, src, make_float4(p[0], p[1], p[2], 0.f));
        float f = 0.f;
        if (a.rho > 0.f) {
            const float4 u4 = field_velocity(a);
            const float u[3] = {u4.x, u4.y, u4.z};
            f = fminf(a.rho / bp.rho0, 1.0f);
            const float sv = vol[t] * f;
            const float lift = bp.fluid_density * sv, kd = bp.drag * sv;
            float r[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                v[k] = kd * (u[k] - wvel[3 * t + k]) - lift * d.grav[k];
                r[k] = p[k] - centre[3 * (size_t)ch.x + k];
            }
            v[3] = r[1] * v[2] - r[2] * v[1];
            v[4] = r[2] * v[0] - r[0] * v[2];
            v[5] = r[0] * v[1] - r[1] * v[0];
            v[6] = sv;
            wet = 1u;
        }
        if (sforce) field_store3(sforce, t, make_float4(v[0], v[1], v[2], 0.f));
        if (sfrac) sfrac[t] = f;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) v[k] = body_wave_tree(v[k]);
    wet = body_wave_count(wet);
    if ((lane & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 7; k++) s_part[lane >> 6][k] = v[k];
        s_part[lane >> 6][7] = __uint_as_float(wet);
    }
    __syncthreads();
    if (lane < 8u) {  // levels 6 and 7: waves 0 + 1 and 2 + 3, then the two
        const bool count = lane == 7u;
        const float lo = body_node(s_part[0][lane], s_part[1][lane], count), hi = body_node(s_part[2][lane], s_part[3][lane], count);
        part[8 * (size_t)blockIdx.x + lane] = body_node(lo, hi, count);
    }
}

__global__ void __launch_bounds__(WS_BLOCK) k_body_finish(const uint32_t *__restrict__ cstart, const float *__restrict__ part,
                                                          uint32_t nb, float *__restrict__ force, float *__restrict__ torque,
                                                          float *__restrict__ volume, uint32_t *__restrict__ wet)
{
    __shared__ float s_stack[WS_BLOCK / 64][WS_BODY_LEVELS][8];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * (WS_BLOCK / 64) + wave;
    if (b >= nb) return;  // (wave-uniform; the kernel has no barrier)
    const uint32_t c0 = cstart[b], nc = cstart[b + 1] - c0;  // the body's chunks (none: an empty body)
    const uint32_t nblk = (nc + 63u) >> 6;
    const bool count = lane == 7u;
    for (uint32_t blk = 0; blk < nblk; blk++) {
        const uint32_t i = blk * 64u + lane;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;  // an absent chunk: +0, count 0
        if (i < nc) {
            const float4 *q = reinterpret_cast<const float4 *>(part + 8 * ((size_t)c0 + i));
            a = q[0];
            c = q[1];
        }
        const float v0 = body_wave_tree(a.x), v1 = body_wave_tree(a.y), v2 = body_wave_tree(a.z), v3 = body_wave_tree(a.w);
        const float v4 = body_wave_tree(c.x), v5 = body_wave_tree(c.y), v6 = body_wave_tree(c.z);
        const float v7 = __uint_as_float(body_wave_count(__float_as_uint(c.w)));
        if (lane < 8u) {  // lane k keeps value k; it alone reads and writes column k of the stack
            float node = lane == 0u ? v0 : lane == 1u ? v1 : lane == 2u ? v2 : lane == 3u ? v3 : lane == 4u ? v4 : lane == 5u ? v5
                         : lane == 6u ? v6 : v7;
            uint32_t l = 0;
            for (; (blk >> l) & 1u; l++) node = body_node(s_stack[wave][l][lane], node, count);
            s_stack[wave][l][lane] = node;
        }
    }
    if (lane >= 8u) return;
    float carry = 0.f;
    for (uint32_t l = 0; (nblk >> l) != 0u; l++)
        if ((nblk >> l) & 1u) carry = body_node(s_stack[wave][l][lane], carry, count);
    if (lane < 3u) {
        if (force) force[3 * (size_t)b + lane] = carry;
    } else if (lane < 6u) {
        if (torque) torque[3 * (size_t)b + (lane - 3u)] = carry;
    } else if (lane == 6u) {
        if (volume) volume[b] = carry;
    } else if (wet) {
        wet[b] = __float_as_uint(carry);
    }
}

uint32_t wsk_body_chunk(void) { return WS_BLOCK; }

void wsk_body_forces(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                     const WsBodyParams &bp, const uint32_t *chunks, uint32_t nchunks, const uint32_t *cstart, uint32_t nb,
                     const float *xyz, const float *vel, const float *vol, const float *centre, float *part, float *sforce,
                     float *sfrac, float *force, float *torque, float *volume, uint32_t *wet)
{
    const FieldVel src = {spos, svel};
    if (nchunks != 0u)
        ws_dispatch([&](auto I) {
            hipLaunchKernelGGL(k_body_forces<I()>, dim3(nchunks), dim3(WS_BLOCK), 0, s, d, start, src, bp,
                               reinterpret_cast<const uint4 *>(chunks), xyz, vel, vol, centre, part, sforce, sfrac);
        }, ieee);
    if (force || torque || volume || wet)
        hipLaunchKernelGGL(k_body_finish, dim3(cdiv(nb, WS_BLOCK / 64)), dim3(WS_BLOCK), 0, s, cstart, part, nb, force, torque,
                           volume, wet);
}

// ---------------------------------------------------------------------------------
// rays at the fluid surface (ws_cast_rays / ws_cast_camera; never inside ws_step)
//
// include/wsfluid.h pins the march bit for bit: samples t_k = t_start + k * dt at p = o + t * v, the first k with
// field >= iso, `refine` bisections of [t_{k-1}, t_k], the gradient at the hit.  The field at a sample is field_sweep,
// the points sampler's own definition, so a host that marches with ws_sample_density_points gets the same bits.
//
// k_ray_cast, one lane per ray: a plain loop that calls field_sweep at every march and bisection sample, then once more
// at the hit for the gradient.  A lane's state is its own: no result depends on what the other lanes of the wave do.
// (An occupancy bit per cell that skips air samples exactly, with a wave vote so that lanes sweep together, is
// tools/ab/patches/rays_occupancy_vote.patch: not measured against this loop, so not adopted.)
// ---------------------------------------------------------------------------------
// The ray of a lane: its origin, direction and output slot; false = the lane has no ray.
// RayList: the m rays of a ws_cast_rays call, ray t on lane t.
struct RayList {
    const float *__restrict__ o;
    const float *__restrict__ v;
    uint32_t m;
    __device__ __forceinline__ bool ray(uint32_t t, size_t &at, float4 &org, float4 &dir) const
    {
        if (t >= m) return false;
        at = t;
        org = make_float4(o[3 * at], o[3 * at + 1], o[3 * at + 2], 0.f);
        dir = make_float4(v[3 * at], v[3 * at + 1], v[3 * at + 2], 0.f);
        return true;
    }
};

// RayCamera: pixel (i, j) of a W x H image (include/wsfluid.h has the formula; su = 2 / W and sv = 2 / H are rounded on
// the host).  A wave is a tile of 8 x 8 pixels, lane l = pixel (l & 7, l >> 3) of it: neighbouring rays walk
// neighbouring cells, so their candidate runs overlap in L1.
struct RayCamera {
    ws_camera cam;
    uint32_t w, h, tiles_x;
    float su, sv;
    __device__ __forceinline__ bool ray(uint32_t t, size_t &at, float4 &org, float4 &dir) const
    {
        const uint32_t tile = t >> 6, lane = t & 63u;
        const uint32_t i = (tile % tiles_x) * 8u + (lane & 7u), j = (tile / tiles_x) * 8u + (lane >> 3);
        if (i >= w || j >= h) return false;
        at = (size_t)j * w + i;
        const float u = ((float)i + 0.5f) * su - 1.0f;
        const float q = 1.0f - ((float)j + 0.5f) * sv;
        org = make_float4(cam.eye[0], cam.eye[1], cam.eye[2], 0.f);
        dir = make_float4((cam.forward[0] + u * cam.right[0]) + q * cam.up[0], (cam.forward[1] + u * cam.right[1]) + q * cam.up[1],
                          (cam.forward[2] + u * cam.right[2]) + q * cam.up[2], 0.f);
        return true;
    }
};

// Where a ray stands: marching at sample k (left == 0) or `left` bisections from the end, between lo and hi.
struct RayState {
    uint32_t k, left;
    float lo, hi, t;  // t: the result (+INFINITY until a hit is final)
    bool done;
    // parameter of the next sample
    __device__ __forceinline__ float next(const ws_ray_params &r) const
    {
        return left ? (lo + hi) * 0.5f : r.t_start + (float)k * r.dt;
    }
    // the field at that sample is rho
    __device__ __forceinline__ void take(const ws_ray_params &r, float ts, float rho)
    {
        const bool inside = rho >= r.iso;
        if (left) {
            if (inside) hi = ts;
            else lo = ts;
            if (--left == 0u) {
                t = hi;
                done = true;
            }
        } else if (inside) {
            if (k == 0u || r.refine == 0u) {
                t = ts;
                done = true;
            } else {
                lo = r.t_start + (float)(k - 1u) * r.dt;
                hi = ts;
                left = r.refine;
            }
        } else if (++k > r.steps) {
            done = true;  // a miss
        }
    }
};

__device__ __forceinline__ float4 ray_point(const float4 &o, const float4 &v, float t)
{
    return make_float4(o.x + t * v.x, o.y + t * v.y, o.z + t * v.z, 0.f);
}

template <bool IEEE, bool NORMALS, class Src, class Rays>
__global__ void __launch_bounds__(WS_BLOCK) k_ray_cast(WsDev d, const uint32_t *__restrict__ start, Src src,
                                                       Rays rays, ws_ray_params r,
                                                       float *__restrict__ out_t, float *__restrict__ out_n)
{
    size_t at = 0;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f), v = o;
    const bool valid = rays.ray(blockIdx.x * WS_BLOCK + threadIdx.x, at, o, v);
    RayState st = {0u, 0u, 0.f, 0.f, INFINITY, !valid};
    while (!st.done) {
        const float ts = st.next(r);
        st.take(r, ts, field_sweep<IEEE, false>(d, start, src, ray_point(o, v, ts)).rho);
    }
    const bool hit = valid && st.t != INFINITY;
    if constexpr (NORMALS) {
        float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hit) {
            const FieldAcc g = field_sweep<IEEE, true>(d, start, src, ray_point(o, v, st.t));
            n = field_unit_normal(g.gx, g.gy, g.gz);
        }
        if (valid) field_store3(out_n, at, n);
    }
    if (valid && out_t) out_t[at] = st.t;
}

template <class Src, class Rays>
void ray_cast_launch(hipStream_t s, const WsDev &d, const uint32_t *start, Src src, Rays rays,
                     uint32_t lanes, const ws_ray_params &r, bool ieee, float *out_t, float *out_n)
{
    ws_dispatch([&](auto I, auto N) {
        hipLaunchKernelGGL((k_ray_cast<I(), N(), Src, Rays>), dim3(cdiv(lanes, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, src,
                           rays, r, out_t, out_n);
    }, ieee, out_n != nullptr);
}

void wsk_ray_cast(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *smf,
                  bool ieee, const ws_ray_params &r, const float *origin, const float *dir, uint32_t m,
                  const ws_camera *cam, const uint32_t *size, float *out_t, float *out_n)
{
    if (cam) {
        const uint32_t tx = cdiv(size[0], 8u), ty = cdiv(size[1], 8u);
        const RayCamera rays = {*cam, size[0], size[1], tx, 2.0f / (float)size[0], 2.0f / (float)size[1]};
        if (smf) ray_cast_launch(s, d, start, FieldAniso{spos, smf}, rays, tx * ty * 64u, r, ieee, out_t, out_n);
        else ray_cast_launch(s, d, start, FieldIso{spos}, rays, tx * ty * 64u, r, ieee, out_t, out_n);
    } else {
        const RayList rays = {origin, dir, m};
        if (smf) ray_cast_launch(s, d, start, FieldAniso{spos, smf}, rays, m, r, ieee, out_t, out_n);
        else ray_cast_launch(s, d, start, FieldIso{spos}, rays, m, r, ieee, out_t, out_n);
    }
}

// ---------------------------------------------------------------------------------
// anisotropic kernels (ws_read_anisotropy / ws_sample_aniso_* / ws_extract_aniso_surface; never inside ws_step)
//
// k_aniso, the per-particle stage (include/wsfluid.h pins it bit for bit): one lane per particle in the sampler's cell
// order of the current positions, so the lanes of a wave sweep neighbouring cells.  One sweep of the 27 cells around
// x_i (the density sampler's canonical order and accept test) gives the weighted moments about x_i; the mean, the
// covariance, a fixed 5-sweep cyclic Jacobi and the ellipsoid are then formed in registers.  IEEE arithmetic whatever
// the handle's flags (correctly rounded sqrt and division, no contraction).  Writes, by id: the centre, M and f
// (mf[2 id], mf[2 id + 1] as FieldAniso reads them) and the neighbour count.
// ---------------------------------------------------------------------------------

// One classic Jacobi rotation zeroing a_pq of the symmetric 3x3 A (r = the third index), R = R J (rp, rq: columns p, q).
__device__ __forceinline__ void aniso_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float *rp, float *rq)
{
    if (apq == 0.f) return;
    const float theta = (aqq - app) / (2.f * apq);
    float t;
    if (fabsf(theta) > 0x1p32f) t = 1.f / (2.f * theta);
    else t = (theta >= 0.f ? 1.f : -1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.f;
    const float xp = arp, xq = arq;
    arp = c * xp - s * xq;
    arq = s * xp + c * xq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float vp = rp[k], vq = rq[k];
        rp[k] = c * vp - s * vq;
        rq[k] = s * vp + c * vq;
    }
}

__global__ void __launch_bounds__(WS_BLOCK) k_aniso(WsDev d, const uint32_t *__restrict__ start, const float4 *__restrict__ spos,
                                                    WsAnisoParams ap, float *__restrict__ cxyz, float4 *__restrict__ mf,
                                                    uint32_t *__restrict__ nb, uint32_t n)
{
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 o = spos[i];
    const uint32_t id = __float_as_uint(o.w);
    float W = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, qxx = 0.f, qyy = 0.f, qzz = 0.f, qxy = 0.f, qxz = 0.f, qyz = 0.f;
    uint32_t cnt = 0;
    const int cx = field_axis_cell(d, 0, o.x), cy = field_axis_cell(d, 1, o.y), cz = field_axis_cell(d, 2, o.z);
    const int z0 = max(cz - 1, 0), z1 = min(cz + 1, d.dim[2] - 1);
    for (int x = max(cx - 1, 0); x <= min(cx + 1, d.dim[0] - 1); x++) {
        for (int y = max(cy - 1, 0); y <= min(cy + 1, d.dim[1] - 1); y++) {
            const uint32_t col = (uint32_t)(x * d.dim[1] + y) * (uint32_t)d.dim[2];
            const uint32_t b = start[col + z0], e = start[col + z1 + 1];
            for (uint32_t j = b; j < e; j++) {
                const float4 q = spos[j];
                const float ex = q.x - o.x, ey = q.y - o.y, ez = q.z - o.z;
                const float d2 = ex * ex + ey * ey + ez * ez;
                if (d2 > d.d2_accept) continue;
                const float r = sqrtf(d2) / d.h;
                const float w = 1.f - (r * r) * r;
                const float wx = w * ex, wy = w * ey, wz = w * ez;
                cnt++;
                W += w;
                sx += wx;
                sy += wy;
                sz += wz;
                qxx += wx * ex;
                qyy += wy * ey;
                qzz += wz * ez;
                qxy += wx * ey;
                qxz += wx * ez;
                qyz += wy * ez;
            }
        }
    }
    const float mx = sx / W, my = sy / W, mz = sz / W;
    cxyz[3 * (size_t)id] = o.x + ap.lambda * mx;
    cxyz[3 * (size_t)id + 1] = o.y + ap.lambda * my;
    cxyz[3 * (size_t)id + 2] = o.z + ap.lambda * mz;
    nb[id] = cnt;
    // covariance: a00 a11 a22 a01 a02 a12
    float a00 = qxx / W - mx * mx, a11 = qyy / W - my * my, a22 = qzz / W - mz * mz;
    float a01 = qxy / W - mx * my, a02 = qxz / W - mx * mz, a12 = qyz / W - my * mz;
    float Mxx, Myy, Mzz, Mxy = 0.f, Mxz = 0.f, Myz = 0.f, f;
    bool lone = cnt < ap.neps;
    if (!lone) {
        float r0[3] = {1.f, 0.f, 0.f}, r1[3] = {0.f, 1.f, 0.f}, r2[3] = {0.f, 0.f, 1.f};  // columns of R
#pragma unroll
        for (int sweep = 0; sweep < 5; sweep++) {
            aniso_rotate(a00, a11, a01, a02, a12, r0, r1);  // (0, 1), r = 2
            aniso_rotate(a00, a22, a02, a01, a12, r0, r2);  // (0, 2), r = 1
            aniso_rotate(a11, a22, a12, a01, a02, r1, r2);  // (1, 2), r = 0
        }
        const float smax = fmaxf(fmaxf(a00, a11), a22);
        if (smax > 0.f) {
            const float fl = smax / ap.kr;
            const float s0 = fmaxf(a00, fl) / smax, s1 = fmaxf(a11, fl) / smax, s2 = fmaxf(a22, fl) / smax;
            const float i0 = 1.f / s0, i1 = 1.f / s1, i2 = 1.f / s2;
            Mxx = 0.f; Myy = 0.f; Mzz = 0.f;
            Mxx = Mxx + (i0 * r0[0]) * r0[0]; Mxx = Mxx + (i1 * r1[0]) * r1[0]; Mxx = Mxx + (i2 * r2[0]) * r2[0];
            Myy = Myy + (i0 * r0[1]) * r0[1]; Myy = Myy + (i1 * r1[1]) * r1[1]; Myy = Myy + (i2 * r2[1]) * r2[1];
            Mzz = Mzz + (i0 * r0[2]) * r0[2]; Mzz = Mzz + (i1 * r1[2]) * r1[2]; Mzz = Mzz + (i2 * r2[2]) * r2[2];
            Mxy = Mxy + (i0 * r0[0]) * r0[1]; Mxy = Mxy + (i1 * r1[0]) * r1[1]; Mxy = Mxy + (i2 * r2[0]) * r2[1];
            Mxz = Mxz + (i0 * r0[0]) * r0[2]; Mxz = Mxz + (i1 * r1[0]) * r1[2]; Mxz = Mxz + (i2 * r2[0]) * r2[2];
            Myz = Myz + (i0 * r0[1]) * r0[2]; Myz = Myz + (i1 * r1[1]) * r1[2]; Myz = Myz + (i2 * r2[1]) * r2[2];
            f = 1.f / ((s0 * s1) * s2);
        } else {
            lone = true;
        }
    }
    if (lone) {
        const float inv = 1.f / ap.kn;
        Mxx = Myy = Mzz = inv;
        Mxy = Mxz = Myz = 0.f;
        f = (inv * inv) * inv;
    }
    mf[2 * (size_t)id] = make_float4(Mxx, Myy, Mzz, Mxy);
    mf[2 * (size_t)id + 1] = make_float4(Mxz, Myz, f, 0.f);
}

void wsk_aniso(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, WsAnisoParams ap, float *cxyz,
               float4 *mf, uint32_t *nb, uint32_t n)
{
    hipLaunchKernelGGL(k_aniso, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, start, spos, ap, cxyz, mf, nb, n);
}

// the centres' records in their cell order: srec[j] = {c, id bits}, smf[2j], smf[2j + 1] = the ellipsoid of id perm[j]
__global__ void __launch_bounds__(WS_BLOCK) k_aniso_gather(const uint32_t *__restrict__ perm, const float *__restrict__ cxyz,
                                                           const float4 *__restrict__ mf, float4 *__restrict__ srec,
                                                           float4 *__restrict__ smf, uint32_t n)
{
    const uint32_t j = blockIdx.x * WS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t id = perm[j];
    srec[j] = make_float4(cxyz[3 * id], cxyz[3 * id + 1], cxyz[3 * id + 2], __uint_as_float((uint32_t)id));
    smf[2 * (size_t)j] = mf[2 * id];
    smf[2 * (size_t)j + 1] = mf[2 * id + 1];
}

void wsk_aniso_gather(hipStream_t s, const uint32_t *perm, const float *cxyz, const float4 *mf, float4 *srec, float4 *smf,
                      uint32_t n)
{
    hipLaunchKernelGGL(k_aniso_gather, dim3(cdiv(n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, perm, cxyz, mf, srec, smf, n);
}

// ---------------------------------------------------------------------------------
// surface extraction (ws_extract_surface; never inside ws_step)
//
// The iso-surface rho = iso of a sampled grid (rho / grad: what k_field_bricks / k_field_points wrote for that grid),
// by marching tetrahedra, exactly as include/wsfluid.h defines it.  Three streaming passes over the nodes, each one
// lane per node in workgroups of WS_BLOCK consecutive linear nodes (workgroup b = nodes [b * WS_BLOCK, + WS_BLOCK),
// dealt to the XCDs with xcd_tile so that each XCD's L2 walks one contiguous range, whose +y / +z neighbours are one
// row and one plane ahead):
//   k_iso_count      node code (bits 0-6: forward edge of type d = bit + 1 crossed; bit 7: inside) and the
//                    workgroup's vertex and triangle totals;
//   (two wsk_scan launches over the totals: every workgroup's first vertex and first triangle; k_iso_totals puts the
//   two grand totals side by side for the host)
//   k_iso_vertices   vertex base of every node with a crossed edge, its vertices' positions and normals;
//   k_iso_triangles  the triangles of the node's cube, as vertex ids.
// Both later passes recompute their lane's count from its code byte and scan it in the workgroup, so the ids are the
// definition's order: nodes by linear index then edges by type; cubes by linear index, then tets, then the case table.
// ---------------------------------------------------------------------------------
#define ISO_INSIDE 0x80u

// The six tets of a cube, corners as bit offsets (x = 1, y = 2, z = 4), all on the 0-7 diagonal: {0, m1, m2, 7}.
// Tets 1, 2 and 5 are negatively oriented (det(c1 - c0, c2 - c0, c3 - c0) < 0): their triangles are reversed.
#define ISO_TET_M1 0x442211u   // nibble t: m1 of tet t = 1 1 2 2 4 4
#define ISO_TET_M2 0x656353u   // nibble t: m2 of tet t = 3 5 3 6 5 6
#define ISO_TET_FLIP 0x26u     // bit t: tet t is negatively oriented

// Case table of a positively oriented tet (local corners q0..q3, case bit k = q_k inside).  Local edges 0..5 =
// (q0 q1) (q0 q2) (q0 q3) (q1 q2) (q1 q3) (q2 q3).  Entry: bits 0-11 the first triangle's three edges (4 bits each,
// v0 lowest), bits 12-23 the second's, bits 24-25 the triangle count.  Every triangle's (v1 - v0) x (v2 - v0) points
// from the inside corners to the outside ones (include/wsfluid.h lists the same table).
#define ISO_T1(a, b, c) (1u << 24 | (a) | (b) << 4 | (c) << 8)
#define ISO_T2(a, b, c, d, e, f) (2u << 24 | (a) | (b) << 4 | (c) << 8 | (d) << 12 | (e) << 16 | (f) << 20)
__constant__ uint32_t c_iso_case[16] = {
    0u,                        // 0: none inside
    ISO_T1(0, 1, 2),           // 1: q0
    ISO_T1(0, 4, 3),           // 2: q1
    ISO_T2(1, 2, 4, 1, 4, 3),  // 3: q0 q1
    ISO_T1(1, 3, 5),           // 4: q2
    ISO_T2(2, 0, 3, 2, 3, 5),  // 5: q0 q2
    ISO_T2(0, 4, 5, 0, 5, 1),  // 6: q1 q2
    ISO_T1(2, 4, 5),           // 7: all but q3
    ISO_T1(2, 5, 4),           // 8: q3
    ISO_T2(0, 1, 5, 0, 5, 4),  // 9: q0 q3
    ISO_T2(3, 0, 2, 3, 2, 5),  // 10: q1 q3
    ISO_T1(1, 5, 3),           // 11: all but q2
    ISO_T2(1, 3, 4, 1, 4, 2),  // 12: q2 q3
    ISO_T1(0, 3, 4),           // 13: all but q1
    ISO_T1(0, 2, 1),           // 14: all but q0
    0u,                        // 15: all inside
};
#undef ISO_T1
#undef ISO_T2
#define ISO_CASE_TRIS 0x16696994u  // 2 bits per case: the table's triangle counts

// corner c of the cube inside (bit c), from the code byte of its corner 0
__device__ __forceinline__ uint32_t iso_corners(uint32_t code)
{
    const uint32_t x = (code & 0x7Fu) << 1;
    return (code & ISO_INSIDE) ? (~x & 0xFFu) : x;
}

__device__ __forceinline__ uint32_t iso_tet_case(uint32_t cm, int t)
{
    const uint32_t m1 = (ISO_TET_M1 >> (4 * t)) & 15u, m2 = (ISO_TET_M2 >> (4 * t)) & 15u;
    return (cm & 1u) | ((cm >> m1) & 1u) << 1 | ((cm >> m2) & 1u) << 2 | ((cm >> 7) & 1u) << 3;
}

__device__ __forceinline__ uint32_t iso_cube_triangles(uint32_t code)
{
    const uint32_t cm = iso_corners(code);
    uint32_t tri = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) tri += (ISO_CASE_TRIS >> (2 * iso_tet_case(cm, t))) & 3u;
    return tri;
}

// Exclusive scan of v over the workgroup (WS_BLOCK lanes); *total = the workgroup's sum.
__device__ __forceinline__ uint32_t iso_block_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t s_wave[WS_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < WS_BLOCK / 64; w++) {
        const uint32_t x = s_wave[w];
        base += w < wave ? x : 0u;
        sum += x;
    }
    *total = sum;
    return base + incl - v;
}

__global__ void __launch_bounds__(WS_BLOCK) k_iso_count(const float *__restrict__ rho, WsFieldGrid g, float iso,
                                                        uint8_t *__restrict__ code, uint32_t *__restrict__ vcnt,
                                                        uint32_t *__restrict__ tcnt, uint32_t nodes)
{
    const uint32_t b = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t n = b * WS_BLOCK + threadIdx.x;
    uint32_t c = 0, tri = 0;
    if (n < nodes) {
        const uint32_t i = n % g.nx, r = n / g.nx, j = r % g.ny, k = r / g.ny;
        const uint32_t row = g.nx, plane = g.nx * g.ny;
        const bool in0 = rho[n] >= iso;
#pragma unroll
        for (uint32_t d = 1; d < 8; d++) {
            const uint32_t dx = d & 1u, dy = (d >> 1) & 1u, dz = d >> 2;
            if (i + dx < g.nx && j + dy < g.ny && k + dz < g.nz) {
                const bool in = rho[n + dx + dy * row + dz * plane] >= iso;
                c |= (in != in0 ? 1u : 0u) << (d - 1u);
            }
        }
        c |= in0 ? ISO_INSIDE : 0u;
        code[n] = (uint8_t)c;
        if (i + 1u < g.nx && j + 1u < g.ny && k + 1u < g.nz) tri = iso_cube_triangles(c);
    }
    uint32_t vtot, ttot;
    iso_block_scan(__builtin_popcount(c & 0x7Fu), &vtot);
    __syncthreads();  // (the scan's LDS is reused)
    iso_block_scan(tri, &ttot);
    if (threadIdx.x == 0) {
        vcnt[b] = vtot;
        tcnt[b] = ttot;
        if (b == 0) {  // the scans run over gridDim.x + 1 totals: the last one, 0, becomes the grand total
            vcnt[gridDim.x] = 0u;
            tcnt[gridDim.x] = 0u;
        }
    }
}

// The vertex on the forward edge of type d at node (i, j, k): t = (iso - ra) / (rb - ra) (correctly rounded),
// p = pa + t * (pb - pa) per axis; the normal -g / sqrtf(g . g) of g = ga + t * (gb - ga), (0, 0, 0) where g . g == 0.
template <bool NORMALS>
__global__ void __launch_bounds__(WS_BLOCK) k_iso_vertices(const float *__restrict__ rho, const float *__restrict__ grad,
                                                           WsFieldGrid g, float iso, const uint8_t *__restrict__ code,
                                                           const uint32_t *__restrict__ vstart, uint32_t *__restrict__ vbase,
                                                           float *__restrict__ xyz, float *__restrict__ nrm, uint32_t nodes)
{
    const uint32_t b = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t n = b * WS_BLOCK + threadIdx.x;
    const uint32_t c = n < nodes ? (uint32_t)code[n] & 0x7Fu : 0u;
    uint32_t total;
    const uint32_t v0 = vstart[b] + iso_block_scan(__builtin_popcount(c), &total);
    if (c == 0u) return;
    vbase[n] = v0;
    const uint32_t i = n % g.nx, r = n / g.nx, j = r % g.ny, k = r / g.ny;
    const float4 pa = field_node(g, i, j, k);
    const float ra = rho[n];
    uint32_t v = v0;
    for (uint32_t d = 1; d < 8; d++) {
        if (!((c >> (d - 1u)) & 1u)) continue;
        const uint32_t dx = d & 1u, dy = (d >> 1) & 1u, dz = d >> 2;
        const uint32_t m = n + dx + dy * g.nx + dz * g.nx * g.ny;
        const float4 pb = field_node(g, i + dx, j + dy, k + dz);
        const float rb = rho[m];
        const float t = (iso - ra) / (rb - ra);
        const size_t at = 3 * (size_t)v;
        xyz[at] = pa.x + t * (pb.x - pa.x);
        xyz[at + 1] = pa.y + t * (pb.y - pa.y);
        xyz[at + 2] = pa.z + t * (pb.z - pa.z);
        if constexpr (NORMALS) {
            const float gx = grad[3 * (size_t)n] + t * (grad[3 * (size_t)m] - grad[3 * (size_t)n]);
            const float gy = grad[3 * (size_t)n + 1] + t * (grad[3 * (size_t)m + 1] - grad[3 * (size_t)n + 1]);
            const float gz = grad[3 * (size_t)n + 2] + t * (grad[3 * (size_t)m + 2] - grad[3 * (size_t)n + 2]);
            const float4 nh = field_unit_normal(gx, gy, gz);
            nrm[at] = nh.x;
            nrm[at + 1] = nh.y;
            nrm[at + 2] = nh.z;
        }
        v++;
    }
}

// vertex id of the forward edge of type d at the node whose code and vertex base are given
__device__ __forceinline__ uint32_t iso_vertex_id(uint32_t code, uint32_t base, uint32_t d)
{
    return base + __builtin_popcount(code & ((1u << (d - 1u)) - 1u));
}

__global__ void __launch_bounds__(WS_BLOCK) k_iso_triangles(WsFieldGrid g, const uint8_t *__restrict__ code,
                                                            const uint32_t *__restrict__ tstart,
                                                            const uint32_t *__restrict__ vbase, uint32_t *__restrict__ tri,
                                                            uint32_t nodes)
{
    const uint32_t b = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t n = b * WS_BLOCK + threadIdx.x;
    uint32_t c = 0, ntri = 0, i = 0, j = 0, k = 0;
    if (n < nodes) {
        const uint32_t r = n / g.nx;
        i = n % g.nx;
        j = r % g.ny;
        k = r / g.ny;
        if (i + 1u < g.nx && j + 1u < g.ny && k + 1u < g.nz) {
            c = code[n];
            ntri = iso_cube_triangles(c);
        }
    }
    uint32_t total;
    uint32_t out = tstart[b] + iso_block_scan(ntri, &total);
    if (ntri == 0u) return;
    // corners 0..6 (n + u): their codes and vertex bases (a corner whose code has no crossed edge carries no vertex)
    const uint32_t row = g.nx, plane = g.nx * g.ny;
    uint32_t cc[7], vb[7];
#pragma unroll
    for (uint32_t u = 0; u < 7; u++) {
        const uint32_t m = n + (u & 1u) + ((u >> 1) & 1u) * row + (u >> 2) * plane;
        cc[u] = u == 0 ? c : (uint32_t)code[m];
        vb[u] = (cc[u] & 0x7Fu) ? vbase[m] : 0u;
    }
    const uint32_t cm = iso_corners(c);
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint32_t e = c_iso_case[iso_tet_case(cm, t)];
        const uint32_t cnt = e >> 24;
        if (cnt == 0u) continue;
        const uint32_t m1 = (ISO_TET_M1 >> (4 * t)) & 15u, m2 = (ISO_TET_M2 >> (4 * t)) & 15u;
        // the tet's six edges (q0 q1) (q0 q2) (q0 q3) (q1 q2) (q1 q3) (q2 q3) as vertex ids: edge (a, b), a a subset of
        // b, is the forward edge of type a ^ b at corner a
        uint32_t vid[6];
        vid[0] = iso_vertex_id(cc[0], vb[0], m1);
        vid[1] = iso_vertex_id(cc[0], vb[0], m2);
        vid[2] = iso_vertex_id(cc[0], vb[0], 7u);
        vid[3] = iso_vertex_id(cc[m1], vb[m1], m1 ^ m2);
        vid[4] = iso_vertex_id(cc[m1], vb[m1], 7u ^ m1);
        vid[5] = iso_vertex_id(cc[m2], vb[m2], 7u ^ m2);
        const bool flip = (ISO_TET_FLIP >> t) & 1u;
        for (uint32_t q = 0; q < cnt; q++) {
            const uint32_t f = e >> (12 * q);
            const uint32_t a = vid[f & 15u], b1 = vid[(f >> 4) & 15u], b2 = vid[(f >> 8) & 15u];
            const size_t at = 3 * (size_t)out++;
            tri[at] = a;
            tri[at + 1] = flip ? b2 : b1;
            tri[at + 2] = flip ? b1 : b2;
        }
    }
}

void wsk_iso_count(hipStream_t s, const float *rho, const float *grid6, const uint32_t *dims, float iso, uint8_t *code,
                   uint32_t *vcnt, uint32_t *tcnt)
{
    const WsFieldGrid g = {grid6[0], grid6[1], grid6[2], grid6[3], grid6[4], grid6[5], dims[0], dims[1], dims[2]};
    const uint32_t nodes = dims[0] * dims[1] * dims[2];
    hipLaunchKernelGGL(k_iso_count, dim3(cdiv(nodes, WS_BLOCK)), dim3(WS_BLOCK), 0, s, rho, g, iso, code, vcnt, tcnt, nodes);
}

uint32_t wsk_iso_blocks(const uint32_t *dims) { return cdiv(dims[0] * dims[1] * dims[2], WS_BLOCK); }

// the two grand totals (the last entries of the two scans) side by side, for one small copy to the host
__global__ void k_iso_totals(const uint32_t *__restrict__ v_total, const uint32_t *__restrict__ t_total, uint32_t *__restrict__ out)
{
    if (threadIdx.x == 0) {
        out[0] = *v_total;
        out[1] = *t_total;
    }
}

void wsk_iso_totals(hipStream_t s, const uint32_t *v_total, const uint32_t *t_total, uint32_t *out)
{
    hipLaunchKernelGGL(k_iso_totals, dim3(1), dim3(64), 0, s, v_total, t_total, out);
}

void wsk_iso_mesh(hipStream_t s, const float *rho, const float *grad, const float *grid6, const uint32_t *dims, float iso,
                  const uint8_t *code, const uint32_t *vstart, const uint32_t *tstart, uint32_t *vbase, float *xyz,
                  float *nrm, uint32_t *tri)
{
    const WsFieldGrid g = {grid6[0], grid6[1], grid6[2], grid6[3], grid6[4], grid6[5], dims[0], dims[1], dims[2]};
    const uint32_t nodes = dims[0] * dims[1] * dims[2];
    const dim3 grid(cdiv(nodes, WS_BLOCK));
    if (nrm) hipLaunchKernelGGL(k_iso_vertices<true>, grid, dim3(WS_BLOCK), 0, s, rho, grad, g, iso, code, vstart, vbase, xyz, nrm, nodes);
    else hipLaunchKernelGGL(k_iso_vertices<false>, grid, dim3(WS_BLOCK), 0, s, rho, grad, g, iso, code, vstart, vbase, xyz, nrm, nodes);
    hipLaunchKernelGGL(k_iso_triangles, grid, dim3(WS_BLOCK), 0, s, g, code, tstart, vbase, tri, nodes);
}
