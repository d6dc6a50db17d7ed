// ws_internal.h -- shared between the C-ABI host code and the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "wsfluid.h"

#include "ws_devhooks.h"

// Everything a kernel needs besides array pointers; passed by value (kernarg / SGPRs).
// Slab handles: where the force kernel's epilogue puts a particle whose new predicted position left the slab
// (one copy in device memory, WsDev::mig points at it)
struct WsMig {
    const uint32_t *cuts;  // world + 1 global x-layer cuts
    uint32_t world, me;
    uint32_t *dyn;         // DY_* words
    uint32_t *hole;        // indices the leavers vacate
    uint32_t hole_cap;
    uint32_t *sendL, *sendR;  // neighbour migration messages (header + mig_cap records of 64 B)
    uint32_t mig_cap;
    uint32_t *far;            // the messages (one per destination rank) for particles that cross several slabs
    uint32_t far_cap;
};

struct WsDev {
    // FluidStaticProps, src/fluid_compute.rs:41-51
    float dt, damping, h, target_density, pressure_scalar, near_pressure_scalar, viscosity;
    // SmoothingKernel, src/fluid_compute.rs:30-38
    float k_pow2, k_pow2_der, k_pow3, k_pow3_der, k_spikey;
    float grav[3];
    float ext_min[3], ext_max[3];
    // Largest f32 T with sqrtf(T) <= h: `!(d2 > T)` is bit-for-bit the reference's
    // `!(distance > smoothing_radius)` without taking the square root first.
    float d2_accept;
    // dense cell grid over the padded container: cell = floor(pred / h) (simulation.wgsl:121-123)
    int32_t org[3];  // grid origin in cell coordinates
    int32_t dim[3];  // grid cells along x, y, z (z fastest in memory, x slowest)
    // A grid cell is cm[c] of the reference's cells wide along axis c (1 everywhere unless the reference-sized grid
    // would not fit the cell budget: a small smoothing radius in a big container, ws_api.cpp derive_dev).  Edges stay
    // >= h, so the 27-cell search still covers every neighbour; candidates a wider cell adds fail the distance test.
    int32_t fdim[3];  // reference-sized cells along x, y, z of the GLOBAL grid (== dim when cm == 1 on one GPU)
    int32_t cm[3];
    uint32_t coarse;  // any cm != 1
    int32_t guard;   // guard entries in front of / behind cell_start
    uint32_t n;      // particles the kernels process: sorted indices [base, base + n)
    uint32_t base;   // first owned slot of the sorted arrays (0 on one GPU; ghosts sit in front of it in a slab)
    int32_t gdim_x;  // cells along x of the GLOBAL grid (== dim[0] on one GPU)
    int32_t xoff;    // global x index of local layer 0 (0 on one GPU)
    uint32_t ncells;
    uint32_t hash_n;  // the reference's `num_particles` in hash_cell (global N)
    // Slab handles only (nullptr / 0 on a single-GPU handle).  A slab's owned count changes with migration and is
    // known on the device alone: kernels are launched over `n` = a host-side UPPER BOUND and read the real count
    // from dyn[DY_N]; the density / force kernels cover the part of the owned range that range_sel names, resolved
    // on the device from the cell starts at lidx (ws_kernels.hip ws_range).
    const uint32_t *dyn;
    uint32_t range_sel;            // WS_RANGE_*
    uint32_t has_left, has_right;  // x-neighbours present
    uint32_t lidx[4];              // cell-start indices: layer 1 begin / end, layer nxl-2 begin / end
    const WsMig *mig;              // device copy; non-null = the force epilogue also does migration part 1
    uint32_t mig_limit;            // records the NEXT step's migration messages will carry (<= WsMig::mig_cap; 0 = all of it)
    uint32_t far_limit;            // ... and each of its far messages (<= WsMig::far_cap; 0 = all of it)
};

// words of the device block `dyn` of a slab handle
enum {
    DY_N = 0,        // owned particles
    DY_NHOLE,        // leavers of the step being migrated (all routes; per route they are counted in the message headers)
    DY_GL,           // ghosts staged in front of / behind the owned range
    DY_GR,
    DY_ERR,          // sticky WS_DYN_ERR_* bits
    DY_LEFT,         // cumulative: particles that left / arrived
    DY_ARRIVED,
    DY_FAR,          // cumulative: leavers that took the far route (crossed more than one slab in a step)
    DY_STEP,         // steps whose migration has run since the handle was created / reset (k_migrate_fill counts): the
                     // stamp of every message and the slot of the status ring come from here, not from the host, so a
                     // captured graph of the step replays unchanged
    DY_HALO_NOW,     // the larger of this step's two boundary-layer populations (k_halo_pack; k_migrate_fill hands it on and clears it)
    DY_PEAK_HALO,    // since the last load: the most particles a boundary layer of this slab held (records of a halo message)
    DY_PEAK_MIG,     // ... and the most particles that left towards ONE neighbour in one step (records of a migration message)
    DY_PEAK_FAR,     // ... and the most that crossed more than one slab in one step (records of the far message)
    // scratch of the multi-kernel migration fill (k_fill_*: a step that moves more than a few ten thousand particles)
    DY_F_FAR, DY_F_NTGT, DY_F_NSRC, DY_F_NOLD, DY_F_NNEW, DY_F_ARR, DY_F_LEAVE, DY_F_NL, DY_F_NR, DY_F_WANTED,
    WS_DYN_WORDS = 32
};
enum {
    WS_DYN_ERR_MIGRATION = 1u,  // more leavers than a migration message holds
    WS_DYN_ERR_CAPACITY = 2u,   // owned count would exceed the slab's capacity
    WS_DYN_ERR_HALO = 4u,       // a boundary layer holds more particles than a halo message
    WS_DYN_ERR_GHOSTS = 8u,     // more ghosts than the ghost range holds
    WS_DYN_ERR_STAMP = 16u,     // a message stamped with another step arrived: the transport delivered out of order
    WS_DYN_ERR_PRED = 32u       // an uploaded particle had to migrate with a predicted position its record cannot reproduce
};
enum { WS_RANGE_ALL = 0, WS_RANGE_EARLY = 1, WS_RANGE_LATE_LEFT = 2, WS_RANGE_LATE_RIGHT = 3, WS_RANGE_LATE_BOTH = 4 };
#define WS_HDR_WORDS_HOST 8u  // words of a message header (ws_kernels.hip WS_HDR_WORDS)
#define WS_MIG_REC_WORDS_HOST 8u  // = WS_MIG_REC_WORDS of ws_kernels.hip: {pos, id}, {vel, 0}
#define WS_HDR_UNKNOWN 0xFFFFFFFFu  // header words 4 / 5 before the first migration / halo of a particle set has been counted

// density / force kernel family (developer builds: WS_VARIANT=simple in the environment, for A/B tests)
enum { WS_VARIANT_SIMPLE = 0, WS_VARIANT_LISTED = 2 };

// Accept masks K4 writes and K5 walks: bit s of owned particle p (sorted order, p = index - base) = its s-th
// candidate in visit order is a neighbour.  words[w][p]: a wave's access to one word row is one coalesced segment.
struct WsMask {
    uint32_t *words;
    uint32_t stride;  // particles per row
};

// The particle set in the order of the last step: ONE 32-byte record {position, id | velocity, cell id} per particle
// (round 5; two arrays until then): k_reorder fetches a particle through its index with two 16-byte loads of ONE line
// (position, velocity and cell id used to be three scattered reads, a 128-byte line each once the fluid has mixed), and it
// is the shape a migrating particle travels in.  The force kernel's epilogue writes it with full-line stores (lane pairs
// exchange halves first: store_records).
struct WsSoA {
    float4 *pv;    // [2 i] = {position.xyz, particle id (bits)}, [2 i + 1] = {velocity.xyz, cell id (bits; = cid_cur[i])}
    float4 *pred;  // xyz = predicted_position: what an upload supplied; the step loop does not maintain it (k_reorder)
    // Optional (single-GPU handles): the particle's arrival rank inside its cell, as returned by the histogram's
    // atomic when the particle was binned.  With it the sort places particles without a second round of atomics.
    uint32_t *rank;
    __host__ __device__ float4 &pos(uint32_t i) const { return pv[2 * (size_t)i]; }
    __host__ __device__ float4 &vel(uint32_t i) const { return pv[2 * (size_t)i + 1]; }
};

// The test-only build (tests/libwsfluid_refcheck.so, -DWS_WITH_REFCHECK -Itests/refcheck) adds a validation mode
// whose declarations, kernels and host code all live under tests/refcheck/; the product build sees none of it.
#ifdef WS_WITH_REFCHECK
#include "ws_refcheck.h"
#endif

// planar copy of the sorted predicted positions (K4's radius tests)
// The cell-sorted copy.  Predicted position and velocity are interleaved: a neighbour's {pred.xyz, density}
// and {vel.xyz, near density} are the two halves of ONE 32-byte record, so the force kernel's two 16-B gathers per
// neighbour hit the same cache line (C3 dense state: -17 % kernel time against two separate arrays), and a halo
// message is one range.
struct WsSorted {
    float4 *pos;  // xyz = position, w = particle id (bits); only the integrator reads it
    float4 *pv;   // [2j] = {pred.xyz, density after K4}, [2j + 1] = {vel.xyz, near density after K4}
    __host__ __device__ float4 &pred(uint32_t j) const { return pv[2 * (size_t)j]; }
    __host__ __device__ float4 &vel(uint32_t j) const { return pv[2 * (size_t)j + 1]; }
    // The gathers of the force kernel's inner loop: a 32-bit byte offset from the (uniform) base lets the load
    // take its base from scalar registers, with no 64-bit address arithmetic per neighbour.  Needs
    // 32 * slots < 2^32, which ws_create / ws_slab_create check (WS_MAX_SLOTS).
    __device__ const float4 &pred_near(uint32_t j) const
    {
        return *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(pv) + j * 32u);
    }
    __device__ const float4 &vel_near(uint32_t j) const
    {
        return *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(pv) + j * 32u + 16u);
    }
};
#define WS_MAX_SLOTS (1u << 27)

struct WsXYZ {
    float *x = nullptr, *y = nullptr, *z = nullptr;
};

// Tile schedule of a full-range launch of K4 / K5 (single-GPU handles).  Workgroup b works for XCD b & 7 (the hardware
// deals workgroups round-robin over the XCDs) and takes the (b >> 3)-th entry of that XCD's part of `perm`:
// perm[split[x] .. split[x + 1]) = the tiles of one contiguous x-slab of the sorted order (so an XCD's L2 keeps seeing one
// neighbourhood), slabs cut so that every XCD gets the same COST, tiles inside a slab in descending cost classes (the
// launch drains through its cheapest tiles, not through whichever came last).  cost[tile] = how long the tile's
// workgroup ran in the previous step (100 MHz ticks), written by the kernels themselves; k_schedule turns it into
// split / perm beside the next step's sort phase.  Any schedule computes the same results.
struct WsSched {
    uint32_t *split = nullptr;  // 9 words
    uint32_t *perm = nullptr;   // ntiles words
    uint32_t *cost = nullptr;   // ntiles words
};

struct WsEventPair {
    uint32_t kernel;
    hipEvent_t a, b;
    bool counts = true;  // false: the second launch of a kernel id within one step (time is added, the launch count is per step)
};

// What every float of a caller's objects and query points is refused for: not finite, or so large that the kernels'
// products and sums of a few of them could overflow.
inline bool ws_bad_float(float x) { return !isfinite(x) || fabsf(x) > 1e15f; }

// ---- who owns device memory ------------------------------------------------------------------------------------------
// Every device allocation and every page-locked host allocation of a ws_handle / WsSlab has exactly ONE owner, of one of
// the two forms below: the ONLY places of the host code that allocate or free (DESIGN.md 2 lists which lifetime owns
// what).  Giving a lifetime up is one release() per owner, which cannot miss a member.  Nothing is freed by a destructor:
// release is an explicit call, made with the handle's device current.
//
// A failed allocation (ws_api.cpp ws_hip_failed) is WS_ERR_OUT_OF_MEMORY when HIP says so, else WS_ERR_HIP; `what`
// names the buffer in ws_last_error; the sticky HIP error is cleared (the next ws_step checks hipGetLastError), so a
// handle whose call could not get its scratch stays usable.
ws_status ws_hip_failed(ws_handle *h, const char *what, hipError_t e);

// Outgrown buffers that could not be freed where they were replaced (WsScratch::grow_parked); freed with the handle.
struct WsParked {
    std::vector<void *> list;
    void release()
    {
        for (void *q : list) (void)hipFree(q);
        list.clear();
    }
};

template <class... Owner>
void release_all(Owner &...o)
{
    (o.release(), ...);
}

// Form 1: a buffer with a size of its own -- allocated on first use, grown on demand.  PINNED: page-locked host memory.
// After a failed alloc() p == nullptr and bytes == 0.
template <class T, bool PINNED = false>
struct WsScratch {
    T *p = nullptr;
    size_t bytes = 0;
    // release(), then `need` bytes
    ws_status alloc(ws_handle *h, size_t need, const char *what)
    {
        release();
        return fresh(h, need, what);
    }
    // nothing when it holds `need` bytes already, else alloc()
    ws_status grow(ws_handle *h, size_t need, const char *what) { return bytes >= need ? WS_OK : alloc(h, need, what); }
    // grow() for a buffer that may be outgrown BETWEEN THE COLLECTIVES of a slab call: the old buffer is PARKED, not freed
    // (WsSlab::retired, released with the handle).  hipFree waits for the whole device, and between the two all-gathers
    // of a collective read a peer that is a step ahead on the host may already have its next transport kernel on the
    // device, waiting for THIS rank's contribution -- with all ranks in one process on one GPU (in-process hosts; the
    // tests' stand-in for librccl) that wait and hipFree's would wait for each other.  Growth is geometric -- to at least
    // bytes + bytes / slack_div -- so the parked buffers add up to less than a small multiple of the live one.  A failure
    // keeps the old buffer.
    ws_status grow_parked(ws_handle *h, size_t need, size_t slack_div, WsParked *parked, const char *what)
    {
        if (bytes >= need) return WS_OK;
        T *const old = p;
        const size_t geometric = bytes + bytes / slack_div;
        const ws_status st = fresh(h, need > geometric ? need : geometric, what);  // (p is replaced on success only)
        if (!st && old) parked->list.push_back(old);
        return st;
    }
    void release()
    {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }

private:
    ws_status fresh(ws_handle *h, size_t want, const char *what)  // overwrites p, on success only
    {
        void *q = nullptr;
        const size_t real = want > 4 ? want : 4;
        const hipError_t e = PINNED ? hipHostMalloc(&q, real, hipHostMallocDefault) : hipMalloc(&q, real);
        if (e != hipSuccess) return ws_hip_failed(h, what, e);
        p = static_cast<T *>(q);
        bytes = want;
        return WS_OK;
    }
};

// Form 2: arrays that are allocated together and released together.  Most of them are members of the by-value
// kernel-argument structs (WsSoA, WsSorted, WsXYZ, WsMask, WsSched, WsMig), which stay plain pointers: the group
// allocates INTO a field and remembers the field's address; release() frees each buffer and nulls its field.  Handles
// (ws_handle, WsSlab) are heap objects that never move or get copied, so the remembered addresses stay valid for as long
// as the group lives.  A pointer that merely aliases a member (ws_handle::start, sched4[1].cost) is nulled by whoever
// releases the group.
struct WsGroup {
    std::vector<void **> fields;
    // zero: also cleared, on the handle's stream (ordered before everything that stream does with it)
    template <class T>
    ws_status alloc(ws_handle *h, T **field, size_t bytes, const char *what, bool zero = false);
    void release()
    {
        for (void **f : fields) {
            (void)hipFree(*f);
            *f = nullptr;
        }
        fields.clear();
    }
    // For a lifetime that is rebuilt at another size BEFORE its buffers are given up (ws_api.cpp grow_particle_arrays):
    // take() empties the group and hands its buffers out -- the fields keep pointing at them until the group allocates into
    // them again; restore() releases what the group has allocated since and makes the held buffers the group's again;
    // drop() frees them.  Exactly one of the two ends a take().
    struct Held {
        std::vector<void **> fields;
        std::vector<void *> bufs;
    };
    Held take()
    {
        Held k;
        k.fields.swap(fields);
        for (void **f : k.fields) k.bufs.push_back(*f);
        return k;
    }
    void restore(Held &k)
    {
        release();
        for (size_t i = 0; i < k.fields.size(); i++) *k.fields[i] = k.bufs[i];
        fields.swap(k.fields);
        k.bufs.clear();
    }
    static void drop(Held &k)
    {
        for (void *q : k.bufs) (void)hipFree(q);
        k.bufs.clear();
        k.fields.clear();
    }
};

// ws_handle::field: the scratch of the derived-field calls -- their own counting sort of the CURRENT positions, allocated
// on the first call, freed by ws_destroy.  Nothing ws_step reads is written.  Per particle: 12 B positions by id
// (single-GPU handles), 3 x 4 B keys / tentative slots / sorted ids, 16 B sorted {position, id} = 40 B; per cell: count,
// cursor and start (4 B each) and the scan state; plus the queries and results of the largest call so far.  
struct WsField {
    // per particle, exact size, keyed by n: a call with another particle count releases EVERYTHING below and starts over
    uint32_t n = 0;                   // particles the arrays hold
    WsScratch<float> xyz;             // positions by id (single-GPU handles; a slab samples the gathered S->g_out); the
                                      // by-id positions the whitewater spawn kernel reads on a single handle
    WsScratch<uint32_t> keys, tmp, perm;  // cell id by id, tentative slots, sorted ids
    WsScratch<float4> spos;           // {position, id} in cell order, id inside a cell; ALIASED: an anisotropic call
                                      // overwrites it with the centres in THEIR cell order (field_aniso_bin)
    // per cell, exact size, keyed by cells: rebuilt after a re-grid (bsum zeroed once at allocation, start[cells] = n
    // written when the tables are made)
    uint32_t cells = 0;               // cells the tables describe
    WsScratch<uint32_t> count, cursor, start, bsum;  // cells (+ 1) words each, and the scan state
    // everything below is grow-only: allocated by the first call that needs it, kept at the largest size seen
    WsScratch<float> q, rho;          // query points and densities on the device
    WsScratch<float> grad;            // gradients; ALIASED: the velocity and advect calls put their velocities here
    // surface extraction (ws_extract_surface): node codes and vertex bases, per-workgroup totals and their scans
    // (2 x blocks + 1 words each, 16 B aligned halves; bstart also the two grand totals) and scan state, the mesh
    WsScratch<uint8_t> code;
    WsScratch<uint32_t> vbase, bcnt, bstart, bstate, tri;
    WsScratch<float> mxyz, mnrm;
    // velocity field (ws_sample_velocity_*, ws_advect_points, whitewater): the velocities by id and in cell order beside
    // spos, and on slab handles the gathered positions by id (the gather brings {position, velocity} records, split into
    // vpos / vxyz); vpos is also the by-id positions the whitewater spawn kernel reads on a slab
    WsScratch<float> vxyz, vpos;
    WsScratch<float4> svel;
    // whitewater (ws_read_whitewater, ws_emit_whitewater, ws_step_whitewater): the normals in spos' order, the stage by id
    // (trapped, crest, align, energy, normal x 3 as one array of 7 n floats; the neighbour counts), the emission counts,
    // their scan and its state, the spawns (xyz, velocity: 3 floats, life, source: 1 word each, as one array), a step's
    // particles (7 floats + 1 byte each)
    WsScratch<float4> wnrm;
    WsScratch<float> wst, wout, wpt;
    WsScratch<uint32_t> wnb, wcnt, woff, wstate;
    // surface tension and XSPH (ws_read_cohesion, ws_apply_cohesion): {normal, density} in spos' order; the stage by id
    // as 16-byte records ({dv, count}, then for the read {normal, density}: n float4 each); the read's outputs (normal
    // x 3, density, dv x 3 as one array of 7 n floats; the neighbour counts)
    WsScratch<float4> cnd, crec;
    WsScratch<float> cst;
    WsScratch<uint32_t> cnb;
    // attributes (ws_diffuse_attributes, ws_sample_attribute_*): the attributes in spos' order, twice (the iterations
    // ping-pong; the field reads the first), the IEEE densities in spos' order, a field call's values (4 per query)
    WsScratch<float4> sattr[2];
    WsScratch<float> srho;
    WsScratch<float4> aval;
    // bodies (ws_body_forces), one array of words: the chunk table (4 per chunk) and the chunks' partial sums (8 per chunk),
    // the bodies' first chunks (nb + 1), the samples (xyz, velocity: 3 floats, volume: 1) and the centres (3 per body), the
    // per-sample results (force: 3, fraction: 1) and the per-body ones (force, torque: 3, volume, wet count: 1)
    WsScratch<float> body;
    // anisotropic kernels (ws_read_anisotropy, ws_sample_aniso_*, ws_extract_aniso_surface): centres, ellipsoids and
    // neighbour counts by id, the centres' ellipsoids in their cell order (their {c, id} reuse spos)
    WsScratch<float> cxyz;
    WsScratch<float4> amf, smf;
    WsScratch<uint32_t> anb;
    // rays (ws_cast_rays / ws_cast_camera): the rays of a list call (origins, then directions: 24 B per ray) and the
    // results (4 B + 12 B per ray)
    WsScratch<float> rays, ray_t, ray_n;
};

// One resident signed-distance volume (ws_volume_upload) as ws_collide_volumes' kernel sees it
struct WsVolumeDesc {
    const float *sdf;  // dims[0] x dims[1] x dims[2] floats on the device, x fastest; nullptr: the slot is empty
    uint32_t dims[3];
    float origin[3];
    float spacing[3];
};

// What a record view's pressures are computed from: the density -> pressure parameters of the step that computed the
// densities, not the handle's current ones (ws_set_params may have come in between).
struct WsPressureParams {
    float pressure_scalar, target_density, near_pressure_scalar;
};

struct ws_handle {
    int device = 0;
    uint32_t flags = 0;
    uint32_t prof_mask = 0xFFFFFFFFu;
    uint32_t n = 0;
    uint32_t cap = 0;  // single-GPU handles: particles the particle arrays and the attribute array hold (>= n; ws_reserve_particles)
    uint64_t steps = 0;
    bool have_step = false;  // single-GPU handles: the sorted copy holds the last step's fields of the CURRENT particle set
                             // (false after a load and after a count change, which leaves `steps` counting)
    ws_params params{};
    ws_smoothing_kernel sk{};
    WsDev dev{};
    WsPressureParams last_pressure{};  // of the last step enqueued (ws_step records them; zero again wherever steps returns to 0)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool done_recorded = false;

    WsSoA cur{};   // state in the order of the last step (written by the force kernel)
    WsSorted srt{};  // cell-sorted copy the density/force kernels read
    WsXYZ sxyz;                   // planar predicted positions in `srt` order
    uint32_t *cid_cur = nullptr;  // cell id per particle of `cur`
    uint32_t *cid_srt = nullptr;  // cell id per particle of `srt`
    int variant = WS_VARIANT_LISTED;  // density / near density ride in srt.pred(i).w / srt.vel(i).w
    float4 *accel = nullptr;      // acceleration in `srt` order
    uint32_t *slot_tmp = nullptr; // particle index per tentative slot
    uint32_t *count = nullptr;    // per-cell particle count (histogram)
    uint32_t *cursor = nullptr;   // per-cell fill cursor
    uint32_t *start = nullptr;    // guard + ncells + 1 + guard exclusive starts
    uint32_t *start_alloc = nullptr;  // its allocation (start sits 0..3 words in: see alloc_grid)
    uint32_t *bsum = nullptr;     // scan state (ticket + tile descriptors), zeroed at allocation
    WsMask mask = {nullptr, 0};   // accept masks (listed variant)
    bool ieee = false;            // WS_FLAG_IEEE_DIVISION: correctly rounded sqrt / division in the pair terms
    uint32_t *stats = nullptr;    // device counters: [0] particle-steps with more candidates than the mask holds
    uint8_t *mult = nullptr;      // 27 stencil multiplicities (hash aliasing), device
    WsScratch<uint32_t> force_cnt;  // ws_apply_forces: WS_MAX_FORCES per-emitter counts (allocated by the first call that asks)
    WsScratch<unsigned long long> solid_sums;  // ws_collide_solids / _volumes: WS_MAX_SOLIDS x WS_SOLID_WORDS sums (allocated by the first call that asks)
    // ws_volume_upload: the resident signed-distance volumes, one exact-size buffer per slot (p == nullptr: empty), what
    // the kernel is told about each and a hash of {dims, origin, spacing, the array's bytes} for the slabs' agreement
    WsScratch<float> volume[WS_MAX_VOLUMES];
    WsVolumeDesc volume_desc[WS_MAX_VOLUMES] = {};
    uint64_t volume_hash[WS_MAX_VOLUMES] = {};
    // the per-particle attributes: one float4 per particle BY ID (n; on slab handles n_global, replicated on every rank),
    // allocated all +0 by the first attribute call (p == nullptr: every attribute is +0), zeroed by ws_reset
    WsScratch<float4> attr;
    // ws_remove_particles / _ids: the per-sink counts, the survivor count and the scan's tile sums (ws_population.hip;
    // allocated by the first removal, a word per 2048 particles)
    WsScratch<uint32_t> pop_words;
    // ws_measure: the sums and keys of up to WS_MAX_REGIONS gauges (WS_GAUGE_OUT_BYTES); ws_select_particles: the ids it
    // lists (ws_gauges.hip; each allocated by the first call that needs it)
    WsScratch<unsigned long long> gauge_out;
    WsScratch<uint32_t> gauge_ids;
    bool alias = false;
    size_t grid_alloc_cells = 0;  // cells that count / cursor hold
    // The owners of the arrays above, one per lifetime (ws_api.cpp):
    WsGroup particles;  // cur, srt, sxyz, cid_*, accel, slot_tmp, mask.words: alloc_particle_arrays .. free_particle_arrays
    WsGroup cells;      // count, cursor: kept by a re-grid that needs no more cells (alloc_grid)
    WsGroup starts;     // start_alloc, bsum: rebuilt by every alloc_grid
    WsGroup sched;      // the tile schedule's split / perm / cost (alloc_schedule .. free_schedule)
    WsGroup fixed;      // stats, mult: created with the handle, freed with it

    // staging for uploads / readback (ws_api.cpp ensure_stage): `stage` is the alias of stage_mem.p that the calls use
    WsScratch<char> stage_mem;
    void *stage = nullptr;
    // asynchronous position readback (ws_read_positions_begin / _end): own staging, own copy stream
    hipStream_t copy_stream = nullptr;
    hipEvent_t rb_gathered = nullptr, rb_done = nullptr;
    WsScratch<float> rb_stage;
    bool rb_inflight = false;
    // ws_read_positions_begin(h, NULL): two page-locked buffers the library owns, filled alternately
    WsScratch<float, true> rb_host[2];
    int rb_fill = 0, rb_last = -1;  // the buffer the readback in flight fills; the one the last finished readback filled
    bool rb_owned = false;          // the readback in flight goes into rb_host[rb_fill]

    // reference-layout sort view (lazy)
    WsScratch<uint32_t> v_keys, v_perm, v_tmp, v_count, v_cursor, v_start, v_bsum, v_off;

    WsField field;  // derived-field calls (csrc/ws_field.inc)

    // profiling
    std::vector<WsEventPair> pending;
    std::vector<hipEvent_t> pool;
    double prof_ms[WS_K_COUNT] = {0};
    uint64_t prof_cnt[WS_K_COUNT] = {0};

#ifdef WS_WITH_REFCHECK
    bool refmode = false;  // WS_FLAG_REFERENCE_ORDER (test-only build)
    WsRef ref;
#endif

    // Cost-guided tile schedule of the two neighbour kernels (single-GPU handles; ws_kernels.hip "tile schedule").
    // Two sets: step t's kernels read set t & 1 while k_schedule, running beside K5(t) on a stream of its own, writes
    // set (t + 1) & 1 from K4(t)'s costs and K5(t - 1)'s.
    WsSched sched4[2], sched5[2];          // K4's (64-particle tiles) and K5's (128-particle tiles); cost4 is shared
    uint32_t sched_tiles4 = 0, sched_tiles5 = 0;
    bool sched_on = false;                 // the schedule arrays exist and describe the current particle count
    uint32_t sched_classes = 8, sched_group = 64;  // cost classes; particles per group of tiles that is classed as one
    uint32_t sched_parity = 0;             // the set the NEXT step's kernels read
    hipStream_t sched_stream = nullptr;
    hipEvent_t ev_sched_in = nullptr, ev_sched_out = nullptr;

    // WS_FLAG_GRAPH on a single-GPU handle: the captured steady-state step
    hipGraphExec_t graph_exec = nullptr;
    bool graph_failed = false;
    uint64_t graph_steps = 0;

    // slab (multi-GPU) state; slab == nullptr on a single-GPU handle
    bool accel_stale = false;  // accel[] is behind the last step (computed on demand: refresh_accel)
    bool pred_stale = false;  // cur.pred is behind cur.pos / cur.vel (the step loop does not store it: k_reorder)
    struct WsSlab *slab = nullptr;
    bool own_stream = true;
    bool dead = false;  // a re-grid failed after the old tables were given up: every later ws_step refuses (err says why)

    std::string err;
};

template <class T>
ws_status WsGroup::alloc(ws_handle *h, T **field, size_t bytes, const char *what, bool zero)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return ws_hip_failed(h, what, e);
    *field = static_cast<T *>(q);
    fields.push_back(reinterpret_cast<void **>(field));
    if (zero && (e = hipMemsetAsync(q, 0, bytes, h->stream)) != hipSuccess) return ws_hip_failed(h, what, e);
    return WS_OK;
}

struct WsGraphEntry {
    uint32_t n_bound = 0, mig_cur = 0, mig_next = 0, halo = 0, far_cur = 0, far_next = 0;  // what a captured step has baked in
    hipGraphExec_t exec = nullptr;
};
struct WsSlab {
    ws_transport tr{};
    uint32_t rank = 0, world = 1;
    uint32_t n_global = 0;
    // fixed capacities, known to both ends of every message
    uint32_t cap = 0;        // owned particles
    uint32_t halo_cap = 0;   // particles of one boundary layer = ghosts per side = records of a halo message
    uint32_t mig_cap = 0;    // records of a neighbour migration message
    uint32_t far_cap = 0;    // records of ONE far message (one per destination rank) for particles that cross several slabs
    uint32_t hole_cap = 0;   // leavers per step (all routes)
    uint32_t max_arrivals = 0;
    // Message SIZES follow the fluid (round 4).  The buffers keep their fixed capacities; what travels each step is a
    // prefix sized from what every rank reported three to four steps ago (header words 4 / 5 / 6 of the far
    // message = the status table): the same table on every rank, hence the same size at both ends of every exchange.
    uint32_t mig_limit_cur = 0;       // records of the migration messages exchanged by the step being enqueued
    uint32_t mig_limit_next = 0;      // ... by the next one (the force kernel of this step fills them: WsDev::mig_limit)
    uint32_t far_limit_cur = 0, far_limit_next = 0, want_far = 0;  // the same for the far messages
    uint32_t halo_limit = 0, halo_limit_next = 0;  // records of this step's / the next step's halo messages
    uint32_t want_mig = 0, want_halo = 0;   // maxima over all ranks (header words 4 / 5) and over the last eight tables
    uint32_t want_ring[3][8] = {};          // the last eight tables' maxima: migration, halo, far
    uint64_t arrivals_hist[4] = {0, 0, 0, 0};  // upper bounds of the arrivals of the last four steps (launch bound)
    uint32_t floor_mig = 4096, floor_far = 256, floor_halo = 8192;  // no message is sized below these (records)
    // WS_FLAG_EXACT_MESSAGES: every message carries exactly what its sender has for it -- ws_step waits for the counts
    // (one all-gather of four words per rank before the migration, one before the halos, behind the early K4)
    bool exact_messages = false;
    uint32_t *xs_send[2] = {nullptr, nullptr}, *xs_all[2] = {nullptr, nullptr};  // [migration | halo]
    WsScratch<uint32_t, true> xs_host[2];
    hipEvent_t ev_sizes[2] = {nullptr, nullptr};
    uint32_t *far_pack = nullptr;     // the far messages at the stride of what travels
    uint32_t exact_now[3] = {0, 0, 0};  // the records the last step's migration / halo / far messages carried
    uint32_t size_waits = 0;            // host waits for message sizes so far (two per step with exact sizes)
    uint32_t limit_hold = 0;          // steps for which the limits stay at the full capacities (after a load / parameter change)
    bool fixed_messages = false;      // WS_FLAG_FIXED_MESSAGES (and a captured step with peers): always the full capacities
    uint32_t mode_word = 0;           // every choice that fixes the step's collective sequence or its results: all ranks must agree (slab_agree_mode)
    std::vector<uint32_t> cuts;       // world + 1 global x-layer cuts
    uint32_t *cuts_dev = nullptr;
    uint32_t *dyn = nullptr;          // WS_DYN_WORDS device words (DY_*)
    WsMig *mig_dev = nullptr;         // device copy of the migration targets (WsDev::mig)
    uint32_t *hole = nullptr, *tgt = nullptr, *src = nullptr;  // migration index lists
    uint32_t *mig_sendL = nullptr, *mig_sendR = nullptr, *mig_recvL = nullptr, *mig_recvR = nullptr;
    uint32_t *far_send = nullptr, *far_all = nullptr;
    uint32_t *halo_sendL = nullptr, *halo_sendR = nullptr, *halo_recvL = nullptr, *halo_recvR = nullptr;
    bool binned = false;              // cid_cur / count describe the current owned set
    // what the host knows about the device state, two steps late
    uint32_t *status_dev = nullptr;  // ring of per-rank header rows, and its page-locked copy on the host
    WsScratch<uint32_t, true> status_host;
    hipEvent_t ev_status[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t n_known = 0;             // owned count as of step n_known_step
    uint64_t n_known_step = 0;
    uint64_t t0 = 0;                  // h->steps when the owned set was last loaded (create / reset / write / re-grid):
                                      // status tables of earlier steps describe another particle set
    uint32_t cfg_ghost_capacity = 0;  // ws_device_cfg.ghost_capacity as given (0 = derive from the grid)
    // id-ordered global views (ws_read_positions & co. on a slab handle): count words, packed records of this rank,
    // every rank's records, the id-ordered result
    WsScratch<uint32_t> cnt_send, cnt_all;
    WsScratch<uint32_t> g_send, g_all, g_out;  // (grown by half: grow_parked)
    WsScratch<uint32_t> hist;         // x-layer histogram of a re-grid (one buffer, grown by doubling: slab_layer_hist)
    WsScratch<uint32_t> agree_send, agree_all;  // one word per rank: verdicts and the mode word (slab_agree_words)
    WsParked retired;                 // outgrown gather and histogram buffers (WsScratch::grow_parked)
    // The owners of the plain pointers of this struct (ws_slab.inc):
    WsGroup fixed;                    // dyn, status_dev, xs_send[], xs_all[]: created with the handle, freed with it
    WsGroup geometry;                 // cuts_dev .. far_pack, the messages: slab_alloc_arrays .. slab_free_arrays (a re-grid)
    std::vector<uint32_t> counts;     // owned particles per rank as of the last gather
    std::vector<uint32_t> caps;       // ... and every rank's owned capacity (a re-grid decides for all ranks alike)
    uint64_t left_base = 0, arrived_base = 0, far_base = 0;  // cumulative counters carried over the loads (ws_slab_counters)
    bool balanced = false;            // the cuts come from ws_slab_rebalance (a re-grid re-balances on the new grid)
    uint32_t failed = 0;              // sticky WS_DYN_ERR_* bits seen on any rank
    bool comm_failed = false;         // a transport call failed: the handle is dead
    // halo / compute overlap: the halos travel on `comm` while the particles that need no ghosts compute
    hipStream_t comm = nullptr, copy = nullptr;
    hipEvent_t ev_sorted = nullptr, ev_halo_a = nullptr, ev_k4_late = nullptr, ev_halo_b = nullptr, ev_filled = nullptr;
    bool overlap = true;              // WS_FLAG_NO_OVERLAP turns it off
    bool last_split = false;          // the last step ran K4 / K5 as early + late launches (refresh_accel repeats that)
    // WS_FLAG_GRAPH: captured steps, one per (quantised) launch bound
    std::vector<struct WsGraphEntry> graphs;
    bool graph_failed = false;        // the step could not be captured (transport / runtime): direct launches
    bool capturing = false;           // a capture is being recorded: a transport refusal is not a communication failure
    uint64_t graph_steps = 0;         // steps replayed from a graph
    hipEvent_t ev_copied = nullptr;
    // cumulative statistics (refreshed by ws_slab_read_particles)
    uint64_t migrated_out = 0;
};

// ws_rccl.cpp (not part of the public header): no-op for a transport that is not the library's own
extern "C" void ws_rccl_transport_bind_stream(const ws_transport *t, void *stream);

// ---- kernel launchers (ws_kernels.hip: the step; ws_edits.hip, ws_population.hip, ws_views.hip, ws_fields.hip: the calls around it) ----
void wsk_upload_positions(hipStream_t s, const float *xyz_dev, WsSoA cur, uint32_t n);
void wsk_upload_particles(hipStream_t s, const ws_particle80 *in_dev, WsSoA cur, uint32_t n);
void wsk_bin(hipStream_t s, const WsDev &d, WsSoA cur, uint32_t *cid, uint32_t *count);  // (cur / cid from the first particle to bin)
void wsk_place(hipStream_t s, const WsDev &d, const uint32_t *cid, const uint32_t *rank, const uint32_t *start, uint32_t *slot_tmp);
void wsk_scan(hipStream_t s, uint32_t *count, uint32_t *start_body, uint32_t *cursor, uint32_t *state, uint32_t nitems,
              bool zero_count, uint32_t base);
uint32_t wsk_scan_state_words(uint32_t nitems);
void wsk_scatter(hipStream_t s, const uint32_t *keys, uint32_t *cursor, uint32_t *slot_tmp, uint32_t n, const uint32_t *n_dev);
void wsk_reorder(hipStream_t s, const WsDev &d, const uint32_t *slot_tmp, const uint32_t *cid_cur, const uint32_t *start, WsSoA cur,
                 WsSorted srt, uint32_t *cid_srt, WsXYZ sxyz, bool recompute_pred);
void wsk_refresh_pred(hipStream_t s, const WsDev &d, WsSoA cur);
// The between-step edits (ws_apply_forces, ws_collide_solids; ws_edits.hip): what a call hands its kernel, ONE by-value kernel argument
// whose objects the wave-uniform loop reads through scalar loads.  outputs(): whether the call wants the kernel's sums.
// Forces: affected = k device words the kernel adds the per-emitter counts to, or nullptr.
// Solids: each solid with its squared reach -- the squared distance from its centre beyond which no particle can be in
// contact (solids_reach2 in ws_api.cpp; +inf = never skipped); sums = WS_MAX_SOLIDS x WS_SOLID_WORDS 64-bit device words
// the kernel adds to ({contacts, 3 x impulse, 3 x angular impulse} in 2^-24 fixed point), or nullptr.
struct WsForceSet {
    ws_force e[WS_MAX_FORCES];
};
struct WsForceArgs {
    WsForceSet fs;
    uint32_t k;
    float dt;
    uint32_t *affected;
    bool outputs() const { return affected != nullptr; }
};
#define WS_SOLID_WORDS 7u
struct WsSolidSet {
    ws_solid e[WS_MAX_SOLIDS];
    float reach2[WS_MAX_SOLIDS];
};
struct WsSolidArgs {
    WsSolidSet ss;
    uint32_t k;
    unsigned long long *sums;
    bool outputs() const { return sums != nullptr; }
};
// Volumes (ws_collide_volumes): the descriptors of the handle's WS_MAX_VOLUMES slots (sdf == nullptr: empty, used by no
// pose that passed validation), the poses with their squared reach (volumes_reach2 in ws_api.cpp) and the solids' sums,
// one row of WS_SOLID_WORDS per pose.  About 1.8 KB, like WsSolidSet.
struct WsVolumeSet {
    WsVolumeDesc vol[WS_MAX_VOLUMES];
    ws_volume_pose e[WS_MAX_VOLUME_POSES];
    float reach2[WS_MAX_VOLUME_POSES];
};
struct WsVolumeArgs {
    WsVolumeSet vs;
    uint32_t k;
    unsigned long long *sums;
    bool outputs() const { return sums != nullptr; }
};
static_assert(WS_MAX_VOLUME_POSES == WS_MAX_SOLIDS, "the poses' sums are the solids' accumulator rows");
// Cohesion (ws_apply_cohesion): what the neighbour stage left by id -- {dv, the contributing-neighbour count (bits)}, one
// float4 per particle of the n the stage saw (a record with an id beyond them is left alone) -- and the device words the
// kernel adds the affected particles to, or nullptr: WS_COHESION_SLOTS partial counts, WS_COHESION_SLOT_WORDS words (one
// cache line) apart, which the host sums.
#define WS_COHESION_SLOTS 64u
#define WS_COHESION_SLOT_WORDS 16u
struct WsCohesionArgs {
    const float4 *dvc;
    uint32_t *affected;
    uint32_t n;
    bool outputs() const { return affected != nullptr; }
};
// The state records a slab handle's edit route has gathered ({id, pos, vel, pred}: 10 words each), as an edit's prepare()
// sees them: rank r's min(cnt[4 r], max_n) records at recs + r * stride_words.
struct WsGathered {
    const uint32_t *recs, *cnt;
    uint32_t world, max_n;
    size_t stride_words;
};
// Args = WsForceArgs, WsSolidArgs, WsVolumeArgs or WsCohesionArgs.The first edits `cur` in place and re-bins it (what bin_current leaves: cid, the
// record's cell id, count, rank); the second edits the gathered {id, pos, vel, pred} records of slab handles (d: the global
// grid, its container and damping).
template <class Args>
void wsk_edit_current(hipStream_t s, const WsDev &d, WsSoA cur, uint32_t *cid, uint32_t *count, const Args &a);
template <class Args>
void wsk_edit_records(hipStream_t s, const WsDev &d, uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                      size_t stride_words, const Args &a);
void wsk_density(hipStream_t s, const WsDev &d, const uint32_t *start, const uint32_t *cid_srt, WsSorted srt,
                 const uint8_t *mult, bool alias, int variant, bool ieee, uint32_t *stats, WsMask mask, WsXYZ sxyz,
                 const WsEventPair *ev = nullptr, WsSched sched = WsSched{});
uint32_t wsk_density_tile(void);  // particles per tile of the listed K4 / K5
uint32_t wsk_force_tile(uint32_t n);  // particles per K5 workgroup in a launch over n particles
uint32_t wsk_sched_grid(uint32_t ntiles);  // workgroups of a scheduled launch over ntiles tiles
// s5_costs: the set whose cost array holds the K5 costs to schedule from (the set being written is read by nobody)
void wsk_schedule(hipStream_t s, WsSched s4, uint32_t ntiles4, WsSched s5, WsSched s5_costs, uint32_t ntiles5, uint32_t nclasses,
                  uint32_t group_particles, uint32_t tile5);
uint32_t wsk_mask_words(void);
void wsk_force(hipStream_t s, const WsDev &d, const uint32_t *start, const uint32_t *cid_srt, WsSorted srt, WsSoA out,
               float4 *accel, uint32_t *cid_out, uint32_t *count, const uint8_t *mult, bool alias, int variant, bool ieee,
               WsMask mask, bool accel_only, const WsEventPair *ev = nullptr, WsSched sched = WsSched{});
void wsk_gather_positions(hipStream_t s, WsSoA cur, float *out_xyz, uint32_t n);
void wsk_gather_speeds(hipStream_t s, WsSoA cur, float *out, uint32_t n);
void wsk_gather_velocities(hipStream_t s, WsSoA cur, float *out_xyz, uint32_t n);
void wsk_gather_particles(hipStream_t s, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                          const WsPressureParams &pp, ws_particle80 *out, uint32_t n);
// reference-layout view (ws_views.hip, as the read-backs above it)
void wsk_view_keys(hipStream_t s, const WsDev &d, WsSorted srt, uint32_t *keys_by_id, uint32_t *count);
void wsk_view_count(hipStream_t s, const uint32_t *keys, uint32_t *count, uint32_t n);
void wsk_view_fix(hipStream_t s, const uint32_t *tmp, const uint32_t *keys, const uint32_t *start,
                  uint32_t *perm, uint32_t n);
void wsk_view_offsets(hipStream_t s, const uint32_t *start, uint32_t *off, uint32_t n);
void wsk_iota(hipStream_t s, uint32_t *p, uint32_t n);
void wsk_set_words4(hipStream_t s, uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d);
// density field sampler (ws_sample_density_*; from here to the surface extraction: ws_fields.hip)
void wsk_field_keys(hipStream_t s, const WsDev &d, const float *xyz, uint32_t *keys, uint32_t n);
void wsk_field_gather(hipStream_t s, const uint32_t *perm, const float *xyz, float4 *spos, uint32_t n);
// grid6 = origin xyz, spacing xyz (nullptr: the m points of xyz); bricks: the brick kernel (grid only); smf = nullptr:
// the density sampler (spos = sorted positions), else the anisotropic field (spos = sorted centres, smf their ellipsoids)
void wsk_field_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *smf, bool ieee,
                      bool grad_on, const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks,
                      float *rho, float *grad);
// velocity field (ws_sample_velocity_* / ws_advect_points): pv = n gathered {position, velocity} records by id, split
// into pos (may be nullptr) and vel; svel = the velocities in spos' order; the sampler (vel or rho may be nullptr; grid6
// and bricks as wsk_field_sample) and the tracer march (pts: m points in, their final positions out)
void wsk_field_split(hipStream_t s, const float *pv, float *pos, float *vel, uint32_t n);
void wsk_field_gather_vel(hipStream_t s, const uint32_t *perm, const float *vxyz, float4 *svel, uint32_t n);
void wsk_velocity_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                         const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks, float *vel,
                         float *rho);
void wsk_advect(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                float *pts, uint32_t m, float dt, uint32_t substeps, float *vel, float *rho);
// whitewater (ws_read_whitewater / ws_emit_whitewater / ws_step_whitewater) over the velocity field's binning: the stage
// (pass A into snrm, in spos' order; pass B by id), the emission counts by id and -- after a wsk_scan of them -- the
// spawns (outputs may be nullptr), and one step of m diffuse particles in place (pts, vel, life; cls = m bytes)
struct WsWhiteEmit {
    float tt0, tt1, tc0, tc1, te0, te1, kt, kc, align, dt, radius, l0, l1;
    uint32_t maxpp, seed;
};
struct WsWhiteStep {
    float dt;
    uint32_t spray_max, bubble_min;
    float buoyancy, drag;
};
void wsk_whitewater_stage(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel,
                          float4 *snrm, float *trapped, float *crest, float *align, float *energy, float *normal, uint32_t *nb,
                          uint32_t n);
void wsk_whitewater_count(hipStream_t s, const WsWhiteEmit &e, const float *vxyz, const float *trapped, const float *crest,
                          const float *align, const float *energy, uint32_t *cnt, uint32_t n);
void wsk_whitewater_spawn(hipStream_t s, const WsWhiteEmit &e, const float *pxyz, const float *vxyz, const uint32_t *cnt,
                          const uint32_t *off, float *out_xyz, float *out_vel, float *out_life, uint32_t *out_src, uint32_t n);
void wsk_whitewater_step(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                         const WsWhiteStep &sp, float *pts, float *vel, float *life, uint8_t *cls, uint32_t m);
// surface tension and XSPH (ws_read_cohesion / ws_apply_cohesion) over the velocity field's binning: the call's strengths,
// rho_0, dt and the two spline constants of the header (kc, h664), and the stage -- pass A into snd ({normal, density} in
// spos' order), pass B by id into dvc ({dv, count}) and, unless nullptr, nrho ({normal, density}); wsk_cohesion_unpack:
// the two as the four output arrays of ws_read_cohesion.  wsk_state_split: the gathered state records of slab handles as
// positions and velocities by id.
struct WsCohesion {
    float cohesion, curvature, xsph, rho0, dt, kc, h664;
};
void wsk_cohesion_stage(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel,
                        float4 *snd, const WsCohesion &k, float4 *dvc, float4 *nrho, uint32_t n);
void wsk_cohesion_unpack(hipStream_t s, const float4 *dvc, const float4 *nrho, float *normal, float *rho, float *dv, uint32_t *nb,
                         uint32_t n);
void wsk_state_split(hipStream_t s, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n, size_t stride_words,
                     uint32_t n_global, float *pos, float *vel);
// per-particle attributes (ws_paint_attributes / ws_diffuse_attributes / ws_sample_attribute_*).  attr: one float4 per
// particle BY ID (ws_handle::attr).  Paint: the brushes by value, as the emitters; painted = k device words the kernel
// adds the per-brush counts to, or nullptr; xyz = the positions by id.  Diffusion over the sampler's binning: the gather
// of attr into spos' order and the scatter back, pass A (srho: the IEEE densities in spos' order) and one iteration of
// pass B from sa into out (both in spos' order; r4 = fl(rate * dt) per channel; affected = WS_COHESION_SLOTS partial
// counts as WsCohesionArgs', or nullptr).  The field: wsk_velocity_sample with sa (spos' order) in place of svel and four
// values per query (value or rho may be nullptr).
struct WsBrushSet {
    ws_brush e[WS_MAX_BRUSHES];
};
struct WsBrushArgs {
    WsBrushSet bs;
    uint32_t k;
    uint32_t *painted;
};
// count changes (ws_remove_particles / ws_remove_particle_ids / ws_add_particles; ws_population.hip).  map: one word per
// particle id.  Mark: the sinks by value, as the emitters (removed = WS_MAX_SINKS device words the kernel adds the
// per-sink claims to), or a map filled with 1 and the named ids cleared.  wsk_pop_scan: map[id] = rank among the survivors
// << 1 | stays, through wsk_pop_tiles(n) words of sums; *total = the survivors.  Compact: the surviving 32-byte records of
// src to slot `new id` of dst, the attributes by id likewise; wsk_pop_new_ids: the host's id map.  Append: m staged
// particles at the slots and ids n0 .. (vel / attr_in / attr may be nullptr).
struct WsSinkSet {
    ws_sink e[WS_MAX_SINKS];
};
struct WsSinkArgs {
    WsSinkSet ss;
    uint32_t k;
    uint32_t *removed;
};
uint32_t wsk_pop_tiles(uint32_t n);
void wsk_pop_mark_sinks(hipStream_t s, WsSoA cur, uint32_t n, const WsSinkArgs &a, uint32_t *map);
void wsk_pop_clear_ids(hipStream_t s, const uint32_t *ids, uint32_t m, uint32_t *map);
void wsk_pop_scan(hipStream_t s, uint32_t *map, uint32_t n, uint32_t *sums, uint32_t *total);
void wsk_pop_compact(hipStream_t s, const float4 *src, uint32_t n, const uint32_t *map, float4 *dst);
void wsk_pop_compact_attr(hipStream_t s, const float4 *attr, uint32_t n, const uint32_t *map, float4 *out);
void wsk_pop_new_ids(hipStream_t s, const uint32_t *map, uint32_t n, uint32_t *out);
void wsk_pop_append(hipStream_t s, const float *pos, const float *vel, const float4 *attr_in, uint32_t m, uint32_t n0, WsSoA cur,
                    float4 *attr);
// gauges (ws_measure / ws_select_particles; ws_gauges.hip).  The regions by value, as the sinks.  Measure: the records of a
// single handle's `cur` (pv) or, posvel != nullptr, a slab's gathered {position, velocity} by id (6 floats; the id is the
// index); attr != nullptr: the attributes by id are summed too.  out: WS_MAX_REGIONS x WS_GAUGE_SUMS 64-bit words {count,
// the 14 fixed-point sums in ws_gauge's order}, then WS_MAX_REGIONS x WS_GAUGE_KEYS 32-bit keys {min_pos[3], max_pos[3],
// max_speed2} of the extremes' total order (WS_GAUGE_OUT_BYTES in all); the launcher sets the identities first, on s.
// Select: map[id] = 1 if any region contains the particle, else 0 (then wsk_pop_scan), and the first cap selected ids in
// ascending order to out.
#define WS_GAUGE_SUMS 15u
#define WS_GAUGE_KEYS 7u
#define WS_GAUGE_OUT_BYTES (WS_MAX_REGIONS * (WS_GAUGE_SUMS * 8u + WS_GAUGE_KEYS * 4u))
struct WsRegionSet {
    ws_region e[WS_MAX_REGIONS];
};
void wsk_gauge_measure(hipStream_t s, const float4 *pv, const float *posvel, const float4 *attr, uint32_t n, const WsRegionSet &rs,
                       uint32_t k, unsigned long long *out);
void wsk_gauge_mark(hipStream_t s, WsSoA cur, uint32_t n, const WsRegionSet &rs, uint32_t k, uint32_t *map);
void wsk_gauge_list(hipStream_t s, const uint32_t *map, uint32_t n, uint32_t cap, uint32_t *out);
void wsk_attr_paint(hipStream_t s, const WsBrushArgs &a, const float *xyz, float4 *attr, uint32_t n);
void wsk_attr_gather(hipStream_t s, const float4 *spos, const float4 *attr, float4 *sa, uint32_t n);
void wsk_attr_scatter(hipStream_t s, const float4 *spos, const float4 *sa, float4 *attr, uint32_t n);
void wsk_attr_density(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, float *srho, uint32_t n);
void wsk_attr_diffuse(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float *srho, const float4 *sa,
                      const float *r4, float4 *out, uint32_t *affected, uint32_t n);
void wsk_attr_sample(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *sa, bool ieee,
                     const float *xyz, uint32_t m, const float *grid6, const uint32_t *dims, bool bricks, float4 *value, float *rho);
// bodies (ws_body_forces) over the velocity field's binning.  chunks: nchunks x {body, first sample, samples (1 .. the
// workgroup size), 0}, a body's chunks consecutive and in order; cstart: the first chunk of every body, nb + 1 entries;
// part: 8 words per chunk (written, then read by the finishing kernel).  One workgroup per chunk sweeps the field at the
// chunk's samples, stores the per-sample results (sforce, sfrac: either may be nullptr) and its node of the body's
// summation tree; then one wave per body finishes the tree into force, torque, volume and wet (any may be nullptr; all:
// no finishing launch).  rho0 is the density a sample counts as fully submerged at.
struct WsBodyParams {
    float fluid_density, drag, rho0;
};
uint32_t wsk_body_chunk(void);  // samples per chunk
void wsk_body_forces(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *svel, bool ieee,
                     const WsBodyParams &bp, const uint32_t *chunks, uint32_t nchunks, const uint32_t *cstart, uint32_t nb,
                     const float *xyz, const float *vel, const float *vol, const float *centre, float *part, float *sforce,
                     float *sfrac, float *force, float *torque, float *volume, uint32_t *wet);
// anisotropic kernels (ws_read_anisotropy / ws_sample_aniso_* / ws_extract_aniso_surface): the per-particle stage over
// the sampler's binning of the positions (by id: centres, ellipsoids as 2 float4, neighbour counts), then the records
// of the centres in their own cell order
struct WsAnisoParams {
    float lambda, kr, kn;
    uint32_t neps;
};
void wsk_aniso(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, WsAnisoParams ap, float *cxyz,
               float4 *mf, uint32_t *nb, uint32_t n);
void wsk_aniso_gather(hipStream_t s, const uint32_t *perm, const float *cxyz, const float4 *mf, float4 *srec, float4 *smf,
                      uint32_t n);
// rays (ws_cast_rays / ws_cast_camera): one lane per ray -- the m rays of origin / dir, or with cam the pixels of a
// size[0] x size[1] image.  spos / smf as wsk_field_sample; out_t or out_n may be nullptr.
void wsk_ray_cast(hipStream_t s, const WsDev &d, const uint32_t *start, const float4 *spos, const float4 *smf,
                  bool ieee, const ws_ray_params &r, const float *origin, const float *dir, uint32_t m,
                  const ws_camera *cam, const uint32_t *size, float *out_t, float *out_n);
// surface extraction (ws_extract_surface) on a sampled grid: node codes and per-workgroup totals (wsk_iso_blocks() of
// them, then one 0 each), then -- after two wsk_scan launches over blocks + 1 totals -- vertices and triangles
uint32_t wsk_iso_blocks(const uint32_t *dims);
void wsk_iso_totals(hipStream_t s, const uint32_t *v_total, const uint32_t *t_total, uint32_t *out);  // out[0..1]
void wsk_iso_count(hipStream_t s, const float *rho, const float *grid6, const uint32_t *dims, float iso, uint8_t *code,
                   uint32_t *vcnt, uint32_t *tcnt);
void wsk_iso_mesh(hipStream_t s, const float *rho, const float *grad, const float *grid6, const uint32_t *dims, float iso,
                  const uint8_t *code, const uint32_t *vstart, const uint32_t *tstart, uint32_t *vbase, float *xyz,
                  float *nrm, uint32_t *tri);
// slabs
void wsk_migrate_mark(hipStream_t s, const WsDev &d, WsSoA cur, uint32_t *cid_cur, uint32_t *count);
void wsk_migrate_fill(hipStream_t s, const WsDev &d, uint32_t world, uint32_t me, uint32_t cap, uint32_t *dyn,
                      const uint32_t *hole, const uint32_t *recvL, const uint32_t *recvR, uint32_t mig_cap,
                      const uint32_t *far_all, uint32_t far_cap, uint32_t *tgt, uint32_t *src, WsSoA cur, uint32_t *cid_cur,
                      uint32_t *count, uint32_t *status_ring, uint32_t status_slots, uint32_t hole_cap, uint32_t *sendL,
                      uint32_t *sendR, uint32_t *far_send, uint32_t far_next, uint64_t leave_bound);
void wsk_far_seal(hipStream_t s, uint32_t world, uint32_t far_cur, uint32_t *far_send, uint32_t *dyn);
void wsk_sizes(hipStream_t s, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *dyn, uint32_t *out);
void wsk_far_pack(hipStream_t s, uint32_t world, uint32_t far_cap, uint32_t far_n, const uint32_t *src, uint32_t *dst);
void wsk_halo_pack(hipStream_t s, const WsDev &d, const uint32_t *start, WsSorted srt, uint32_t *dyn, uint32_t rowy,
                   uint32_t halo_cap, uint32_t *sendL, uint32_t *sendR, bool densities);
void wsk_halo_unpack(hipStream_t s, const WsDev &d, uint32_t *start, WsSorted srt, WsXYZ sxyz, uint32_t *dyn, uint32_t rowy,
                     uint32_t nxl, uint32_t ghost_cap, const uint32_t *recvL, const uint32_t *recvR, bool densities);
void wsk_gather_slab(hipStream_t s, const WsDev &d, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                     const WsPressureParams &pp, ws_particle80 *out, uint32_t *ids);
void wsk_upload_positions_ids(hipStream_t s, const float *xyz_dev, const uint32_t *ids_dev, WsSoA cur, uint32_t n);
// id-ordered global views / loads of slab handles (ws_views.hip "slab handles: the id-ordered GLOBAL views")
enum { WS_PACK_POS_H = 0, WS_PACK_SPEED_H = 1, WS_PACK_RECORD_H = 2, WS_PACK_STATE_H = 3, WS_PACK_KEY_H = 4, WS_PACK_POSVEL_H = 5 };
uint32_t wsk_pack_words(int kind);  // payload words per record (the record carries one more: the particle id)
void wsk_slab_pack(hipStream_t s, const WsDev &d, int kind, WsSoA cur, WsSorted srt, const float4 *accel, bool have_step,
                   const WsPressureParams &pp, uint32_t *out);
void wsk_slab_unpack_by_id(hipStream_t s, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                           size_t stride_words, uint32_t pw, uint32_t n_global, uint32_t *out);
void wsk_slab_layer_hist(hipStream_t s, const WsDev &d, const uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                         size_t stride_words, uint32_t *hist);
void wsk_slab_select(hipStream_t s, const WsDev &d, int src, const uint32_t *cuts, uint32_t world, uint32_t me,
                     const void *chunk, uint32_t id0, uint32_t m, const uint32_t *cnt, size_t stride_words, WsSoA cur,
                     uint32_t cap, uint32_t *dyn);
