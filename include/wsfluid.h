/*
 * wsfluid.h -- C ABI of the MI355X-native SPH fluid step (libwsfluid.so).
 *
 * This is the drop-in boundary for the one hot path of qts8n/water-sandbox: the
 * per-frame SPH step that the reference builds in src/fluid_compute.rs and runs as
 * assets/simulation.wgsl + assets/bitonic_sort.wgsl through bevy_app_compute's
 * AppComputeWorker.  Each entry point names the reference interface it replaces
 * (paths relative to the reference tree).  The reference-side binding (the Rust
 * `extern "C"` block and the Bevy systems that call it) is in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; the library owns all device memory;
 * the caller owns every pointer it passes and the library never keeps one after the
 * call returns; every function returns a ws_status (0 = ok) and never throws or
 * aborts; a handle is not re-entrant (calls on one handle must be serialised by the
 * caller -- Bevy's ResMut does this) but may be used from any host thread.
 * There is NO CPU fallback: without a gfx950 device ws_create fails with
 * WS_ERR_NO_DEVICE.
 */
#ifndef WSFLUID_H
#define WSFLUID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): ws_transport starts with struct_size and has four callbacks; flags 64 / 128 / 256 have meanings; ws_read_stats out[5..14] are assigned.  A host built against
 * version 1 must not pass its structs to this library: compare ws_abi_version() with WS_ABI_VERSION at start-up. */
#define WS_ABI_VERSION 2

typedef enum ws_status {
    WS_OK = 0,
    WS_ERR_INVALID_ARG = 1,   /* null pointer, n == 0, non-finite / non-positive h, empty box */
    WS_ERR_NO_DEVICE = 2,     /* no HIP device / not gfx950 / bad device index */
    WS_ERR_OUT_OF_MEMORY = 3, /* hipMalloc failed or the cell grid would not fit */
    WS_ERR_HIP = 4,           /* any other HIP runtime error (text in ws_last_error) */
    WS_ERR_COMM = 5,          /* RCCL error in the multi-GPU halo exchange */
    WS_ERR_UNSUPPORTED = 6,   /* e.g. WS_FLAG_REFERENCE_ORDER on the product library, ws_create with world_size > 1 */
    WS_ERR_NOT_READY = 7      /* ws_try_* variants only */
} ws_status;

/*
 * Everything the reference uploads as uniforms, in one POD.
 *   fields 0..6   FluidStaticProps        src/fluid_compute.rs:41-51 (defaults :20-27,:67-79)
 *   gravity       Gravity.value           src/gravity.rs:9-13 (default (0,-9.8,0,0) :29-33)
 *   ext_min/max   FluidContainerExt       src/fluid_container.rs:17-22, from get_ext(0.1) :42-50
 * The five SmoothingKernel constants (src/fluid_compute.rs:30-38) are NOT passed in:
 * the library derives them exactly as get_smoothing_kernel does (:55-63) whenever
 * smoothing_radius is set, which is what update() does every frame (:480).
 */
typedef struct ws_params {
    float delta_time;
    float collision_damping;
    float smoothing_radius;
    float target_density;
    float pressure_scalar;
    float near_pressure_scalar;
    float viscosity_strength;
    float reserved0; /* must be 0 */
    float gravity[4];
    float ext_min[4];
    float ext_max[4];
} ws_params;

/* SmoothingKernel, src/fluid_compute.rs:30-38 */
typedef struct ws_smoothing_kernel {
    float pow2;
    float pow2_der;
    float pow3;
    float pow3_der;
    float spikey_pow3;
} ws_smoothing_kernel;

/* FluidParticle, src/fluid_compute.rs:106-115 == assets/simulation.wgsl:69-76.
 * 80 bytes, same field order and offsets, so a Rust Vec<FluidParticle> can be
 * passed straight in and out. */
typedef struct ws_particle80 {
    float position[4];
    float density[2];
    float pressure[2];
    float velocity[4];
    float acceleration[4];
    float predicted_position[4];
} ws_particle80;

/* Placement of this handle's share of the domain.  Zero-initialise for one GPU. */
typedef struct ws_device_cfg {
    int32_t device;          /* HIP device ordinal */
    uint32_t flags;          /* WS_FLAG_* */
    uint32_t rank;           /* slab index along x, 0-based (0 for one GPU) */
    uint32_t world_size;     /* number of slabs (0 or 1 = single GPU) */
    uint32_t capacity;       /* slabs: max particles this handle may own (0 = 2 n_local + 2^20);
                                head-room for particles migrating in */
    uint32_t ghost_capacity; /* slabs: max particles of ONE boundary layer = ghosts per face = the capacity of a halo
                                message (0 = 16 n_global / nx + 2^15, nx = cell layers along x: sixteen times an evenly
                                spread layer; what travels per step is sized by the layer's actual population) */
    uint32_t reserved[2];
    void *stream;            /* hipStream_t to enqueue on, or NULL: the library creates its own.
                                A host that moves halos with its own communication library passes
                                that library's stream here so both are ordered on it. */
} ws_device_cfg;

#define WS_FLAG_NONE 0u
#define WS_FLAG_PROFILE 1u /* record HIP events around every kernel of ws_step */
/* Validation mode: execute the reference's six passes literally on the GPU -- N-bucket hashed table,
 * the bitonic network stage by stage on the persisted permutation (src/fluid_compute.rs:256-271,
 * assets/bitonic_sort.wgsl:22-46), atomicMin cell offsets, bucket walks in OFFSET_TABLE order -- with
 * the same IEEE arithmetic.  It reproduces the reference's summation order, so it is comparable with
 * a bit-faithful CPU restatement on every float and on particle_indicies itself.  Slow (S dispatches
 * per step); single GPU only; never the benchmarked path. */
#define WS_FLAG_REFERENCE_ORDER 2u
/* Pair terms of K4/K5 with correctly rounded sqrt and division (the CPU oracle's arithmetic) instead of the
 * default hardware v_sqrt_f32 / v_rcp_f32 forms (1 ULP each; x / y evaluated as x * rcp(y)), which stay inside the
 * accuracy WGSL grants the reference's own GPU execution (x / y: 2.5 ULP).  ~2x slower density/force kernels. */
#define WS_FLAG_IEEE_DIVISION 4u
/* Replay the step from a captured hipGraph instead of launching its kernels one by one: what the reference does with
 * its pass graph (built once in FluidWorker::build, replayed by AppComputeWorker::run every frame,
 * src/fluid_compute.rs:309-363,:396).  The step is captured on the first steady-state ws_step (and again when a slab's
 * launch bound moves by more than 65 536 particles); results are identical to direct launches.  On slab handles the
 * flag is honoured with the library's own RCCL transport (and for a world of one); a host-supplied transport may
 * synchronise the stream inside its callbacks, so such handles keep launching directly.  Ignores WS_FLAG_PROFILE.  Off by default: direct launches already pipeline on the
 * stream and measure as fast on one MI355X. */
#define WS_FLAG_GRAPH 8u
/* Slab handles, how the messages of a step are sized.
 * DEFAULT (neither flag, no WS_FLAG_GRAPH): every message carries exactly what its sender has for it.  ws_step gathers
 * four words per rank and waits for them twice per step -- before the migration (the GPU idles for one small all-gather
 * and a copy) and before the halos (behind the kernel that needs no ghosts).  Nothing can overrun below the buffers'
 * capacities, and the messages are as small as they can be.
 * WS_FLAG_LAGGED_MESSAGES (implied by WS_FLAG_GRAPH: a captured step has its sizes baked in): ws_step never waits for
 * the device; every rank derives the sizes from the demand all ranks reported a few steps earlier (x 4 headroom on the
 * largest of the last eight reports).  A demand that outgrows that within four steps FAILS the run -- on every rank at the
 * same step, cleanly, but it fails: a pressure front that crosses a slab face broadside multiplies the particles changing
 * owner tenfold in one step.  For flows known to be smooth across the slab faces -- the benchmark
 * trajectories are.
 * WS_FLAG_FIXED_MESSAGES: every message travels at its full CAPACITY.  ws_step never waits, nothing below the
 * capacities can overrun, the sizes never change (so a captured step is never re-captured) -- and every link moves the
 * capacity every step (DESIGN.md 6 has the bytes).  This is what WS_FLAG_GRAPH uses on a handle with peers unless
 * WS_FLAG_LAGGED_MESSAGES is given with it: a captured multi-rank step is safe by default, the bet is the opt-in.
 * WS_FLAG_EXACT_MESSAGES asks for the default explicitly (and wins over WS_FLAG_GRAPH, which is then ignored).
 * Every rank must choose alike: ws_slab_create compares the ranks' choices and fails on ALL of them
 * (WS_ERR_INVALID_ARG) when they differ. */
#define WS_FLAG_EXACT_MESSAGES 16u
#define WS_FLAG_LAGGED_MESSAGES 32u
#define WS_FLAG_FIXED_MESSAGES 64u
/* Slab handles: keep the halo exchanges on the step's own stream (no early / late split of K4 / K5, no second
 * communicator).  Same results; for transports that cannot drive two streams, and for A/B runs.  Every rank alike. */
#define WS_FLAG_NO_OVERLAP 128u
/* Slab handles with peers: let WS_FLAG_GRAPH capture the step although no run on two or more GPUs has executed a
 * captured transport call yet (the path runs through the tests' stand-in for librccl only: DESIGN.md 6).  Needs the
 * library's own RCCL transport with two communicators.  Without it a multi-rank handle launches directly.  Every rank
 * alike. */
#define WS_FLAG_GRAPH_MULTIRANK 256u

typedef struct ws_handle ws_handle;

/* ---- host-side functions of the path (pure CPU, no device needed) ----------- */

/* FluidStaticProps::default + Gravity::default + FluidContainer::default().get_ext(0.1)
 * (src/fluid_compute.rs:67-79, src/gravity.rs:29-33, src/fluid_container.rs:8-9,34-40). */
ws_status ws_default_params(ws_params *out);
/* FluidStaticProps::get_smoothing_kernel, src/fluid_compute.rs:55-63. */
ws_status ws_get_smoothing_kernel(const ws_params *p, ws_smoothing_kernel *out);
/* helpers::cube_fluid, src/helpers.rs:3-20. out_xyz holds ni*nj*nk*3 floats. */
ws_status ws_cube_fluid(uint32_t ni, uint32_t nj, uint32_t nk, float particle_rad, float *out_xyz);
/* FluidContainer::get_ext, src/fluid_container.rs:42-50. */
ws_status ws_get_ext(const float position[3], const float size[3], float padding,
                     float ext_min[4], float ext_max[4]);
/* FluidWorker::get_bit_sorter_stages count, src/fluid_compute.rs:251-273.  The HIP
 * path does not run the network; exposed because the reference prints it (:321). */
uint32_t ws_bit_sorter_stage_count(uint32_t data_length);
const char *ws_status_string(ws_status s);
uint32_t ws_abi_version(void);

/* ---- lifetime: replaces FluidWorker::build + AppComputeWorkerBuilder --------- */

/* src/fluid_compute.rs:277-366.  pos_xyz: n*3 floats, particle id = index (the id
 * FluidParticleLabel carries, :416-417,:459).  Uploads the particles with
 * position = predicted_position = point and everything else 0 (:118-130), identity
 * permutation (:293).  cfg may be NULL (device 0, single GPU). */
ws_status ws_create(const ws_params *params, const float *pos_xyz, uint32_t n,
                    const ws_device_cfg *cfg, ws_handle **out);
ws_status ws_destroy(ws_handle *h);

/* ---- per frame ---------------------------------------------------------------- */

/* AppComputeWorker::run in ShaderPhysicsSet::Pass (src/fluid_compute.rs:396): enqueue
 * one full step hash -> sort -> cell starts -> density -> force -> integrate
 * (pass order :309-363) on the handle's stream and return without waiting. */
ws_status ws_step(ws_handle *h);
/* AppComputeWorker::ready (src/fluid_compute.rs:474,:511): *ready = 1 when every
 * enqueued step has finished, else 0.  Never blocks. */
ws_status ws_ready(ws_handle *h, int *ready);
/* Block until every enqueued step has finished (the reference has no equivalent; its
 * host simply skips the frame while !ready()). */
ws_status ws_sync(ws_handle *h);
/* The three worker.write calls of update() (src/fluid_compute.rs:479-481):
 * fluid_props, smoothing_kernel (re-derived here) and gravity; the container is
 * taken too (the reference uploads it once, :302).  Takes effect at the next ws_step.
 * Errors: WS_ERR_INVALID_ARG / WS_ERR_OUT_OF_MEMORY from the checks made BEFORE anything is touched (a radius <= 0, a
 * grid beyond the cell budget, on slab handles a slab whose share of the fluid on the new grid exceeds its capacity --
 * decided from the gathered state for every rank alike): the handle keeps its previous parameters and goes on.  A new
 * smoothing radius or container rebuilds the cell tables; an allocation that fails AFTER the old ones were given up
 * leaves the handle dead -- every later ws_step returns WS_ERR_HIP with the reason -- never half-built tables under
 * a handle that still steps. */
ws_status ws_set_params(ws_handle *h, const ws_params *params);
/* worker.read_vec::<FluidParticle>("particles") followed by `.position.xyz()` per
 * label (src/fluid_compute.rs:478,:483-485): n*3 floats in ORIGINAL-ID order.
 * Waits for enqueued steps first. */
ws_status ws_read_positions(ws_handle *h, float *out_xyz);
/* The same readback split in two for a frame loop that overlaps it with the next step (SURVEY 8(b) "pipelining
 * contract"): _begin captures the positions as of the steps enqueued so far and starts the copy into out_xyz
 * (page-lock it: ws_pin_host_buffer) on a separate stream and returns; ws_step calls made after it run while
 * the copy is in flight; _end waits for the copy.  One readback in flight per handle; out_xyz must stay valid
 * until _end. */
ws_status ws_read_positions_begin(ws_handle *h, float *out_xyz);
ws_status ws_read_positions_end(ws_handle *h);
/* out_xyz == NULL in ws_read_positions_begin: the copy goes into one of TWO page-locked buffers the library owns
 * (SURVEY 8(b) "Ownership": the library owns all pinned staging), filled alternately; after _end,
 * ws_read_positions_view hands out the buffer the last finished readback filled.  It stays untouched until the
 * second-next _begin(h, NULL), so update() can still scatter frame k's positions into its Transforms
 * (src/fluid_compute.rs:483-485) while frame k+1's copy is in flight.  The copy runs on an SDMA engine, on a stream
 * of a priority of its own (it never shares a hardware queue with the step's stream). */
ws_status ws_read_positions_view(ws_handle *h, const float **out_xyz);
/* `velocities.length()` per particle in ORIGINAL-ID order: n floats -- what the reference's (commented-out)
 * speed colouring system reads back 80 B per particle for (src/fluid_compute.rs:489-502).  Waits for
 * enqueued steps first. */
ws_status ws_read_speeds(ws_handle *h, float *out_speed);
/* Optional: page-lock a host buffer the caller owns and keeps alive -- typically the position buffer
 * update() fills every frame -- so that ws_read_positions / ws_read_particles into it run at PCIe rate
 * (no pageable staging).  The caller must ws_unpin_host_buffer it before freeing it. */
ws_status ws_pin_host_buffer(ws_handle *h, void *ptr, uint64_t bytes);
ws_status ws_unpin_host_buffer(ws_handle *h, void *ptr);
/* The full read_vec view (src/fluid_compute.rs:478): n records of 80 bytes in
 * original-id order.  density/pressure/acceleration are the values the last step
 * computed (0 before the first step).  The step itself keeps positions and velocities only: the acceleration
 * field (read by nothing in the reference but this view) is produced here by one more pass of the force kernel over
 * the state the last step left behind -- the same bits the step used; a frame loop that reads positions pays
 * nothing for it. */
ws_status ws_read_particles(ws_handle *h, ws_particle80 *out);
/* despawn_liquid's four write_slice calls (src/fluid_compute.rs:517-524): particles
 * <- initial state from pos_xyz, index buffers <- identity. */
ws_status ws_reset(ws_handle *h, const float *pos_xyz);
/* worker.write_slice("particles", ..) with an arbitrary state (position, velocity,
 * predicted_position are taken; the other fields are recomputed by the next step
 * before they are read, as in the reference).  Checkpoint/restore and the tests'
 * teacher forcing use this. */
ws_status ws_write_particles(ws_handle *h, const ws_particle80 *in);

/* ---- the per-frame calls above on a SLAB handle (multi-GPU, below) ---------------------------------------------
 * ws_read_positions / _begin / _end, ws_read_speeds, ws_read_velocities, ws_read_particles, ws_read_sort_view, ws_reset,
 * ws_write_particles
 * and a ws_set_params that changes the smoothing radius or the container work on slab handles too, over GLOBAL,
 * id-ordered arrays (n_global entries), as COLLECTIVE calls: every rank makes the same call at the same point of its
 * frame, as the ranks of a multi-GPU host do anyway.
 *   reads:   every rank receives the whole array (the owned records of all slabs are all-gathered and scattered by id
 *            on the device); a rank that does not need it passes NULL and only contributes.
 *   loads:   every rank passes the SAME global array (what FluidParticlesInitial holds, src/fluid_compute.rs:82-85) and
 *            keeps the particles its cuts own; no data moves between ranks.  Sticky errors are cleared.
 *   re-grid: the particles are redistributed by the new cuts (any particle may change owner).
 * ws_num_particles stays the number of particles THIS slab owns. */

/* ---- multi-GPU: one handle = one x-slab of the domain, one process per GPU ------------------
 *
 * The domain is cut into world_size slabs along x on cell boundaries (x is the slowest axis of the
 * cell grid, so a slab is a contiguous range of the global cell order and its boundary layers are
 * contiguous particle ranges).  Interactions reach one cell, so a slab needs one ghost layer from
 * each x-neighbour.  ws_step on a slab handle enqueues, per step:
 *   hand particles whose predicted position left the slab to their new owner (migration: one send/recv with each
 *   neighbour, plus one all-to-all for the particles that cross several slabs in a step and for the status words) -> sort own
 *   particles -> send the two boundary layers' records to the neighbours (halo A) -> K4 -> send their densities
 *   (halo B) -> K5+K6; with the halos on a second stream while the particles that need no ghosts compute.
 * ws_step never waits for the END of the step it enqueues on a slab handle either: every message has a fixed capacity known
 * to both ends (ghost_capacity and sizes derived from it) and carries its record count in a header; the owned count, the
 * layer ranges and the ghost counts stay on the device.  By default it waits, twice per step, for four words per rank --
 * the record counts its messages are sized from (WS_FLAG_EXACT_MESSAGES, above); the rest of the step -- the late
 * kernels, the second halo, the force kernel -- is still running when it returns.  With WS_FLAG_LAGGED_MESSAGES it
 * waits for nothing of the step at all (only, a bounded run-ahead, for the status table of the step enqueued two
 * calls earlier) and launches its kernels over host-side upper bounds.  A capacity
 * overrun clamps, sets a sticky error bit that reaches every rank with the next step's all-to-all, and makes ws_step
 * return WS_ERR_OUT_OF_MEMORY on ALL ranks at the same step (two steps later), before any collective of that step --
 * no rank is left waiting in one.  ws_sync / ws_slab_read_particles / ws_slab_counters report the bits too, as soon
 * as this rank knows them -- which may be one or two steps before the other ranks do: such a report is information,
 * not the signal to stop; keep calling ws_step until IT fails (it does on every rank at the same step, and until
 * then it keeps issuing the step's collectives so that no peer waits alone).  ws_num_particles of a slab is exact
 * after ws_sync.
 * All data movement goes through the three transport callbacks below (bench.py uses the library's own RCCL
 * transport, ws_rccl_transport_create; tests also drive them with torch.distributed and with an in-process
 * loopback).  The particle order inside a cell is canonical (by id), so an N-slab run reproduces the single-GPU
 * run bit for bit.  The reference has no multi-device path; this is the scale-out row of SURVEY.md 8(e). */
typedef struct ws_transport {
    uint64_t struct_size; /* sizeof(ws_transport) of the host's build: ws_slab_create refuses a table that is shorter
                             than the one it was compiled with (a version-1 host's three-callback struct) instead of
                             calling through whatever lies behind it */
    void *ctx;
    /* Stream-ordered exchange of nseg buffers with each x-neighbour, d = 0 (rank - 1) and d = 1 (rank + 1), as
     * ONE group of point-to-point transfers: for segment k send send_bytes[2k + d] bytes from DEVICE pointer
     * send_ptr[2k + d] and receive recv_bytes[2k + d] bytes into DEVICE pointer recv_ptr[2k + d].  Zero bytes =
     * no transfer.  Both sides list their segments in the same order.  Returns 0 on success. */
    int (*sendrecv)(void *ctx, uint32_t nseg, void *const send_ptr[], const uint64_t send_bytes[],
                    void *const recv_ptr[], const uint64_t recv_bytes[], void *stream);
    /* Stream-ordered all-gather of bytes_each DEVICE bytes per rank into recv_ptr[world_size * bytes_each]. */
    int (*allgather_dev)(void *ctx, const void *send_ptr, void *recv_ptr, uint64_t bytes_each, void *stream);
    /* Stream-ordered all-to-all of DEVICE buffers: bytes [r * bytes_each, (r + 1) * bytes_each) of send_ptr go to rank
     * r, which stores them at [this rank * bytes_each, ...) of its recv_ptr; the segment a rank addresses to itself is
     * copied too (RCCL: ncclAllToAll).  Once per step on the handle's stream: the per-destination messages for particles
     * that cross more than one slab in a step, each headed by the sender's status words -- so every rank also ends up
     * with every rank's status.  Required when world_size > 1. */
    int (*alltoall_dev)(void *ctx, const void *send_ptr, void *recv_ptr, uint64_t bytes_each, void *stream);
} ws_transport;

/* A ws_transport implemented inside the library with RCCL (ncclSend / ncclRecv groups with the two x-neighbours,
 * ncclAllToAll for the far messages and the status words, ncclAllGather for the host's collective reads), for hosts
 * that have no communication layer of their own.  librccl is loaded at run time.  Rank 0 draws a unique id and the host hands its 128 bytes to every rank (any out-of-band channel);
 * every rank then creates its transport -- a collective call -- on the device its slab will live on.  The
 * transport must outlive the slab handle created with it. */
#define WS_RCCL_UNIQUE_ID_BYTES 128
ws_status ws_rccl_unique_id(void *out128);
ws_status ws_rccl_transport_create(const void *unique_id, uint32_t rank, uint32_t world_size, int32_t device,
                                   ws_transport *out);
void ws_rccl_transport_destroy(ws_transport *t);
const char *ws_rccl_last_error(void);
/* Communicators the transport drives: 2 = the step's two streams (migration / all-to-all on the handle's stream, halos on
 * its communication stream) each keep to a communicator of their own (the second one is split off the first), so no
 * communicator ever sees operations from two streams; 1 = an RCCL without ncclCommSplit (or the developer build's WS_RCCL_SINGLE_COMM=1 hook). */
uint32_t ws_rccl_transport_communicators(const ws_transport *t);

/* A ws_transport for several slabs inside ONE process, one host thread per slab (one GPU or several): plain
 * device-to-device copies between the slabs' message buffers with a host rendezvous.  For hosts that drive all their GPUs
 * from one process, and for exercising the whole slab protocol on a one-GPU box (host/frame_loop.cpp, tests).  Every
 * call synchronises its stream: correct, not fast, and not capturable (WS_FLAG_GRAPH falls back to direct launches).  A
 * rank that is left alone in a collective for 300 s breaks the hub (every call then fails) instead of hanging.  The hub
 * must outlive its transports, a transport the handle created with it. */
ws_status ws_local_hub_create(uint32_t world_size, void **hub_out);
void ws_local_hub_destroy(void *hub);
ws_status ws_local_transport_create(void *hub, uint32_t rank, ws_transport *out);
void ws_local_transport_destroy(ws_transport *t);

/* Host-only: which slab owns each position (by the x cell of floor(x / h) in the global grid, equal
 * cell-count cuts S_r = r * nx / world_size).  out_rank holds n entries. */
ws_status ws_slab_assign(const ws_params *params, const float *pos_xyz, uint32_t n, uint32_t world_size,
                         uint32_t *out_rank);
/* Create the slab cfg->rank of cfg->world_size.  pos_xyz / ids: the n_local particles this slab owns at
 * t = 0 (as ws_slab_assign says) and their global ids; n_global: the reference's num_particles.  The
 * transport struct is copied; its ctx must outlive the handle. */
ws_status ws_slab_create(const ws_params *params, const float *pos_xyz, const uint32_t *ids, uint32_t n_local,
                         uint32_t n_global, const ws_device_cfg *cfg, const ws_transport *transport, ws_handle **out);
/* The particles this slab owns now (count varies with migration): up to cap records and their global
 * ids, in no particular order; *n_out = number owned.  Waits for enqueued steps. */
ws_status ws_slab_read_particles(ws_handle *h, ws_particle80 *out, uint32_t *out_ids, uint32_t cap, uint32_t *n_out);
/* COLLECTIVE re-cut: move the slab boundaries so that every slab owns about n_global / world_size particles again (cuts
 * stay on cell-layer boundaries; every slab keeps at least one layer).  ws_slab_assign's cuts give every slab the same
 * number of cell LAYERS, which is balanced while the fluid is spread evenly along x; a gravity with an x component
 * (the HUD can set any, src/hud.rs:151-162) piles it up at one end until that slab's capacity overruns.  A host that sees
 * the owned counts drift apart (ws_slab_counters / ws_num_particles) calls this on every rank at the same point; the
 * particles are redistributed like on a re-grid and the run continues bit-identically to a single handle.  Cheap
 * when nothing needs to move (one gather; every rank decides alike). */
ws_status ws_slab_rebalance(ws_handle *h);
/* (After a re-cut, a later ws_set_params that rebuilds the grid re-applies the equal-COUNT rule on the new grid instead of
 * falling back to equal layers.  After any load of a slab handle -- ws_reset, ws_write_particles, a re-grid, a re-cut --
 * the 80-byte record view reports zero density / pressure / acceleration until the next ws_step, as a freshly created
 * handle does; a single-GPU handle keeps the last step's values over a re-grid.) */
/* Host-only: the cuts ws_slab_rebalance chooses for an x-layer histogram (hist[nx] particles per cell layer; cuts_out holds
 * world_size + 1 entries, cuts_out[0] = 0, cuts_out[world_size] = nx, strictly increasing). */
ws_status ws_slab_balanced_cuts(const uint32_t *hist, uint32_t nx, uint32_t world_size, uint32_t *cuts_out);
/* Migration counters of this slab since it was created (cumulative over ws_reset, ws_write_particles, a re-grid and a
 * re-cut), as of the last migration that has run (waits for enqueued steps): out[0] = particles owned now, out[1] = particles that left, out[2] = particles that arrived, out[3] = of
 * those that left, the ones that crossed more than one slab in a step (the all-to-all route).  The reference is a
 * single-GPU program and has no counterpart; diagnostics for the host and for the tests. */
ws_status ws_slab_counters(ws_handle *h, uint64_t out[4]);

/* ---- reference-layout views of the sort (diagnostic; computed on demand by HIP
 *      kernels, never inside ws_step) ---------------------------------------------
 * What the reference's three index buffers hold after the same number of steps:
 *   keys[id]    = particle_cell_indicies: hash_cell(get_cell(predicted)) % N of the
 *                 predicted position the last step STARTED from
 *                 (assets/simulation.wgsl:121-141)
 *   perm[slot]  = particle_indicies: a permutation with keys[perm] ascending.  The
 *                 reference's bitonic network is unstable, so only the key SEQUENCE
 *                 keys[perm[.]] is comparable bit for bit; this library returns the
 *                 stable order (ties by ascending particle id).
 *   offsets[k]  = cell_offsets: first slot of key k or 999999999
 *                 (assets/bitonic_sort.wgsl:48-59)
 * Before the first step all three are the identity (src/fluid_compute.rs:306-308).
 * Any of the three output pointers may be NULL. */
ws_status ws_read_sort_view(ws_handle *h, uint32_t *keys_by_id, uint32_t *perm,
                            uint32_t *cell_offsets);

/* ---- the fluid as a field (render / probe coupling; no reference counterpart) ------------------------------------
 * SURVEY 8(f) row 2, "readback / render coupling": what a renderer (raymarching, marching cubes, normals) or a probe
 * ("how much fluid is here?") needs, without reading back every position (src/fluid_compute.rs:478-485) and rebuilding
 * a neighbour search on the CPU.
 * Density field of the particles' current POSITIONS (the state the enqueued steps leave; the uploaded positions before
 * the first step), at the nodes of a regular grid:
 *   node (i, j, k) = origin + (i, j, k) * spacing, each coordinate as fl(origin[a] + fl((float)i * spacing[a]))
 *   out_density[(k * dims[1] + j) * dims[0] + i] = sum over particles p with |node - x_p| <= h of (h - d)^2 * pow2
 *   out_gradient (3 floats per node, same order; NULL = not computed) = sum of (d - h) * pow2_der * (node - x_p) / d
 *       (a particle at d == 0 contributes 0)
 * x-fastest, like a 3D texture.  Waits for enqueued steps.  Slab handles: COLLECTIVE, like ws_read_positions;
 * a rank that passes both outputs NULL only contributes.
 * The kernels are smoothing_kernel / smoothing_kernel_derivative (assets/simulation.wgsl:93-107) with the constants
 * ws_get_smoothing_kernel derives.  "|node - x_p| <= h" is the step's own test: with e = x_p - node,
 * d2 = e.x*e.x + e.y*e.y + e.z*e.z, a particle counts unless d2 > (largest f32 T with sqrtf(T) <= h), and d = sqrt(d2).
 * Arithmetic follows the handle: hardware sqrt / reciprocal by default, gradient term (node - x_p) * ((d - h) * pow2_der
 * * rcp(d)); correctly rounded with WS_FLAG_IEEE_DIVISION, ((node - x_p) / d) * ((d - h) * pow2_der).  Every particle in
 * the support counts exactly once: the reference's hash-aliasing multiplicity reproduces its own neighbour sets of
 * particles, and a field has no reference counterpart.  Summation order is canonical (cells in increasing linear id of
 * the handle's grid, ascending particle id inside a cell), so the result depends on the particle set and the query
 * alone -- not on grid versus points call, slab count, WS_FLAG_GRAPH or the tile schedule.  Nothing the next ws_step
 * reads is written (the sampler bins the positions into scratch of its own, allocated on the first call).
 * Errors: WS_ERR_INVALID_ARG (NULL handle; both outputs NULL on a single handle; m == 0; a dims entry of 0; a non-finite
 * origin or point; spacing <= 0 or non-finite; more than 2^31 nodes), WS_ERR_OUT_OF_MEMORY (scratch allocation failed:
 * the handle stays usable), WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles), WS_ERR_HIP on an unusable handle. */
ws_status ws_sample_density_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                 float *out_density, float *out_gradient);
/* The same field at m arbitrary points (xyz: m*3 floats). */
ws_status ws_sample_density_points(ws_handle *h, const float *xyz, uint32_t m, float *out_density, float *out_gradient);

/* The fluid's surface, rho = iso, as a triangle mesh (marching tetrahedra on the sampled grid).  The volume
 * never leaves the device: only vertices, normals and triangles are copied out.  A pure function of the grid field:
 *   Field: exactly what ws_sample_density_grid returns for the same origin, spacing and dims (density, gradient, node
 *     coordinates fl(origin + fl(i * spacing)), the handle's arithmetic).  A node is INSIDE iff rho >= iso.
 *   Edges and vertices: node n = (i, j, k) has 7 forward edges of type d = 1..7, to n + (d & 1, d >> 1 & 1, d >> 2 & 1)
 *     when that node exists.  An edge is crossed iff its ends differ in "inside"; each crossed edge carries one vertex,
 *     at t = (iso - rho_a) / (rho_b - rho_a), p = p_a + t * (p_b - p_a) per axis (a = n, b = its neighbour; every
 *     operation rounded to float, divisions correctly rounded).  Vertices are ordered by the node's linear index
 *     (k * ny + j) * nx + i, then by d.
 *   Normals: g = g_a + t * (g_b - g_a) per axis, n = -g / sqrtf(g.g), g.g = gx*gx + gy*gy + gz*gz left to right,
 *     correctly rounded sqrt and divisions; (0, 0, 0) where g.g == 0.  This arithmetic is IEEE whatever the handle's
 *     flags: only the sampled field follows WS_FLAG_IEEE_DIVISION.
 *   Tetrahedra: the cube at n exists when i < nx-1, j < ny-1, k < nz-1; corner c = 0..7 lies at
 *     n + (c & 1, c >> 1 & 1, c >> 2 & 1).  It is split along its 0-7 diagonal into six tets, in this order:
 *     {0,1,3,7} {0,1,5,7} {0,2,3,7} {0,2,6,7} {0,4,5,7} {0,4,6,7} (corners q0 q1 q2 q3 as listed).  A tet edge (u, v)
 *     has u a bitwise subset of v: it is the forward edge of type u ^ v at node n + u.  Neighbouring cubes cut their
 *     shared face along the same diagonal, so the mesh has no cracks and needs no ambiguity table.
 *   Triangles: case s = sum of 2^k over the tet's inside corners q_k.  Local edges 0..5 = (q0 q1) (q0 q2) (q0 q3)
 *     (q1 q2) (q1 q3) (q2 q3).  Triangles per case, as local edges (v0 v1 v2):
 *        1: 0 1 2     2: 0 4 3     4: 1 3 5     8: 2 5 4
 *       14: 0 2 1    13: 0 3 4    11: 1 5 3     7: 2 4 5
 *        3: 1 2 4, 1 4 3     12: 1 3 4, 1 4 2
 *        5: 2 0 3, 2 3 5     10: 3 0 2, 3 2 5
 *        9: 0 1 5, 0 5 4      6: 0 4 5, 0 5 1       (0 and 15: none)
 *     Tets 1, 2 and 5 are negatively oriented (det(q1 - q0, q2 - q0, q3 - q0) < 0): their triangles are written as
 *     (v0 v2 v1).  So (v1 - v0) x (v2 - v0) points from the inside corners to the outside ones: out of the fluid.
 *     Triangles are ordered by cube (linear index of its corner 0), then tet 0..5, then table order; out_tri holds
 *     three vertex indices (0-based, into out_xyz) per triangle.
 *   Counts and capacity, like snprintf: on WS_OK *n_vertices and *n_triangles hold the full counts.  The mesh (out_xyz
 *     3 floats per vertex, out_normal the same, out_tri) is written only when out_xyz and out_tri are both non-NULL and
 *     both counts fit max_vertices / max_triangles; otherwise nothing else is written.  The gradient is sampled only
 *     when out_normal, out_xyz and out_tri are all non-NULL (out_normal == NULL: neither sampled nor copied).
 *   Boundary: the surface is clipped open at the grid's boundary.  If every boundary node is outside (a grid reaching
 *     h beyond the fluid) the mesh is closed: every edge is shared by exactly two triangles, in opposite directions.
 *     A node whose density equals iso exactly may give zero-area triangles.
 * Waits for enqueued steps.  Nothing ws_step reads is written.  Slab handles: COLLECTIVE (the global particle set,
 * bit-identical to a single handle); a rank that passes all five outputs NULL only contributes, and a rank validates
 * its query (origin, spacing and dims included) only after the gather, so a refused rank leaves no peer waiting.
 * Errors: WS_ERR_INVALID_ARG (NULL handle, origin, spacing or dims; NULL count pointers on a rank that wants output; a
 * dims entry < 2; a non-finite origin; spacing <= 0 or non-finite; iso <= 0 or non-finite; more than 2^28 nodes, which
 * keeps every vertex id below 2^31 and the triangle count below 2^32), WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER
 * handles), WS_ERR_OUT_OF_MEMORY (scratch allocation failed: the handle stays usable), WS_ERR_HIP on an unusable handle. */
ws_status ws_extract_surface(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                             float iso, uint32_t max_vertices, uint32_t max_triangles,
                             float *out_xyz, float *out_normal, uint32_t *out_tri,
                             uint32_t *n_vertices, uint32_t *n_triangles);

/* ---- smooth surfaces: anisotropic particle kernels (Yu & Turk, ACM TOG 2013) ----------------------
 * The field above gives every particle a ball of radius h: flat water shows bumps at the particle spacing, thin sheets
 * break into blobs and a lone droplet is a ball about h wide.  Here each particle's kernel is an ellipsoid shaped by
 * the weighted covariance of its neighbours (flat along the normal at a free surface, about round in the bulk, small
 * and round with few neighbours), and its centre moves toward its neighbourhood mean.
 *
 * Per-particle stage.  IEEE arithmetic whatever the handle's flags: every operation rounded to float, divisions and
 * sqrt correctly rounded, no contraction; sums run left to right in the order given, starting from 0.
 *   Neighbours: N_i = the particles j (i included) the density sampler's sweep visits around o = x_i and accepts: the
 *     27 cells of the handle's grid around x_i's (clamped) cell, cells in increasing linear id, ids ascending inside a
 *     cell; e = x_j - x_i, d2 = e.x*e.x + e.y*e.y + e.z*e.z, j counts unless d2 > d2_accept.  n_i = |N_i|.
 *   Weights and moments, from that one sweep: d = sqrt(d2), q = d / h, w = 1 - (q*q)*q; W = sum w, S_a = sum w*e_a,
 *     Q_ab = sum (w*e_a)*e_b for ab = xx, yy, zz, xy, xz, yz.
 *   Mean and covariance: m_a = S_a / W, C_ab = Q_ab / W - m_a*m_b (W >= 1: the self term; the moments are taken about
 *     x_i, so |e| <= h and the one-pass form loses only a few bits).  Centre: c_a = x_a + lambda*m_a.
 *   Lone branch, taken if n_i < N_eps or if the anisotropic branch finds sigma_max not > 0: inv = 1 / k_n, M = inv*I
 *     (off-diagonals +0), f = (inv*inv)*inv.
 *   Anisotropic branch: cyclic Jacobi on A = C, R = I, exactly 5 sweeps of the pairs (p, q) = (0,1), (0,2), (1,2), r
 *     the third index; no convergence exit.  A rotation is skipped iff a_pq == 0; otherwise, in this order:
 *       theta = (a_qq - a_pp) / (2*a_pq);
 *       t = 1 / (2*theta) if |theta| > 2^32, else t = g / (|theta| + sqrt(theta*theta + 1)), g = +1 if theta >= 0 else -1;
 *       c = 1 / sqrt(t*t + 1), s = t*c;
 *       a_pp = a_pp - t*a_pq; a_qq = a_qq + t*a_pq; a_pq = 0;
 *       a_rp, a_rq = c*a_rp - s*a_rq, s*a_rp + c*a_rq (both from the old values);
 *       for k = 0, 1, 2: R_kp, R_kq = c*R_kp - s*R_kq, s*R_kp + c*R_kq.
 *     sigma_k = the final a_kk and r_k = column k of R (unsorted); sigma_max = fmaxf(fmaxf(sigma_0, sigma_1), sigma_2);
 *     floor = sigma_max / k_r; s_k = fmaxf(sigma_k, floor) / sigma_max (the longest axis is exactly 1; a slightly
 *     negative sigma from rounding is floored); M_ab = sum over k = 0, 1, 2 of ((1/s_k)*r_k[a])*r_k[b], from 0;
 *     f = 1 / ((s_0*s_1)*s_2).
 *   Every 1/s_k >= 1, so the ellipsoid |M e| <= h lies inside the ball |e| <= h, and the 27-cell stencil stays valid.
 *   This departs from Yu & Turk's k_s: the longest axis is normalised to h, where Y&T scale the whole kernel (which
 *   could grow wider than h).
 * Field at a node or point o, in the handle's arithmetic exactly as ws_sample_density_grid: the particles are binned by
 *   their CENTRES c_j on the handle's grid and visited in the canonical order.  A particle counts iff e = c_j - o has
 *   !(d2 > d2_accept) and u = M_j e, u_a = (M_a0*e.x + M_a1*e.y) + M_a2*e.z, has !(dM2 > d2_accept), dM2 = u.x*u.x +
 *   u.y*u.y + u.z*u.z.  Density term sk_density(dM) * f_j, dM = sqrt(dM2) (the handle's sqrt); gradient term: the
 *   density sampler's expression (both arithmetic forms) with e replaced by v = M_j u (same row order as u) and d by
 *   dM, then times f_j; f_j is the last operation of both (0 at dM == 0).
 * Mesh: ws_extract_surface's definition, word for word, on this grid field.
 * The isotropic limit is a contract: with smoothing 0, lone_scale 1 and min_neighbours 0xFFFFFFFF every particle takes
 *   the lone branch with M = I, f = 1 and c = x, and the field, gradient, points output and mesh are bit-identical to
 *   ws_sample_density_grid / _points and ws_extract_surface.
 * All four calls wait for enqueued steps, write nothing ws_step reads, recompute everything from the current positions
 * and keep their scratch in the sampler's (grow-only, freed by ws_destroy).  Slab handles: COLLECTIVE on the gathered
 * global set, the same bits as a single handle; a rank validates its query and its params only after the gather.
 * Errors: as the corresponding density / surface call, plus WS_ERR_INVALID_ARG for NULL params, smoothing outside
 * [0, 1], max_ratio < 1, lone_scale outside (0, 1] or a non-finite value. */
typedef struct ws_aniso_params {
    float smoothing;         /* lambda in [0, 1]: centre = x + lambda * (weighted mean offset)       default 0.9 */
    float max_ratio;         /* k_r >= 1: shortest axis >= longest / k_r                             default 4   */
    float lone_scale;        /* k_n in (0, 1]: radius of a lone particle's ball, in units of h       default 0.5 */
    uint32_t min_neighbours; /* N_eps: fewer neighbours (self included) -> lone ball                 default 12  */
} ws_aniso_params;
/* The defaults above (host-only: no handle, no device). */
ws_status ws_default_aniso_params(ws_aniso_params *out);
/* The stage, per particle in original-id order: out_centre n*3 (c), out_matrix n*6 (M: xx yy zz xy xz yz), out_scale n
 * (f = det M), out_neighbours n (n_i).  n = ws_num_particles, or the global count on slab handles.  Any output may be
 * NULL; a single handle with all four NULL only checks a. */
ws_status ws_read_anisotropy(ws_handle *h, const ws_aniso_params *a, float *out_centre, float *out_matrix, float *out_scale,
                             uint32_t *out_neighbours);
/* ws_sample_density_grid / _points with the anisotropic field. */
ws_status ws_sample_aniso_grid(ws_handle *h, const ws_aniso_params *a, const float origin[3], const float spacing[3],
                               const uint32_t dims[3], float *out_field, float *out_gradient);
ws_status ws_sample_aniso_points(ws_handle *h, const ws_aniso_params *a, const float *xyz, uint32_t m, float *out_field,
                                 float *out_gradient);
/* ws_extract_surface on the anisotropic field (same arguments, same capacity protocol). */
ws_status ws_extract_aniso_surface(ws_handle *h, const ws_aniso_params *a, const float origin[3], const float spacing[3],
                                   const uint32_t dims[3], float iso, uint32_t max_vertices, uint32_t max_triangles,
                                   float *out_xyz, float *out_normal, uint32_t *out_tri, uint32_t *n_vertices,
                                   uint32_t *n_triangles);

/* ---- rays at the fluid surface: first-hit distance and normal (picking, probes, depth images) ------
 * Where does a ray enter the fluid?  A fixed-step march along the ray, a bisection of the step that crossed rho = iso and
 * the field's gradient at the hit, all on the device: the host sends rays (or a camera) and receives one float of
 * distance and three of normal per ray.  A pure function of the particle set, the ray and the parameters:
 *   Field: exactly what ws_sample_density_points returns at a point -- with a non-NULL ws_aniso_params what
 *     ws_sample_aniso_points returns: the handle's arithmetic (WS_FLAG_IEEE_DIVISION or not), the canonical summation
 *     order, the 27 cells of the point's clamped cell.
 *   Ray march: a ray has origin o and direction v; v is used as given (not normalised), so t is in units of |v|.
 *     Sample parameter t_k = fl(t_start + fl((float)k * dt)) for k = 0 .. steps; sample point p_a(t) = fl(o_a + fl(t * v_a))
 *     per axis; rho_k = the field at p(t_k).  The hit index K is the smallest k with rho_k >= iso.
 *     No such k: a miss, out_t = +INFINITY and out_normal = (0, 0, 0).
 *     K = 0: the ray starts inside, t = t_0, no refinement.
 *     K >= 1: bisection from lo = t_{K-1}, hi = t_K, exactly `refine` times with no early exit: mid = fl(fl(lo + hi) *
 *     0.5f); if rho(p(mid)) >= iso then hi = mid else lo = mid.  The result is t = hi, so the field at the reported
 *     point p(t) is always >= iso.
 *   Normal (sampled only when out_normal != NULL): g = the field's gradient at p(t) in the handle's arithmetic,
 *     n = -g / sqrtf(g.g), g.g = gx*gx + gy*gy + gz*gz left to right, correctly rounded sqrt and divisions whatever the
 *     handle's flags; (0, 0, 0) where g.g == 0 -- ws_extract_surface's rule for a vertex normal, word for word.
 *   Camera rays (ws_cast_camera) are generated on the device: pixel (i, j) of a W x H image has
 *     u = ((float)i + 0.5f) * (2.0f / (float)W) - 1.0f, w = 1.0f - ((float)j + 0.5f) * (2.0f / (float)H), every operation
 *     rounded; o = eye, v_a = (forward_a + u * right_a) + w * up_a.  The host puts the field of view and the aspect ratio
 *     into the lengths of right and up; with unit forward, and right and up perpendicular to it, out_t is the view-space
 *     depth.  Outputs are H * W entries, x fastest (pixel (i, j) at j * W + i).  ws_cast_camera returns the bits
 *     ws_cast_rays returns on those rays.
 * Both calls wait for enqueued steps, write nothing ws_step reads, recompute the binning from the current positions (with
 * params also the per-particle stage and the centres' binning) on every call and keep their scratch in the sampler's
 * (grow-only, freed by ws_destroy).  A ray's result does not depend on the other rays of the call.  Either output may be
 * NULL, not both on a single handle.  Slab handles: COLLECTIVE on the gathered global set, the same bits as a single
 * handle; a rank that passes both outputs NULL only contributes, and a rank validates its query only after the gather.
 * Errors: as ws_sample_density_points (ws_sample_aniso_points with params), plus WS_ERR_INVALID_ARG for: both outputs
 * NULL on a single handle; NULL r; NULL
 * origins or directions; NULL cam or size; steps outside 1 .. 65535; refine > 24; dt or iso not finite or not > 0; a
 * non-finite t_start, origin or direction (camera: eye, forward, right, up); a direction (camera: forward) that is
 * (0, 0, 0); any of |t_start| + steps * dt, |o_a|, |v_a| (camera: any component of the four vectors) above 1e15, which
 * keeps every sample point finite; m == 0, a size of 0, more than 2^28 rays. */
typedef struct ws_ray_params {
    float t_start;   /* parameter of the first sample                                              */
    float dt;        /* march step, > 0 (in units of |v|)                                          */
    uint32_t steps;  /* samples k = 0 .. steps, 1 .. 65535                                         */
    uint32_t refine; /* bisection steps of the crossing interval, 0 .. 24                          */
    float iso;       /* the surface's level, > 0                                                   */
} ws_ray_params;
typedef struct ws_camera {
    float eye[3];
    float forward[3];
    float right[3];
    float up[3];
} ws_camera;
/* m rays: origin_xyz and dir_xyz hold m*3 floats; out_t m floats, out_normal m*3. */
ws_status ws_cast_rays(ws_handle *h, const ws_aniso_params *a, const ws_ray_params *r, const float *origin_xyz,
                       const float *dir_xyz, uint32_t m, float *out_t, float *out_normal);
/* One ray per pixel of a size[0] x size[1] (W x H) image. */
ws_status ws_cast_camera(ws_handle *h, const ws_aniso_params *a, const ws_ray_params *r, const ws_camera *cam,
                         const uint32_t size[2], float *out_t, float *out_normal);

/* ---- the fluid's velocity as a field, and tracers carried by it (no reference counterpart) ----------
 * The calls above read positions only.  These give the other half of the state by place, not by particle: colour the
 * extracted mesh by flow speed (the reference's commented-out speed colouring, src/fluid_compute.rs:489-502, moved from
 * the particles to the surface), draw streamlines, carry foam, dye or debris with the water, probe the flow at a point.
 *
 * ws_read_velocities: n*3 floats in ORIGINAL-ID order (n = ws_num_particles, or the global count on slab handles), the
 *   companion of ws_read_positions: the velocities the enqueued steps leave; before the first step zeros, or what
 *   ws_write_particles loaded.  Slab handles: COLLECTIVE, out_xyz == NULL only contributes.
 *
 * Velocity field at a node or point o (ws_sample_velocity_grid / _points): the node formula, node order, accept test,
 *   27-cell stencil of the clamped cell, canonical summation order and argument errors of ws_sample_density_grid /
 *   _points.  Per accepted candidate j, in canonical order:
 *     d = sqrt(d2) (the handle's sqrt), w = (h - d)^2 * pow2 -- the density sampler's term, the same bits;
 *     rho += w; M_a += fl(w * v_j,a) for a = x, y, z: each product rounded, then each sum; all four sums start at 0.
 *   After the sweep u_a = M_a / rho, correctly rounded whatever the handle's flags, if rho > 0; otherwise u = (+0, +0, +0).
 *   Only the sqrt inside w follows WS_FLAG_IEEE_DIVISION (the split the surface normals use).
 *   out_velocity: 3 floats per node or point (u); out_density: rho, BIT-IDENTICAL to what ws_sample_density_grid /
 *   _points return for the same query.  v_j is what ws_read_velocities returns for particle j, x_j what
 *   ws_read_positions returns.  Either output may be NULL, not both on a single handle.  The field is isotropic.
 *
 * ws_advect_points moves m tracer points through the FROZEN field of the current state (the fluid does not move during
 *   the call).  Per point, independently of the other points, `substeps` times (midpoint rule; hdt = fl(0.5f * dt)):
 *     1. (u1, rho1) = the field at p exactly as ws_sample_velocity_points defines it.  rho1 == 0: the tracer is outside
 *        the fluid; p stays and the loop ends.
 *     2. q_a = fl(p_a + fl(hdt * u1_a)); (u2, rho2) = the field at q.  rho2 == 0: u2 = u1 (the midpoint left the fluid:
 *        an Euler step).
 *     3. p_a = fl(p_a + fl(dt * u2_a)).
 *   out_xyz (required on a rank that wants output): the final p, m*3 floats; xyz and out_xyz may be the same buffer.
 *   out_velocity / out_density (optional): the field at the final p, from one more sweep.  There is no container clamp.
 *   A host that performs this march itself with ws_sample_velocity_points and float arithmetic gets the same bits, in
 *   either arithmetic of the handle.
 * All of them wait for enqueued steps, write nothing ws_step reads, recompute the binning from the current state on every
 * call and keep their scratch in the sampler's (grow-only, freed by ws_destroy; the velocity arrays are allocated on the
 * first velocity call only).  Slab handles: COLLECTIVE on the gathered global set (one gather of {position, velocity}),
 * the same bits as a single handle; a rank that passes every output NULL only contributes, and a rank validates its query
 * only after the gather, so a refused rank leaves no peer waiting.
 * Errors: as ws_sample_density_grid / _points; WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles, ws_read_velocities
 * included); WS_ERR_HIP on an unusable handle; ws_advect_points also WS_ERR_INVALID_ARG for: NULL a; substeps outside
 * 1 .. 4096; dt non-finite or |dt| > 1e6 (0 and negative dt are allowed: backward tracing); NULL xyz; a non-finite
 * coordinate or |coordinate| > 1e15; m == 0, more than 2^28 points; NULL out_xyz with another output given. */
typedef struct ws_advect_params {
    float dt;          /* time the tracers travel per substep (any sign)                             */
    uint32_t substeps; /* midpoint steps of dt each, 1 .. 4096                                       */
} ws_advect_params;
ws_status ws_read_velocities(ws_handle *h, float *out_xyz);
ws_status ws_sample_velocity_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                  float *out_velocity, float *out_density);
ws_status ws_sample_velocity_points(ws_handle *h, const float *xyz, uint32_t m, float *out_velocity, float *out_density);
ws_status ws_advect_points(ws_handle *h, const ws_advect_params *a, const float *xyz, uint32_t m, float *out_xyz,
                           float *out_velocity, float *out_density);

/* ---- whitewater: where foam, spray and bubbles are born, and how they move (no reference counterpart) --
 * The diffuse-particle model of Ihmsen, Akinci, Akinci and Teschner, "Unified spray, foam and air bubbles for
 * particle-based fluids" (2012), on the state the step leaves: ws_read_whitewater gives every fluid particle its
 * potentials, ws_emit_whitewater turns them into new diffuse particles, ws_step_whitewater classifies and moves diffuse
 * particles by one time step.  The HOST owns the diffuse particles; the library keeps none between calls.
 * All three wait for enqueued steps, write nothing ws_step reads, recompute the sampler's binning from the current state
 * on every call and keep their scratch in the sampler's (grow-only, freed by ws_destroy; the whitewater arrays are
 * allocated on the first whitewater call only).  Slab handles: COLLECTIVE on the gathered global {position, velocity}
 * set, the same bits as a single handle; a rank that passes every output NULL only contributes, and a rank validates
 * its arguments only after the gather, so a refused rank leaves no peer waiting.
 * Below fl() is a rounding to float; every operation is rounded once, nothing is contracted; x_j, v_j are what
 * ws_read_positions / ws_read_velocities return for particle j; dot(a, b) = fl(fl(fl(a.x*b.x) + fl(a.y*b.y)) + fl(a.z*b.z)).
 *
 * ws_read_whitewater: the per-particle stage, n entries in ORIGINAL-ID order.  IEEE arithmetic whatever the handle's
 *   flags (correctly rounded sqrt and division), as the anisotropy stage.  The candidates of particle i are those the
 *   density sampler's sweep visits around x_i and accepts: the 27 cells of the clamped cell in increasing linear id,
 *   ids ascending inside a cell, e = x_j - x_i, d2 = dot(e, e), rejected iff d2 > d2_accept.  d = sqrt(d2).  A candidate
 *   at d == 0 (i itself, a coincident particle) contributes to nothing below.  All sums start at +0 and take their
 *   terms in that order.
 *   Pass A: g_i = the gradient ws_sample_density_points returns at x_i in its WS_FLAG_IEEE_DIVISION form;
 *     gg = dot(g, g); nh_i = -g / sqrt(gg) per axis, (0, 0, 0) where gg == 0 -- ws_extract_surface's normal rule.
 *   Pass B, per contributing candidate j (d > 0): xh_a = (-e_a) / d (the unit vector from j to i); w = 1 - d / h;
 *     r_a = v_i,a - v_j,a; s = sqrt(dot(r, r));
 *     trapped air:  if s > 0:  rh_a = r_a / s;  T_i += (s * (1 - dot(rh, xh))) * w;
 *     crest:        m_a = -xh_a;  if dot(m, nh_i) < 0:  K_i += (1 - dot(nh_i, nh_j)) * w;
 *     count:        c_i += 1.
 *   After the sweep: vv = dot(v_i, v_i); E_i = 0.5 * vv; sv = sqrt(vv);
 *     alignment a_i = dot(v_i / sv, nh_i) (each component divided first) if sv > 0, else +0.
 *   Outputs, any of which may be NULL (all NULL: WS_ERR_INVALID_ARG on a single handle, contribute-only on a slab):
 *     out_trapped n (T), out_crest n (K, not gated by the alignment), out_align n (a), out_energy n (E),
 *     out_normal n*3 (nh), out_neighbours n (c).
 *
 * ws_emit_whitewater: new diffuse particles from the stage (which it runs itself).  With
 *     clamp(I, lo, hi) = (fminf(I, hi) - fminf(I, lo)) / (hi - lo)                   (in [0, 1]; three roundings)
 *     rate_i = (clamp(E_i, tau_energy) * (k_trapped * clamp(T_i, tau_trapped) + C_i)) * dt,
 *     C_i = k_crest * clamp(K_i, tau_crest) if a_i >= crest_align, else +0,
 *   particle i emits m_i = 0 if sv == 0 (it has no axis), else with f = floorf(rate_i + U(i, 0)): 0 unless f >= 1,
 *   max_per_particle if f >= max_per_particle, else (uint32_t)f -- a stochastic, deterministic rounding of the rate.
 *   Random numbers are counter-based, in 32-bit unsigned arithmetic (wrapping):
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;
 *     word(i, c) = mix(mix(seed + i * 0x9E3779B9) + c);  U(i, c) = (float)(word(i, c) >> 8) * 2^-24, in [0, 1).
 *   Counter 0 rounds the count.  Spawn k of particle i (k < m_i) owns the 18 counters from b = 1 + 18 * k:
 *     b: U_h (the height along the axis), b + 1: U_l (the lifetime), b + 2 + 2 t and b + 3 + 2 t (t = 0 .. 7): the disc.
 *   Axis vh_a = v_i,a / sv.  Let q be the axis of the smallest |vh_q| (the lowest axis on a tie, strict <) and
 *     c = (0, -vh_z, vh_y) for q = x, (vh_z, 0, -vh_x) for q = y, (-vh_y, vh_x, 0) for q = z;
 *     e1 = c / sqrt(dot(c, c)) per axis;  e2 = vh x e1: e2_x = vh_y * e1_z - vh_z * e1_y, and cyclically.
 *   Disc point (a, b) by rejection: for t = 0 .. 7, a = 2 * U(i, b + 2 + 2 t) - 1, b likewise from the next counter;
 *     the first t with a * a + b * b <= 1 is taken; none: (a, b) = (0, 0).  There is no trigonometry.
 *   o_a = radius * (a * e1_a + b * e2_a);  p_a = (x_i,a + o_a) + (U_h * dt) * v_i,a;  v_a = v_i,a + o_a;
 *   life = lifetime[0] + U_l * (lifetime[1] - lifetime[0]).
 *   Spawns are ordered by particle id, then k (their offsets are an exclusive scan of m_i), so the order does not depend
 *   on the launch shape or the slab count.  Counts and capacity, like snprintf (ws_extract_surface): on WS_OK
 *   *n_emitted holds the full count; out_xyz and out_velocity (3 floats per spawn), out_life and out_source (the emitting
 *   id, uint32_t), each of which may be NULL, are written only when the count fits max_emitted.
 *
 * ws_step_whitewater: m host-owned diffuse particles, one dt.  Per particle, independently of the others:
 *   (u, rho) = the field at p exactly as ws_sample_velocity_points defines it in the HANDLE's arithmetic; c = the number
 *   of candidates that sweep accepted (d == 0 included); g = the handle's gravity.  Then
 *     spray  (c < spray_max):   v_a = v_a + dt * g_a;                                      p_a = p_a + dt * v_a;
 *     bubble (c > bubble_min):  v_a = (v_a + dt * ((-buoyancy) * g_a)) + drag * (u_a - v_a);   p_a = p_a + dt * v_a;
 *     foam   (otherwise):       v_a = u_a;  p_a = p_a + dt * u_a;  life = life - dt;
 *   then the step's own container rule, per axis: nd = -1 * collision_damping; if p_a < ext_min_a: v_a = v_a * nd,
 *   p_a = ext_min_a; else if p_a > ext_max_a: v_a = v_a * nd, p_a = ext_max_a.
 *   Class: 3 (dead; the host drops it) if life <= 0 after the above, else 0 spray, 1 foam, 2 bubble.
 *   xyz, velocity and life hold the m particles on entry; out_xyz, out_velocity, out_life receive them and may be the
 *   same buffers; out_class holds m bytes.  Any output may be NULL, not all on a single handle.
 * Errors: WS_ERR_INVALID_ARG (NULL handle; every output NULL on a single handle; ws_emit_whitewater: NULL e or
 *   n_emitted on a rank that wants output, a tau pair that is not finite with 0 <= tau[0] < tau[1], a rate that is not
 *   finite and >= 0, crest_align not finite, dt or radius not finite and > 0, lifetime not finite with
 *   0 <= lifetime[0] <= lifetime[1], max_per_particle outside 1 .. 64; ws_step_whitewater: NULL p, xyz, velocity or life,
 *   dt not finite and > 0, buoyancy not finite, drag outside [0, 1], m == 0 or more than 2^28, a non-finite coordinate,
 *   velocity or life, a |coordinate| or |velocity| > 1e15); WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles);
 *   WS_ERR_OUT_OF_MEMORY (scratch allocation failed: the handle stays usable); WS_ERR_HIP on an unusable handle. */
typedef struct ws_whitewater_emit_params {
    float tau_trapped[2]; /* T below [0] emits nothing, above [1] at the full rate                    */
    float tau_crest[2];   /* the same for K                                                           */
    float tau_energy[2];  /* ... and for E, which scales both                                         */
    float k_trapped;      /* diffuse particles per second at full trapped-air potential               */
    float k_crest;        /* ... at full crest potential                                              */
    float crest_align;    /* a crest counts where a_i >= this (0.6)                                   */
    float dt;             /* the time the rates are integrated over                                   */
    float radius;         /* radius of the spawn cylinder around x_i, along v_i                       */
    float lifetime[2];    /* a spawn's lifetime is uniform in [[0], [1])                              */
    uint32_t max_per_particle; /* 1 .. 64                                                             */
    uint32_t seed;
} ws_whitewater_emit_params;
typedef struct ws_whitewater_step_params {
    float dt;
    uint32_t spray_max;   /* fewer accepted fluid neighbours than this: spray (6)                     */
    uint32_t bubble_min;  /* more than this: a bubble (20); in between: foam                          */
    float buoyancy;       /* k_b: bubbles accelerate by -k_b * gravity                                */
    float drag;           /* k_d in [0, 1]: the share of (u - v) a bubble takes per step              */
} ws_whitewater_step_params;
/* Host-only (no device needed; WS_ERR_INVALID_ARG for NULL): taus (5, 50) (0.5, 4) (1, 25), rates 400 and 400, crest_align 0.6, dt 1/60, radius 0.1,
 * lifetime (2, 5), max_per_particle 8, seed 0; dt 1/60, spray_max 6, bubble_min 20, buoyancy 2, drag 0.5. */
ws_status ws_default_whitewater_emit_params(ws_whitewater_emit_params *out);
ws_status ws_default_whitewater_step_params(ws_whitewater_step_params *out);
ws_status ws_read_whitewater(ws_handle *h, float *out_trapped, float *out_crest, float *out_align, float *out_energy,
                             float *out_normal, uint32_t *out_neighbours);
ws_status ws_emit_whitewater(ws_handle *h, const ws_whitewater_emit_params *e, uint32_t max_emitted, float *out_xyz,
                             float *out_velocity, float *out_life, uint32_t *out_source, uint32_t *n_emitted);
ws_status ws_step_whitewater(ws_handle *h, const ws_whitewater_step_params *p, const float *xyz, const float *velocity,
                             const float *life, uint32_t m, float *out_xyz, float *out_velocity, float *out_life,
                             uint8_t *out_class);

/* ---- acting on the fluid: push, pull, blow on and stir it (the "interaction force" of the simulation the
 *      reference descends from, which the reference dropped) ----------------------------------------------------------
 * Every call above this block reads the fluid.  ws_apply_forces changes the VELOCITIES of the state the enqueued steps
 * leave, by one explicit Euler step of the acceleration of k emitters, stream-ordered after the steps enqueued so far and
 * before the next ws_step -- where the step itself applies gravity (v += a * dt, then the predicted position, then the
 * cell).  A host calls it once per frame while the mouse button is held, with the hit point of ws_cast_camera as centre.
 * Positions do not change.  The predicted position of EVERY particle becomes the library's own rule on the new velocity,
 * pred_a = fl(x_a + fl(v'_a * 0.02f)), and the next step starts from it exactly as if gravity had produced that velocity.
 * Below fl() is a rounding to float; arithmetic is IEEE whatever the handle's flags: every operation is rounded once, sqrt
 * and division are correctly rounded, nothing is contracted; dot(a, b) = fl(fl(fl(a.x*b.x) + fl(a.y*b.y)) + fl(a.z*b.z))
 * (the whitewater block's).  x, v are what ws_read_positions / ws_read_velocities return.
 * Per particle, with A = (+0, +0, +0), for the emitters e = 0 .. k-1 in the order given (c = centre, R = radius):
 *   1. q_a = x_a - c_a; d = sqrt(dot(q, q)).  If !(d < R) the emitter does not see the particle: on to the next one.
 *      Otherwise the particle is AFFECTED and n_e += 1.
 *   2. w = 1 - d / R; s = strength * w.
 *   3. WS_FORCE_RADIAL: if d > 0: A_a = A_a - (q_a / d) * s (a particle exactly at the centre gets no radial term);
 *      WS_FORCE_JET:    A_a = A_a + axis_a * s;
 *      WS_FORCE_VORTEX: t = axis x q, t_x = axis_y*q_z - axis_z*q_y and cyclically (each product rounded, then the
 *                       difference); A_a = A_a + t_a * s.
 *   4. every kind: g = damping * w; A_a = A_a - v_a * g, with v the velocity BEFORE the call, not a running value.
 * After the loop an affected particle gets v'_a = v_a + dt * A_a; a particle no emitter sees keeps its velocity bit for
 * bit (a -0 stays -0).  out_affected, if not NULL, receives the k counts n_e.
 * Afterwards, on a single handle: ws_steps_done is unchanged; ws_read_particles reports the old position, the new velocity
 * and predicted position and the LAST STEP's density, pressure and acceleration; every read-only call sees the new
 * velocities; a WS_FLAG_GRAPH handle keeps replaying its captured step (the emitters travel in the kernel's arguments, the
 * kernel is launched outside the graph, no array moves).  The call may be made between ws_read_positions_begin and _end.
 * With out_affected == NULL a single handle only enqueues and returns without waiting; with it the call waits for the
 * counts.
 * Slab handles: COLLECTIVE, the same bits as a single handle: every rank makes the same call with the same arguments at the
 * same point of its frame.  The state is gathered, every rank applies the definition to the global set and reloads the
 * particles it owns on the unchanged geometry -- so, as after any load of a slab handle, the 80-byte view reports zero
 * density / pressure / acceleration until the next ws_step, cumulative counters carry over and captured steps are
 * re-captured.  out_affected is the GLOBAL count on every rank that passes it.  The verdict is common: a rank validates its
 * arguments after the gather, and if any rank refuses, or the ranks' arguments differ, ALL return WS_ERR_INVALID_ARG and
 * nothing is changed.
 * Errors: WS_ERR_INVALID_ARG (NULL handle or f; k outside 1 .. WS_MAX_FORCES; dt not finite or not > 0; a kind > 2; a
 * non-zero reserved word; a non-finite centre, axis, strength or damping; damping < 0; radius not finite or not > 0; any
 * magnitude above 1e15): nothing is touched and the handle steps on.  WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER
 * handles); WS_ERR_HIP on an unusable handle.  Whether a huge strength drives a velocity to infinity is the host's
 * business, as it is with gravity. */
#define WS_FORCE_RADIAL 0u   /* toward the centre (strength > 0) or away from it (< 0) */
#define WS_FORCE_JET    1u   /* along `axis` */
#define WS_FORCE_VORTEX 2u   /* around `axis` through the centre */
#define WS_MAX_FORCES   16u
typedef struct ws_force {      /* 48 bytes */
    uint32_t kind;             /* offset 0 */
    float centre[3];           /* 4  */
    float axis[3];             /* 16: used as given, never normalised; ignored by RADIAL */
    float radius;              /* 28: R > 0; a particle is in reach iff d < R */
    float strength;            /* 32 */
    float damping;             /* 36: >= 0; velocity removed per second at the centre (a brake, a spoon) */
    uint32_t reserved[2];      /* 40: must be 0 */
} ws_force;
ws_status ws_apply_forces(ws_handle *h, const ws_force *f, uint32_t k, float dt, uint32_t *out_affected);

/* ---- solid things in the water: the fluid goes round them, and they feel it (no reference counterpart) --
 * An emitter is a hint; a solid is a wall.  ws_collide_solids resolves the state the enqueued steps leave against k solids
 * (spheres, boxes, capsules, each optionally HOLLOW: the fluid is kept inside), stream-ordered after the steps enqueued so
 * far and before the next ws_step; ws_step itself knows nothing of solids.  A particle nearer to a solid than `margin` is
 * pushed out along the surface normal to exactly that distance, the part of its velocity that goes into the solid is
 * reflected (restitution) and its sliding braked (friction), both relative to the solid's own motion, and the momentum
 * the particles took is summed per solid: with ws_body_forces (what the water does to a body) and this call (what the
 * body does to the water, and the reaction) a floating body is complete.
 * Below fl() is a rounding to float; arithmetic is IEEE whatever the handle's flags: every operation is rounded once, sqrt
 * and division are correctly rounded, nothing is contracted; dot(a, b) = fl(fl(fl(a.x*b.x) + fl(a.y*b.y)) + fl(a.z*b.z))
 * (the whitewater block's); a cross product a x b has x = fl(fl(a.y*b.z) - fl(a.z*b.y)) and cyclically (the forces
 * block's); x * y + z is fl(fl(x*y) + z).  Indices a, i run over 0 .. 2.
 * Per particle, with a RUNNING (p, v) that starts from what ws_read_positions / ws_read_velocities return, for the solids
 * e = 0 .. k-1 in the order given -- collisions resolve in sequence -- with c = centre, R_i = rot[3i .. 3i+2] (row i: the
 * solid's i-th local axis in world coordinates, used as given), V = velocity, W = angular_velocity:
 *   1. q_a = p_a - c_a; for BOX and CAPSULE l_i = dot(R_i, q).
 *   2. signed distance s and outward unit normal n:
 *      WS_SOLID_SPHERE:  r = size[0]; d = sqrt(dot(q, q)); s = d - r; n_a = q_a / d if d > 0, else n = (0, 1, 0).
 *      WS_SOLID_CAPSULE: r = size[0], L = size[1]; t = fminf(fmaxf(l_1, -L), L); w_a = q_a - t * R_1,a;
 *                        d = sqrt(dot(w, w)); s = d - r; n_a = w_a / d if d > 0, else n = R_0.
 *      WS_SOLID_BOX:     b = size; a_i = |l_i| - b_i; g = fmaxf(fmaxf(a_0, a_1), a_2).
 *                        If g > 0: u_i = copysignf(fmaxf(a_i, 0), l_i); d = sqrt(dot(u, u)); s = d; m_i = u_i / d.
 *                        Otherwise: i* = the lowest i with a_i == g; s = g; m = copysignf(1, l_i*) at i*, +0 elsewhere.
 *                        n_a = (m_0 * R_0,a + m_1 * R_1,a) + m_2 * R_2,a.
 *      WS_SOLID_HOLLOW (flags bit 0): s = -s, n_a = -n_a.
 *   3. a contact exists iff s < margin.  Without one: on to the next solid.  With one the particle is TOUCHED and the
 *      solid's contact count n_e rises by one.
 *   4. push out: p_a = p_a + (margin - s) * n_a.
 *   5. with the new p: r_a = p_a - c_a; u_a = V_a + (W x r)_a; rel_a = v_a - u_a; vn = dot(rel, n).
 *      If vn < 0: j = (1 + restitution) * (-vn); tang_a = rel_a - vn * n_a; dv_a = j * n_a - friction * tang_a;
 *      v_a = v_a + dv_a.  Otherwise the particle is moved, not kicked, and contributes nothing to 6.
 *   6. the reaction on the solid per unit of particle mass: I_a = -dv_a, H = r x I.  Each of the six floats x enters a
 *      64-bit FIXED-POINT sum as llrintf(fminf(fmaxf(x, -0x1p31f), 0x1p31f) * 0x1p24f) (the scaling is exact, llrintf
 *      rounds to nearest, ties to even); the sums wrap modulo 2^64.  Integer addition has no order: the result does not
 *      depend on the launch shape, on the number of slabs or on graphs.  out_impulse[3e + a] = (double)sum * 0x1p-24, the
 *      sum of I_a over the contacts of solid e; out_angular likewise for H (about `centre`); the host multiplies by its
 *      particle mass and divides by its frame time to get a force and a torque.
 * After the loop a TOUCHED particle goes through the step's own container rule: nd = -1 * collision_damping; per axis, if
 * p_a < ext_min_a: v_a = v_a * nd, p_a = ext_min_a; else if p_a > ext_max_a: v_a = v_a * nd, p_a = ext_max_a.  That
 * velocity change does not enter the reaction.  A particle no solid touches keeps its position and velocity bit for bit
 * (a -0 stays -0).  The predicted position of EVERY particle becomes pred_a = fl(p_a + fl(v_a * 0.02f)) and the state is
 * binned again, as after ws_apply_forces.  out_contacts, if not NULL, receives the k counts n_e.
 * Afterwards, on a single handle: ws_steps_done is unchanged; ws_read_particles reports the new position, velocity and
 * predicted position and the LAST STEP's density, pressure and acceleration; every read-only call sees the new positions;
 * a WS_FLAG_GRAPH handle keeps replaying its captured step.  The call may be made between ws_read_positions_begin and
 * _end (the readback keeps the positions it captured).  With all three outputs NULL a single handle only enqueues and
 * returns without waiting; with any of them the call waits for the sums.
 * Slab handles: COLLECTIVE, the same bits as a single handle, by ws_apply_forces' route (gather, every rank applies the
 * definition to the global set and reloads the particles it owns; the 80-byte view reports zero density / pressure /
 * acceleration until the next ws_step).  The outputs are the GLOBAL sums on every rank that passes them.  The verdict is
 * common: if any rank refuses its arguments, or the ranks' solids differ, ALL return WS_ERR_INVALID_ARG and nothing is
 * changed.
 * Errors: WS_ERR_INVALID_ARG (NULL handle or s; k outside 1 .. WS_MAX_SOLIDS; a kind > 2; flag bits other than bit 0; a
 * non-zero reserved word; any non-finite value or magnitude above 1e15 in any field, used or not; a used size not > 0 --
 * SPHERE size[0], BOX size[0 .. 2], CAPSULE size[0]; a capsule's half length size[1] may be 0 but not negative;
 * restitution or friction outside [0, 1]; margin < 0): nothing is touched and the handle steps on.  `rot` is not checked
 * for orthonormality: it is the host's, as an emitter's axis is.  WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles);
 * WS_ERR_HIP on an unusable handle. */
#define WS_SOLID_SPHERE  0u
#define WS_SOLID_BOX     1u
#define WS_SOLID_CAPSULE 2u
#define WS_SOLID_HOLLOW  1u   /* flags bit 0: the fluid is kept INSIDE (a glass, a bowl) */
#define WS_MAX_SOLIDS    16u
typedef struct ws_solid {      /* 112 bytes */
    uint32_t kind;             /* offset 0 */
    uint32_t flags;            /* offset 4 */
    float centre[3];           /* offset 8 */
    float rot[9];              /* offset 20: rows R_0 R_1 R_2 = the solid's local axes in world coordinates; ignored by SPHERE */
    float size[3];             /* offset 56: SPHERE [0] = radius; BOX half extents; CAPSULE [0] = radius, [1] = half length along R_1 */
    float velocity[3];         /* offset 68: of the solid */
    float angular_velocity[3]; /* offset 80: of the solid, about `centre` (radians per unit of time) */
    float restitution;         /* offset 92: in [0, 1] */
    float friction;            /* offset 96: in [0, 1] */
    float margin;              /* offset 100: >= 0 */
    uint32_t reserved[2];      /* offset 104: must be 0 */
} ws_solid;
ws_status ws_collide_solids(ws_handle *h, const ws_solid *s, uint32_t k, uint32_t *out_contacts, double *out_impulse,
                            double *out_angular);

/* ---- solids given as signed-distance volumes: terrain, a hull, a bowl, whatever a mesh tool can voxelise (DESIGN.md 9.9;
 *      no reference counterpart) ----------------------------------------------------------------------------------------
 * A VOLUME is a regular grid of signed distances in the solid's local coordinates, negative inside the solid, that the host
 * uploads once per shape into one of WS_MAX_VOLUMES slots of the handle.  ws_collide_volumes then is ws_collide_solids
 * with the analytic shapes replaced by k POSES (instances) of resident volumes -- several poses may use one slot: the
 * distance is the trilinear interpolant of the grid and the normal is that interpolant's own gradient.
 *
 * ws_volume_upload: node (i, j, k) lies at the local coordinates origin_a + (i, j, k)_a * spacing_a and holds
 * sdf[(k * dims[1] + j) * dims[0] + i] -- x fastest, like ws_sample_density_grid.  The call first waits for the work enqueued
 * so far (an enqueued edit may still be reading the old array), copies the array to the device and replaces whatever the
 * slot held; sdf == NULL releases the slot, and the other arguments are then ignored.  On slab handles the call is LOCAL:
 * no communication; every rank uploads its own copy.  A volume survives ws_reset, ws_write_particles, ws_set_params (a
 * re-grid included) and ws_slab_rebalance; ws_destroy frees it.  A refused upload leaves the slot as it was.
 * Errors: WS_ERR_INVALID_ARG (NULL handle; slot >= WS_MAX_VOLUMES; with a non-NULL sdf: NULL origin, spacing or dims; a dims
 * entry outside 2 .. 1024; more than 2^26 nodes; a spacing that is not finite and > 0; an origin that is not finite; any
 * origin, spacing or extent (dims_a - 1) * spacing_a above 1e15 in magnitude; any sdf value that is not finite or above 1e15
 * in magnitude); WS_ERR_OUT_OF_MEMORY if the allocation fails (the handle stays usable and the slot is EMPTY);
 * WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles); WS_ERR_HIP on an unusable handle.
 *
 * ws_collide_volumes: fl(), dot, the cross product and x * y + z as the solids block defines them; arithmetic is IEEE
 * whatever the handle's flags: every operation is rounded once, sqrt and division are correctly rounded, nothing is
 * contracted.  Per particle, with a RUNNING (p, v), for the poses e = 0 .. k-1 in the order given, with c = centre, R_i =
 * rot[3i .. 3i+2], V = velocity, W = angular_velocity and origin, spacing, dims, sdf those of the pose's slot:
 *   1. q_a = p_a - c_a; l_i = dot(R_i, q).
 *   2. grid coordinate g_a = (l_a - origin_a) / spacing_a.  The particle is IN THE DOMAIN iff 0 <= g_a <= (float)(dims_a - 1)
 *      on all three axes.  Outside the domain the volume says nothing: on to the next pose (a host pads its volume with
 *      positive distances).  Inside: cell i_a = min((uint32_t)g_a, dims_a - 2); fraction f_a = g_a - (float)i_a (exact; f_a
 *      == 1 occurs only on the far face); the corners c_xyz = sdf at node (i_0 + x, i_1 + y, i_2 + z), x, y, z in {0, 1}.
 *      Interpolate along x, then y, then z, keeping the differences:
 *        d_yz = c_1yz - c_0yz,  cx_yz = c_0yz + f_0 * d_yz     (four each);
 *        e_z  = cx_1z - cx_0z,  cy_z  = cx_0z + f_1 * e_z      (two each);
 *        hh   = cy_1 - cy_0,    s     = cy_0 + f_2 * hh.
 *      The gradient of that same interpolant, in local coordinates:
 *        dz_z = d_0z + f_1 * (d_1z - d_0z);
 *        G_0 = (dz_0 + f_2 * (dz_1 - dz_0)) / spacing_0;  G_1 = (e_0 + f_2 * (e_1 - e_0)) / spacing_1;  G_2 = hh / spacing_2.
 *      gg = dot(G, G); m_a = G_a / sqrt(gg) if gg > 0, else m = (0, 1, 0): local up, the sphere's centre rule.
 *      n_a = (m_0 * R_0,a + m_1 * R_1,a) + m_2 * R_2,a.
 *   3. to 6. are ws_collide_solids' steps 3 to 6 unchanged: a contact exists iff s < margin; the push-out p_a = p_a +
 *      (margin - s) * n_a; the response against V + W x r with restitution and friction; the 2^24 fixed-point 64-bit
 *      reaction sums about `centre`, per POSE.
 * After the loop, as there: the container rule for TOUCHED particles; an untouched particle keeps its bits; the predicted
 * position of EVERY particle is recomputed and the state is binned again.  Outputs (k counts, k x 3 impulses, k x 3 angular
 * impulses, each optional), waiting behaviour, WS_FLAG_GRAPH handles, the ws_read_positions_begin / _end window and
 * ws_steps_done: all as ws_collide_solids.
 * Slab handles: COLLECTIVE, by ws_collide_solids' route, the same bits as a single handle.  The verdict is common: if any
 * rank refuses its arguments, or the ranks' poses differ, or the volumes in the slots the poses use differ between ranks
 * (dims, origin, spacing or any byte of the array -- compared by a 64-bit hash taken at upload), ALL return
 * WS_ERR_INVALID_ARG and nothing is changed.
 * Errors: WS_ERR_INVALID_ARG (NULL handle or v; k outside 1 .. WS_MAX_VOLUME_POSES; slot >= WS_MAX_VOLUMES or an EMPTY slot;
 * non-zero flags or reserved; any non-finite value or magnitude above 1e15; restitution or friction outside [0, 1]; margin
 * < 0): nothing is touched and the handle steps on.  `rot` is the host's, as a solid's is.  WS_ERR_UNSUPPORTED
 * (WS_FLAG_REFERENCE_ORDER handles); WS_ERR_HIP on an unusable handle. */
#define WS_MAX_VOLUMES      4u    /* resident volumes (slots) per handle */
#define WS_MAX_VOLUME_POSES 16u   /* instances per call; several may use one slot */
typedef struct ws_volume_pose {   /* 96 bytes */
    uint32_t slot;                /* offset 0: < WS_MAX_VOLUMES, holding a volume */
    uint32_t flags;               /* offset 4: must be 0 */
    float centre[3];              /* offset 8: world position of the volume's local (0, 0, 0); the centre of rotation */
    float rot[9];                 /* offset 20: rows R_0 R_1 R_2 = the local axes in world coordinates, used as given */
    float velocity[3];            /* offset 56: of the solid */
    float angular_velocity[3];    /* offset 68: of the solid, about `centre` (radians per unit of time) */
    float restitution;            /* offset 80: in [0, 1] */
    float friction;               /* offset 84: in [0, 1] */
    float margin;                 /* offset 88: >= 0 */
    uint32_t reserved;            /* offset 92: must be 0 */
} ws_volume_pose;
ws_status ws_volume_upload(ws_handle *h, uint32_t slot, const float origin[3], const float spacing[3],
                           const uint32_t dims[3], const float *sdf);
ws_status ws_collide_volumes(ws_handle *h, const ws_volume_pose *v, uint32_t k, uint32_t *out_contacts,
                             double *out_impulse, double *out_angular);

/* ---- the fluid holding together: surface tension and XSPH velocity smoothing (no reference counterpart) --
 * The first edit that looks at a particle's neighbours.  The model is Akinci, Akinci and Teschner, "Versatile surface
 * tension and adhesion for SPH fluids" (2013) -- a pairwise cohesion spline plus a normal-difference (curvature) term,
 * with the symmetrising density factor -- and Monaghan's XSPH (1989).  ws_read_cohesion is the per-particle stage,
 * read-only; ws_apply_cohesion adds the stage's dv to the velocities of the state the enqueued steps leave, by
 * ws_apply_forces' route.  ws_step itself knows nothing of either.
 * Below fl() is a rounding to float; arithmetic is IEEE whatever the handle's flags, as for the whitewater stage: every
 * operation is rounded once, sqrt and division are correctly rounded, nothing is contracted, sums start at +0 and take
 * their terms in the canonical order.  x, v are what ws_read_positions / ws_read_velocities return; h is the smoothing
 * radius; rho_0 = rest_density, or the handle's target_density when rest_density == 0.
 * Constants, as float operations in this order: h3 = (h*h)*h; h6 = h3*h3; h9 = h6*h3; kc = 32.0f / (3.14159274f * h9);
 *   h664 = h6 * 0.015625f.
 * Candidates of particle i: exactly the whitewater stage's -- those the density sampler's sweep visits around x_i and
 *   accepts: the 27 cells of the clamped cell in increasing linear id, ids ascending inside a cell, e = x_j - x_i,
 *   d2 = dot(e, e) (the whitewater block's dot), rejected iff d2 > d2_accept.  d = sqrt(d2).  A candidate at d == 0 (i
 *   itself, a coincident particle) contributes nothing to pass B.
 * Pass A, per particle: (rho_i, g_i) = the density and gradient ws_sample_density_points returns at x_i in its
 *   WS_FLAG_IEEE_DIVISION form (rho_i includes i's own term, so rho_i > 0);  n_i,a = (h * g_i,a) / rho_i -- a
 *   dimensionless normal that points into the fluid, about 1 at a free surface and about 0 in the bulk.
 * Pass B, with A = X = (+0, +0, +0) and c_i = 0, per contributing candidate j (d > 0), in order:
 *    1. xh_a = (-e_a) / d                                   (the unit vector from j to i)
 *    2. q = 2.0f / (rho_i + rho_j)
 *    3. K = rho_0 * q
 *    4. t = h - d
 *    5. t3 = (t*t)*t
 *    6. d3 = (d*d)*d
 *    7. pp = t3*d3
 *    8. s = pp if 2.0f*d > h, else s = 2.0f*pp - h664
 *    9. C = kc * s                                          (Akinci's spline: attraction beyond about h/3, repulsion closer)
 *   10. fc = cohesion * C
 *   11. T_a = fc * xh_a + curvature * (n_i,a - n_j,a)       (each product rounded, then the sum)
 *   12. A_a = A_a - K * T_a
 *   13. w = the density sampler's term at d, (h - d)^2 * pow2, the same bits
 *   14. X_a = X_a + ((v_j,a - v_i,a) * w) * q
 *   15. c_i += 1
 * After the sweep: if c_i == 0 the particle is UNAFFECTED and dv = (+0, +0, +0); otherwise dv_a = dt * A_a + xsph * X_a
 *   (each product rounded, then the sum).
 * ws_read_cohesion: the stage, n entries in ORIGINAL-ID order, with every convention of ws_read_whitewater.  Outputs, any
 *   of which may be NULL (all NULL: WS_ERR_INVALID_ARG on a single handle, contribute-only on a slab): out_normal n*3 (n_i),
 *   out_density n (rho_i), out_dv n*3, out_neighbours n (c_i).  It waits for enqueued steps, writes nothing ws_step reads
 *   and keeps its scratch in the sampler's.  Slab handles: COLLECTIVE on the gathered {position, velocity} set, the same
 *   bits as a single handle; a rank that passes every output NULL only contributes; a rank validates its arguments after
 *   the gather.
 * ws_apply_cohesion: an affected particle (c_i > 0) gets v'_a = v_a + dv_a; an unaffected particle keeps its velocity bit
 *   for bit (a -0 stays -0).  Positions do not change.  The predicted position of EVERY particle is recomputed by the
 *   library's own rule and the state is binned again, as after ws_apply_forces.  out_affected, if not NULL, receives ONE
 *   count: the particles with c_i > 0 (on slabs the global count).  Everything else is ws_apply_forces' contract:
 *   ws_steps_done is unchanged; the 80-byte view keeps the last step's density, pressure and acceleration; a WS_FLAG_GRAPH
 *   handle keeps replaying its captured step; the call may be made between ws_read_positions_begin and _end; slab handles
 *   take the gather / common verdict / reload route, with p and dt in the agreement -- ranks whose arguments differ, or
 *   any of which refuses, ALL return WS_ERR_INVALID_ARG and nothing is changed.
 * Errors, with nothing touched: WS_ERR_INVALID_ARG (NULL handle or p; a non-zero reserved; any non-finite value or any
 *   magnitude above 1e15; cohesion, curvature or rest_density < 0; xsph outside [0, 1]; dt not > 0; ws_read_cohesion:
 *   every output NULL on a single handle); WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles); WS_ERR_OUT_OF_MEMORY
 *   (scratch cannot grow: the handle stays usable); WS_ERR_HIP on an unusable handle.  Whether a strength is stable at the
 *   host's dt is the host's business, as a huge emitter strength is. */
typedef struct ws_cohesion_params {   /* 20 bytes */
    float cohesion;       /* offset 0:  gamma_c >= 0, the pairwise attraction                      */
    float curvature;      /* offset 4:  gamma_n >= 0, the normal-difference (area-minimising) term */
    float xsph;           /* offset 8:  epsilon in [0, 1]                                          */
    float rest_density;   /* offset 12: rho_0; 0 = the handle's target_density (as ws_body_params) */
    uint32_t reserved;    /* offset 16: must be 0                                                  */
} ws_cohesion_params;
/* Host-only (no device needed; WS_ERR_INVALID_ARG for NULL): 1, 1, 0.1, 0, 0. */
ws_status ws_default_cohesion_params(ws_cohesion_params *out);
ws_status ws_read_cohesion(ws_handle *h, const ws_cohesion_params *p, float dt, float *out_normal, float *out_density,
                           float *out_dv, uint32_t *out_neighbours);
ws_status ws_apply_cohesion(ws_handle *h, const ws_cohesion_params *p, float dt, uint32_t *out_affected);

/* ---- what the fluid carries: per-particle attributes -- paint, mix and sample them (no reference
 *      counterpart) ----------------------------------------------------------------------------------------------------
 * Every particle carries one ATTRIBUTE A = (A_0, A_1, A_2, A_3), four floats whose meaning is the host's (RGB dye plus a
 * temperature, four dyes, ...).  The handle keeps them on the device in ORIGINAL-ID order; nothing of a particle's physics
 * reads them.  The array is allocated by the first attribute call, all +0, and freed by ws_destroy.  ws_reset returns it
 * to +0; ws_write_particles, ws_set_params (a re-grid included), ws_slab_rebalance and every step leave it alone.
 * Below fl() is a rounding to float; arithmetic is IEEE whatever the handle's flags, except where the field says
 * otherwise: every operation is rounded once, sqrt and division are correctly rounded, nothing is contracted, sums start
 * at +0 and take their terms in the canonical order; dot is the whitewater block's; x is what ws_read_positions returns.
 * ws_write_attributes: n*4 floats by id, used as given (a NaN spreads as it would in the host's own arithmetic); NULL =
 *   all +0.  ws_read_attributes: n*4 floats by id; a handle that never made an attribute call reads all +0.
 * ws_paint_attributes, per particle, for the brushes e = 0 .. k-1 in the order given, on the RUNNING value of A:
 *    1. q_a = x_a - c_a; d = sqrt(dot(q, q)).  If !(d < R) go on to the next brush; otherwise the particle is PAINTED by e
 *       and n_e += 1.
 *    2. t = d / R; w = 1 - falloff * t; s = strength * w.
 *    3. For every channel c in `channels`:
 *         MIX: A_c = fl(fl(1 - s) * A_c) + fl(s * value_c)    (strength 1, falloff 0: a finite A_c becomes value_c exactly)
 *         ADD: A_c = A_c + fl(s * value_c)
 *   A particle no brush reaches keeps its four floats bit for bit; channels outside the mask keep theirs.  out_painted,
 *   if not NULL, receives the k counts n_e.
 * ws_diffuse_attributes: a kernel-weighted exchange between neighbours -- XSPH's form (Monaghan 1989) applied to A, NOT a
 *   Laplacian with a physical diffusivity: the spiky kernel's W'(d)/d is unbounded for close pairs, so an explicit
 *   Laplacian step would not be stable at the host's dt.  r_c = fl(rate_c * dt).
 *   Candidates of particle i: exactly the cohesion stage's -- the 27 cells of the clamped cell in increasing linear id,
 *   ids ascending inside a cell, e = x_j - x_i, d2 = dot(e, e), rejected iff d2 > d2_accept.  d = sqrt(d2).  A candidate
 *   at d == 0 (i itself, a coincident particle) contributes nothing.
 *   Pass A, once per call: rho_i = the density ws_sample_density_points returns at x_i in its WS_FLAG_IEEE_DIVISION form
 *   -- the cohesion pass A's rho_i, the same bits.
 *   Pass B, run `iterations` times, every particle reading the A of the previous iteration.  With S = (+0, +0, +0, +0) and
 *   c_i = 0, per contributing candidate j (d > 0), in order:
 *    1. q = 2.0f / (rho_i + rho_j)
 *    2. w = the density sampler's term at d, (h - d)^2 * pow2, the same bits
 *    3. g = w * q
 *    4. S_c = S_c + (A_j,c - A_i,c) * g
 *    5. c_i += 1
 *   After the sweep: if c_i == 0 the particle is UNAFFECTED and keeps its bits; otherwise A'_c = A_c + r_c * S_c (the
 *   product rounded, then the sum) for every channel with rate_c != 0, and a channel with rate_c == 0 keeps its bits.
 *   out_affected, if not NULL, receives ONE count: the particles with c_i > 0.  A call with iterations = k equals k calls
 *   with iterations = 1 bit for bit; it bins and runs pass A once.
 *   Two properties follow.  g_ij and g_ji are the same bits and the differences are exact negatives, so sum_i A_i changes
 *   only by the rounding of the particles' own sums.  And sum_{j != i} g_ij < 2, because q < 2 / rho_i and sum w <= rho_i:
 *   with r_c <= 0.5 every A'_i,c is a convex combination of values in i's neighbourhood in exact arithmetic, which is why
 *   r_c > 0.5 is refused.
 * ws_sample_attribute_grid / _points: at a node or point exactly ws_sample_velocity_grid / _points with A_j (four
 *   channels) in place of v_j: per accepted candidate w = the density sampler's term, rho += w, M_c += fl(w * A_j,c);
 *   value_c = M_c / rho, correctly rounded, where rho > 0, +0 elsewhere.  Only the sqrt inside w follows
 *   WS_FLAG_IEEE_DIVISION.  out_value: 4 floats per node (nodes x fastest) or point; out_density is bit-identical to
 *   ws_sample_density_* for the same query; grid and points calls return the same bits at the same place.  Either output
 *   may be NULL, not both on a single handle.  The typical use: sample at the out_xyz of ws_extract_surface to colour the
 *   mesh.
 * Every call waits for enqueued steps, writes nothing ws_step reads and leaves ws_steps_done unchanged; it may be made
 * between ws_read_positions_begin and _end; a WS_FLAG_GRAPH handle keeps replaying its captured step.  The binning is
 * recomputed from the current positions on every call that needs neighbours; scratch lives in the sampler's (grow-only).
 * Slab handles: every call is COLLECTIVE, with the same arguments on every rank.  The attribute array is replicated --
 *   n_global * 16 bytes on every rank, by global id -- positions come from the gather the field calls make, and every rank
 *   computes the definition on the global set, so the bits are a single handle's.  A rank that passes every output NULL
 *   only contributes (and still keeps its replica current).  The verdict of the calls that change A is common: arguments
 *   are validated after the gather and compared across ranks (ws_write_attributes: a hash of the array); if ranks differ,
 *   or any rank refuses, ALL return WS_ERR_INVALID_ARG and nothing changes.
 * Errors, with nothing touched: WS_ERR_INVALID_ARG (a NULL handle, b or p; k outside 1 .. WS_MAX_BRUSHES; a kind above 1;
 *   channels 0 or above 15; a non-finite value or a magnitude above 1e15 in a brush or in p; radius not > 0; falloff
 *   outside [0, 1]; a MIX strength outside [0, 1]; a rate below 0; dt not finite or not > 0; any r_c > 0.5; iterations
 *   outside 1 .. 64; a non-zero reserved; NULL out of ws_read_attributes on a single handle; the density sampler's query
 *   errors for the two field calls); WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles); WS_ERR_OUT_OF_MEMORY (the
 *   handle stays usable); WS_ERR_HIP on an unusable handle. */
#define WS_MAX_BRUSHES 16u
#define WS_BRUSH_MIX 0u
#define WS_BRUSH_ADD 1u
typedef struct ws_brush {        /* 48 bytes */
    uint32_t kind;               /* offset 0:  WS_BRUSH_MIX or WS_BRUSH_ADD */
    float centre[3];             /* 4  */
    float radius;                /* 16: R > 0; a particle is in reach iff d < R */
    float falloff;               /* 20: in [0, 1]: 0 = hard edge, 1 = linear to zero at the rim */
    float strength;              /* 24: MIX: in [0, 1]; ADD: any finite */
    uint32_t channels;           /* 28: bit c set = channel c is painted; 1 .. 15 */
    float value[4];              /* 32 */
} ws_brush;
typedef struct ws_diffuse_params {   /* 24 bytes */
    float rate[4];               /* offset 0: per channel, 1 / time, >= 0; 0 = the channel keeps its bits */
    uint32_t iterations;         /* 16: 1 .. 64 */
    uint32_t reserved;           /* 20: must be 0 */
} ws_diffuse_params;
/* Host-only (no device needed; WS_ERR_INVALID_ARG for NULL): rate 1, 1, 1, 1; iterations 1; reserved 0. */
ws_status ws_default_diffuse_params(ws_diffuse_params *out);
ws_status ws_write_attributes(ws_handle *h, const float *in);
ws_status ws_read_attributes(ws_handle *h, float *out);
ws_status ws_paint_attributes(ws_handle *h, const ws_brush *b, uint32_t k, uint32_t *out_painted);
ws_status ws_diffuse_attributes(ws_handle *h, const ws_diffuse_params *p, float dt, uint32_t *out_affected);
ws_status ws_sample_attribute_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                   float *out_value, float *out_density);
ws_status ws_sample_attribute_points(ws_handle *h, const float *xyz, uint32_t m, float *out_value, float *out_density);

/* ---- the fluid acting on things that float in it: buoyancy and drag on host-owned bodies (no reference
 *      counterpart) ----------------------------------------------------------------------------------------------------
 * One-way coupling, water to body.  The HOST owns the bodies, as it owns whitewater's diffuse particles: it describes each
 * body by sample points (position p_s, material velocity w_s -- from the body's linear and angular velocity -- and the
 * share V_s of the body's volume the sample stands for), gets one force and one torque per body back, and integrates the
 * bodies itself.  The library keeps nothing between calls and ws_step is not touched; a host that wants the body to shove
 * water aside puts a WS_FORCE_RADIAL emitter at it with ws_apply_forces, or makes it a solid with ws_collide_solids.
 * m samples in all, grouped by body: body b owns the samples body_start[b] .. body_start[b+1]-1 (nb + 1 entries,
 * non-decreasing, body_start[0] == 0, body_start[nb] == m; an empty body is allowed).  body_centre: nb*3 floats, the point
 * c_b the torque of body b is taken about.
 * Below fl() is a rounding to float; every operation is rounded once, nothing is contracted, and division is correctly
 * rounded whatever the handle's flags -- only the field itself follows WS_FLAG_IEEE_DIVISION (ws_step_whitewater's split).
 * Per sample, independently of every other sample:
 *   1. (u, rho) = the field at p_s exactly as ws_sample_velocity_points defines it, in the HANDLE's arithmetic; g = the
 *      handle's gravity; rho_0 = rest_density, or the handle's target_density when rest_density == 0.
 *   2. If !(rho > 0) the sample is DRY: f = +0, vol = +0, F = T = (+0, +0, +0), wet = 0.
 *   3. Otherwise it is WET: f = fminf(rho / rho_0, 1.0f); vol = fl(V_s * f); lift = fl(fluid_density * vol);
 *      kd = fl(drag * vol); per axis F_a = fl(fl(kd * fl(u_a - w_a)) - fl(lift * g_a)); wet = 1.
 *   4. (wet samples) r_a = fl(p_a - c_b,a); T_x = fl(fl(r_y * F_z) - fl(r_z * F_y)), and cyclically for T_y and T_z.
 * Per body, the CANONICAL SUM of each of the seven floats F (3), T (3) and vol: a fixed binary tree over the body's c
 * samples in the order given.  With P the smallest power of two > c, the leaves are t_0 .. t_{c-1} followed by +0 up to
 * P; every level computes v[i] = fl(v[2i] + v[2i+1]) until one value is left.  An empty body gives +0.  Consequences: at
 * least one +0 leaf always enters, so no per-body output is ever -0; and padding further with +0 changes no bit, so the
 * library is free to sum a fixed number of levels per pass.  The wet count is an integer sum.  The order is part of the
 * contract: the results are bit-identical across launch shapes, slab counts and WS_FLAG_GRAPH, and a host that repeats
 * the arithmetic above on ws_sample_velocity_points' output gets the same bits, in either arithmetic of the handle.
 * Outputs, any of which may be NULL (all NULL: WS_ERR_INVALID_ARG on a single handle, contribute-only on a slab):
 *   out_force, out_torque nb*3 (the sums of F and T), out_volume nb (the submerged volume), out_wet nb (wet samples),
 *   out_sample_force m*3 (F per sample), out_sample_fraction m (f per sample).
 * The call waits for enqueued steps, writes nothing ws_step reads, recomputes the sampler's binning from the current state
 * on every call and keeps its scratch in the sampler's (grow-only, freed by ws_destroy, allocated on the first body call
 * only).  It may be made between ws_read_positions_begin and _end; ws_steps_done is unchanged.
 * Slab handles: COLLECTIVE on the gathered global {position, velocity} set, the same bits as a single handle; a rank that
 * passes every output NULL only contributes, and a rank validates its arguments only after the gather, so a refused rank
 * leaves no peer waiting.
 * Errors: WS_ERR_INVALID_ARG (NULL handle, p, sample_xyz, sample_velocity, sample_volume, body_start or body_centre; every
 *   output NULL on a single handle; m == 0 or more than 2^28; nb == 0 or more than 2^24; a body_start that does not start
 *   at 0, does not end at m or decreases; a non-finite value or a magnitude above 1e15 in any input array; a negative
 *   volume; fluid_density, drag or rest_density not finite or negative; a non-zero reserved): nothing is written;
 *   WS_ERR_UNSUPPORTED (WS_FLAG_REFERENCE_ORDER handles); WS_ERR_OUT_OF_MEMORY (scratch allocation failed: the handle
 *   stays usable); WS_ERR_HIP on an unusable handle. */
typedef struct ws_body_params {   /* 16 bytes */
    float fluid_density;          /* offset 0: lift per unit of submerged volume, in units of -gravity (Archimedes); finite, >= 0 */
    float drag;                   /* 4: force per unit of submerged volume and of (u - w); finite, >= 0 */
    float rest_density;           /* 8: field density at which a sample counts as fully submerged; 0 = the handle's target_density */
    uint32_t reserved;            /* 12: must be 0 */
} ws_body_params;
/* Host-only (no device needed; WS_ERR_INVALID_ARG for NULL): fluid_density 1000 (water, SI), drag 500 (half of it: a unit of
 * relative velocity pulls half as hard as a unit of -gravity lifts), rest_density 0 (the handle's target_density). */
ws_status ws_default_body_params(ws_body_params *out);
ws_status ws_body_forces(ws_handle *h, const ws_body_params *p, const float *sample_xyz, const float *sample_velocity,
                         const float *sample_volume, uint32_t m, const uint32_t *body_start, const float *body_centre,
                         uint32_t nb, float *out_force, float *out_torque, float *out_volume, uint32_t *out_wet,
                         float *out_sample_force, float *out_sample_fraction);

/* ---- pouring water in and draining it: the particle count as a variable (no reference counterpart) -----
 * ws_create fixes a handle's particle count n and its CAPACITY, the particles its arrays hold, at the same value.  The
 * three count-changing calls below add particles at the end of the id range or remove some and renumber the rest, on the
 * device, between two steps: stream-ordered after the steps enqueued so far, before the next ws_step, and SYNCHRONOUS --
 * each returns with the new count visible in ws_num_particles (a removal waits for one 4-byte readback, the survivor
 * count, next to the per-sink counts; an addition may wait too).  x, v are what ws_read_positions / ws_read_velocities
 * return; fl() is a rounding to float; arithmetic is IEEE whatever the handle's flags: every operation is rounded once,
 * sqrt is correctly rounded, nothing is contracted; dot() is ws_apply_forces'.
 * ws_remove_particles, per particle, for the sinks e = 0 .. k-1 in the order given (c = centre):
 *   1. q_a = x_a - c_a.  WS_SINK_SPHERE contains the particle iff d < R with d = sqrt(dot(q, q)) and R = half[0] -- step 1
 *      of ws_apply_forces, operation for operation.  WS_SINK_BOX contains it iff fabsf(q_a) <= half_a on all three axes (a
 *      particle exactly on a face is inside; one at d == R of a sphere is outside).  A particle with a NaN coordinate is
 *      contained by nothing and stays.
 *   2. The FIRST sink that contains the particle claims it: n_e += 1 for that sink alone, and the particle is removed.
 *   out_removed, if not NULL, receives the k counts n_e.
 * ws_remove_particle_ids removes the m particles named in ids; an id may be named more than once and counts once.
 * Renumbering, for both: ids stay dense.  A survivor's new id is its rank among the survivors by old id; its position and
 * velocity keep their bits and its four attributes move with it.  out_new_id, if not NULL, receives n words (n = the count
 * BEFORE the call): out_new_id[old id] = new id, or 0xFFFFFFFF for a removed particle, so that a host can remap its own
 * per-particle data.
 * ws_add_particles: the m new particles get the ids n .. n+m-1 in the order given, position and velocity as given (vel_xyz
 * == NULL: at rest, +0) and the attributes of attr (m*4 floats), or +0 with attr == NULL.  With attr given on a handle whose
 * attribute array does not exist yet, the array is created and every old particle's attributes are +0.
 * A count change is an EDIT: afterwards the predicted position of EVERY particle is the library's own rule, pred_a =
 * fl(x_a + fl(v_a * 0.02f)), exactly as after ws_apply_forces -- predictions a preceding ws_write_particles supplied are
 * dropped, as any edit drops them.  The views of the LAST STEP's fields behave between the count change and the next
 * ws_step as they do between ws_write_particles and the next ws_step (ws_read_particles: zero density, pressure and
 * acceleration; ws_read_sort_view: the identity), but ws_steps_done keeps counting.  The next step hashes with the NEW
 * count (the reference's num_particles in hash_cell), and is bit for bit the step of a fresh handle created at the new
 * count and loaded, with ws_write_particles, with the records ws_read_particles returns after the change.  A captured
 * step (WS_FLAG_GRAPH) is dropped and captured again; with WS_FLAG_PROFILE a count change counts one WS_K_BIN launch.
 * NO-OPS -- m == 0 on the two calls that take m, and a ws_remove_particles whose sinks claim nothing -- return WS_OK and
 * leave the handle exactly as it was: the last-step views stay valid, a captured step is kept, nothing is binned again.
 * The no-op removal still writes its outputs: all counts 0, the id map the identity.
 * A removal that would leave NO particle is WS_ERR_INVALID_ARG: decided after the scan and before anything is moved, the
 * handle and the outputs untouched.
 * Capacity: ws_reserve_particles raises it to at least `capacity` and never lowers it (state, views and results are
 * unchanged; a captured step is captured again).  An addition beyond the capacity grows it to n' + n'/2 for the new count
 * n', capped at 2^27 - 16, the largest count ws_create accepts; the new arrays are allocated before the old ones are given
 * up, so a failure is WS_ERR_OUT_OF_MEMORY with state and count as they were.  An addition within the capacity allocates no
 * particle array.  Removals never shrink it.  ws_particle_capacity answers on every handle (a slab: the owned capacity; a
 * NULL handle: 0).
 * Slab handles are OUT OF SCOPE of these calls: ids and attributes are replicated on every rank, so a count change would
 * have to be collective.  They, and WS_FLAG_REFERENCE_ORDER handles, return WS_ERR_UNSUPPORTED from the three
 * count-changing calls and from ws_reserve_particles.
 * Errors: WS_ERR_INVALID_ARG, with nothing touched -- a NULL handle; a ws_read_positions_begin in flight (call
 * ws_read_positions_end first); sinks: s NULL, k outside 1 .. WS_MAX_SINKS, a kind > 1, a non-zero reserved word, a
 * non-finite centre or half or a magnitude above 1e15, a box half extent or sphere radius not > 0, a sphere with half[1]
 * or half[2] not 0; ids: NULL with m > 0, an id >= n (checked on the host); an addition: pos_xyz NULL with m > 0, any
 * float of pos_xyz, vel_xyz or attr not finite or above 1e15 in magnitude, a count beyond 2^27 - 16; a removal that would
 * empty the handle; ws_reserve_particles beyond 2^27 - 16.  WS_ERR_UNSUPPORTED as above.  WS_ERR_OUT_OF_MEMORY (growth or
 * scratch: the handle stays usable, unless the cell tables of the new count could not be rebuilt after the old ones were
 * given up: then the handle is unusable, as after a failed re-grid).  WS_ERR_HIP on an unusable handle. */
#define WS_MAX_SINKS 16u
enum { WS_SINK_SPHERE = 0, WS_SINK_BOX = 1 };
typedef struct ws_sink {      /* 32 bytes */
    uint32_t kind;            /* offset 0: WS_SINK_* */
    uint32_t reserved;        /* 4: must be 0 */
    float centre[3];          /* 8 */
    float half[3];            /* 20: box: half extents, each > 0.  sphere: half[0] = radius > 0, half[1] = half[2] = 0 */
} ws_sink;
ws_status ws_reserve_particles(ws_handle *h, uint32_t capacity);
uint32_t ws_particle_capacity(ws_handle *h);
ws_status ws_add_particles(ws_handle *h, const float *pos_xyz, const float *vel_xyz, const float *attr, uint32_t m);
ws_status ws_remove_particles(ws_handle *h, const ws_sink *s, uint32_t k, uint32_t *out_removed, uint32_t *out_new_id);
ws_status ws_remove_particle_ids(ws_handle *h, const uint32_t *ids, uint32_t m, uint32_t *out_new_id);

/* ---- gauges: measure and select the fluid inside regions (no reference counterpart) ---------------------
 * How much water is in the bucket, how fast does it flow through the gate, where is its centre of mass, how high does it
 * stand, what is the largest speed, which particles did the player lasso -- answered on the device, for up to
 * WS_MAX_REGIONS regions in one pass over the particle records, instead of through ws_read_particles and a host loop.
 * A REGION is a ws_sink by another name: the same 32 bytes, the same validation and the same containment as step 1 of
 * ws_remove_particles.  x, v are what ws_read_positions / ws_read_velocities return; arithmetic is IEEE whatever the
 * handle's flags: every operation is rounded once, sqrt is correctly rounded, nothing is contracted; dot() and the cross
 * product are ws_apply_forces'.
 * ws_measure, per region e = 0 .. k-1 (c = centre) and per particle:
 *   Containment.  q_a = x_a - c_a.  A sphere contains the particle iff d < R with d = sqrt(dot(q, q)), R = half[0]; a box
 *     iff fabsf(q_a) <= half_a on all three axes -- ws_remove_particles step 1 operation for operation (on a face: inside;
 *     at d == R: outside; a NaN coordinate: contained by nothing).  Every region is independent: a particle counts in
 *     EVERY region that contains it, there is no first claim.
 *   Sums.  count += 1.  Each float t enters a sum as the 64-bit integer llrintf(fminf(fmaxf(t, -0x1p31f), 0x1p31f) *
 *     0x1p24f) -- step 6 of ws_collide_solids -- and the sums wrap modulo 2^64, so they depend on no order.  Per contained
 *     particle: x_a into sum_pos[a]; v_a into sum_vel[a]; the three components of q x v (q is containment's own value:
 *     x = fl(fl(q_y*v_z) - fl(q_z*v_y)) and cyclically) into sum_ang[a]; dot(v, v) into sum_speed2; and with
 *     WS_GAUGE_ATTRIBUTES on a handle that has attributes, the particle's four attribute floats into sum_attr[c] (else
 *     sum_attr stays 0).  The host divides by 2^24, and by count for a mean.  A sum is free of wrap as long as the
 *     magnitudes it adds up stay below 2^39 in total (2^63 / 2^24); a term beyond 2^31 in magnitude enters as 2^31.
 *   Extremes.  min_pos[a], max_pos[a] over x_a and max_speed2 over dot(v, v) are taken under the TOTAL order of the key
 *     bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) of a float's bits, so that -0 < +0 and the result depends on no visit
 *     order.  max_speed2 starts from +0 and skips a NaN, as fmaxf does.
 *   An EMPTY region: count 0, every sum 0, min_pos = +inf, max_pos = -inf, max_speed2 = +0.  reserved is written 0.
 * The call is stream-ordered after the steps enqueued so far and SYNCHRONOUS: it waits for its k * 152 bytes.  It is
 * READ-ONLY: nothing is binned again, the predicted positions and the last step's views stay as they are, a captured step
 * (WS_FLAG_GRAPH) is kept, ws_steps_done does not move, and with WS_FLAG_PROFILE no launch is counted under any WS_K_* id.
 * It is allowed between ws_read_positions_begin and _end on a single-GPU handle (a slab handle's gather refuses there, as
 * for every collective read).
 * Slab handles: COLLECTIVE, by the velocity field's route (one gather of {position, velocity} by id); every rank measures
 * the global set, attributes are replicated by id already, and every rank that passes out gets the single handle's bits
 * (out may be NULL on a slab handle: this rank only contributes).  The verdict on the arguments is common, as in
 * ws_collide_solids: ranks that refuse, or that were given different regions or flags, ALL return WS_ERR_INVALID_ARG.
 * ws_select_particles: the ids of the particles that AT LEAST ONE of the k regions contains, in ascending id order.
 * *out_total = how many there are; the first min(total, cap) are written to out_ids, which may be NULL with cap == 0 (a
 * count only).  Read-only in the sense above, synchronous (the count is read back, then the min(total, cap) ids).  The list feeds
 * ws_remove_particle_ids and a host's own per-particle data.  Single-GPU handles only: slab handles return
 * WS_ERR_UNSUPPORTED.
 * Errors, both calls: WS_ERR_INVALID_ARG with nothing written -- NULL h, r or out (single-GPU handles); k outside 1 ..
 * WS_MAX_REGIONS; flag bits other than bit 0; every refusal ws_remove_particles has for a sink (a kind > 1, a non-zero
 * reserved word, a non-finite centre or half or a magnitude above 1e15, a box half extent or sphere radius not > 0, a
 * sphere with half[1] or half[2] not 0); ws_select_particles also: out_total NULL, out_ids NULL with cap > 0.
 * WS_ERR_UNSUPPORTED on WS_FLAG_REFERENCE_ORDER handles.  WS_ERR_OUT_OF_MEMORY (scratch: the handle stays usable).
 * WS_ERR_HIP on an unusable handle.
 * Left out: density or pressure sums (they need the last step's sorted copy), oriented regions, an asynchronous form,
 * ws_select_particles on slab handles, one id list per region. */
typedef ws_sink ws_region;            /* the same 32 bytes, validation and containment as ws_remove_particles step 1 */
#define WS_MAX_REGIONS 16u
#define WS_GAUGE_ATTRIBUTES 1u        /* flags bit 0: also sum the four attributes (a gather by id) */
typedef struct ws_gauge {             /* 152 bytes */
    uint64_t count;                   /* offset 0 */
    int64_t  sum_pos[3];              /* 8: fixed point, 2^-24 */
    int64_t  sum_vel[3];              /* 32 */
    int64_t  sum_ang[3];              /* 56: q x v, q = x - the region's centre */
    int64_t  sum_speed2;              /* 80: dot(v, v) */
    int64_t  sum_attr[4];             /* 88: 0 unless WS_GAUGE_ATTRIBUTES and the handle has attributes */
    float    min_pos[3];              /* 120 */
    float    max_pos[3];              /* 132 */
    float    max_speed2;              /* 144 */
    uint32_t reserved;                /* 148: written 0 */
} ws_gauge;
ws_status ws_measure(ws_handle *h, const ws_region *r, uint32_t k, uint32_t flags, ws_gauge *out);
ws_status ws_select_particles(ws_handle *h, const ws_region *r, uint32_t k, uint32_t cap, uint32_t *out_ids, uint32_t *out_total);

/* ---- introspection ------------------------------------------------------------- */
const char *ws_last_error(ws_handle *h);
uint32_t ws_num_particles(ws_handle *h);
uint64_t ws_steps_done(ws_handle *h);

/* Kernel ids for ws_profile_read (stable; names via ws_kernel_name). */
enum {
    WS_K_SCAN = 0,     /* cell-count exclusive scan (one launch per step)       */
    WS_K_SCATTER = 1,  /* slot assignment inside each cell                      */
    WS_K_REORDER = 2,  /* stable in-cell order + physical SoA reorder           */
    WS_K_DENSITY = 3,  /* K4 update_density                                     */
    WS_K_FORCE = 4,    /* K5 update_pressure_force + K6 integrate + next K1 bin */
    WS_K_BIN = 5,      /* stand-alone cell binning (first step after upload)    */
    WS_K_COUNT = 6
};
const char *ws_kernel_name(uint32_t kernel_id);
/* With WS_FLAG_PROFILE: total milliseconds and launch count per kernel id since the
 * last ws_profile_reset, measured with HIP events on the handle's own stream.  Waits
 * for enqueued steps.  Scan, scatter, reorder and bin are timed by an event pair recorded
 * around the launch, K4 and K5 by events the launch itself carries.  A step counts one
 * launch per kernel id: a slab step that runs K4 and K5 as an early and a late range
 * contributes ONE launch and the SUM of its two ranges' times.  WS_K_BIN counts the
 * stand-alone binning of ws_create, ws_reset, ws_write_particles and a ws_set_params that
 * re-grids on a single-GPU handle, and every count change (ws_add_particles, ws_remove_particles,
 * ws_remove_particle_ids).  A WS_FLAG_GRAPH handle records nothing: all zeros.
 * Either output pointer may be NULL; kernel_id >= WS_K_COUNT is WS_ERR_INVALID_ARG. */
ws_status ws_profile_read(ws_handle *h, uint32_t kernel_id, double *total_ms, uint64_t *launches);
ws_status ws_profile_reset(ws_handle *h);
/* Restrict WS_FLAG_PROFILE's events to the kernel ids whose bit is set in mask (default: all),
 * so that a timed region carries two events per step instead of two per kernel. */
ws_status ws_profile_select(ws_handle *h, uint32_t kernel_mask);
/* out[0] = cumulative particle-steps with more candidates than the accept mask holds (their waves took the full
 * sweep in the force kernel); out[1..3] = how many of the reference's cells (edge = smoothing radius) one cell of the
 * device grid spans along x, y, z -- 1 unless the reference-sized grid would exceed the cell budget (a small
 * smoothing radius in a big container), see ws_grid_dims; out[4] = steps replayed from a captured hipGraph
 * (WS_FLAG_GRAPH); slab handles: out[5] = the most particles one of this slab's boundary layers has held since the last
 * load and out[6] = the halo capacity it must stay under (ws_device_cfg.ghost_capacity), out[7] = the most particles
 * that left towards one neighbour in one step and out[8] = the migration message's capacity, out[9] = the most that crossed
 * more than one slab towards ONE destination rank in one step and out[10] = the capacity of a far message (one per destination); out[11..13] = the records the migration, halo
 * and far messages carry: with exact sizes (the default) what the LAST step's carried, with WS_FLAG_LAGGED_MESSAGES what
 * the NEXT step's will (sized from what every rank reported a few steps ago; the capacities with
 * WS_FLAG_FIXED_MESSAGES); 0 without peers; out[14] = how often ws_step has waited for message sizes so far (two per
 * step with exact sizes, never with WS_FLAG_LAGGED_MESSAGES); out[15] = 1 when the cost-guided tile schedule drives the
 * neighbour kernels (single-GPU handles of 2^18 <= n < 2^20 particles, not in a captured step: DESIGN.md 3). */
ws_status ws_read_stats(ws_handle *h, uint32_t out[16]);
/* Device cell grid actually in use (cells along x,y,z incl. padding).  The reference's N-bucket hashed table has the
 * same size for every smoothing radius (assets/simulation.wgsl:125-128); a dense grid does not, so when
 * container volume / h^3 exceeds the cell budget (max(16 N, 2^24) cells) the library merges cells along z, then y,
 * then x.  Results are unaffected (cell edges stay >= h; the distance test decides); no radius the reference accepts
 * makes ws_create / ws_set_params run out of table memory. */
ws_status ws_grid_dims(ws_handle *h, uint32_t dims[3]);

#ifdef __cplusplus
}
#endif
#endif
