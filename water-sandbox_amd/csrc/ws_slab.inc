// ws_slab.inc -- multi-GPU: one handle = one x-slab (included at the end of ws_api.cpp, same
// translation unit, so it shares its helpers).  The reference is a single-GPU desktop app
// (SURVEY.md section 2: no multi-device code); this is the scale-out row 8(e): 1-D slabs along x,
// one-cell halo from each x-neighbour, data moved by the host's transport (RCCL send/recv with
// the two neighbours + one all-to-all of per-destination messages for particles that cross several slabs in a step).
//
// Sorted-array layout of a slab (x is the slowest cell axis, so layers are contiguous ranges):
//     [ .. unused .. | left ghosts (gL) | owned particles (n) | right ghosts (gR) | .. ]
//                                        ^ base = ghost capacity (fixed)
// Local cell grid: layer 0 = left ghost layer, layers 1 .. nxl-2 = owned, layer nxl-1 = right ghost
// layer; y and z extents are the global ones, so a neighbour's boundary layer arrives already in
// this slab's cell order and only its cell-start slice has to be rebased (k_halo_unpack).
//
// ws_step on a slab never waits for the device.  Every data-dependent number of the step -- the owned count
// after migration, the boundary-layer ranges, ghost and migration counts -- stays on the device (`dyn`, message
// headers); messages have FIXED capacities known to both ends (ghost_capacity, mig_cap, far_cap), kernels are
// launched over host-side upper bounds.  The host learns the owned count and the error bits of every rank two
// steps late (a 4-slot pinned ring filled by asynchronous copies): enough to tighten the launch bounds and to fail
// ws_step on ALL ranks alike when any rank overran a capacity -- no rank ever leaves a collective alone.

namespace {

constexpr uint32_t kStatusLag = 2;    // ws_step t reads the status table written by step t - kStatusLag
constexpr uint32_t kStatusSlots = 4;  // > kStatusLag

// A transport call that fails leaves the step half enqueued on this rank and the other ranks inside (or in front of)
// the matching call: there is nothing to resume.  The handle is dead from here on -- every later ws_step returns
// WS_ERR_COMM at once instead of enqueuing on top of the wreck; the host tears the job down.
ws_status slab_fail_tr(ws_handle *h, const char *what, int rc)
{
    char buf[160];
    if (h->slab->capturing) {
        // Not a communication failure: a host transport that cannot be recorded into a graph (it synchronises the
        // stream) refused to be.  Nothing was sent; ws_step ends the capture and goes on with direct launches.
        snprintf(buf, sizeof buf, "transport %s cannot be captured into a hipGraph (rc %d)", what, rc);
        return fail(h, WS_ERR_UNSUPPORTED, buf);
    }
    snprintf(buf, sizeof buf, "transport %s failed (rc %d); the slab handle is unusable from here on", what, rc);
    h->slab->comm_failed = true;
    return fail(h, WS_ERR_COMM, buf);
}

size_t mig_msg_bytes(uint32_t cap) { return ((size_t)WS_HDR_WORDS_HOST + (size_t)cap * WS_MIG_REC_WORDS_HOST) * 4; }
size_t halo_slice_words_host(uint32_t rowy) { return ((size_t)rowy + 1 + 3) & ~(size_t)3; }
size_t halo_msg_bytes(uint32_t rowy, uint32_t cap) { return ((size_t)WS_HDR_WORDS_HOST + halo_slice_words_host(rowy) + (size_t)cap * 8) * 4; }

// exchange one fixed-size message with each x-neighbour (a single grouped transport call)
ws_status slab_exchange(ws_handle *h, hipStream_t stream, void *sendL, void *sendR, void *recvL, void *recvR, uint64_t bytes)
{
    WsSlab *S = h->slab;
    const bool left = S->rank > 0, right = S->rank + 1 < S->world;
    if (!left && !right) return WS_OK;
    void *sp[2] = {sendL, sendR}, *rp[2] = {recvL, recvR};
    const uint64_t sb[2] = {left ? bytes : 0, right ? bytes : 0};
    const int rc = S->tr.sendrecv(S->tr.ctx, 1, sp, sb, rp, sb, stream);
    return rc ? slab_fail_tr(h, "sendrecv", rc) : WS_OK;
}

// the same with its own size for every transfer (exact message sizes): [0] = towards / from the left neighbour, [1] = the right
ws_status slab_exchange2(ws_handle *h, hipStream_t stream, void *sendL, void *sendR, void *recvL, void *recvR, const uint64_t send_bytes[2],
                         const uint64_t recv_bytes[2])
{
    WsSlab *S = h->slab;
    const bool left = S->rank > 0, right = S->rank + 1 < S->world;
    if (!left && !right) return WS_OK;
    void *sp[2] = {sendL, sendR}, *rp[2] = {recvL, recvR};
    const uint64_t sb[2] = {left ? send_bytes[0] : 0, right ? send_bytes[1] : 0}, rb[2] = {left ? recv_bytes[0] : 0, right ? recv_bytes[1] : 0};
    const int rc = S->tr.sendrecv(S->tr.ctx, 1, sp, sb, rp, rb, stream);
    return rc ? slab_fail_tr(h, "sendrecv", rc) : WS_OK;
}

// Exact message sizes: {records in message a, in message b, the largest far message (word 6 of c), the owned count} of
// every rank, all-gathered and copied to the host -- begin enqueues, end waits.  which: 0 = migration, 1 = halo.
ws_status slab_sizes_begin(ws_handle *h, hipStream_t stream, int which, const uint32_t *a, const uint32_t *b, const uint32_t *c)
{
    WsSlab *S = h->slab;
    wsk_sizes(stream, a, b, c, S->dyn, S->xs_send[which]);
    HIP_TRY(h, hipGetLastError());
    const int rc = S->tr.allgather_dev(S->tr.ctx, S->xs_send[which], S->xs_all[which], 16, stream);
    if (rc) return slab_fail_tr(h, "allgather_dev", rc);
    HIP_TRY(h, hipMemcpyAsync(S->xs_host[which].p, S->xs_all[which], (size_t)S->world * 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipEventRecord(S->ev_sizes[which], stream));
    return WS_OK;
}
ws_status slab_sizes_end(ws_handle *h, int which)
{
    HIP_TRY(h, hipEventSynchronize(h->slab->ev_sizes[which]));
    h->slab->size_waits++;
    return WS_OK;
}
uint32_t slab_round_records(uint32_t v, uint32_t cap) { return std::min(cap, (v + 63u) & ~63u); }

const char *dyn_error_text(uint32_t err)
{
    if (err & WS_DYN_ERR_CAPACITY) return "slab capacity exceeded by migration (ws_device_cfg.capacity)";
    if (err & WS_DYN_ERR_MIGRATION) return "more particles left a slab in one step than its migration messages hold";
    if (err & WS_DYN_ERR_HALO) return "a boundary layer holds more particles than a halo message (ws_device_cfg.ghost_capacity)";
    if (err & WS_DYN_ERR_GHOSTS) return "ghost capacity exceeded (ws_device_cfg.ghost_capacity)";
    if (err & WS_DYN_ERR_STAMP) return "a message of another step arrived: the transport does not keep its calls in issue order";
    if (err & WS_DYN_ERR_PRED)
        return "an uploaded particle lies outside its slab with a predicted position other than position + velocity / 50 (migration records do "
               "not carry predicted positions)";
    return "slab error";
}
ws_status dyn_error_status(uint32_t err)
{
    if (err & WS_DYN_ERR_PRED) return WS_ERR_INVALID_ARG;
    return (err & ~(uint32_t)WS_DYN_ERR_STAMP) ? WS_ERR_OUT_OF_MEMORY : WS_ERR_COMM;
}

// The status table of step `step` (one header row per rank: the headers of the far messages received with that step's migration): owned counts
// and sticky error bits.  Waits for that step's copy only -- two steps behind the one being enqueued.
ws_status slab_consume_status(ws_handle *h, uint64_t step)
{
    WsSlab *S = h->slab;
    const uint32_t slot = (uint32_t)(step % kStatusSlots);
    HIP_TRY(h, hipEventSynchronize(S->ev_status[slot]));
    const uint32_t *tab = S->status_host.p + (size_t)slot * S->world * WS_HDR_WORDS_HOST;
    uint32_t err = 0;
    for (uint32_t r = 0; r < S->world; r++) err |= tab[r * WS_HDR_WORDS_HOST + 1];
    S->n_known = tab[S->rank * WS_HDR_WORDS_HOST + 2];
    S->n_known_step = step;
    if (err) {
        S->failed = err;
        return fail(h, dyn_error_status(err), dyn_error_text(err));
    }
    // what every rank's messages wanted to carry at that step (the same table on every rank: the same sizes below)
    uint32_t want_mig = 0, want_halo = 0;
    uint32_t want_far = 0;
    for (uint32_t r = 0; r < S->world; r++) {
        want_far = std::max(want_far, tab[r * WS_HDR_WORDS_HOST + 6]);  // (the most records any ONE of the rank's far messages wanted to carry)
        want_mig = std::max(want_mig, tab[r * WS_HDR_WORDS_HOST + 4]);
        want_halo = std::max(want_halo, tab[r * WS_HDR_WORDS_HOST + 5]);
    }
    // (demand is bursty at the onset of a rebound: a pressure wave reaching a slab face triples the count within a step
    // or two.  The sizes follow the LARGEST of the last eight tables, not the newest.)
    // (`unknown` in the NEWEST table -- the first two after a load -- means full capacities; it does not linger in the ring)
    const uint32_t slot8 = (uint32_t)(step % 8);
    const bool unknown = want_mig == WS_HDR_UNKNOWN || want_halo == WS_HDR_UNKNOWN;
    S->want_ring[0][slot8] = unknown ? 0u : want_mig;
    S->want_ring[1][slot8] = unknown ? 0u : want_halo;
    S->want_ring[2][slot8] = unknown ? 0u : want_far;
    S->want_mig = unknown ? WS_HDR_UNKNOWN : *std::max_element(S->want_ring[0], S->want_ring[0] + 8);
    S->want_halo = unknown ? WS_HDR_UNKNOWN : *std::max_element(S->want_ring[1], S->want_ring[1] + 8);
    S->want_far = *std::max_element(S->want_ring[2], S->want_ring[2] + 8);
    return WS_OK;
}

// The sizes of the messages the NEXT step exchanges, from what the table of three steps ago says they wanted to carry
// (four steps lie between the count and its use; "wanted" = the largest of the last eight tables).  Headroom: x 4 for
// the neighbour messages -- along the C3x2 / C4 / C5 trajectories the five-step sums grow at most x 2.7, single steps
// more (x 3 was not enough at C5, step 144) --, x 6 for the burstier far message, x 2 for the boundary-layer
// populations, which move slowly; rounded up to a quarter of an octave, so that the
// sizes (which a captured graph has baked in) change rarely; never below a floor, never above the buffers' capacities.
// `unknown` (no count yet for this particle set) and the hold after a load or a parameter change keep the capacities.
uint32_t slab_quantise_up(uint64_t v)
{
    uint64_t p = 1;
    while (p * 2 <= v) p <<= 1;  // p <= v < 2 p
    const uint64_t g = std::max<uint64_t>(p / 4, 256);
    return (uint32_t)std::min<uint64_t>((v + g - 1) / g * g, 0x80000000ull);
}
void slab_choose_limits(WsSlab *S, bool have_table)
{
    uint32_t mig = S->mig_cap, halo = S->halo_cap, far = S->far_cap;
    if (!S->fixed_messages && have_table && !S->limit_hold && S->want_mig != WS_HDR_UNKNOWN && S->want_halo != WS_HDR_UNKNOWN) {
        mig = std::min(S->mig_cap, std::max(S->floor_mig, slab_quantise_up(4ull * S->want_mig + 1024u)));
        far = std::min(S->far_cap, std::max(S->floor_far, slab_quantise_up(6ull * S->want_far + 64u)));
        halo = std::min(S->halo_cap, std::max(S->floor_halo, slab_quantise_up(2ull * S->want_halo + 1024u)));
        halo = (halo + 63u) & ~63u;
    }
    if (S->limit_hold) S->limit_hold--;
    S->mig_limit_next = mig;
    S->halo_limit_next = halo;
    S->far_limit_next = far;
}

// Everything ws_step puts on the streams for one step (no host logic, no waiting): the migration exchange and its
// bookkeeping kernel, the sort, halo A, K4, halo B, K5 -- halos on the communication stream when the step is split.
// `capturing`: the calls are being recorded into a hipGraph (WS_FLAG_GRAPH): nothing here may depend on the step
// number (stamps and the status slot come from dyn[DY_STEP] on the device), the status ring is copied whole, and the
// side streams are joined back into the handle's stream at the end.
ws_status slab_enqueue(ws_handle *h, uint32_t n_bound, bool first, bool capturing)
{
    WsSlab *S = h->slab;
    hipStream_t s = h->stream;
    const uint32_t W = S->world, me = S->rank;
    const bool left = me > 0, right = me + 1 < W;
    WsDev d = h->dev;
    d.n = n_bound;
    d.dyn = S->dyn;
    d.range_sel = 0;
    d.mig_limit = S->mig_limit_next;  // what this step's force kernel may put into the messages the NEXT step exchanges
    d.far_limit = S->far_limit_next;
    const uint32_t base = d.base, rowy = (uint32_t)(d.dim[1] * d.dim[2]), nxl = (uint32_t)d.dim[0], G = (uint32_t)d.guard;
    int rc;

    // ---- migration: leavers out, arrivals in; afterwards cur[base, base + n) is the new owned set ---------
    // Part 1 -- leavers into the messages, holes remembered, histogram without them -- was done by the previous
    // step's force kernel in its epilogue (force_store_integrate_bin, d.mig).  Only the uploaded particles of the
    // first step need a pass of their own.
    if (first) {
        HIP_TRY(h, hipMemsetAsync(h->count, 0, (size_t)d.ncells * 4, s));
        if (n_bound) {
            wsk_bin(s, d, WsSoA{h->cur.pv + 2 * (size_t)base, h->cur.pred + base, nullptr}, h->cid_cur + base, h->count);
            wsk_migrate_mark(s, d, h->cur, h->cid_cur, h->count);
        }
        HIP_TRY(h, hipGetLastError());
    }
    // the far messages: one to every rank, each headed by this rank's status words (a world of one needs no collective:
    // the message it addresses to itself is the received buffer)
    wsk_far_seal(s, W, S->far_limit_cur, S->far_send, S->dyn);
    ws_status st = WS_OK;
    // (developer builds: WS_SLAB_EXACT_ONE_RANK=1 makes a slab without peers gather and wait for its counts all the same --
    // what the two host waits of a step cost, measured through the real transport on a one-GPU box)
    static const bool exact_one_rank = [] {
        const char *v = WS_DEV_ENV("WS_SLAB_EXACT_ONE_RANK");
        return v && atoi(v) != 0;
    }();
    const bool exact = S->exact_messages && (W > 1 || exact_one_rank) && !capturing;
    uint32_t mig_lim = S->mig_limit_cur, far_lim = S->far_limit_cur;  // the records the fill kernels look at
    uint64_t leave_bound = 0;  // (0: as many can have left as can arrive -- the same limits at both ends)
    const uint32_t *far_src = S->far_send;
    if (exact) {
        // every message at exactly the size of what its sender has for it (the limits are the capacities in this mode:
        // nothing was clamped below them, and the far messages lie at the capacity's stride)
        st = slab_sizes_begin(h, s, 0, S->mig_sendL, S->mig_sendR, S->far_send);
        if (!st) st = slab_sizes_end(h, 0);
        if (st) return st;
        const uint32_t *x = S->xs_host[0].p;
        const uint32_t sL = slab_round_records(x[4 * me], S->mig_cap), sR = slab_round_records(x[4 * me + 1], S->mig_cap);
        const uint32_t rL = left ? slab_round_records(x[4 * (me - 1) + 1], S->mig_cap) : 0u;
        const uint32_t rR = right ? slab_round_records(x[4 * (me + 1)], S->mig_cap) : 0u;
        uint32_t far_most = 0;
        for (uint32_t r = 0; r < W; r++) far_most = std::max(far_most, x[4 * r + 2]);
        far_lim = std::max(64u, slab_round_records(far_most, S->far_cap));
        mig_lim = std::max(64u, std::max(rL, rR));
        const uint64_t sb[2] = {mig_msg_bytes(sL), mig_msg_bytes(sR)}, rb[2] = {mig_msg_bytes(rL), mig_msg_bytes(rR)};
        st = slab_exchange2(h, s, S->mig_sendL, S->mig_sendR, S->mig_recvL, S->mig_recvR, sb, rb);
        if (far_lim < S->far_cap) {
            wsk_far_pack(s, W, S->far_cap, far_lim, S->far_send, S->far_pack);
            far_src = S->far_pack;
        }
        // the owned count as of this moment, and what can arrive now: the launch bound of everything below
        n_bound = (uint32_t)std::min<uint64_t>(S->cap, (uint64_t)x[4 * me + 3] + rL + rR + (uint64_t)(W - 1) * far_lim);
        d.n = n_bound;
        leave_bound = (uint64_t)sL + sR + (uint64_t)W * far_lim;  // what this rank sent
        S->exact_now[0] = std::max(std::max(sL, sR), std::max(rL, rR));
        S->exact_now[2] = far_lim;
    } else {
        st = slab_exchange(h, s, S->mig_sendL, S->mig_sendR, S->mig_recvL, S->mig_recvR, mig_msg_bytes(S->mig_limit_cur));
    }
    if (st) return st;
    const uint32_t *far_all = W > 1 ? S->far_all : S->far_send;
    if (W > 1) {
        rc = S->tr.alltoall_dev(S->tr.ctx, far_src, S->far_all, mig_msg_bytes(far_lim), s);
        if (rc) return slab_fail_tr(h, "alltoall_dev", rc);
    }
    wsk_migrate_fill(s, d, W, me, S->cap, S->dyn, S->hole, S->mig_recvL, S->mig_recvR, mig_lim, far_all, far_lim,
                     S->tgt, S->src, h->cur, h->cid_cur, h->count, S->status_dev, kStatusSlots, S->hole_cap, S->mig_sendL,
                     S->mig_sendR, S->far_send, S->far_limit_next, leave_bound);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(S->ev_filled, s));

    // ---- sort the owned particles; ghost layers are empty in the histogram, so their starts come out as
    //      `base` (layer 0) and `base + n` (layer nxl-1) until k_halo_unpack rebases them ---------------------
    {
        Prof p(h, WS_K_SCAN);
        wsk_scan(s, h->count, h->start + G, first ? h->cursor : nullptr, h->bsum, d.ncells, true, base);
    }
    if (n_bound) {
        {
            // slot = cell start + the rank the particle drew when it was binned (force epilogue / k_migrate_fill); the
            // first step's ranks have holes where k_migrate_mark took leavers out: fill cursors instead, once
            Prof p(h, WS_K_SCATTER);
            if (first)
                wsk_scatter(s, h->cid_cur + base, h->cursor, h->slot_tmp, n_bound, S->dyn + DY_N);
            else
                wsk_place(s, d, h->cid_cur + base, h->cur.rank + base, h->start, h->slot_tmp);
        }
        {
            Prof p(h, WS_K_REORDER);
            WsSoA cur_owned = {h->cur.pv + 2 * (size_t)base, h->cur.pred + base, nullptr};
            wsk_reorder(s, d, h->slot_tmp, h->cid_cur + base, h->start, cur_owned, h->srt, h->cid_srt, h->sxyz, h->pred_stale);
        }
    }
    HIP_TRY(h, hipGetLastError());

    // K4 / K5 over a part of the owned range, named by d.range_sel and resolved on the device from the cell starts
    // (timed by the events the launch itself carries: a bracket recorded around the launches of a split step would
    // also measure the wait for the halo in between)
    auto density = [&](hipStream_t q, uint32_t sel, uint32_t bound, ProfLaunch &p) {
        if (!bound) return;
        WsDev dd = d;
        dd.range_sel = sel;
        dd.n = bound;
        wsk_density(q, dd, h->start, h->cid_srt, h->srt, h->mult, h->alias, h->variant, h->ieee, h->stats, h->mask, h->sxyz,
                    p.events());
    };
    auto force = [&](hipStream_t q, uint32_t sel, uint32_t bound, ProfLaunch &p) {
        if (!bound) return;
        WsDev dd = d;
        dd.range_sel = sel;
        dd.n = bound;
        wsk_force(q, dd, h->start, h->cid_srt, h->srt, h->cur, h->accel, h->cid_cur, h->count, h->mult, h->alias, h->variant,
                  h->ieee, h->mask, false, p.events());
    };
    // Particles of the owned layers next to a neighbour slab ("late": their searches reach into ghosts) and the
    // rest ("early": one contiguous range, x being the slowest axis of the sort).  With fewer than three owned
    // layers everything is late.
    // (the same decision on every rank: the halos of a split step travel on the communication stream, which the RCCL
    // transport binds to a communicator of its own -- a rank that kept them on the compute stream would talk to its
    // neighbours through the other communicator)
    uint32_t thinnest = nxl - 2u;
    for (uint32_t r = 0; r < W; r++) thinnest = std::min(thinnest, S->cuts[r + 1] - S->cuts[r]);
    const bool split = S->overlap && thinnest >= 3u && W > 1;
    S->last_split = split;
    uint32_t late_bound = std::min(n_bound, S->halo_limit);  // a boundary layer never holds more than a halo message
    const size_t a_bytes = halo_msg_bytes(rowy, S->halo_limit), b_bytes = (size_t)S->halo_limit * 8;
    uint64_t a_sb[2] = {a_bytes, a_bytes}, a_rb[2] = {a_bytes, a_bytes}, b_sb[2] = {b_bytes, b_bytes}, b_rb[2] = {b_bytes, b_bytes};
    uint32_t pack_bound = S->halo_limit, ghost_bound = S->halo_cap;
    hipStream_t c = split ? S->comm : s;  // the halos travel on a second stream while the early range computes
    if (split) {
        HIP_TRY(h, hipEventRecord(S->ev_sorted, s));
        HIP_TRY(h, hipStreamWaitEvent(c, S->ev_sorted, 0));
    }
    // halo A: the boundary layers' records (K4 needs their predicted positions) + their cell-start slices
    if (left || right) wsk_halo_pack(c, d, h->start, h->srt, S->dyn, rowy, S->halo_limit, S->halo_sendL, S->halo_sendR, false);
    HIP_TRY(h, hipGetLastError());
    bool early_k4_launched = false;
    if (exact) {
        // the boundary layers' populations are known on the device only now (after the sort): gather them, and wait
        // for them behind the early range of K4, which needs no ghost
        st = slab_sizes_begin(h, c, 1, left ? S->halo_sendL : nullptr, right ? S->halo_sendR : nullptr, nullptr);
        if (st) return st;
        if (split) {
            ProfLaunch pe(h, WS_K_DENSITY);
            density(s, WS_RANGE_EARLY, n_bound, pe);
            HIP_TRY(h, hipGetLastError());
            early_k4_launched = true;
        }
        st = slab_sizes_end(h, 1);
        if (st) return st;
        const uint32_t *x = S->xs_host[1].p;
        const uint32_t sL = slab_round_records(x[4 * me], S->halo_cap), sR = slab_round_records(x[4 * me + 1], S->halo_cap);
        const uint32_t rL = left ? slab_round_records(x[4 * (me - 1) + 1], S->halo_cap) : 0u;
        const uint32_t rR = right ? slab_round_records(x[4 * (me + 1)], S->halo_cap) : 0u;
        a_sb[0] = halo_msg_bytes(rowy, sL); a_sb[1] = halo_msg_bytes(rowy, sR);
        a_rb[0] = halo_msg_bytes(rowy, rL); a_rb[1] = halo_msg_bytes(rowy, rR);
        b_sb[0] = (uint64_t)sL * 8; b_sb[1] = (uint64_t)sR * 8; b_rb[0] = (uint64_t)rL * 8; b_rb[1] = (uint64_t)rR * 8;
        pack_bound = std::max(64u, std::max(sL, sR));
        ghost_bound = std::max(64u, std::max(rL, rR));
        late_bound = std::min(n_bound, pack_bound);
        S->exact_now[1] = std::max(pack_bound, ghost_bound);
    }
    st = slab_exchange2(h, c, S->halo_sendL, S->halo_sendR, S->halo_recvL, S->halo_recvR, a_sb, a_rb);
    if (st) return st;
    wsk_halo_unpack(c, d, h->start, h->srt, h->sxyz, S->dyn, rowy, nxl, ghost_bound, S->halo_recvL, S->halo_recvR, false);
    HIP_TRY(h, hipGetLastError());
    if (split) {
        //   compute: K4(early) . wait A . K4(late) . record B1 . K5(early) . wait B . K5(late)
        //   comm:    wait sorted . halo A . record A ; wait B1 . halo B . record B
        HIP_TRY(h, hipEventRecord(S->ev_halo_a, c));
        {
            ProfLaunch pe(h, WS_K_DENSITY), pl(h, WS_K_DENSITY, false);  // kernel time of a step = early + late
            if (!early_k4_launched) density(s, WS_RANGE_EARLY, n_bound, pe);
            HIP_TRY(h, hipStreamWaitEvent(s, S->ev_halo_a, 0));
            // the boundary layers -- one launch for both when the slab has two neighbours
            if (left && right) density(s, WS_RANGE_LATE_BOTH, (uint32_t)std::min<uint64_t>(n_bound, 2ull * late_bound), pl);
            else density(s, left ? WS_RANGE_LATE_LEFT : WS_RANGE_LATE_RIGHT, late_bound, pl);
        }
        HIP_TRY(h, hipEventRecord(S->ev_k4_late, s));
        HIP_TRY(h, hipStreamWaitEvent(c, S->ev_k4_late, 0));
    } else {
        ProfLaunch p(h, WS_K_DENSITY);
        density(s, WS_RANGE_ALL, n_bound, p);
    }
    // halo B: the densities K4 just wrote for the same particles (a ghost's own neighbours are not all here)
    if (left || right) {
        wsk_halo_pack(c, d, h->start, h->srt, S->dyn, rowy, pack_bound, S->halo_sendL, S->halo_sendR, true);
        HIP_TRY(h, hipGetLastError());
        st = slab_exchange2(h, c, S->halo_sendL, S->halo_sendR, S->halo_recvL, S->halo_recvR, b_sb, b_rb);
        if (st) return st;
        wsk_halo_unpack(c, d, h->start, h->srt, h->sxyz, S->dyn, rowy, nxl, ghost_bound, S->halo_recvL, S->halo_recvR, true);
        HIP_TRY(h, hipGetLastError());
    }
    if (split) {
        HIP_TRY(h, hipEventRecord(S->ev_halo_b, c));
        {
            ProfLaunch pe(h, WS_K_FORCE), pl(h, WS_K_FORCE, false);
            force(s, WS_RANGE_EARLY, n_bound, pe);
            HIP_TRY(h, hipStreamWaitEvent(s, S->ev_halo_b, 0));
            if (left && right) force(s, WS_RANGE_LATE_BOTH, (uint32_t)std::min<uint64_t>(n_bound, 2ull * late_bound), pl);
            else force(s, left ? WS_RANGE_LATE_LEFT : WS_RANGE_LATE_RIGHT, late_bound, pl);
        }
    } else {
        ProfLaunch p(h, WS_K_FORCE);
        force(s, WS_RANGE_ALL, n_bound, p);
    }
    HIP_TRY(h, hipGetLastError());
    // this step's status table (filled by k_migrate_fill) to the host, off the compute stream
    HIP_TRY(h, hipStreamWaitEvent(S->copy, S->ev_filled, 0));
    const size_t row_bytes = (size_t)W * WS_HDR_WORDS_HOST * 4;
    if (capturing) {
        // the slot depends on the step: copy the whole ring (a few hundred bytes) and join the copy stream back, which
        // also orders the next step's k_migrate_fill behind this copy -- no slot is ever read while it is written
        HIP_TRY(h, hipMemcpyAsync(S->status_host.p, S->status_dev, row_bytes * kStatusSlots, hipMemcpyDeviceToHost, S->copy));
        HIP_TRY(h, hipEventRecord(S->ev_copied, S->copy));
        HIP_TRY(h, hipStreamWaitEvent(s, S->ev_copied, 0));
    } else {
        const uint32_t slot = (uint32_t)(h->steps % kStatusSlots);
        HIP_TRY(h, hipMemcpyAsync(S->status_host.p + (size_t)slot * W * WS_HDR_WORDS_HOST,
                                  S->status_dev + (size_t)slot * W * WS_HDR_WORDS_HOST, row_bytes, hipMemcpyDeviceToHost, S->copy));
        HIP_TRY(h, hipEventRecord(S->ev_status[slot], S->copy));
    }
    return WS_OK;
}

// WS_FLAG_GRAPH: the step as a hipGraph, captured once per launch bound and replayed.  The reference builds its pass
// graph once and replays it every frame (src/fluid_compute.rs:309-363, AppComputeWorker::run); this is that, for the
// 14+ launches and 4 transport calls of a slab step.  Everything step-dependent inside the step lives on the device
// (dyn[DY_STEP], the scan's ticket counter); the launch bound is quantised so that migration rarely asks for a new
// capture.  A transport that cannot be captured (one that synchronises the stream, like the tests' loopback) makes the
// capture fail: the handle then falls back to direct launches for good.
typedef WsGraphEntry WsGraph;

ws_status slab_step(ws_handle *h)
{
    WsSlab *S = h->slab;
    hipStream_t s = h->stream;
    if (h->dead) return fail(h, WS_ERR_HIP, h->err.c_str());
    if (S->comm_failed) return fail(h, WS_ERR_COMM, "an earlier transport call failed; the slab handle is unusable");
    if (S->failed) return fail(h, dyn_error_status(S->failed), dyn_error_text(S->failed));
    bound_pending(h);
    note_step_params(h);
    const uint64_t t = h->steps;
    if (t >= S->t0 + kStatusLag) {  // (tables of steps before the last load describe another particle set)
        const ws_status st = slab_consume_status(h, t - kStatusLag);
        if (st) return st;
    }
    // message sizes: this step exchanges what the previous call announced; the next step's follow the newest table
    S->mig_limit_cur = S->mig_limit_next;
    S->halo_limit = S->halo_limit_next;
    S->far_limit_cur = S->far_limit_next;
    slab_choose_limits(S, t >= S->t0 + kStatusLag);
    S->arrivals_hist[t % 4] = 2ull * S->mig_limit_cur + (uint64_t)S->world * S->far_limit_cur;
    // upper bound of the owned count during this step: what the host last saw, plus what can have arrived since
    const uint64_t since = t - S->n_known_step + 1;
    uint64_t arrivals = 0;
    for (uint64_t k = 0; k < std::min<uint64_t>(since, 4); k++) arrivals += S->arrivals_hist[(t - k) % 4];
    if (since > 4) arrivals += (since - 4) * (uint64_t)S->max_arrivals;
    uint32_t n_bound = (uint32_t)std::min<uint64_t>(S->cap, (uint64_t)S->n_known + arrivals);
    const bool first = !S->binned;
    // Only what is known to be stream-ordered is captured: a single slab (no transport calls at all) or the library's
    // own RCCL transport.  A host transport may synchronise the stream or rendezvous on the host inside its callbacks
    // (the in-process ones do); recording that would fail half-way through a collective and leave the ranks out of
    // step with each other, so such handles are launched directly without trying.
    // With peers the capture additionally needs one communicator per stream (a single communicator driven from two
    // captured streams would depend on the order RCCL serialises them in) and -- because no run with two or more GPUs
    // has executed a captured transport call yet -- the explicit WS_FLAG_GRAPH_MULTIRANK (experimental; every rank must
    // set it alike: ws_slab_create checks).  On the one-GPU test box the path is exercised through the tests' stand-in
    // for librccl (tests/test_gpu_fake_rccl.py).  Without the flag a multi-rank handle launches directly.
    const bool multirank_ok = (h->flags & WS_FLAG_GRAPH_MULTIRANK) != 0;
    const bool capturable = (S->world == 1 || (multirank_ok && ws_rccl_transport_communicators(&S->tr) == 2)) &&
                            !(S->exact_messages && S->world > 1);  // (exact sizes come from the host, step by step)
    const bool graph = (h->flags & WS_FLAG_GRAPH) && capturable && !S->graph_failed && !first && h->pred_stale;
    ws_status st = WS_OK;
    if (graph) {
        // quantise the bound: a new capture only when the owned count has drifted by tens of thousands
        const uint32_t q = 1u << 16;
        n_bound = (uint32_t)std::min<uint64_t>(S->cap, ((uint64_t)n_bound + q - 1) / q * q);
        hipGraphExec_t exec = nullptr;
        for (const WsGraph &g : S->graphs)
            if (g.n_bound == n_bound && g.mig_cur == S->mig_limit_cur && g.mig_next == S->mig_limit_next && g.halo == S->halo_limit &&
                g.far_cur == S->far_limit_cur && g.far_next == S->far_limit_next)
                exec = g.exec;
        if (!exec) {
            hipGraph_t gr = nullptr;
            // (relaxed mode: a host may drive several handles from several threads -- in-process slabs, or simply two fluids --
            // and in the other modes one thread's capture makes ANOTHER thread's legacy-stream hipMemcpy fail with
            // hipErrorStreamCaptureImplicit; this thread itself issues nothing but launches, events and async copies here)
            hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
            if (e == hipSuccess) {
                S->capturing = true;
                st = slab_enqueue(h, n_bound, false, true);
                S->capturing = false;
                e = hipStreamEndCapture(s, &gr);
                if (st == WS_OK && e == hipSuccess) e = hipGraphInstantiate(&exec, gr, nullptr, nullptr, 0);
                if (gr) hipGraphDestroy(gr);
            }
            if (st != WS_OK || e != hipSuccess || !exec) {
                // not capturable with this transport / runtime: direct launches from here on
                (void)hipGetLastError();
                S->graph_failed = true;
                h->err = std::string("WS_FLAG_GRAPH: capture failed (") + hipGetErrorName(e) + "), using direct launches";
                exec = nullptr;
            } else {
                if (S->graphs.size() >= 8) {
                    hipGraphExecDestroy(S->graphs.front().exec);
                    S->graphs.erase(S->graphs.begin());
                }
                S->graphs.push_back({n_bound, S->mig_limit_cur, S->mig_limit_next, S->halo_limit, S->far_limit_cur, S->far_limit_next, exec});
            }
        }
        if (exec) {
            HIP_TRY(h, hipGraphLaunch(exec, s));
            // (the graph copies the status ring whole: "step t's table is on the host" = "graph t has finished")
            HIP_TRY(h, hipEventRecord(S->ev_status[t % kStatusSlots], s));
            S->graph_steps++;
        } else {
            st = slab_enqueue(h, n_bound, false, false);
            if (st) return st;
        }
    } else {
        st = slab_enqueue(h, n_bound, first, false);
        if (st) return st;
    }
    S->binned = true;
    h->pred_stale = true;   // the force epilogue stores position and velocity only (k_reorder)
    h->accel_stale = true;  // ... and no accelerations (refresh_accel)
    HIP_TRY(h, hipEventRecord(h->done, s));
    h->done_recorded = true;
    h->steps++;
    return WS_OK;
}

// Everything enqueued so far has run: the exact owned count, and the error bits -- this rank's own, straight from
// the device, and every rank's as of the status tables gathered so far.  This only REPORTS: it never latches
// S->failed.  A rank that stopped stepping on what it alone knows would leave its peers inside the next step's
// collectives without a partner; ws_step keeps issuing every step's collectives until the status table shows
// the bit on all ranks at once (slab_consume_status, the one place that decides to stop), so a host may sync or
// read after every step -- the normal frame pattern -- and every rank still fails at the same ws_step.
// `bits` = this rank's sticky bits straight from the device, OR-ed with every rank's as of the status tables gathered so
// far.  Returns HIP errors only.
ws_status slab_settle_bits(ws_handle *h, uint32_t *bits)
{
    WsSlab *S = h->slab;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipStreamSynchronize(S->comm));
    HIP_TRY(h, hipStreamSynchronize(S->copy));
    uint32_t dyn[WS_DYN_WORDS];
    HIP_TRY(h, copy_now(h, dyn, S->dyn, sizeof dyn, hipMemcpyDeviceToHost));
    h->n = dyn[DY_N];
    S->n_known = dyn[DY_N];
    S->n_known_step = h->steps;  // as of the steps enqueued so far
    S->migrated_out = S->left_base + dyn[DY_LEFT];
    uint32_t err = dyn[DY_ERR];
    // the other ranks' bits arrive with the status tables: look at every table written so far
    for (uint64_t k = std::max<uint64_t>(h->steps > kStatusSlots ? h->steps - kStatusSlots : 0, S->t0); k < h->steps; k++) {
        const uint32_t *tab = S->status_host.p + (size_t)(k % kStatusSlots) * S->world * WS_HDR_WORDS_HOST;
        for (uint32_t r = 0; r < S->world; r++) err |= tab[r * WS_HDR_WORDS_HOST + 1];
    }
    *bits = err;
    return WS_OK;
}

ws_status slab_settle(ws_handle *h)
{
    uint32_t bits = 0;
    const ws_status st = slab_settle_bits(h, &bits);
    if (st) return st;
    if (bits) return fail(h, dyn_error_status(bits), dyn_error_text(bits));
    return WS_OK;
}

void slab_drop_graphs(WsSlab *S)
{
    for (auto &g : S->graphs)
        if (g.exec) hipGraphExecDestroy(g.exec);
    S->graphs.clear();
}

// the arrays whose size follows from the slab's geometry (cell grid, capacities, message sizes)
void slab_free_arrays(ws_handle *h)
{
    free_particle_arrays(h);
    free_grid(h);
    h->slab->geometry.release();
}

void slab_free(ws_handle *h)
{
    WsSlab *S = h->slab;
    if (!S) return;
    if (S->comm) hipStreamSynchronize(S->comm);
    if (S->copy) hipStreamSynchronize(S->copy);
    slab_free_arrays(h);
    release_all(S->fixed, S->hist, S->agree_send, S->agree_all, S->cnt_send, S->cnt_all, S->g_send, S->g_all, S->g_out, S->retired,
                S->xs_host[0], S->xs_host[1], S->status_host);
    for (hipEvent_t e : S->ev_sizes)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : {S->ev_sorted, S->ev_halo_a, S->ev_k4_late, S->ev_halo_b, S->ev_filled, S->ev_copied})
        if (e) hipEventDestroy(e);
    slab_drop_graphs(S);
    for (hipEvent_t e : S->ev_status)
        if (e) hipEventDestroy(e);
    if (S->comm) hipStreamDestroy(S->comm);
    if (S->copy) hipStreamDestroy(S->copy);
    delete S;
    h->slab = nullptr;
}

// global grid of a parameter set (org / dim / guard as on a single GPU)
ws_status global_grid(const ws_params *params, uint32_t n_global, WsDev *out)
{
    ws_handle tmp;
    const ws_status st = derive_dev(&tmp, *params, n_global, out);
    if (st) g_create_error = tmp.err;
    return st;
}

// What a parameter set means for this slab: the global grid, the cuts, the local grid with its ghost layers, and the
// fixed capacities every message size follows from.  Pure host arithmetic (nothing is touched): a re-grid validates
// the new geometry with it before it gives up the old one.
struct SlabGeometry {
    WsDev d;
    std::vector<uint32_t> cuts;
    uint32_t halo_cap, mig_cap, far_cap, hole_cap, max_arrivals;
    size_t tot;  // slots of the particle arrays: ghosts | owned | ghosts
};

// cuts: explicit x-layer cuts (a re-cut, ws_slab_rebalance), or nullptr = equal cell counts (what ws_slab_assign tells
// the host at t = 0)
ws_status slab_geometry(ws_handle *h, const ws_params *params, SlabGeometry *out, const std::vector<uint32_t> *cuts = nullptr)
{
    WsSlab *S = h->slab;
    WsDev g;
    ws_status st = global_grid(params, S->n_global, &g);
    if (st) return fail(h, st, g_create_error.c_str());
    const uint32_t W = S->world, nx = (uint32_t)g.dim[0];
    if (W > nx) return fail(h, WS_ERR_INVALID_ARG, "more slabs than cell layers along x");
    out->cuts.resize(W + 1);
    for (uint32_t r = 0; r <= W; r++) out->cuts[r] = cuts ? (*cuts)[r] : (uint32_t)((uint64_t)r * nx / W);
    // A boundary layer is one cell layer of the global grid: n_global / nx particles when the fluid is spread evenly
    // along x (gravity acts along y, so it stays that way); the default leaves a factor of four.  Halo messages,
    // ghost ranges and migration messages all have this FIXED size, known to both ends: nothing is sized by a
    // count that only the device knows.
    // Round 4: the defaults follow what the benchmark trajectories need (tools/migration_peak.py, profiles/r04/
    // migration_peak_*.log; peaks while the collapsed cloud rebounds, steps ~150-250, in average layers of n / nx
    // particles): a boundary layer holds up to 3.8 (C3x2), 5.2 (C4), 1.8 (C5) layers; up to 9.3 / 11 / 19 layers' worth
    // of particles leave towards ONE neighbour in one step, and up to 0 / 3.5 / 13.7 cross MORE than one slab (speeds
    // reach 10^4 units/s with the reference's parameters).  Rounds 1-3 sized for 4 + 1 + 1/64 layers and overran.
    // 16 layers + 32 K for a halo (three times the peaks and as much again: a shock front can pile a third of a small
    // system into one cell layer, tools/slab_fuzz.py; a ghost slot costs ~100 bytes), 64 layers + 64 K for a migration and
    // for each far message (three times the peaks).  These are CAPACITIES of
    // buffers; what travels per step is sized from the fluid's recent behaviour (slab_choose_limits).
    const uint32_t layer = (uint32_t)((uint64_t)S->n_global / nx);
    uint32_t halo_cap = S->cfg_ghost_capacity ? S->cfg_ghost_capacity : 16 * layer + 32768u;
    halo_cap = (halo_cap + 63u) & ~63u;  // = the owned range's base: a wave's tile starts on a 256-byte boundary of the planes
    out->halo_cap = halo_cap;
    // Leavers per step and direction are the part of a boundary layer that crosses the slab face, v dt / h of it: a
    // whole layer's worth (a quarter of the halo capacity) is a wide margin, and the message is on the step's critical
    // path at full size (nothing overlaps the migration exchange), so it is not sized like a halo.
    out->mig_cap = S->cfg_ghost_capacity ? std::max(halo_cap / 4u, 1024u) : 64 * layer + 65536u;  // (the same on every rank)
    // the per-destination messages for particles that cross MORE than one slab in a step: none for most of a run, but while
    // the collapsed cloud rebounds tens of thousands per slab and step do (C4 in four slabs: 114 K, C5 in eight: more than 400 K per slab and step; speeds
    // reach 10^4 units/s with the reference's parameters); its per-step size follows the same table
    out->far_cap = S->cfg_ghost_capacity ? 1024u : 64 * layer + 65536u;
    out->hole_cap = 2 * out->mig_cap + std::min(W, 4u) * out->far_cap;  // (every far message full at once is not a state of a fluid)
    out->max_arrivals = 2 * out->mig_cap + W * out->far_cap;
    out->tot = (size_t)halo_cap + S->cap + halo_cap;
    if (out->tot > WS_MAX_SLOTS - 16u) return fail(h, WS_ERR_INVALID_ARG, "more than 2^27 particle slots on one device");
    // local grid: one ghost layer on each side of the owned layers [cuts[rank], cuts[rank+1])
    WsDev d = g;
    d.gdim_x = (int32_t)nx;
    d.xoff = (int32_t)out->cuts[S->rank] - 1;
    d.dim[0] = (int32_t)(out->cuts[S->rank + 1] - out->cuts[S->rank]) + 2;
    d.ncells = (uint32_t)((uint64_t)d.dim[0] * d.dim[1] * d.dim[2]);
    d.base = halo_cap;
    d.n = 0;
    d.hash_n = S->n_global;
    d.has_left = S->rank > 0 ? 1u : 0u;
    d.has_right = S->rank + 1 < W ? 1u : 0u;
    const uint32_t rowy = (uint32_t)(d.dim[1] * d.dim[2]), G = (uint32_t)d.guard, nxl = (uint32_t)d.dim[0];
    d.lidx[0] = G + rowy;               // first cell start of layer 1 (the left boundary layer)
    d.lidx[1] = G + 2 * rowy;           // ... its end = first particle that needs no left ghost
    d.lidx[2] = G + (nxl - 2) * rowy;   // first cell start of layer nxl - 2 (the right boundary layer)
    d.lidx[3] = G + (nxl - 1) * rowy;   // ... its end
    out->d = d;
    return WS_OK;
}

// Adopt a geometry: allocate everything sized by it (the handle holds none of it at this point).
ws_status slab_alloc_arrays(ws_handle *h, const SlabGeometry &geo)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    S->cuts = geo.cuts;
    S->halo_cap = geo.halo_cap; S->mig_cap = geo.mig_cap; S->far_cap = geo.far_cap; S->hole_cap = geo.hole_cap;
    S->max_arrivals = geo.max_arrivals;
    h->dev = geo.d;
    ws_status st = alloc_particle_arrays(h, geo.tot, S->cap);
    WsGroup &G = S->geometry;
    if (!st) st = G.alloc(h, &S->cuts_dev, (size_t)(W + 1) * 4, "slab cuts");
    if (st) return st;
    HIP_TRY(h, copy_now(h, S->cuts_dev, S->cuts.data(), (size_t)(W + 1) * 4, hipMemcpyHostToDevice));
    st = G.alloc(h, &S->hole, (size_t)S->hole_cap * 4, "migration index lists");
    if (!st) st = G.alloc(h, &S->tgt, (size_t)(S->hole_cap + S->max_arrivals) * 4, "migration index lists");
    if (!st) st = G.alloc(h, &S->src, (size_t)(S->hole_cap + S->max_arrivals) * 4, "migration index lists");
    // every message starts zeroed
    const size_t mb = mig_msg_bytes(S->mig_cap), fb = mig_msg_bytes(S->far_cap);
    for (uint32_t **p : {&S->mig_sendL, &S->mig_sendR, &S->mig_recvL, &S->mig_recvR})
        if (!st) st = G.alloc(h, p, mb, "migration messages", true);
    // far messages: one per destination rank out, one per source rank in (exchanged all-to-all)
    if (!st) st = G.alloc(h, &S->far_send, fb * W, "far messages", true);
    if (!st) st = G.alloc(h, &S->far_all, fb * W, "far messages", true);
    if (!st && S->exact_messages) st = G.alloc(h, &S->far_pack, fb * W, "far messages");
    if (!st) st = G.alloc(h, &S->mig_dev, sizeof(WsMig), "migration targets");
    if (st) return st;
    {
        // where the force kernel's epilogue sends a particle that left the slab (migration part 1, fused)
        const WsMig m = {S->cuts_dev, W, S->rank, S->dyn, S->hole, S->hole_cap, S->mig_sendL, S->mig_sendR, S->mig_cap,
                         S->far_send, S->far_cap};
        HIP_TRY(h, copy_now(h, S->mig_dev, &m, sizeof m, hipMemcpyHostToDevice));
        h->dev.mig = S->mig_dev;
    }
    const size_t hb = halo_msg_bytes((uint32_t)(geo.d.dim[1] * geo.d.dim[2]), S->halo_cap);
    for (uint32_t **p : {&S->halo_sendL, &S->halo_sendR, &S->halo_recvL, &S->halo_recvR})
        if ((st = G.alloc(h, p, hb, "halo messages", true))) return st;
    return alloc_grid(h);
}

// ---- loads: a new owned set (create, ws_reset, ws_write_particles, a re-grid) ---------------------------------
// Every load starts from an empty owned range, appends the particles this slab owns (the caller's kernels count
// them in dyn[DY_N]) and ends with the bookkeeping every ws_step starts from.
ws_status slab_load_begin(ws_handle *h)
{
    WsSlab *S = h->slab;
    // the migration counters are cumulative "since the handle was created" (ws_slab_counters): carry them over the load
    uint32_t dyn[WS_DYN_WORDS];
    HIP_TRY(h, copy_now(h, dyn, S->dyn, sizeof dyn, hipMemcpyDeviceToHost));
    S->left_base += dyn[DY_LEFT];
    S->arrived_base += dyn[DY_ARRIVED];
    S->far_base += dyn[DY_FAR];
    HIP_TRY(h, hipMemsetAsync(S->dyn, 0, WS_DYN_WORDS * 4, h->stream));
    return WS_OK;
}

ws_status slab_load_end(ws_handle *h)
{
    WsSlab *S = h->slab;
    uint32_t dyn[WS_DYN_WORDS];
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, copy_now(h, dyn, S->dyn, sizeof dyn, hipMemcpyDeviceToHost));
    const uint32_t want = dyn[DY_N], n_local = std::min(want, S->cap), step0 = (uint32_t)h->steps;
    if (want > S->cap) HIP_TRY(h, copy_now(h, S->dyn + DY_N, &n_local, 4, hipMemcpyHostToDevice));
    HIP_TRY(h, copy_now(h, S->dyn + DY_STEP, &step0, 4, hipMemcpyHostToDevice));
    const uint32_t unknown = WS_HDR_UNKNOWN;  // (no halo of this particle set has been packed yet: k_migrate_fill hands it on)
    HIP_TRY(h, copy_now(h, S->dyn + DY_HALO_NOW, &unknown, 4, hipMemcpyHostToDevice));
    slab_drop_graphs(S);  // captured for other arrays / another geometry
    // outgoing migration messages empty; the first step's far header: no records, no error, the owned count
    // (k_migrate_fill writes it for every later step)
    // (word 3: the step the message belongs to -- the receiver checks it)
    const uint32_t hdr0[WS_HDR_WORDS_HOST] = {0u, 0u, n_local, (uint32_t)h->steps, WS_HDR_UNKNOWN, WS_HDR_UNKNOWN, 0u, 0u};
    // (words 4 / 5: nothing has been counted for this particle set yet -- full-capacity messages until a table says otherwise)
    S->mig_limit_cur = S->mig_limit_next = S->mig_cap;
    S->halo_limit = S->halo_limit_next = S->halo_cap;
    S->far_limit_cur = S->far_limit_next = S->far_cap;
    S->want_mig = S->want_halo = WS_HDR_UNKNOWN;
    S->want_far = 0;
    for (auto &ring : S->want_ring)
        for (uint32_t &w : ring) w = 0;
    S->limit_hold = 0;
    for (uint64_t &a : S->arrivals_hist) a = S->max_arrivals;
    HIP_TRY(h, copy_now(h, S->mig_sendL, hdr0, sizeof hdr0, hipMemcpyHostToDevice));
    HIP_TRY(h, copy_now(h, S->mig_sendR, hdr0, sizeof hdr0, hipMemcpyHostToDevice));
    for (uint32_t r = 0; r < S->world; r++)  // one far message per destination, at the stride of the full capacity
        HIP_TRY(h, copy_now(h, S->far_send + (size_t)r * (mig_msg_bytes(S->far_cap) / 4), hdr0, sizeof hdr0, hipMemcpyHostToDevice));
    h->n = n_local;
    S->binned = false;  // the first ws_step bins (and migrates: a no-op when ownership follows the cuts)
    S->n_known = n_local;
    S->n_known_step = h->steps;
    S->t0 = h->steps;
    S->failed = 0;
    h->pred_stale = false;   // the caller's predicted positions, as they are
    h->accel_stale = false;  // no step on this set yet: the views report zero density / acceleration
    if (want > S->cap)
        return fail(h, WS_ERR_OUT_OF_MEMORY, "this slab would own more particles than its capacity (ws_device_cfg.capacity)");
    return WS_OK;
}

// a chunk of a global host array through the staging buffer into the select kernel
ws_status slab_load_global(ws_handle *h, int src, const void *host, size_t rec_bytes)
{
    WsSlab *S = h->slab;
    const uint32_t n = S->n_global, chunk = 1u << 21;
    ws_status st = ensure_stage(h, (size_t)std::min(n, chunk) * rec_bytes);
    if (st) return st;
    st = slab_load_begin(h);
    if (st) return st;
    WsDev d = h->dev;
    for (uint32_t s0 = 0; s0 < n; s0 += chunk) {
        const uint32_t m = std::min(chunk, n - s0);
        HIP_TRY(h, hipMemcpyAsync(h->stage, (const char *)host + (size_t)s0 * rec_bytes, (size_t)m * rec_bytes,
                                  hipMemcpyHostToDevice, h->stream));
        wsk_slab_select(h->stream, d, src, S->cuts_dev, S->world, S->rank, h->stage, s0, m, nullptr, 0, h->cur, S->cap, S->dyn);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // the staging buffer is reused; the caller's buffer is not kept
    }
    return slab_load_end(h);
}

// Quiesce for a collective host-level call.  Reports nothing: a load replaces the particle set, errors included.
ws_status slab_quiesce(ws_handle *h)
{
    WsSlab *S = h->slab;
    if (S->comm_failed) return fail(h, WS_ERR_COMM, "an earlier transport call failed; the slab handle is unusable");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipStreamSynchronize(S->comm));
    HIP_TRY(h, hipStreamSynchronize(S->copy));
    drain_profile(h);
    return WS_OK;
}

// ws_reset on a slab handle (COLLECTIVE in the sense that every rank must call it with the same array before any of
// them steps again; it moves no data between ranks): pos_xyz holds ALL n_global initial positions, as
// FluidParticlesInitial does (src/fluid_compute.rs:82-85,:517-521); each slab keeps what its cuts own.
ws_status slab_reset(ws_handle *h, const float *pos_xyz)
{
    ws_status st = slab_quiesce(h);
    if (st) return st;
    h->steps = 0;
    h->last_pressure = {};
    return slab_load_global(h, 0, pos_xyz, 12);
}

ws_status slab_write_particles(ws_handle *h, const ws_particle80 *in)
{
    ws_status st = slab_quiesce(h);
    if (st) return st;
    h->steps = 0;
    h->last_pressure = {};
    return slab_load_global(h, 1, in, sizeof(ws_particle80));
}

// ---- id-ordered global views -------------------------------------------------------------------------------
// COLLECTIVE: every rank packs {id, payload} records of the particles it owns, one all-gather of the counts and one
// of the records bring every rank's records to every rank.  On return S->g_all holds them (rank r at r * stride),
// S->cnt_all the counts (device) and S->counts (host).
ws_status slab_gather(ws_handle *h, int kind, size_t *stride_words_out, uint32_t *max_n_out)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    // exact owned count, and the sticky error bits this rank knows of.  A rank must NOT leave here on what it alone
    // knows (a halo / ghost overrun of the last step is known to the rank it happened on only, until the next step's
    // all-gather): its peers would wait in the all-gathers below for ever.  The bits travel in the count words and
    // every rank refuses the view of an invalid step at the same call, after the first all-gather.
    uint32_t my_bits = 0;
    ws_status st = slab_settle_bits(h, &my_bits);
    if (st) return st;
    if (S->comm_failed) return fail(h, WS_ERR_COMM, "an earlier transport call failed; the slab handle is unusable");
    if ((st = S->cnt_send.grow(h, 16, "gather counts")) || (st = S->cnt_all.grow(h, (size_t)W * 16, "gather counts"))) return st;
    const uint32_t mine[4] = {h->n, (uint32_t)kind, my_bits, S->cap};
    wsk_set_words4(h->stream, S->cnt_send.p, mine[0], mine[1], mine[2], mine[3]);
    HIP_TRY(h, hipGetLastError());
    if (W > 1) {
        const int rc = S->tr.allgather_dev(S->tr.ctx, S->cnt_send.p, S->cnt_all.p, 16, h->stream);
        if (rc) return slab_fail_tr(h, "allgather_dev", rc);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        HIP_TRY(h, copy_now(h, S->cnt_all.p, S->cnt_send.p, 16, hipMemcpyDeviceToDevice));
    }
    std::vector<uint32_t> tab((size_t)W * 4);
    HIP_TRY(h, copy_now(h, tab.data(), S->cnt_all.p, tab.size() * 4, hipMemcpyDeviceToHost));
    S->counts.resize(W);
    uint64_t total = 0;
    uint32_t max_n = 0;
    if (tab[4 * S->rank] != mine[0] || tab[4 * S->rank + 1] != mine[1]) {  // (a transport that is not ordered on the stream it was given)
        return fail(h, WS_ERR_COMM, "the all-gather did not deliver this rank's own contribution");
    }
    uint32_t all_bits = 0;
    S->caps.resize(W);
    for (uint32_t r = 0; r < W; r++) all_bits |= tab[4 * r + 2];
    if (all_bits) return fail(h, dyn_error_status(all_bits), dyn_error_text(all_bits));  // (every rank alike: same table)
    for (uint32_t r = 0; r < W; r++) {
        if (tab[4 * r + 1] != (uint32_t)kind) return fail(h, WS_ERR_COMM, "the ranks are not in the same collective read");
        S->caps[r] = tab[4 * r + 3];
        S->counts[r] = tab[4 * r];
        total += tab[4 * r];
        max_n = std::max(max_n, tab[4 * r]);
    }
    if (total != S->n_global) return fail(h, WS_ERR_HIP, "particle count not conserved across slabs");
    max_n = (max_n + 63u) & ~63u;
    const uint32_t rw = wsk_pack_words(kind) + 1u;
    const size_t stride = (size_t)max_n * rw, each = stride * 4;
    st = S->g_send.grow_parked(h, each, 2, &S->retired, "gather buffer");  // (by half; no hipFree between the collectives of a read)
    if (st) return st;
    if (W > 1) {
        st = S->g_all.grow_parked(h, each * W, 2, &S->retired, "gather buffer");
        if (st) return st;
    }
    WsDev d = h->dev;
    d.n = h->n;
    if (kind != WS_PACK_KEY_H) refresh_pred(h, d);
    if (kind == WS_PACK_RECORD_H) {
        st = refresh_accel(h);
        if (st) return st;
    }
    wsk_slab_pack(h->stream, d, kind, h->cur, h->srt, h->accel, h->steps > S->t0, h->last_pressure, S->g_send.p);
    HIP_TRY(h, hipGetLastError());
    if (W > 1) {
        const int rc = S->tr.allgather_dev(S->tr.ctx, S->g_send.p, S->g_all.p, each, h->stream);
        if (rc) return slab_fail_tr(h, "allgather_dev", rc);
    }
    *stride_words_out = stride;
    *max_n_out = max_n;
    return WS_OK;
}

const uint32_t *slab_gathered(const WsSlab *S) { return S->world > 1 ? S->g_all.p : S->g_send.p; }

// ... scattered by id into S->g_out (n_global records of the kind's payload words) on the handle's stream
ws_status slab_gather_by_id(ws_handle *h, int kind)
{
    WsSlab *S = h->slab;
    if (h->rb_inflight)  // its device-to-host copy is still reading the id-ordered result buffer this call would rewrite
        return fail(h, WS_ERR_INVALID_ARG, "a position readback is in flight (call ws_read_positions_end first)");
    size_t stride = 0;
    uint32_t max_n = 0;
    ws_status st = slab_gather(h, kind, &stride, &max_n);
    if (st) return st;
    const uint32_t pw = wsk_pack_words(kind);
    const size_t bytes = (size_t)S->n_global * pw * 4;
    st = S->g_out.grow_parked(h, bytes, 2, &S->retired, "gather buffer");
    if (st) return st;
    wsk_slab_unpack_by_id(h->stream, slab_gathered(S), S->cnt_all.p, S->world, max_n, stride, pw, S->n_global, S->g_out.p);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

// ws_read_positions / ws_read_speeds / ws_read_particles on a slab handle.  COLLECTIVE: every rank calls it at the
// same point; every rank gets the global, id-ordered array (out == NULL: this rank only contributes).
ws_status slab_read_by_id(ws_handle *h, int kind, void *out)
{
    WsSlab *S = h->slab;
    ws_status st = slab_gather_by_id(h, kind);
    if (st) return st;
    if (out)
        HIP_TRY(h, hipMemcpyAsync(out, S->g_out.p, (size_t)S->n_global * wsk_pack_words(kind) * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WS_OK;
}

// A new smoothing radius / container on slab handles (COLLECTIVE; ws_set_params): the cell size changes, so the
// global grid, the cuts, every slab's layers and all capacities do.  Every rank gathers the full state of all
// particles -- migration generalised: any particle may change owner --, rebuilds its geometry and keeps what the
// new cuts give it.  The HUD does this on a key press (src/hud.rs:135-138), not per frame.
extern "C" ws_status ws_slab_balanced_cuts(const uint32_t *hist, uint32_t nx, uint32_t world_size, uint32_t *cuts_out);

// rebalance: keep the parameters, move the cuts so that every slab owns about n_global / world particles (the layer
// histogram is computed from the gathered state, identically on every rank).
// One word from every rank, OR-ed: the common verdict on something every rank did locally (COLLECTIVE).
// (buffers of its own: cnt_all holds the per-rank counts of the last gather, which a re-grid still needs after agreeing)
ws_status slab_agree_words(ws_handle *h, uint32_t mine, std::vector<uint32_t> *table)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    ws_status st = S->agree_send.grow(h, 16, "agreement words");
    if (!st) st = S->agree_all.grow(h, (size_t)W * 16, "agreement words");
    if (st) return st;
    wsk_set_words4(h->stream, S->agree_send.p, mine, 0u, 0u, 0u);
    HIP_TRY(h, hipGetLastError());
    const int rc = S->tr.allgather_dev(S->tr.ctx, S->agree_send.p, S->agree_all.p, 16, h->stream);
    if (rc) return slab_fail_tr(h, "allgather_dev", rc);
    table->resize((size_t)W * 4);
    HIP_TRY(h, copy_now(h, table->data(), S->agree_all.p, table->size() * 4, hipMemcpyDeviceToHost));
    return WS_OK;
}

ws_status slab_agree(ws_handle *h, uint32_t mine, uint32_t *all)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    *all = mine;
    if (W == 1) return WS_OK;
    std::vector<uint32_t> tab;
    const ws_status st = slab_agree_words(h, mine, &tab);
    if (st) return st;
    for (uint32_t r = 0; r < W; r++) *all |= tab[4 * r];
    return WS_OK;
}

// THE COMMON VERDICT of a collective call on its arguments, before it has changed anything: every rank reaches it, a
// rank that refuses included, and all refuse or go on alike -- a rank that left early would keep its peers waiting
// inside the transport (ADVICE r4).  why: this rank's argument error, or nullptr; mine: a failure that is this rank's
// alone (its scratch), with its text in h->err; hash: of its arguments (ArgHash).  One all-gather of one word, and no
// other collective: bit 0 = this rank refuses, the rest = the hash.  A rank reports, in this order: its own argument
// error, its own failure, a refusal elsewhere, a difference -- the last two as WS_ERR_INVALID_ARG in the call's words
// (VerdictText).  A single handle, or a world of one, answers for itself without a transport call.
ws_status slab_verdict(ws_handle *h, const VerdictText &text, const char *why, ws_status mine, uint32_t hash)
{
    const std::string mine_text = h->err;
    bool anybody = false, differ = false;
    if (h->slab && h->slab->world > 1) {
        const uint32_t word = (hash << 1) | ((why || mine) ? 1u : 0u);
        std::vector<uint32_t> tab;
        const ws_status st = slab_agree_words(h, word, &tab);
        if (st) return st;
        for (uint32_t r = 0; r < h->slab->world; r++) {
            anybody = anybody || (tab[4 * r] & 1u);
            differ = differ || (tab[4 * r] >> 1) != (word >> 1);
        }
    }
    if (why) return fail(h, WS_ERR_INVALID_ARG, why);
    if (mine) return fail(h, mine, mine_text.c_str());
    if (!anybody && !differ) return WS_OK;
    const std::string what = anybody ? "another slab refused its arguments" : std::string("the slabs were given different ") + text.things;
    return fail(h, WS_ERR_INVALID_ARG, (std::string(text.tag) + ": " + what + (text.mutates ? "; nothing was changed" : "")).c_str());
}

// A failure that is this rank's alone (`mine`, its text in h->err: an allocation, a copy) made common BEFORE the
// mutation, so that no peer gives its arrays up and then waits for this rank in the next collective (ADVICE r4): one
// agreement, and every rank returns -- its own failure as "<pre><text>; nothing was changed", one elsewhere as
// WS_ERR_OUT_OF_MEMORY with `elsewhere`.
ws_status slab_refuse_in_common(ws_handle *h, ws_status mine, const std::string &pre, const char *elsewhere)
{
    const std::string why = h->err;
    uint32_t anybody = 0;
    const ws_status st_agree = slab_agree(h, mine ? 1u : 0u, &anybody);
    if (st_agree) return st_agree;
    if (mine) return fail(h, mine, (pre + why + "; nothing was changed").c_str());
    if (anybody) return fail(h, WS_ERR_OUT_OF_MEMORY, elsewhere);
    return WS_OK;
}

// The same AFTER the mutation (st: this rank's reload, its text in h->err): one agreement, and if any rank failed every
// handle is DEAD -- never half-built arrays under a handle that still steps.  failed: "<this rank's step> failed";
// step: its name in a peer's message.
ws_status slab_die_in_common(ws_handle *h, ws_status st, const std::string &failed, const char *step)
{
    const std::string why = h->err;
    uint32_t anybody = 0;
    const ws_status st_agree = slab_agree(h, st ? 1u : 0u, &anybody);
    if (!st && !st_agree && !anybody) return WS_OK;
    h->dead = true;
    h->err = st ? failed + " after the old state was given up (" + why + "); the handle is unusable"
                : std::string("another slab failed its ") + step + "; the handle is unusable";
    return st ? st : (st_agree ? st_agree : WS_ERR_OUT_OF_MEMORY);
}

// Every rank must have chosen alike whatever fixes the step's collective sequence (how messages are sized, which
// stream / communicator carries the halos, whether the step is captured), the record formats and the arithmetic: a
// rank that differs would issue its size all-gathers or halos where its peers do not, and the run would hang inside
// the transport instead of failing (ADVICE r4).  One all-gather of the mode word at the end of ws_slab_create; every
// rank sees every word, so every rank fails -- or goes on -- alike.
ws_status slab_agree_mode(ws_handle *h)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    if (W == 1) return WS_OK;
    std::vector<uint32_t> tab;
    const ws_status st = slab_agree_words(h, S->mode_word, &tab);
    if (st) return st;
    for (uint32_t r = 0; r < W; r++)
        if (tab[4 * r] != S->mode_word) {
            char buf[200];
            snprintf(buf, sizeof buf, "the slabs were created with different flags / library versions: rank %u has mode word 0x%08x, rank %u has 0x%08x",
                     S->rank, S->mode_word, r, tab[4 * r]);
            return fail(h, WS_ERR_INVALID_ARG, buf);
        }
    return WS_OK;
}

// The x-layer histogram of the gathered records `recs` on the grid of `d`, on the host: the same on every rank.
// ONE histogram buffer per handle, grown by doubling (a HUD that changes the radius on every key press re-grids every
// time: round 4 allocated a new buffer per re-grid and parked it until ws_destroy); the outgrown one is parked -- the
// callers stand between collectives (WsScratch::grow_parked).  A failure here is this rank's alone -- an allocation, a
// copy -- so the callers make it common before anybody goes on: the peers would otherwise give their arrays up and wait
// for this rank in the next collective (ADVICE r4).
ws_status slab_layer_hist(ws_handle *h, const WsDev &d, const uint32_t *recs, uint32_t max_n, size_t stride, std::vector<uint32_t> *hist)
{
    WsSlab *S = h->slab;
    const size_t bytes = hist->size() * 4;
    const ws_status st = S->hist.grow_parked(h, bytes, 1, &S->retired, "x-layer histogram");
    if (st) return st;
    hipError_t e = hipMemsetAsync(S->hist.p, 0, bytes, h->stream);
    if (e == hipSuccess) {
        wsk_slab_layer_hist(h->stream, d, recs, S->cnt_all.p, S->world, max_n, stride, S->hist.p);
        e = copy_now(h, hist->data(), S->hist.p, bytes, hipMemcpyDeviceToHost);
    }
    return e == hipSuccess ? WS_OK : ws_hip_failed(h, "x-layer histogram", e);
}

ws_status slab_regrid(ws_handle *h, const ws_params *params, bool rebalance)
{
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    SlabGeometry geo;
    // Everything up to "mutation" below is decided from data every rank holds identically (the parameters, the gathered
    // state, every rank's capacity), so every rank refuses or goes on alike, and nothing has been touched when it refuses.
    ws_status st = slab_geometry(h, params, &geo, rebalance ? &S->cuts : nullptr);
    if (st) return st;
    size_t stride = 0;
    uint32_t max_n = 0;
    st = slab_gather(h, WS_PACK_STATE_H, &stride, &max_n);  // (also brings every rank's capacity: S->caps)
    if (st) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the x-layer histogram of ALL particles on the NEW grid: the same on every rank
    const uint32_t nx = (uint32_t)geo.d.gdim_x;
    std::vector<uint32_t> hist(nx);
    st = slab_refuse_in_common(h, slab_layer_hist(h, geo.d, slab_gathered(S), max_n, stride, &hist), "re-grid: ",
                               "re-grid: another slab could not build its layer histogram; nothing was changed");
    if (st) return st;
    // cuts of equal particle counts where the host asked for them -- now (ws_slab_rebalance) or earlier (a re-grid
    // keeps the fluid balanced: the rule is re-applied on the new grid instead of falling back to equal layers)
    if (rebalance || S->balanced) {
        std::vector<uint32_t> cuts(W + 1, 0);
        ws_slab_balanced_cuts(hist.data(), nx, W, cuts.data());
        if (rebalance && cuts == S->cuts) return WS_OK;  // already balanced (every rank decides alike)
        st = slab_geometry(h, params, &geo, &cuts);
        if (st) return st;
    }
    // every rank's owned count under the new cuts against every rank's capacity: all refuse alike, before the old state
    // is given up (round 3 found the overrun on the overrun rank alone, after its arrays were gone)
    for (uint32_t r = 0; r < W; r++) {
        uint64_t cnt = 0;
        for (uint32_t l = geo.cuts[r]; l < geo.cuts[r + 1]; l++) cnt += hist[l];
        if (cnt > S->caps[r]) {
            char buf[200];
            snprintf(buf, sizeof buf, "slab %u would own %llu particles on the new grid, its capacity is %u (ws_device_cfg.capacity; "
                     "ws_slab_rebalance re-cuts by particle count); nothing was changed", r, (unsigned long long)cnt, S->caps[r]);
            return fail(h, WS_ERR_OUT_OF_MEMORY, buf);
        }
    }
    // ---- mutation: from here on a failure is this rank's alone (an allocation).  It leaves the handle DEAD -- never
    //      half-built arrays under a handle that still steps -- and the verdict is made common before anybody goes on.
    slab_free_arrays(h);
    h->params = *params;
    ws_get_smoothing_kernel(params, &h->sk);
    st = slab_alloc_arrays(h, geo);
    if (!st) st = upload_mult(h);
    if (!st) st = slab_load_begin(h);
    if (!st) {
        wsk_slab_select(h->stream, h->dev, 2, S->cuts_dev, S->world, S->rank, slab_gathered(S), 0, max_n, S->cnt_all.p, stride, h->cur,
                        S->cap, S->dyn);
        if (hipGetLastError() != hipSuccess) st = fail(h, WS_ERR_HIP, "k_slab_select");
    }
    if (!st) st = slab_load_end(h);
    if ((st = slab_die_in_common(h, st, "re-grid failed", "re-grid"))) return st;
    if (rebalance) S->balanced = true;
    return WS_OK;
}

// ws_apply_forces and ws_collide_solids on slab handles (COLLECTIVE).  The re-grid's route on the UNCHANGED geometry:
// gather the state, run the definition on the gathered global set on every rank (a pure per-particle function: the same
// records and the same global sums everywhere), and reload the owned set from the edited records -- ownership follows the
// new predicted position, exactly as a host edit through ws_write_particles would have it.  No array is freed or
// allocated.  (A kernel applied in place to the steady-state arrays would have to undo migration decisions the force
// epilogue has already packed; the form that moves only the particles in reach is the scale-out follow-up: DESIGN.md 9.6.)
// The call mutates state, so its verdict is made common before anything is touched (slab_verdict).
// call: the description ws_api.cpp's edit_fluid documents (tag, things, refuse, prepare, mix, args, fetch).
template <class Call>
ws_status slab_edit_gathered(ws_handle *h, Call &call)
{
    const char *const tag = call.tag;
    WsSlab *S = h->slab;
    const uint32_t W = S->world;
    const std::string pre = std::string(tag) + ": ";
    size_t stride = 0;
    uint32_t max_n = 0;
    ws_status st = slab_gather(h, WS_PACK_STATE_H, &stride, &max_n);  // (also brings every rank's capacity: S->caps)
    if (st) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const char *why = call.refuse();
    // (this rank's alone: it refuses for all.  An edit that looks at neighbours runs its stage here, on the records just
    // gathered and with no collective call of its own: a rank that refused skips it and keeps nobody waiting.)
    const WsGathered gathered = {slab_gathered(S), S->cnt_all.p, W, max_n, stride};
    const ws_status st_cnt = !why ? call.prepare(h, &gathered) : WS_OK;
    ArgHash hash;
    call.mix(std::ref(hash), !why);
    if ((st = slab_verdict(h, {tag, call.things, true}, why, st_cnt, hash.word))) return st;
    uint32_t *recs = const_cast<uint32_t *>(slab_gathered(S));  // (scratch of the gather: nothing the step reads)
    // the edit, and the x-layer histogram of the edited set: every slab's owned count under the cuts against every slab's
    // capacity, all alike, before the old state is given up (slab_regrid).  A failure in here is this rank's alone and is
    // made common before anybody goes on.
    const uint32_t nx = (uint32_t)h->dev.gdim_x;
    std::vector<uint32_t> hist(nx);
    wsk_edit_records(h->stream, h->dev, recs, S->cnt_all.p, W, max_n, stride, call.args);
    ws_status mine = slab_layer_hist(h, h->dev, recs, max_n, stride, &hist);
    if (!mine) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = call.fetch(h);
        if (e != hipSuccess) mine = ws_hip_failed(h, "edit of the gathered state", e);
    }
    st = slab_refuse_in_common(h, mine, pre, (pre + "another slab could not edit the gathered state; nothing was changed").c_str());
    if (st) return st;
    for (uint32_t r = 0; r < W; r++) {
        uint64_t cnt = 0;
        for (uint32_t l = S->cuts[r]; l < S->cuts[r + 1] && l < nx; l++) cnt += hist[l];
        if (cnt > S->caps[r]) {
            char buf[200];
            snprintf(buf, sizeof buf, "%s: slab %u would own %llu particles, its capacity is %u (ws_device_cfg.capacity); nothing was changed",
                     tag, r, (unsigned long long)cnt, S->caps[r]);
            return fail(h, WS_ERR_OUT_OF_MEMORY, buf);
        }
    }
    // ---- mutation: the re-grid's tail on the unchanged geometry
    st = slab_load_begin(h);
    if (!st) {
        wsk_slab_select(h->stream, h->dev, 2, S->cuts_dev, W, S->rank, recs, 0, max_n, S->cnt_all.p, stride, h->cur, S->cap, S->dyn);
        if (hipGetLastError() != hipSuccess) st = fail(h, WS_ERR_HIP, "k_slab_select");
    }
    if (!st) st = slab_load_end(h);
    return slab_die_in_common(h, st, pre + "the reload failed", "reload");
}

// ws_sample_density_* on a slab handle (COLLECTIVE): every rank's current positions all-gathered by id into S->g_out
// (what ws_read_positions does) and the GLOBAL single-GPU grid, so that the single-GPU binning and sampler run on the
// whole particle set -- bit-identical to a single handle by construction.  (A ghost-layer sampler that avoids the
// all-gather is the scale-out follow-up: DESIGN.md 8.)
// with_vel (the velocity calls): {position, velocity} records instead, 6 floats per id, for wsk_field_split.
ws_status slab_field_positions(ws_handle *h, const float **xyz, WsDev *global, bool with_vel)
{
    WsSlab *S = h->slab;
    ws_status st = slab_gather_by_id(h, with_vel ? WS_PACK_POSVEL_H : WS_PACK_POS_H);
    if (st) return st;
    st = global_grid(&h->params, S->n_global, global);
    if (st) return fail(h, st, g_create_error.c_str());
    *xyz = reinterpret_cast<const float *>(S->g_out.p);
    return WS_OK;
}

}  // namespace

extern "C" {

ws_status ws_slab_assign(const ws_params *params, const float *pos_xyz, uint32_t n, uint32_t world_size,
                         uint32_t *out_rank)
{
    if (!pos_xyz || !out_rank || world_size == 0) return WS_ERR_INVALID_ARG;
    ws_status st = validate_params(nullptr, params);
    if (st) return st;
    WsDev g;
    st = global_grid(params, n, &g);
    if (st) return st;
    const uint32_t nx = (uint32_t)g.dim[0];
    if (world_size > nx) return fail(nullptr, WS_ERR_INVALID_ARG, "more slabs than cell layers along x");
    for (uint32_t i = 0; i < n; i++) {
        const float fx = floorf(pos_xyz[3 * (size_t)i] / g.h) - (float)g.org[0];
        const uint32_t gx = (uint32_t)((int)fminf(fmaxf(fx, 0.0f), (float)(g.fdim[0] - 1)) / g.cm[0]);  // grid_layer_x
        uint32_t r = 0;
        while (r + 1 < world_size && gx >= (uint32_t)((uint64_t)(r + 1) * nx / world_size)) r++;
        out_rank[i] = r;
    }
    return WS_OK;
}

ws_status ws_slab_create(const ws_params *params, const float *pos_xyz, const uint32_t *ids, uint32_t n_local,
                         uint32_t n_global, const ws_device_cfg *cfg, const ws_transport *transport, ws_handle **out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    *out = nullptr;
    if (transport && transport->struct_size < sizeof(ws_transport))
        return fail(nullptr, WS_ERR_INVALID_ARG,
                    "ws_transport.struct_size is smaller than this library's ws_transport (a host built against ABI version 1?)");
    if (!cfg || !transport || !transport->sendrecv || !transport->allgather_dev || (cfg->world_size > 1 && !transport->alltoall_dev))
        return fail(nullptr, WS_ERR_INVALID_ARG, "slab needs a device cfg and a complete transport (sendrecv, allgather_dev, alltoall_dev)");
    if (n_local && (!pos_xyz || !ids)) return fail(nullptr, WS_ERR_INVALID_ARG, "pos_xyz / ids missing");
    if (cfg->world_size < 1 || cfg->rank >= cfg->world_size || n_global == 0)
        return fail(nullptr, WS_ERR_INVALID_ARG, "bad rank / world_size / n_global");
    if (cfg->world_size > 1024)
        return fail(nullptr, WS_ERR_UNSUPPORTED, "more than 1024 slabs (one workgroup reads every rank's status row)");
    if (cfg->flags & WS_FLAG_REFERENCE_ORDER)
        return fail(nullptr, WS_ERR_UNSUPPORTED, "the reference-order validation mode is single-GPU only");
    ws_status st = validate_params(nullptr, params);
    if (st) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, WS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, WS_ERR_NO_DEVICE, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, WS_ERR_NO_DEVICE, "device is not gfx950 (kernels are built for MI355X only)");

    ws_handle *h = new (std::nothrow) ws_handle();
    WsSlab *S = new (std::nothrow) WsSlab();
    if (!h || !S) {
        delete h;
        delete S;
        return fail(nullptr, WS_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    h->slab = S;
    h->device = cfg->device;
    h->flags = cfg->flags;
    h->params = *params;
    h->n = n_local;
    configure_kernels(h);
    if (h->flags & WS_FLAG_GRAPH) h->flags &= ~(uint32_t)WS_FLAG_PROFILE;  // event brackets are not part of a captured step
    S->tr = *transport;
    S->rank = cfg->rank;
    S->world = cfg->world_size;
    S->n_global = n_global;
    S->cap = cfg->capacity ? cfg->capacity : 2 * n_local + (1u << 20);
    if (S->cap < n_local) S->cap = n_local;
    S->cfg_ghost_capacity = cfg->ghost_capacity;
    const uint32_t W = S->world;

    auto bail = [&](ws_status s_) {
        g_create_error = h->err;
        free_all(h);
        delete h;
        return s_;
    };
    SlabGeometry geo;
    CREATE_TRY(slab_geometry(h, params, &geo));
    CREATE_HIP(hipSetDevice(cfg->device));
    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
        h->own_stream = false;
    } else {
        CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    }
    CREATE_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
    ws_rccl_transport_bind_stream(&S->tr, h->stream);  // (the library's own RCCL transport: one communicator per stream)
    ws_get_smoothing_kernel(params, &h->sk);
    CREATE_TRY(h->fixed.alloc(h, &h->stats, 64, "device counters", true));
    CREATE_TRY(S->fixed.alloc(h, &S->dyn, WS_DYN_WORDS * 4, "slab state words", true));
    const size_t status_words = (size_t)kStatusSlots * W * WS_HDR_WORDS_HOST;
    CREATE_TRY(S->fixed.alloc(h, &S->status_dev, status_words * 4, "status ring", true));
    CREATE_TRY(S->status_host.alloc(h, status_words * 4, "page-locked status ring"));
    memset(S->status_host.p, 0, status_words * 4);
    for (hipEvent_t *e : {&S->ev_sorted, &S->ev_halo_a, &S->ev_k4_late, &S->ev_halo_b, &S->ev_filled, &S->ev_copied})
        CREATE_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (hipEvent_t &e : S->ev_status) CREATE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    {
        // The communication stream gets the HIGHEST priority: halo pack -> transport -> unpack are a few short kernels
        // that run behind an early K4 which fills every CU with one-wave workgroups; at the step stream's priority
        // their workgroups queue up behind K4's (the runtime multiplexes the streams of one priority onto the same few
        // hardware queues: ws_api.cpp, the readback's copy stream).  Developer builds: WS_SLAB_COMM_PRIORITY=default
        // keeps the step stream's priority (A/B runs).
        int lo = 0, hi = 0;
        const char *pr = WS_DEV_ENV("WS_SLAB_COMM_PRIORITY");
        if (pr && strcmp(pr, "default") == 0) {
            CREATE_HIP(hipStreamCreateWithFlags(&S->comm, hipStreamNonBlocking));
        } else {
            CREATE_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));  // (numerically lowest = highest priority)
            CREATE_HIP(hipStreamCreateWithPriority(&S->comm, hipStreamNonBlocking, hi));
        }
    }
    CREATE_HIP(hipStreamCreateWithFlags(&S->copy, hipStreamNonBlocking));
    // halo / compute overlap: on unless WS_FLAG_NO_OVERLAP
    S->overlap = !(cfg->flags & WS_FLAG_NO_OVERLAP);
    // How the messages are sized (include/wsfluid.h): exact (the default; host-synchronised, cannot be captured),
    // lagged (WS_FLAG_LAGGED_MESSAGES: the bet), fixed (WS_FLAG_FIXED_MESSAGES: always the capacities).  A captured
    // step (WS_FLAG_GRAPH) with peers takes FIXED sizes unless the host asks for the lagged ones with it: nothing can
    // overrun below the capacities and the graph is never re-captured for a size (VERDICT r4 item 5; the lagged rule
    // overran in 27 of 100 violent random cases).  A world of one exchanges nothing: its captured step keeps the
    // lagged bookkeeping (smaller launch bounds).
    const bool want_graph = (cfg->flags & WS_FLAG_GRAPH) != 0, want_lagged = (cfg->flags & WS_FLAG_LAGGED_MESSAGES) != 0;
    S->fixed_messages = (cfg->flags & WS_FLAG_FIXED_MESSAGES) != 0 || (want_graph && W > 1 && !want_lagged);
    S->exact_messages = (cfg->flags & WS_FLAG_EXACT_MESSAGES) != 0 || !(want_lagged || want_graph || S->fixed_messages);
    if (cfg->flags & WS_FLAG_EXACT_MESSAGES) S->fixed_messages = false;
    S->mode_word = (S->exact_messages ? 1u : 0u) | (S->fixed_messages ? 2u : 0u) | (S->overlap ? 4u : 0u) | (want_graph ? 8u : 0u) |
                   ((cfg->flags & WS_FLAG_GRAPH_MULTIRANK) ? 16u : 0u) | ((cfg->flags & WS_FLAG_IEEE_DIVISION) ? 32u : 0u) |
                   (WS_HDR_WORDS_HOST << 8) | (WS_MIG_REC_WORDS_HOST << 16) | ((uint32_t)WS_ABI_VERSION << 24);
    if (S->exact_messages) {
        S->fixed_messages = true;
        for (int k = 0; k < 2; k++) {
            CREATE_TRY(S->fixed.alloc(h, &S->xs_send[k], 16, "message sizes"));
            CREATE_TRY(S->fixed.alloc(h, &S->xs_all[k], (size_t)W * 16, "message sizes"));
            CREATE_TRY(S->xs_host[k].alloc(h, (size_t)W * 16, "page-locked message sizes"));
            CREATE_HIP(hipEventCreateWithFlags(&S->ev_sizes[k], hipEventDisableTiming));
        }
    }
    // (developer builds: the floors of the message sizes, records)
    if (const char *v = WS_DEV_ENV("WS_SLAB_FLOOR_MIGRATION")) S->floor_mig = (uint32_t)std::max(1, atoi(v));
    if (const char *v = WS_DEV_ENV("WS_SLAB_FLOOR_FAR")) S->floor_far = (uint32_t)std::max(1, atoi(v));
    if (const char *v = WS_DEV_ENV("WS_SLAB_FLOOR_HALO")) S->floor_halo = ((uint32_t)std::max(64, atoi(v)) + 63u) & ~63u;
    CREATE_TRY(slab_alloc_arrays(h, geo));
    CREATE_TRY(upload_mult(h));
    // upload this slab's particles at the owned base; the first ws_step migrates (a no-op when the
    // caller followed ws_slab_assign) and bins them
    CREATE_TRY(slab_load_begin(h));
    if (n_local) {
        const size_t pb = (size_t)n_local * 12, ib = (size_t)n_local * 4;
        CREATE_TRY(ensure_stage(h, pb + ib));
        CREATE_HIP(hipMemcpyAsync(h->stage, pos_xyz, pb, hipMemcpyHostToDevice, h->stream));
        CREATE_HIP(hipMemcpyAsync((char *)h->stage + pb, ids, ib, hipMemcpyHostToDevice, h->stream));
        const uint32_t base = h->dev.base;
        WsSoA cur_owned = {h->cur.pv + 2 * (size_t)base, h->cur.pred + base, nullptr};
        wsk_upload_positions_ids(h->stream, (const float *)h->stage, (const uint32_t *)((char *)h->stage + pb), cur_owned,
                                 n_local);
        CREATE_HIP(hipGetLastError());
        CREATE_HIP(hipMemcpyAsync(S->dyn + DY_N, &n_local, 4, hipMemcpyHostToDevice, h->stream));
    }
    CREATE_TRY(slab_load_end(h));
    CREATE_TRY(slab_agree_mode(h));
    *out = h;
    return WS_OK;
}

ws_status ws_slab_read_particles(ws_handle *h, ws_particle80 *out, uint32_t *out_ids, uint32_t cap, uint32_t *n_out)
{
    if (!h || !h->slab || !out || !out_ids || !n_out) return WS_ERR_INVALID_ARG;
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    ws_status st = slab_settle(h);  // the owned count lives on the device
    if (st) return st;
    if (h->n > cap) return fail(h, WS_ERR_INVALID_ARG, "output buffers smaller than the owned particle count");
    *n_out = h->n;
    if (!h->n) return WS_OK;
    const size_t pb = (size_t)h->n * sizeof(ws_particle80), ib = (size_t)h->n * 4;
    st = ensure_stage(h, pb + ib);
    if (st) return st;
    WsDev d = h->dev;
    d.n = h->n;
    refresh_pred(h, d);
    st = refresh_accel(h);
    if (st) return st;
    wsk_gather_slab(h->stream, d, h->cur, h->srt, h->accel, h->steps > h->slab->t0, h->last_pressure, (ws_particle80 *)h->stage,
                    (uint32_t *)((char *)h->stage + pb));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->stage, pb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out_ids, (char *)h->stage + pb, ib, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

// Host-only: cuts of (about) equal particle counts from an x-layer histogram.  cut r = the first layer at which the
// running count passes r / W of the particles; cuts stay strictly increasing (every slab keeps at least one layer)
// and leave room for the slabs still to come.  Deterministic: every rank computes the same cuts from the same histogram.
ws_status ws_slab_balanced_cuts(const uint32_t *hist, uint32_t nx, uint32_t world_size, uint32_t *cuts_out)
{
    if (!hist || !cuts_out || world_size == 0 || world_size > nx) return WS_ERR_INVALID_ARG;
    uint64_t total = 0;
    for (uint32_t l = 0; l < nx; l++) total += hist[l];
    cuts_out[0] = 0;
    uint64_t run = 0;
    uint32_t layer = 0;
    for (uint32_t r = 1; r < world_size; r++) {
        const uint64_t want = total * r / world_size;
        while (layer < nx && run + hist[layer] <= want) run += hist[layer++];
        uint32_t c = std::max(layer, cuts_out[r - 1] + 1u);
        c = std::min(c, nx - (world_size - r));
        while (layer < c) run += hist[layer++];
        cuts_out[r] = c;
    }
    cuts_out[world_size] = nx;
    return WS_OK;
}

ws_status ws_slab_rebalance(ws_handle *h)
{
    if (!h) return WS_ERR_INVALID_ARG;
    if (!h->slab) return fail(h, WS_ERR_INVALID_ARG, "not a slab handle");
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    return slab_regrid(h, &h->params, true);
}

ws_status ws_slab_counters(ws_handle *h, uint64_t out[4])
{
    if (!h || !out) return WS_ERR_INVALID_ARG;
    if (!h->slab) return fail(h, WS_ERR_INVALID_ARG, "not a slab handle");
    WS_DEAD_CHECK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    const ws_status st = slab_settle(h);
    if (st) return st;
    uint32_t dyn[WS_DYN_WORDS];
    HIP_TRY(h, copy_now(h, dyn, h->slab->dyn, sizeof dyn, hipMemcpyDeviceToHost));
    out[0] = dyn[DY_N];
    out[1] = h->slab->left_base + dyn[DY_LEFT];
    out[2] = h->slab->arrived_base + dyn[DY_ARRIVED];
    out[3] = h->slab->far_base + dyn[DY_FAR];
    return WS_OK;
}

}  // extern "C"
