// ws_field.inc -- the derived-field calls of include/wsfluid.h (density field, surface, anisotropic kernels, rays, velocity
// field and advection, whitewater, bodies): host-only, part of ws_api.cpp's translation unit.  Every call is a list of stages over
// ws_handle::field (ws_internal.h WsField):
//   field_enter         dead handle, reference-order mode, nothing wanted on a single handle
//   field_source        the collective protocol and the inputs by id: positions, on request velocities
//   field_bin_particles the counting sort of the positions by cell (field_bin) and the gathers into cell order
//   field_aniso_stage   the anisotropic per-particle stage;  field_aniso_bin: its centres binned the same way
//   field_sample ...    the call's own kernels over the binning
//   field_finish        results out, synchronise, profile
// (SURVEY 8(f) row 2: readback / render coupling.)

// ---- scratch ---------------------------------------------------------------------------------------------------------
// Every allocation of the layer is a WsScratch of ws_handle::field (ws_internal.h): a failure leaves no sticky HIP error
// behind (the next ws_step checks hipGetLastError), so the handle stays usable.
namespace {

constexpr const char *kFieldScratch = "density field scratch";

void free_field_cells(ws_handle *h)
{
    auto &F = h->field;
    release_all(F.count, F.cursor, F.start, F.bsum);
    F.cells = 0;
}

void free_field(ws_handle *h)
{
    auto &F = h->field;
    release_all(F.sattr[0], F.sattr[1], F.srho, F.aval);
    release_all(F.body, F.cnd, F.crec, F.cst, F.cnb);
    free_field_cells(h);
    release_all(F.xyz, F.keys, F.tmp, F.perm, F.spos, F.q, F.rho, F.grad, F.code, F.vbase, F.bcnt, F.bstart, F.bstate, F.tri,
                F.mxyz, F.mnrm, F.vxyz, F.vpos, F.svel, F.wnrm, F.wst, F.wout, F.wpt, F.wnb, F.wcnt, F.woff, F.wstate, F.cxyz,
                F.amf, F.smf, F.anb, F.rays, F.ray_t, F.ray_n);
    F.n = 0;
}

// The exact-size groups: the per-particle arrays of n particles, the per-cell tables of ncells cells.
ws_status field_alloc(ws_handle *h, uint32_t n, uint32_t ncells)
{
    auto &F = h->field;
    ws_status st = WS_OK;
    if (F.n != n) {
        free_field(h);
        if (!h->slab) st = F.xyz.alloc(h, (size_t)n * 12, kFieldScratch);
        if (!st) st = F.keys.alloc(h, (size_t)n * 4, kFieldScratch);
        if (!st) st = F.tmp.alloc(h, (size_t)n * 4, kFieldScratch);
        if (!st) st = F.perm.alloc(h, (size_t)n * 4, kFieldScratch);
        if (!st) st = F.spos.alloc(h, (size_t)n * 16, kFieldScratch);
        if (st) {
            free_field(h);
            return st;
        }
        F.n = n;
    }
    if (F.cells != ncells) {  // (new handle, or a re-grid since the last call)
        free_field_cells(h);
        const size_t sw = (size_t)wsk_scan_state_words(ncells) * 4;
        st = F.count.alloc(h, (size_t)ncells * 4, kFieldScratch);
        if (!st) st = F.cursor.alloc(h, (size_t)ncells * 4, kFieldScratch);
        if (!st) st = F.start.alloc(h, ((size_t)ncells + 1) * 4, kFieldScratch);
        if (!st) st = F.bsum.alloc(h, sw, kFieldScratch);
        if (!st && hipMemsetAsync(F.bsum.p, 0, sw, h->stream) != hipSuccess) st = fail(h, WS_ERR_HIP, "density field scan state");
        if (!st && hipMemcpyAsync(F.start.p + ncells, &n, 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)
            st = fail(h, WS_ERR_HIP, "density field cell starts");
        if (!st && hipStreamSynchronize(h->stream) != hipSuccess) st = fail(h, WS_ERR_HIP, "density field scratch");
        if (st) {
            free_field_cells(h);
            return st;
        }
        F.cells = ncells;
    }
    return WS_OK;
}

// ---- queries ---------------------------------------------------------------------------------------------------------
// The query of a sample call: a grid (origin + spacing in g6, dims; nodes x fastest) or m points of xyz.
struct FieldQuery {
    bool grid = false;
    bool given = false;  // grid form: origin, spacing and dims were all passed (g6 / dims hold placeholders otherwise)
    float g6[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
    uint32_t dims[3] = {0u, 0u, 0u};
    const float *xyz = nullptr;
    uint32_t m = 0;

    // A slab rank that only contributes may pass no query: it still takes part in the gather, with a placeholder of
    // `least` nodes per axis (the smallest grid the call accepts) that no kernel ever sees.
    static FieldQuery of_grid(const float *origin, const float *spacing, const uint32_t *dims, uint32_t least)
    {
        FieldQuery q;
        q.grid = true;
        q.given = origin && spacing && dims;
        for (int a = 0; a < 3; a++) {
            if (q.given) {
                q.g6[a] = origin[a];
                q.g6[3 + a] = spacing[a];
            }
            q.dims[a] = q.given ? dims[a] : least;
        }
        return q;
    }
    static FieldQuery of_points(const float *xyz, uint32_t m)
    {
        FieldQuery q;
        q.xyz = xyz;
        q.m = m;
        return q;
    }
    const float *grid6() const { return grid ? g6 : nullptr; }
    const uint32_t *dims3() const { return grid ? dims : nullptr; }
    uint64_t count() const { return grid ? (uint64_t)dims[0] * dims[1] * dims[2] : m; }
    // the brick kernel from one node per cell up (spacing <= h on every axis); the points form below
    bool bricks(const WsDev &d) const { return grid && g6[3] <= d.h && g6[4] <= d.h && g6[5] <= d.h; }
};

ws_status field_check(ws_handle *h, const FieldQuery &q)
{
    if (q.grid) {
        uint64_t nodes = 1;
        for (int a = 0; a < 3; a++) {
            if (!isfinite(q.g6[a])) return fail(h, WS_ERR_INVALID_ARG, "density field: origin must be finite");
            if (!(q.g6[3 + a] > 0.0f) || !isfinite(q.g6[3 + a]))
                return fail(h, WS_ERR_INVALID_ARG, "density field: spacing must be finite and > 0");
            if (q.dims[a] == 0u) return fail(h, WS_ERR_INVALID_ARG, "density field: dims must be >= 1");
            nodes *= q.dims[a];
        }
        if (nodes > (1ull << 31)) return fail(h, WS_ERR_INVALID_ARG, "density field: more than 2^31 nodes");
    } else {
        if (!q.xyz || q.m == 0u) return fail(h, WS_ERR_INVALID_ARG, "density field: no points");
        for (size_t t = 0; t < (size_t)q.m * 3; t++)
            if (!isfinite(q.xyz[t])) return fail(h, WS_ERR_INVALID_ARG, "density field: points must be finite");
    }
    return WS_OK;
}

// The points of a query into F.q.
ws_status field_upload(ws_handle *h, const FieldQuery &q)
{
    auto &F = h->field;
    const ws_status st = F.q.grow(h, (size_t)q.m * 12, kFieldScratch);
    if (st) return st;
    HIP_TRY(h, hipMemcpyAsync(F.q.p, q.xyz, (size_t)q.m * 12, hipMemcpyHostToDevice, h->stream));
    return WS_OK;
}

// The anisotropy parameters of a call (include/wsfluid.h ws_aniso_params).
ws_status aniso_check(ws_handle *h, const ws_aniso_params *a)
{
    if (!a) return fail(h, WS_ERR_INVALID_ARG, "anisotropy: the parameters are required");
    if (!isfinite(a->smoothing) || !isfinite(a->max_ratio) || !isfinite(a->lone_scale))
        return fail(h, WS_ERR_INVALID_ARG, "anisotropy: parameters must be finite");
    if (!(a->smoothing >= 0.0f && a->smoothing <= 1.0f)) return fail(h, WS_ERR_INVALID_ARG, "anisotropy: smoothing must lie in [0, 1]");
    if (!(a->max_ratio >= 1.0f)) return fail(h, WS_ERR_INVALID_ARG, "anisotropy: max_ratio must be >= 1");
    if (!(a->lone_scale > 0.0f && a->lone_scale <= 1.0f)) return fail(h, WS_ERR_INVALID_ARG, "anisotropy: lone_scale must lie in (0, 1]");
    return WS_OK;
}

// Which field a call evaluates: the SPH density of the particles, or the anisotropic kernels around their centres.
enum FieldKind { FIELD_ISOTROPIC, FIELD_ANISOTROPIC };
// What field_source brings by id.
enum FieldInputs { FIELD_POSITIONS, FIELD_POSITIONS_AND_VELOCITIES };

// ---- stages ----------------------------------------------------------------------------------------------------------
// What a call's stages share: whether the caller passed any output, and after field_source the grid the particles are
// binned on, their positions by id and their number.
struct FieldCtx {
    bool want = false;
    WsDev d;
    const float *pos = nullptr;
    uint32_t n = 0;
    FieldInputs inputs = FIELD_POSITIONS;
    bool contributed = false;  // a slab rank that wants nothing took part in the gather and has nothing more to do
};

// The preamble of every call, in this order: a dead handle, the reference-order validation mode (`name` leads its
// message), and on a single handle a call that wants nothing (none_msg; nullptr: the caller has a rule of its own).
ws_status field_enter(ws_handle *h, const FieldCtx &c, const char *name, const char *none_msg)
{
    WS_DEAD_CHECK(h);
    if (h->flags & WS_FLAG_REFERENCE_ORDER) return reference_order_refused(h, name);
    if (none_msg && !c.want && !h->slab) return fail(h, WS_ERR_INVALID_ARG, none_msg);
    return WS_OK;
}

// The inputs by id.  check() validates the query: before anything else on a single handle, after the collective gather
// on a slab rank (a rank with a bad query leaves no peer waiting).  With velocities: by id in F.vxyz; a slab gathers
// {position, velocity} records once and splits them into F.vpos / F.vxyz.
template <class Check>
ws_status field_source(ws_handle *h, FieldCtx *c, FieldInputs inputs, Check check)
{
    c->inputs = inputs;
    c->contributed = false;
    const bool vel = inputs == FIELD_POSITIONS_AND_VELOCITIES;
    if (!h->slab && c->want) {
        const ws_status st = check();
        if (st) return st;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    c->d = h->dev;
    c->n = h->n;
    if (h->slab) {
        ws_status st = slab_field_positions(h, &c->pos, &c->d, vel);
        if (st) return st;
        c->n = h->slab->n_global;
        if (!c->want) {
            HIP_TRY(h, hipStreamSynchronize(s));
            c->contributed = true;
            return WS_OK;
        }
        st = check();
        if (st) {
            HIP_TRY(h, hipStreamSynchronize(s));
            return st;
        }
    }
    auto &F = h->field;
    const size_t n = c->n;
    ws_status st = field_alloc(h, c->n, c->d.ncells);
    if (st) return st;
    if (!h->slab) {
        wsk_gather_positions(s, h->cur, F.xyz.p, c->n);
        c->pos = F.xyz.p;
    }
    if (vel) {
        if ((st = F.vxyz.grow(h, n * 12, kFieldScratch))) return st;
        if ((st = F.svel.grow(h, n * 16, kFieldScratch))) return st;
        if (h->slab) {
            if ((st = F.vpos.grow(h, n * 12, kFieldScratch))) return st;
            wsk_field_split(s, c->pos, F.vpos.p, F.vxyz.p, c->n);
            c->pos = F.vpos.p;
        } else {
            wsk_gather_velocities(s, h->cur, F.vxyz.p, c->n);
        }
    }
    return WS_OK;
}

// Counting sort of n points by cell, ascending id inside a cell (the sort view's passes on the layer's own arrays):
// F.start = the cells' first slots, F.perm = the ids in cell order.
ws_status field_bin(ws_handle *h, const FieldCtx &c, const float *xyz)
{
    auto &F = h->field;
    hipStream_t s = h->stream;
    wsk_field_keys(s, c.d, xyz, F.keys.p, c.n);
    HIP_TRY(h, hipMemsetAsync(F.count.p, 0, (size_t)c.d.ncells * 4, s));
    wsk_view_count(s, F.keys.p, F.count.p, c.n);
    wsk_scan(s, F.count.p, F.start.p, F.cursor.p, F.bsum.p, c.d.ncells, false, 0);
    wsk_scatter(s, F.keys.p, F.cursor.p, F.tmp.p, c.n, nullptr);
    wsk_view_fix(s, F.tmp.p, F.keys.p, F.start.p, F.perm.p, c.n);
    return WS_OK;
}

// The particles binned: F.spos = {position, id} in cell order, with velocities F.svel beside it.
ws_status field_bin_particles(ws_handle *h, const FieldCtx &c)
{
    auto &F = h->field;
    const ws_status st = field_bin(h, c, c.pos);
    if (st) return st;
    wsk_field_gather(h->stream, F.perm.p, c.pos, F.spos.p, c.n);
    if (c.inputs == FIELD_POSITIONS_AND_VELOCITIES) wsk_field_gather_vel(h->stream, F.perm.p, F.vxyz.p, F.svel.p, c.n);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

// The anisotropic per-particle stage over the binned positions: F.cxyz, F.amf and F.anb by id.
ws_status field_aniso_stage(ws_handle *h, const FieldCtx &c, const ws_aniso_params *ap)
{
    auto &F = h->field;
    const size_t n = c.n;
    ws_status st;
    if ((st = F.cxyz.grow(h, n * 12, kFieldScratch))) return st;
    if ((st = F.amf.grow(h, n * 32, kFieldScratch))) return st;
    if ((st = F.anb.grow(h, n * 4, kFieldScratch))) return st;
    const WsAnisoParams a = {ap->smoothing, ap->max_ratio, ap->lone_scale, ap->min_neighbours};
    wsk_aniso(h->stream, c.d, F.start.p, F.spos.p, a, F.cxyz.p, F.amf.p, F.anb.p, c.n);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

// The centres binned by the same passes: F.spos = {centre, id} and F.smf in THEIR cell order.  The positions' binning is
// consumed (the stage ran before, in stream order).
ws_status field_aniso_bin(ws_handle *h, const FieldCtx &c)
{
    auto &F = h->field;
    ws_status st;
    if ((st = F.smf.grow(h, (size_t)c.n * 32, kFieldScratch))) return st;
    if ((st = field_bin(h, c, F.cxyz.p))) return st;
    wsk_aniso_gather(h->stream, F.perm.p, F.cxyz.p, F.amf.p, F.spos.p, F.smf.p, c.n);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

// The binning of a call that evaluates `kind`: the particles, and for the anisotropic field the stage and its centres.
ws_status field_bin_kind(ws_handle *h, const FieldCtx &c, FieldKind kind, const ws_aniso_params *ap)
{
    ws_status st = field_bin_particles(h, c);
    if (st || kind == FIELD_ISOTROPIC) return st;
    if ((st = field_aniso_stage(h, c, ap))) return st;
    return field_aniso_bin(h, c);
}

// The field of `kind` at the query into *rho and *grad (nullptr: not wanted), nodes x fastest or the m points.
ws_status field_sample(ws_handle *h, const FieldCtx &c, const FieldQuery &q, FieldKind kind, WsScratch<float> *rho,
                       WsScratch<float> *grad)
{
    auto &F = h->field;
    const uint64_t nq = q.count();
    ws_status st;
    if (!q.grid && (st = field_upload(h, q))) return st;
    if (rho && (st = rho->grow(h, (size_t)nq * 4, kFieldScratch))) return st;
    if (grad && (st = grad->grow(h, (size_t)nq * 12, kFieldScratch))) return st;
    wsk_field_sample(h->stream, c.d, F.start.p, F.spos.p, kind == FIELD_ANISOTROPIC ? F.smf.p : nullptr, h->ieee, grad != nullptr,
                     F.q.p, (uint32_t)nq, q.grid6(), q.dims3(), q.bricks(c.d), rho ? rho->p : nullptr, grad ? grad->p : nullptr);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

// The end of a call: the results that have a destination copied out, the stream synchronised, the profile drained.
struct FieldCopy {
    void *dst;
    const void *src;
    size_t bytes;
};

ws_status field_finish(ws_handle *h, std::initializer_list<FieldCopy> out)
{
    for (const FieldCopy &c : out)
        if (c.dst) HIP_TRY(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_profile(h);
    return WS_OK;
}

// ---- density field, isotropic or anisotropic --------------------------------------------------------------------------
// Both sample calls: the field into device scratch, then copied out.
ws_status sample_density(ws_handle *h, const FieldQuery &q, FieldKind kind, const ws_aniso_params *ap, float *out_rho,
                         float *out_grad)
{
    FieldCtx c;
    c.want = out_rho || out_grad;
    if (q.grid && !q.given && (c.want || !h->slab))
        return fail(h, WS_ERR_INVALID_ARG, "density field: origin, spacing and dims are required");
    ws_status st = field_enter(h, c, "density field", "density field: both outputs are NULL");
    if (st) return st;
    auto check = [&]() -> ws_status {
        if (kind == FIELD_ANISOTROPIC) {
            const ws_status bad = aniso_check(h, ap);
            if (bad) return bad;
        }
        return field_check(h, q);
    };
    st = field_source(h, &c, FIELD_POSITIONS, check);
    if (st || c.contributed) return st;
    auto &F = h->field;
    if ((st = field_bin_kind(h, c, kind, ap))) return st;
    if ((st = field_sample(h, c, q, kind, out_rho ? &F.rho : nullptr, out_grad ? &F.grad : nullptr))) return st;
    const size_t nq = (size_t)q.count();
    return field_finish(h, {{out_rho, F.rho.p, nq * 4}, {out_grad, F.grad.p, nq * 12}});
}

// ws_extract_surface / ws_extract_aniso_surface: the grid field into device scratch, the node codes and per-workgroup
// totals, their scans, the counts back to the host and -- when the caller's buffers hold them -- the mesh.  A slab rank
// without a query still takes part in the gather, then fails.
ws_status extract_surface(ws_handle *h, const FieldQuery &q, FieldKind kind, const ws_aniso_params *ap, float iso, uint32_t max_v,
                          uint32_t max_t, float *out_xyz, float *out_nrm, uint32_t *out_tri, uint32_t *n_v, uint32_t *n_t)
{
    if (!q.given && !h->slab) return fail(h, WS_ERR_INVALID_ARG, "surface: origin, spacing and dims are required");
    FieldCtx c;
    c.want = out_xyz || out_nrm || out_tri || n_v || n_t;
    ws_status st = field_enter(h, c, "surface", nullptr);
    if (st) return st;
    // a single handle always wants the counts (field_source validates a single handle's query only if it wants)
    if (!h->slab && (!n_v || !n_t)) return fail(h, WS_ERR_INVALID_ARG, "surface: the count pointers are required");
    auto check = [&]() -> ws_status {
        if (!q.given) return fail(h, WS_ERR_INVALID_ARG, "surface: origin, spacing and dims are required");
        if (!n_v || !n_t) return fail(h, WS_ERR_INVALID_ARG, "surface: the count pointers are required");
        uint64_t nodes = 1;
        for (int a = 0; a < 3; a++) {
            if (q.dims[a] < 2u) return fail(h, WS_ERR_INVALID_ARG, "surface: dims must be >= 2");
            nodes *= q.dims[a];
        }
        if (nodes > (1ull << 28)) return fail(h, WS_ERR_INVALID_ARG, "surface: more than 2^28 nodes");
        if (!(iso > 0.0f) || !isfinite(iso)) return fail(h, WS_ERR_INVALID_ARG, "surface: iso must be finite and > 0");
        if (kind == FIELD_ANISOTROPIC) {
            const ws_status bad = aniso_check(h, ap);
            if (bad) return bad;
        }
        return field_check(h, q);
    };
    st = field_source(h, &c, FIELD_POSITIONS, check);
    if (st || c.contributed) return st;
    auto &F = h->field;
    // the gradient only for a call that asks for normals and passes both mesh buffers (a call whose counts then exceed
    // its capacities has sampled it for nothing; FluidWorker sizes its first guess from the previous mesh)
    const bool grad_on = out_nrm && out_xyz && out_tri;
    if ((st = field_bin_kind(h, c, kind, ap))) return st;
    if ((st = field_sample(h, c, q, kind, &F.rho, grad_on ? &F.grad : nullptr))) return st;
    hipStream_t s = h->stream;
    const float *grid6 = q.grid6();
    const uint32_t *dims = q.dims3();
    const size_t nodes = (size_t)q.count();
    const uint32_t nb = wsk_iso_blocks(dims);
    const size_t half = ((size_t)nb + 4) & ~(size_t)3;  // nb + 1 totals, 16 B aligned for the scan's uint4 accesses
    const size_t sw = (size_t)wsk_scan_state_words(nb + 1) * 4;
    if ((st = F.code.grow(h, nodes, kFieldScratch))) return st;
    if ((st = F.bcnt.grow(h, 2 * half * 4, kFieldScratch))) return st;
    if ((st = F.bstart.grow(h, (2 * half + 4) * 4, kFieldScratch))) return st;  // (+ the two grand totals)
    if ((st = F.bstate.grow(h, sw, kFieldScratch))) return st;
    // (the scan's tickets number its launches on a state buffer of a fixed length: fresh state for every call)
    HIP_TRY(h, hipMemsetAsync(F.bstate.p, 0, sw, s));
    wsk_iso_count(s, F.rho.p, grid6, dims, iso, F.code.p, F.bcnt.p, F.bcnt.p + half);
    wsk_scan(s, F.bcnt.p, F.bstart.p, nullptr, F.bstate.p, nb + 1, false, 0);
    wsk_scan(s, F.bcnt.p + half, F.bstart.p + half, nullptr, F.bstate.p, nb + 1, false, 0);
    wsk_iso_totals(s, F.bstart.p + nb, F.bstart.p + half + nb, F.bstart.p + 2 * half);
    HIP_TRY(h, hipGetLastError());
    uint32_t counts[2] = {0u, 0u};
    HIP_TRY(h, hipMemcpyAsync(counts, F.bstart.p + 2 * half, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *n_v = counts[0];
    *n_t = counts[1];
    if (!(out_xyz && out_tri && counts[0] <= max_v && counts[1] <= max_t)) {
        drain_profile(h);
        return WS_OK;
    }
    const size_t V = counts[0], T = counts[1];
    if ((st = F.vbase.grow(h, nodes * 4, kFieldScratch))) return st;
    if ((st = F.mxyz.grow(h, V * 12, kFieldScratch))) return st;
    if (grad_on && (st = F.mnrm.grow(h, V * 12, kFieldScratch))) return st;
    if ((st = F.tri.grow(h, T * 12, kFieldScratch))) return st;
    wsk_iso_mesh(s, F.rho.p, F.grad.p, grid6, dims, iso, F.code.p, F.bstart.p, F.bstart.p + half, F.vbase.p, F.mxyz.p,
                 grad_on ? F.mnrm.p : nullptr, F.tri.p);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{V ? out_xyz : nullptr, F.mxyz.p, V * 12},
                            {V && grad_on ? out_nrm : nullptr, F.mnrm.p, V * 12},
                            {T ? out_tri : nullptr, F.tri.p, T * 12}});
}

// ws_read_anisotropy: the stage alone, copied out by id (the ellipsoids split into M and f on the host).
ws_status read_anisotropy(ws_handle *h, const ws_aniso_params *ap, float *out_c, float *out_m, float *out_f, uint32_t *out_n)
{
    FieldCtx c;
    c.want = out_c || out_m || out_f || out_n;
    ws_status st = field_enter(h, c, "anisotropy", nullptr);
    if (st) return st;
    if (!c.want && !h->slab) return aniso_check(h, ap);
    st = field_source(h, &c, FIELD_POSITIONS, [&]() { return aniso_check(h, ap); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    if ((st = field_aniso_stage(h, c, ap))) return st;
    auto &F = h->field;
    const size_t n = c.n;
    std::vector<float> mf;
    if (out_m || out_f) mf.resize(n * 8);
    if ((st = field_finish(h, {{out_c, F.cxyz.p, n * 12}, {out_n, F.anb.p, n * 4}, {mf.empty() ? nullptr : mf.data(), F.amf.p, n * 32}})))
        return st;
    for (size_t i = 0; i < n && (out_m || out_f); i++) {
        if (out_m)
            for (int k = 0; k < 6; k++) out_m[6 * i + k] = mf[8 * i + k];
        if (out_f) out_f[i] = mf[8 * i + 6];
    }
    return WS_OK;
}

// ---- rays at the fluid surface ---------------------------------------------------------------------------------------
// The rays of a call (include/wsfluid.h): the m rays of origin / dir, or the camera and its image size.
struct RayQuery {
    const float *origin, *dir;
    uint32_t m;
    const ws_camera *cam;
    const uint32_t *size;
    bool camera;

    static RayQuery of_list(const float *origin, const float *dir, uint32_t m) { return {origin, dir, m, nullptr, nullptr, false}; }
    static RayQuery of_camera(const ws_camera *cam, const uint32_t *size) { return {nullptr, nullptr, 0u, cam, size, true}; }
    size_t count() const { return camera ? (size_t)size[0] * size[1] : m; }
};

// The march, then the rays.
ws_status ray_check(ws_handle *h, const ws_ray_params *r, const RayQuery &q)
{
    const float far = 1e15f;  // keeps every sample point finite: |t| * |v| <= 1e30
    if (!r) return fail(h, WS_ERR_INVALID_ARG, "rays: the march parameters are required");
    if (r->steps < 1u || r->steps > 65535u) return fail(h, WS_ERR_INVALID_ARG, "rays: steps must lie in 1 .. 65535");
    if (r->refine > 24u) return fail(h, WS_ERR_INVALID_ARG, "rays: refine must be <= 24");
    if (!isfinite(r->dt) || !(r->dt > 0.0f)) return fail(h, WS_ERR_INVALID_ARG, "rays: dt must be finite and > 0");
    if (!isfinite(r->iso) || !(r->iso > 0.0f)) return fail(h, WS_ERR_INVALID_ARG, "rays: iso must be finite and > 0");
    if (!isfinite(r->t_start)) return fail(h, WS_ERR_INVALID_ARG, "rays: t_start must be finite");
    if (fabs((double)r->t_start) + (double)r->steps * (double)r->dt > (double)far)
        return fail(h, WS_ERR_INVALID_ARG, "rays: |t_start| + steps * dt must be <= 1e15");
    auto in_range = [&](const float *v, size_t k) {
        for (size_t t = 0; t < k; t++)
            if (!isfinite(v[t]) || fabsf(v[t]) > far) return false;
        return true;
    };
    if (q.camera) {
        const ws_camera *cam = q.cam;
        const uint32_t *size = q.size;
        if (!cam || !size) return fail(h, WS_ERR_INVALID_ARG, "rays: the camera and the image size are required");
        if (size[0] == 0u || size[1] == 0u) return fail(h, WS_ERR_INVALID_ARG, "rays: the image size must be >= 1");
        if ((uint64_t)size[0] * size[1] > (1ull << 28)) return fail(h, WS_ERR_INVALID_ARG, "rays: more than 2^28 rays");
        if (!in_range(cam->eye, 3) || !in_range(cam->forward, 3) || !in_range(cam->right, 3) || !in_range(cam->up, 3))
            return fail(h, WS_ERR_INVALID_ARG, "rays: the camera must be finite and within 1e15");
        if (cam->forward[0] == 0.0f && cam->forward[1] == 0.0f && cam->forward[2] == 0.0f)
            return fail(h, WS_ERR_INVALID_ARG, "rays: the camera's forward is (0, 0, 0)");
        return WS_OK;
    }
    const float *origin = q.origin, *dir = q.dir;
    const uint32_t m = q.m;
    if (!origin || !dir || m == 0u) return fail(h, WS_ERR_INVALID_ARG, "rays: no rays");
    if (m > (1u << 28)) return fail(h, WS_ERR_INVALID_ARG, "rays: more than 2^28 rays");
    if (!in_range(origin, (size_t)m * 3) || !in_range(dir, (size_t)m * 3))
        return fail(h, WS_ERR_INVALID_ARG, "rays: origins and directions must be finite and within 1e15");
    for (size_t t = 0; t < m; t++)
        if (dir[3 * t] == 0.0f && dir[3 * t + 1] == 0.0f && dir[3 * t + 2] == 0.0f)
            return fail(h, WS_ERR_INVALID_ARG, "rays: a direction is (0, 0, 0)");
    return WS_OK;
}

// ws_cast_rays / ws_cast_camera: the binning (with ap the stage and the centres' binning), the cast kernel, the results
// copied out.
ws_status cast_rays(ws_handle *h, const ws_aniso_params *ap, const ws_ray_params *r, const RayQuery &q, float *out_t, float *out_n)
{
    FieldCtx c;
    c.want = out_t || out_n;
    ws_status st = field_enter(h, c, "rays", "rays: both outputs are NULL");
    if (st) return st;
    auto check = [&]() -> ws_status {
        if (ap) {
            const ws_status bad = aniso_check(h, ap);
            if (bad) return bad;
        }
        return ray_check(h, r, q);
    };
    st = field_source(h, &c, FIELD_POSITIONS, check);
    if (st || c.contributed) return st;
    if ((st = field_bin_kind(h, c, ap ? FIELD_ANISOTROPIC : FIELD_ISOTROPIC, ap))) return st;
    hipStream_t s = h->stream;
    auto &F = h->field;
    const size_t nr = q.count();
    if (out_t && (st = F.ray_t.grow(h, nr * 4, kFieldScratch))) return st;
    if (out_n && (st = F.ray_n.grow(h, nr * 12, kFieldScratch))) return st;
    if (!q.camera) {
        if ((st = F.rays.grow(h, nr * 24, kFieldScratch))) return st;
        HIP_TRY(h, hipMemcpyAsync(F.rays.p, q.origin, nr * 12, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(F.rays.p + 3 * nr, q.dir, nr * 12, hipMemcpyHostToDevice, s));
    }
    wsk_ray_cast(s, c.d, F.start.p, F.spos.p, ap ? F.smf.p : nullptr, h->ieee, *r, F.rays.p, q.camera ? nullptr : F.rays.p + 3 * nr,
                 (uint32_t)nr, q.cam, q.size, out_t ? F.ray_t.p : nullptr, out_n ? F.ray_n.p : nullptr);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_t, F.ray_t.p, nr * 4}, {out_n, F.ray_n.p, nr * 12}});
}

// ---- velocity field and tracer advection -----------------------------------------------------------------------------
// ws_sample_velocity_grid / _points: the binning with the velocities beside the positions, the velocity kernel, the
// results copied out (the velocities travel in F.grad).  The query is the density sampler's, errors included.
ws_status sample_velocity(ws_handle *h, const FieldQuery &q, float *out_vel, float *out_rho)
{
    FieldCtx c;
    c.want = out_vel || out_rho;
    if (q.grid && !q.given && (c.want || !h->slab))
        return fail(h, WS_ERR_INVALID_ARG, "velocity field: origin, spacing and dims are required");
    ws_status st = field_enter(h, c, "velocity field", "velocity field: both outputs are NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() { return field_check(h, q); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    auto &F = h->field;
    const size_t nq = (size_t)q.count();
    if (!q.grid && (st = field_upload(h, q))) return st;
    if (out_rho && (st = F.rho.grow(h, nq * 4, kFieldScratch))) return st;
    if (out_vel && (st = F.grad.grow(h, nq * 12, kFieldScratch))) return st;
    wsk_velocity_sample(h->stream, c.d, F.start.p, F.spos.p, F.svel.p, h->ieee, F.q.p, (uint32_t)nq, q.grid6(), q.dims3(),
                        q.bricks(c.d), out_vel ? F.grad.p : nullptr, out_rho ? F.rho.p : nullptr);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_rho, F.rho.p, nq * 4}, {out_vel, F.grad.p, nq * 12}});
}

// The query of ws_advect_points (include/wsfluid.h).
ws_status advect_check(ws_handle *h, const ws_advect_params *a, const float *xyz, uint32_t m, const float *out_xyz)
{
    if (!a) return fail(h, WS_ERR_INVALID_ARG, "advection: the parameters are required");
    if (a->substeps < 1u || a->substeps > 4096u) return fail(h, WS_ERR_INVALID_ARG, "advection: substeps must lie in 1 .. 4096");
    if (!isfinite(a->dt) || fabsf(a->dt) > 1e6f) return fail(h, WS_ERR_INVALID_ARG, "advection: dt must be finite and within 1e6");
    if (!xyz || m == 0u) return fail(h, WS_ERR_INVALID_ARG, "advection: no points");
    if (m > (1u << 28)) return fail(h, WS_ERR_INVALID_ARG, "advection: more than 2^28 points");
    if (!out_xyz) return fail(h, WS_ERR_INVALID_ARG, "advection: out_xyz is required");
    for (size_t t = 0; t < (size_t)m * 3; t++)
        if (ws_bad_float(xyz[t]))
            return fail(h, WS_ERR_INVALID_ARG, "advection: points must be finite and within 1e15");
    return WS_OK;
}

// ws_advect_points: the binning with velocities, the march kernel (in place on the uploaded points), the results out.
ws_status advect_points(ws_handle *h, const ws_advect_params *a, const float *xyz, uint32_t m, float *out_xyz, float *out_vel,
                        float *out_rho)
{
    FieldCtx c;
    c.want = out_xyz || out_vel || out_rho;
    ws_status st = field_enter(h, c, "advection", "advection: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() { return advect_check(h, a, xyz, m, out_xyz); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    auto &F = h->field;
    if ((st = F.q.grow(h, (size_t)m * 12, kFieldScratch))) return st;
    if (out_rho && (st = F.rho.grow(h, (size_t)m * 4, kFieldScratch))) return st;
    if (out_vel && (st = F.grad.grow(h, (size_t)m * 12, kFieldScratch))) return st;
    HIP_TRY(h, hipMemcpyAsync(F.q.p, xyz, (size_t)m * 12, hipMemcpyHostToDevice, h->stream));
    wsk_advect(h->stream, c.d, F.start.p, F.spos.p, F.svel.p, h->ieee, F.q.p, m, a->dt, a->substeps, out_vel ? F.grad.p : nullptr,
               out_rho ? F.rho.p : nullptr);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_xyz, F.q.p, (size_t)m * 12}, {out_rho, F.rho.p, (size_t)m * 4}, {out_vel, F.grad.p, (size_t)m * 12}});
}

// ---- whitewater (include/wsfluid.h defines the stage, the emission and the step) ---------------------------------------
// The per-particle stage into F.wst (T, K, a, E: n floats each, then the normals) and F.wnb, by id.
ws_status whitewater_stage(ws_handle *h, const FieldCtx &c)
{
    auto &F = h->field;
    const size_t n = c.n;
    ws_status st;
    if ((st = F.wnrm.grow(h, n * 16, kFieldScratch))) return st;
    if ((st = F.wst.grow(h, n * 28, kFieldScratch))) return st;
    if ((st = F.wnb.grow(h, n * 4, kFieldScratch))) return st;
    wsk_whitewater_stage(h->stream, c.d, F.start.p, F.spos.p, F.svel.p, F.wnrm.p, F.wst.p, F.wst.p + n, F.wst.p + 2 * n,
                         F.wst.p + 3 * n, F.wst.p + 4 * n, F.wnb.p, (uint32_t)n);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

ws_status read_whitewater(ws_handle *h, float *out_t, float *out_k, float *out_a, float *out_e, float *out_nrm, uint32_t *out_nb)
{
    FieldCtx c;
    c.want = out_t || out_k || out_a || out_e || out_nrm || out_nb;
    ws_status st = field_enter(h, c, "whitewater", "whitewater: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, []() { return WS_OK; });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    if ((st = whitewater_stage(h, c))) return st;
    auto &F = h->field;
    const size_t n = c.n;
    return field_finish(h, {{out_t, F.wst.p, n * 4}, {out_k, F.wst.p + n, n * 4}, {out_a, F.wst.p + 2 * n, n * 4},
                            {out_e, F.wst.p + 3 * n, n * 4}, {out_nrm, F.wst.p + 4 * n, n * 12}, {out_nb, F.wnb.p, n * 4}});
}

ws_status whitewater_emit_check(ws_handle *h, const ws_whitewater_emit_params *e, const uint32_t *n_emitted)
{
    if (!e) return fail(h, WS_ERR_INVALID_ARG, "whitewater: the emission parameters are required");
    if (!n_emitted) return fail(h, WS_ERR_INVALID_ARG, "whitewater: n_emitted is required");
    for (const float *tau : {e->tau_trapped, e->tau_crest, e->tau_energy})
        if (!isfinite(tau[0]) || !isfinite(tau[1]) || !(tau[0] >= 0.0f) || !(tau[0] < tau[1]))
            return fail(h, WS_ERR_INVALID_ARG, "whitewater: a tau pair must be finite with 0 <= tau[0] < tau[1]");
    if (!isfinite(e->k_trapped) || !isfinite(e->k_crest) || !(e->k_trapped >= 0.0f) || !(e->k_crest >= 0.0f))
        return fail(h, WS_ERR_INVALID_ARG, "whitewater: the rates must be finite and >= 0");
    if (!isfinite(e->crest_align)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: crest_align must be finite");
    if (!isfinite(e->dt) || !(e->dt > 0.0f)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: dt must be finite and > 0");
    if (!isfinite(e->radius) || !(e->radius > 0.0f)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: radius must be finite and > 0");
    if (!isfinite(e->lifetime[0]) || !isfinite(e->lifetime[1]) || !(e->lifetime[0] >= 0.0f) || !(e->lifetime[0] <= e->lifetime[1]))
        return fail(h, WS_ERR_INVALID_ARG, "whitewater: lifetime must be finite with 0 <= lifetime[0] <= lifetime[1]");
    if (e->max_per_particle < 1u || e->max_per_particle > 64u)
        return fail(h, WS_ERR_INVALID_ARG, "whitewater: max_per_particle must lie in 1 .. 64");
    return WS_OK;
}

// ws_emit_whitewater: the stage, the counts by id, their scan (n + 1 entries: the last is the total), the total back to
// the host and -- when the caller's buffers hold them -- the spawns.
ws_status emit_whitewater(ws_handle *h, const ws_whitewater_emit_params *e, uint32_t max_emitted, float *out_xyz, float *out_vel,
                          float *out_life, uint32_t *out_src, uint32_t *n_emitted)
{
    FieldCtx c;
    c.want = out_xyz || out_vel || out_life || out_src || n_emitted;
    ws_status st = field_enter(h, c, "whitewater", "whitewater: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() { return whitewater_emit_check(h, e, n_emitted); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    if ((st = whitewater_stage(h, c))) return st;
    hipStream_t s = h->stream;
    auto &F = h->field;
    const size_t n = c.n;
    if (n * e->max_per_particle > 0xFFFFFFFFull) return fail(h, WS_ERR_INVALID_ARG, "whitewater: n * max_per_particle exceeds 2^32 - 1");
    const size_t words = (n + 1 + 3) & ~(size_t)3;  // whole uint4 for the scan
    const size_t sw = (size_t)wsk_scan_state_words((uint32_t)n + 1u) * 4;
    if ((st = F.wcnt.grow(h, words * 4, kFieldScratch))) return st;
    if ((st = F.woff.grow(h, words * 4, kFieldScratch))) return st;
    if ((st = F.wstate.grow(h, sw, kFieldScratch))) return st;
    // (the scan's tickets number its launches on a state buffer of a fixed length: fresh state for every call)
    HIP_TRY(h, hipMemsetAsync(F.wstate.p, 0, sw, s));
    HIP_TRY(h, hipMemsetAsync(F.wcnt.p, 0, words * 4, s));
    const WsWhiteEmit we = {e->tau_trapped[0], e->tau_trapped[1], e->tau_crest[0], e->tau_crest[1], e->tau_energy[0],
                            e->tau_energy[1], e->k_trapped,     e->k_crest,      e->crest_align,  e->dt,
                            e->radius,         e->lifetime[0],  e->lifetime[1],  e->max_per_particle, e->seed};
    wsk_whitewater_count(s, we, F.vxyz.p, F.wst.p, F.wst.p + n, F.wst.p + 2 * n, F.wst.p + 3 * n, F.wcnt.p, (uint32_t)n);
    wsk_scan(s, F.wcnt.p, F.woff.p, nullptr, F.wstate.p, (uint32_t)n + 1u, false, 0);
    HIP_TRY(h, hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, F.woff.p + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *n_emitted = total;
    if (!((out_xyz || out_vel || out_life || out_src) && total != 0u && total <= max_emitted)) {
        drain_profile(h);
        return WS_OK;
    }
    const size_t T = total;
    if ((st = F.wout.grow(h, T * 32, kFieldScratch))) return st;
    float *xyz = F.wout.p, *vel = F.wout.p + 3 * T, *life = F.wout.p + 6 * T;
    uint32_t *src = reinterpret_cast<uint32_t *>(F.wout.p + 7 * T);
    // (the positions by id: field_source left them in F.vpos on a slab, in F.xyz on a single handle)
    wsk_whitewater_spawn(s, we, c.pos, F.vxyz.p, F.wcnt.p, F.woff.p, out_xyz ? xyz : nullptr, out_vel ? vel : nullptr,
                         out_life ? life : nullptr, out_src ? src : nullptr, (uint32_t)n);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_xyz, xyz, T * 12}, {out_vel, vel, T * 12}, {out_life, life, T * 4}, {out_src, src, T * 4}});
}

ws_status whitewater_step_check(ws_handle *h, const ws_whitewater_step_params *p, const float *xyz, const float *vel,
                                const float *life, uint32_t m)
{
    if (!p) return fail(h, WS_ERR_INVALID_ARG, "whitewater: the step parameters are required");
    if (!isfinite(p->dt) || !(p->dt > 0.0f)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: dt must be finite and > 0");
    if (!isfinite(p->buoyancy)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: buoyancy must be finite");
    if (!(p->drag >= 0.0f && p->drag <= 1.0f)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: drag must lie in [0, 1]");
    if (!xyz || !vel || !life || m == 0u) return fail(h, WS_ERR_INVALID_ARG, "whitewater: no diffuse particles");
    if (m > (1u << 28)) return fail(h, WS_ERR_INVALID_ARG, "whitewater: more than 2^28 diffuse particles");
    for (size_t t = 0; t < (size_t)m * 3; t++)
        if (ws_bad_float(xyz[t]) || ws_bad_float(vel[t]))
            return fail(h, WS_ERR_INVALID_ARG, "whitewater: positions and velocities must be finite and within 1e15");
    for (size_t t = 0; t < m; t++)
        if (!isfinite(life[t])) return fail(h, WS_ERR_INVALID_ARG, "whitewater: lifetimes must be finite");
    return WS_OK;
}

// ws_step_whitewater: the binning with velocities, the particles up, one kernel in place, the results out.
ws_status step_whitewater(ws_handle *h, const ws_whitewater_step_params *p, const float *xyz, const float *vel, const float *life,
                          uint32_t m, float *out_xyz, float *out_vel, float *out_life, uint8_t *out_class)
{
    FieldCtx c;
    c.want = out_xyz || out_vel || out_life || out_class;
    ws_status st = field_enter(h, c, "whitewater", "whitewater: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() { return whitewater_step_check(h, p, xyz, vel, life, m); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    hipStream_t s = h->stream;
    auto &F = h->field;
    const size_t M = m;
    if ((st = F.wpt.grow(h, M * 28 + M, kFieldScratch))) return st;
    float *dp = F.wpt.p, *dv = F.wpt.p + 3 * M, *dl = F.wpt.p + 6 * M;
    uint8_t *dc = reinterpret_cast<uint8_t *>(F.wpt.p + 7 * M);
    HIP_TRY(h, hipMemcpyAsync(dp, xyz, M * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(dv, vel, M * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(dl, life, M * 4, hipMemcpyHostToDevice, s));
    const WsWhiteStep sp = {p->dt, p->spray_max, p->bubble_min, p->buoyancy, p->drag};
    wsk_whitewater_step(s, c.d, F.start.p, F.spos.p, F.svel.p, h->ieee, sp, dp, dv, dl, dc, m);
    HIP_TRY(h, hipGetLastError());
    // (the uploads have left the caller's buffers before the kernel runs: outputs may alias inputs)
    return field_finish(h, {{out_xyz, dp, M * 12}, {out_vel, dv, M * 12}, {out_life, dl, M * 4}, {out_class, dc, M}});
}

// ---- surface tension and XSPH (include/wsfluid.h defines the stage and the edit) ----------------------------------------
// the argument errors of ws_read_cohesion / ws_apply_cohesion (nullptr = acceptable)
const char *cohesion_refusal(const ws_cohesion_params *p, float dt)
{
    if (!p) return "cohesion: p is NULL";
    if (p->reserved != 0u) return "cohesion: reserved must be 0";
    if (ws_bad_float(p->cohesion) || ws_bad_float(p->curvature) || ws_bad_float(p->xsph) || ws_bad_float(p->rest_density))
        return "cohesion: the parameters must be finite and at most 1e15 in magnitude";
    if (p->cohesion < 0.f || p->curvature < 0.f || p->rest_density < 0.f) return "cohesion: cohesion, curvature and rest_density must be >= 0";
    if (!(p->xsph >= 0.f && p->xsph <= 1.f)) return "cohesion: xsph must lie in [0, 1]";
    if (ws_bad_float(dt) || !(dt > 0.f)) return "cohesion: dt must be finite, > 0 and at most 1e15";
    return nullptr;
}

// The per-particle stage over the binned positions and velocities into F.crec, by id: {dv, count}, and with `outputs`
// (ws_read_cohesion) {normal, density} behind them, split into F.cst (the normals, the densities, then dv: 3 n, n and 3 n
// floats) and F.cnb.  The spline's constants are the header's float operations, in its order.
ws_status cohesion_stage(ws_handle *h, const FieldCtx &c, const ws_cohesion_params *p, float dt, bool outputs)
{
    auto &F = h->field;
    const size_t n = c.n;
    ws_status st;
    if ((st = F.cnd.grow(h, n * 16, kFieldScratch))) return st;
    if ((st = F.crec.grow(h, n * (outputs ? 32 : 16), kFieldScratch))) return st;
    if (outputs && (st = F.cst.grow(h, n * 28, kFieldScratch))) return st;
    if (outputs && (st = F.cnb.grow(h, n * 4, kFieldScratch))) return st;
    const float hh = c.d.h, h3 = (hh * hh) * hh, h6 = h3 * h3, h9 = h6 * h3;
    const WsCohesion k = {p->cohesion, p->curvature, p->xsph, p->rest_density == 0.0f ? c.d.target_density : p->rest_density, dt,
                          32.0f / (3.14159274f * h9), h6 * 0.015625f};
    wsk_cohesion_stage(h->stream, c.d, F.start.p, F.spos.p, F.svel.p, F.cnd.p, k, F.crec.p, outputs ? F.crec.p + n : nullptr, (uint32_t)n);
    if (outputs) wsk_cohesion_unpack(h->stream, F.crec.p, F.crec.p + n, F.cst.p, F.cst.p + 3 * n, F.cst.p + 4 * n, F.cnb.p, (uint32_t)n);
    HIP_TRY(h, hipGetLastError());
    return WS_OK;
}

ws_status read_cohesion(ws_handle *h, const ws_cohesion_params *p, float dt, float *out_nrm, float *out_rho, float *out_dv,
                        uint32_t *out_nb)
{
    FieldCtx c;
    c.want = out_nrm || out_rho || out_dv || out_nb;
    ws_status st = field_enter(h, c, "cohesion", "cohesion: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() -> ws_status {
        const char *why = cohesion_refusal(p, dt);
        return why ? fail(h, WS_ERR_INVALID_ARG, why) : WS_OK;
    });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    if ((st = cohesion_stage(h, c, p, dt, true))) return st;
    auto &F = h->field;
    const size_t n = c.n;
    return field_finish(h, {{out_nrm, F.cst.p, n * 12}, {out_rho, F.cst.p + 3 * n, n * 4}, {out_dv, F.cst.p + 4 * n, n * 12},
                            {out_nb, F.cnb.p, n * 4}});
}

// ws_apply_cohesion's prepare(): the stage on the handle's stream, and what the edit kernel reads of it.  A single handle
// (g == nullptr) takes positions and velocities from `cur`, as every field call; a slab handle takes them from the state
// records its edit route has ALREADY gathered, unpacked by id on the global grid the slabs' field calls bin on -- no
// further collective call.  The arguments have passed cohesion_refusal.
ws_status cohesion_prepare(ws_handle *h, const WsGathered *g, const ws_cohesion_params *p, float dt, WsCohesionArgs *args)
{
    auto &F = h->field;
    FieldCtx c;
    c.want = true;
    ws_status st;
    if (!g) {
        if ((st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, []() { return WS_OK; }))) return st;
    } else {
        c.inputs = FIELD_POSITIONS_AND_VELOCITIES;
        c.n = h->slab->n_global;
        if ((st = global_grid(&h->params, c.n, &c.d))) return fail(h, st, g_create_error.c_str());
        const size_t n = c.n;
        if ((st = field_alloc(h, c.n, c.d.ncells))) return st;
        if ((st = F.vxyz.grow(h, n * 12, kFieldScratch))) return st;
        if ((st = F.svel.grow(h, n * 16, kFieldScratch))) return st;
        if ((st = F.vpos.grow(h, n * 12, kFieldScratch))) return st;
        wsk_state_split(h->stream, g->recs, g->cnt, g->world, g->max_n, g->stride_words, c.n, F.vpos.p, F.vxyz.p);
        c.pos = F.vpos.p;
    }
    if ((st = field_bin_particles(h, c))) return st;
    if ((st = cohesion_stage(h, c, p, dt, false))) return st;
    args->dvc = F.crec.p;
    args->affected = nullptr;
    args->n = c.n;
    return WS_OK;
}

// ---- bodies in the fluid (include/wsfluid.h defines a sample's terms and the order of a body's sums) -------------------
ws_status body_check(ws_handle *h, const ws_body_params *p, const float *xyz, const float *vel, const float *vol, uint32_t m,
                     const uint32_t *body_start, const float *centre, uint32_t nb)
{
    if (!p) return fail(h, WS_ERR_INVALID_ARG, "bodies: the parameters are required");
    if (!isfinite(p->fluid_density) || !(p->fluid_density >= 0.0f) || !isfinite(p->drag) || !(p->drag >= 0.0f))
        return fail(h, WS_ERR_INVALID_ARG, "bodies: fluid_density and drag must be finite and >= 0");
    if (!isfinite(p->rest_density) || !(p->rest_density >= 0.0f))
        return fail(h, WS_ERR_INVALID_ARG, "bodies: rest_density must be finite and >= 0");
    if (p->reserved != 0u) return fail(h, WS_ERR_INVALID_ARG, "bodies: reserved must be 0");
    if (!xyz || !vel || !vol || m == 0u) return fail(h, WS_ERR_INVALID_ARG, "bodies: no samples");
    if (m > (1u << 28)) return fail(h, WS_ERR_INVALID_ARG, "bodies: more than 2^28 samples");
    if (!body_start || !centre || nb == 0u) return fail(h, WS_ERR_INVALID_ARG, "bodies: no bodies");
    if (nb > (1u << 24)) return fail(h, WS_ERR_INVALID_ARG, "bodies: more than 2^24 bodies");
    if (body_start[0] != 0u || body_start[nb] != m)
        return fail(h, WS_ERR_INVALID_ARG, "bodies: body_start must start at 0 and end at m");
    for (size_t b = 0; b < nb; b++)
        if (body_start[b] > body_start[b + 1]) return fail(h, WS_ERR_INVALID_ARG, "bodies: body_start must not decrease");
    auto in_range = [](const float *v, size_t k) {
        for (size_t t = 0; t < k; t++)
            if (ws_bad_float(v[t])) return false;
        return true;
    };
    if (!in_range(xyz, (size_t)m * 3) || !in_range(vel, (size_t)m * 3) || !in_range(vol, m) || !in_range(centre, (size_t)nb * 3))
        return fail(h, WS_ERR_INVALID_ARG, "bodies: positions, velocities, volumes and centres must be finite and within 1e15");
    for (size_t t = 0; t < m; t++)
        if (vol[t] < 0.0f) return fail(h, WS_ERR_INVALID_ARG, "bodies: a volume is negative");
    return WS_OK;
}

// ws_body_forces: the binning with velocities, the chunk table (built here from body_start), samples and centres up, the
// sweep with the first eight levels of every body's tree, the finishing kernel, the results out.
ws_status body_forces(ws_handle *h, const ws_body_params *p, const float *xyz, const float *vel, const float *vol, uint32_t m,
                      const uint32_t *body_start, const float *centre, uint32_t nb, float *out_force, float *out_torque,
                      float *out_volume, uint32_t *out_wet, float *out_sforce, float *out_sfrac)
{
    FieldCtx c;
    c.want = out_force || out_torque || out_volume || out_wet || out_sforce || out_sfrac;
    ws_status st = field_enter(h, c, "bodies", "bodies: every output is NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS_AND_VELOCITIES, [&]() { return body_check(h, p, xyz, vel, vol, m, body_start, centre, nb); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    hipStream_t s = h->stream;
    auto &F = h->field;
    // the chunks: wsk_body_chunk() consecutive samples of one body each, then the bodies' first chunks
    const uint32_t per = wsk_body_chunk();
    size_t nch = 0;
    for (size_t b = 0; b < nb; b++) nch += ((size_t)(body_start[b + 1] - body_start[b]) + per - 1) / per;
    std::vector<uint32_t> table(4 * nch + nb + 1);
    uint32_t *cstart = table.data() + 4 * nch;
    size_t at = 0;
    for (size_t b = 0; b < nb; b++) {
        cstart[b] = (uint32_t)at;
        for (uint32_t first = body_start[b]; first < body_start[b + 1]; first += per, at++) {
            uint32_t *ch = table.data() + 4 * at;
            ch[0] = (uint32_t)b;
            ch[1] = first;
            ch[2] = std::min(per, body_start[b + 1] - first);
            ch[3] = 0u;
        }
    }
    cstart[nb] = (uint32_t)at;
    // F.body in words: chunks 4 nch | partials 8 nch | first chunks nb + 1 | xyz 3 m | velocity 3 m | volume m | centres 3 nb |
    // sample force 3 m | sample fraction m | force 3 nb | torque 3 nb | volume nb | wet nb
    const size_t M = m, NB = nb;
    if ((st = F.body.grow(h, (12 * nch + 11 * M + 12 * NB + 1) * 4, kFieldScratch))) return st;
    float *d_chunks = F.body.p, *d_part = d_chunks + 4 * nch, *d_cstart = d_part + 8 * nch, *d_xyz = d_cstart + NB + 1;
    float *d_vel = d_xyz + 3 * M, *d_vol = d_vel + 3 * M, *d_centre = d_vol + M, *d_sforce = d_centre + 3 * NB;
    float *d_sfrac = d_sforce + 3 * M, *d_force = d_sfrac + M, *d_torque = d_force + 3 * NB, *d_volume = d_torque + 3 * NB;
    uint32_t *d_wet = reinterpret_cast<uint32_t *>(d_volume + NB);
    HIP_TRY(h, hipMemcpyAsync(d_chunks, table.data(), 4 * nch * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_cstart, cstart, (NB + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_xyz, xyz, M * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_vel, vel, M * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_vol, vol, M * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d_centre, centre, NB * 12, hipMemcpyHostToDevice, s));
    const float rho0 = p->rest_density == 0.0f ? c.d.target_density : p->rest_density;
    const WsBodyParams bp = {p->fluid_density, p->drag, rho0};
    wsk_body_forces(s, c.d, F.start.p, F.spos.p, F.svel.p, h->ieee, bp, reinterpret_cast<const uint32_t *>(d_chunks), (uint32_t)nch,
                    reinterpret_cast<const uint32_t *>(d_cstart), nb, d_xyz, d_vel, d_vol, d_centre, d_part,
                    out_sforce ? d_sforce : nullptr, out_sfrac ? d_sfrac : nullptr, out_force ? d_force : nullptr,
                    out_torque ? d_torque : nullptr, out_volume ? d_volume : nullptr, out_wet ? d_wet : nullptr);
    HIP_TRY(h, hipGetLastError());
    // (field_finish synchronises: the table outlives its upload)
    return field_finish(h, {{out_force, d_force, NB * 12}, {out_torque, d_torque, NB * 12}, {out_volume, d_volume, NB * 4},
                            {out_wet, d_wet, NB * 4}, {out_sforce, d_sforce, M * 12}, {out_sfrac, d_sfrac, M * 4}});
}

// ---- per-particle attributes (include/wsfluid.h defines paint, diffusion and the field) ---------------------------------
// The array lives in ws_handle::attr, by id: n float4, on slab handles n_global (replicated).
uint32_t attr_count(const ws_handle *h) { return h->slab ? h->slab->n_global : h->n; }

// the array, all +0, on the first call that needs it (a single handle: of its capacity, so that ws_add_particles within
// the capacity allocates nothing; the calls work on the first attr_count(h) entries)
ws_status attr_ensure(ws_handle *h)
{
    if (h->attr.p) return WS_OK;
    const size_t bytes = (size_t)(h->slab ? h->slab->n_global : h->cap) * 16;
    const ws_status st = h->attr.alloc(h, bytes, "attribute array");
    if (st) return st;
    if (hipMemsetAsync(h->attr.p, 0, bytes, h->stream) != hipSuccess) {
        (void)hipGetLastError();
        h->attr.release();
        return fail(h, WS_ERR_HIP, "attribute array");
    }
    return WS_OK;
}

// the preamble of the attribute calls: a dead handle, the reference-order validation mode
ws_status attr_enter(ws_handle *h)
{
    FieldCtx c;
    c.want = true;
    return field_enter(h, c, "attributes", nullptr);
}

// What the three calls that change the attributes say in the slabs' common verdict (slab_verdict: before anything is
// changed; a single handle answers for itself).
constexpr VerdictText kAttrVerdict = {"attributes", "arguments", true};

// field_source for the calls that change the attributes: the positions by id and the grid they are binned on.  What a
// slab's peers take part in (the gather) fails through the return value; what is this rank's alone (the scratch) comes
// back in *mine and goes into the common verdict, so that no peer waits there for a rank that has left.
ws_status attr_positions(ws_handle *h, FieldCtx *c, ws_status *mine)
{
    *mine = WS_OK;
    c->want = true;
    c->inputs = FIELD_POSITIONS;
    c->contributed = false;
    HIP_TRY(h, hipSetDevice(h->device));
    c->d = h->dev;
    c->n = h->n;
    if (h->slab) {
        const ws_status st = slab_field_positions(h, &c->pos, &c->d, false);
        if (st) return st;
        c->n = h->slab->n_global;
    }
    *mine = field_alloc(h, c->n, c->d.ncells);
    if (!*mine && !h->slab) {
        wsk_gather_positions(h->stream, h->cur, h->field.xyz.p, c->n);
        c->pos = h->field.xyz.p;
    }
    return WS_OK;
}

ws_status write_attributes(ws_handle *h, const float *in)
{
    ws_status st = attr_enter(h);
    if (st) return st;
    HIP_TRY(h, hipSetDevice(h->device));
    const ws_status mine = attr_ensure(h);
    const size_t n = attr_count(h);
    uint64_t hash = 14695981039346656037ull;  // (volume_hash's form, folded to the agreement's word)
    if (in && h->slab) hash = volume_mix(hash, in, n * 4);
    const uint32_t given = in ? 1u : 0u;
    if ((st = slab_verdict(h, kAttrVerdict, nullptr, mine, ((uint32_t)(hash ^ (hash >> 32)) << 1) | given))) return st;
    if (in) HIP_TRY(h, hipMemcpyAsync(h->attr.p, in, n * 16, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(h->attr.p, 0, n * 16, h->stream));
    return field_finish(h, {});
}

ws_status read_attributes(ws_handle *h, float *out)
{
    ws_status st = attr_enter(h);
    if (st) return st;
    if (!out) return h->slab ? WS_OK : fail(h, WS_ERR_INVALID_ARG, "attributes: out is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    if ((st = attr_ensure(h))) return st;
    return field_finish(h, {{out, h->attr.p, (size_t)attr_count(h) * 16}});
}

// the argument errors of ws_paint_attributes (nullptr = acceptable)
const char *brush_refusal(const ws_brush *b, uint32_t k)
{
    if (!b) return "attributes: b is NULL";
    if (k < 1u || k > WS_MAX_BRUSHES) return "attributes: k outside 1 .. WS_MAX_BRUSHES";
    for (uint32_t e = 0; e < k; e++) {
        if (b[e].kind > WS_BRUSH_ADD) return "attributes: unknown brush kind";
        if (b[e].channels < 1u || b[e].channels > 15u) return "attributes: channels must lie in 1 .. 15";
        for (int c = 0; c < 3; c++)
            if (ws_bad_float(b[e].centre[c])) return "attributes: a brush must be finite and at most 1e15 in magnitude";
        for (int c = 0; c < 4; c++)
            if (ws_bad_float(b[e].value[c])) return "attributes: a brush must be finite and at most 1e15 in magnitude";
        if (ws_bad_float(b[e].radius) || ws_bad_float(b[e].falloff) || ws_bad_float(b[e].strength))
            return "attributes: a brush must be finite and at most 1e15 in magnitude";
        if (!(b[e].radius > 0.f)) return "attributes: radius must be > 0";
        if (!(b[e].falloff >= 0.f && b[e].falloff <= 1.f)) return "attributes: falloff must lie in [0, 1]";
        if (b[e].kind == WS_BRUSH_MIX && !(b[e].strength >= 0.f && b[e].strength <= 1.f))
            return "attributes: a MIX strength must lie in [0, 1]";
    }
    return nullptr;
}

// ws_paint_attributes: the positions by id, one streaming pass over the array; the per-brush counts through the emitters'
// counters (ws_handle::force_cnt).
ws_status paint_attributes(ws_handle *h, const ws_brush *b, uint32_t k, uint32_t *out_painted)
{
    ws_status st = attr_enter(h);
    if (st) return st;
    const char *why = brush_refusal(b, k);
    if (why && !h->slab) return fail(h, WS_ERR_INVALID_ARG, why);
    FieldCtx c;
    ws_status mine = WS_OK;
    if ((st = attr_positions(h, &c, &mine))) return st;
    if (!mine) mine = attr_ensure(h);
    WsBrushArgs args{};
    ArgHash hash;
    hash(&k, 4);
    if (!why) {
        memcpy(args.bs.e, b, (size_t)k * sizeof(ws_brush));
        args.k = k;
        hash(b, (size_t)k * sizeof(ws_brush));
        if (!mine && out_painted) {
            mine = scratch_zeroed(h, h->force_cnt, WS_MAX_BRUSHES * 4, "brush counters");
            args.painted = h->force_cnt.p;
        }
    }
    if ((st = slab_verdict(h, kAttrVerdict, why, mine, hash.word))) return st;
    wsk_attr_paint(h->stream, args, c.pos, h->attr.p, c.n);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_painted, h->force_cnt.p, (size_t)k * 4}});
}

// the argument errors of ws_diffuse_attributes (nullptr = acceptable); r = fl(rate * dt) per channel
const char *diffuse_refusal(const ws_diffuse_params *p, float dt, float r[4])
{
    if (!p) return "attributes: p is NULL";
    if (p->reserved != 0u) return "attributes: reserved must be 0";
    if (p->iterations < 1u || p->iterations > 64u) return "attributes: iterations must lie in 1 .. 64";
    if (!isfinite(dt) || !(dt > 0.f)) return "attributes: dt must be finite and > 0";
    for (int c = 0; c < 4; c++) {
        if (ws_bad_float(p->rate[c])) return "attributes: the rates must be finite and at most 1e15 in magnitude";
        if (p->rate[c] < 0.f) return "attributes: the rates must be >= 0";
        r[c] = p->rate[c] * dt;
        if (!(r[c] <= 0.5f)) return "attributes: rate * dt must be at most 0.5";
    }
    return nullptr;
}

// ws_diffuse_attributes: the binning, the attributes gathered into cell order and pass A once; pass B `iterations` times
// between the two cell-ordered arrays; one scatter back by id.  The count goes through the cohesion edit's partial counters.
ws_status diffuse_attributes(ws_handle *h, const ws_diffuse_params *p, float dt, uint32_t *out_affected)
{
    ws_status st = attr_enter(h);
    if (st) return st;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    const char *why = diffuse_refusal(p, dt, r);
    if (why && !h->slab) return fail(h, WS_ERR_INVALID_ARG, why);
    FieldCtx c;
    ws_status mine = WS_OK;
    if ((st = attr_positions(h, &c, &mine))) return st;
    auto &F = h->field;
    const size_t n = c.n;
    uint32_t partial[WS_COHESION_SLOTS * WS_COHESION_SLOT_WORDS];
    if (!mine) mine = attr_ensure(h);
    if (!mine) mine = F.sattr[0].grow(h, n * 16, kFieldScratch);
    if (!mine) mine = F.sattr[1].grow(h, n * 16, kFieldScratch);
    if (!mine) mine = F.srho.grow(h, n * 4, kFieldScratch);
    if (!mine && out_affected) mine = scratch_zeroed(h, h->force_cnt, sizeof partial, "diffusion counters");
    ArgHash hash;
    hash(&dt, 4);
    if (!why) hash(p, sizeof *p);
    if ((st = slab_verdict(h, kAttrVerdict, why, mine, hash.word))) return st;
    if ((st = field_bin_particles(h, c))) return st;
    hipStream_t s = h->stream;
    wsk_attr_gather(s, F.spos.p, h->attr.p, F.sattr[0].p, c.n);
    wsk_attr_density(s, c.d, F.start.p, F.spos.p, F.srho.p, c.n);
    for (uint32_t it = 0; it < p->iterations; it++)
        wsk_attr_diffuse(s, c.d, F.start.p, F.spos.p, F.srho.p, F.sattr[it & 1u].p, r, F.sattr[(it + 1u) & 1u].p,
                         it == 0u && out_affected ? h->force_cnt.p : nullptr, c.n);
    wsk_attr_scatter(s, F.spos.p, F.sattr[p->iterations & 1u].p, h->attr.p, c.n);
    HIP_TRY(h, hipGetLastError());
    if ((st = field_finish(h, {{out_affected ? partial : nullptr, h->force_cnt.p, sizeof partial}}))) return st;
    if (out_affected) {
        uint32_t total = 0;
        for (uint32_t t = 0; t < WS_COHESION_SLOTS; t++) total += partial[t * WS_COHESION_SLOT_WORDS];
        *out_affected = total;
    }
    return WS_OK;
}

// ws_sample_attribute_grid / _points: sample_velocity with the attributes gathered into cell order in place of the
// velocities.  The query is the density sampler's, errors included.
ws_status sample_attributes(ws_handle *h, const FieldQuery &q, float *out_val, float *out_rho)
{
    FieldCtx c;
    c.want = out_val || out_rho;
    if (q.grid && !q.given && (c.want || !h->slab))
        return fail(h, WS_ERR_INVALID_ARG, "attribute field: origin, spacing and dims are required");
    ws_status st = field_enter(h, c, "attribute field", "attribute field: both outputs are NULL");
    if (st) return st;
    st = field_source(h, &c, FIELD_POSITIONS, [&]() { return field_check(h, q); });
    if (st || c.contributed) return st;
    if ((st = field_bin_particles(h, c))) return st;
    auto &F = h->field;
    const size_t nq = (size_t)q.count();
    if (!q.grid && (st = field_upload(h, q))) return st;
    if (out_rho && (st = F.rho.grow(h, nq * 4, kFieldScratch))) return st;
    if (out_val) {
        if ((st = attr_ensure(h))) return st;
        if ((st = F.sattr[0].grow(h, (size_t)c.n * 16, kFieldScratch))) return st;
        if ((st = F.aval.grow(h, nq * 16, kFieldScratch))) return st;
        wsk_attr_gather(h->stream, F.spos.p, h->attr.p, F.sattr[0].p, c.n);
    }
    wsk_attr_sample(h->stream, c.d, F.start.p, F.spos.p, F.sattr[0].p, h->ieee, F.q.p, (uint32_t)nq, q.grid6(), q.dims3(),
                    q.bricks(c.d), out_val ? F.aval.p : nullptr, out_rho ? F.rho.p : nullptr);
    HIP_TRY(h, hipGetLastError());
    return field_finish(h, {{out_rho, F.rho.p, nq * 4}, {out_val, F.aval.p, nq * 16}});
}

}  // namespace

extern "C" {

// ======================================================================================
// density field and its surface
// ======================================================================================
ws_status ws_sample_density_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                 float *out_density, float *out_gradient)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_density(h, FieldQuery::of_grid(origin, spacing, dims, 1u), FIELD_ISOTROPIC, nullptr, out_density, out_gradient);
}

ws_status ws_sample_density_points(ws_handle *h, const float *xyz, uint32_t m, float *out_density, float *out_gradient)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_density(h, FieldQuery::of_points(xyz, m), FIELD_ISOTROPIC, nullptr, out_density, out_gradient);
}

ws_status ws_extract_surface(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3], float iso,
                             uint32_t max_vertices, uint32_t max_triangles, float *out_xyz, float *out_normal,
                             uint32_t *out_tri, uint32_t *n_vertices, uint32_t *n_triangles)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return extract_surface(h, FieldQuery::of_grid(origin, spacing, dims, 2u), FIELD_ISOTROPIC, nullptr, iso, max_vertices,
                           max_triangles, out_xyz, out_normal, out_tri, n_vertices, n_triangles);
}

// ======================================================================================
// anisotropic kernels (Yu & Turk 2013; include/wsfluid.h defines the stage, the field and the mesh)
// ======================================================================================
ws_status ws_default_aniso_params(ws_aniso_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    out->smoothing = 0.9f;
    out->max_ratio = 4.0f;
    out->lone_scale = 0.5f;
    out->min_neighbours = 12u;
    return WS_OK;
}

ws_status ws_read_anisotropy(ws_handle *h, const ws_aniso_params *a, float *out_centre, float *out_matrix, float *out_scale,
                             uint32_t *out_neighbours)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return read_anisotropy(h, a, out_centre, out_matrix, out_scale, out_neighbours);
}

ws_status ws_sample_aniso_grid(ws_handle *h, const ws_aniso_params *a, const float origin[3], const float spacing[3],
                               const uint32_t dims[3], float *out_field, float *out_gradient)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_density(h, FieldQuery::of_grid(origin, spacing, dims, 1u), FIELD_ANISOTROPIC, a, out_field, out_gradient);
}

ws_status ws_sample_aniso_points(ws_handle *h, const ws_aniso_params *a, const float *xyz, uint32_t m, float *out_field,
                                 float *out_gradient)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_density(h, FieldQuery::of_points(xyz, m), FIELD_ANISOTROPIC, a, out_field, out_gradient);
}

ws_status ws_extract_aniso_surface(ws_handle *h, const ws_aniso_params *a, const float origin[3], const float spacing[3],
                                   const uint32_t dims[3], float iso, uint32_t max_vertices, uint32_t max_triangles,
                                   float *out_xyz, float *out_normal, uint32_t *out_tri, uint32_t *n_vertices,
                                   uint32_t *n_triangles)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return extract_surface(h, FieldQuery::of_grid(origin, spacing, dims, 2u), FIELD_ANISOTROPIC, a, iso, max_vertices,
                           max_triangles, out_xyz, out_normal, out_tri, n_vertices, n_triangles);
}

// ======================================================================================
// rays at the fluid surface (include/wsfluid.h defines the march, the hit and the normal)
// ======================================================================================
ws_status ws_cast_rays(ws_handle *h, const ws_aniso_params *a, const ws_ray_params *r, const float *origin_xyz,
                       const float *dir_xyz, uint32_t m, float *out_t, float *out_normal)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return cast_rays(h, a, r, RayQuery::of_list(origin_xyz, dir_xyz, m), out_t, out_normal);
}

ws_status ws_cast_camera(ws_handle *h, const ws_aniso_params *a, const ws_ray_params *r, const ws_camera *cam,
                         const uint32_t size[2], float *out_t, float *out_normal)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return cast_rays(h, a, r, RayQuery::of_camera(cam, size), out_t, out_normal);
}

// ======================================================================================
// velocity field and tracer advection (include/wsfluid.h defines the field and the march)
// ======================================================================================
ws_status ws_sample_velocity_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                  float *out_velocity, float *out_density)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_velocity(h, FieldQuery::of_grid(origin, spacing, dims, 1u), out_velocity, out_density);
}

ws_status ws_sample_velocity_points(ws_handle *h, const float *xyz, uint32_t m, float *out_velocity, float *out_density)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_velocity(h, FieldQuery::of_points(xyz, m), out_velocity, out_density);
}

ws_status ws_advect_points(ws_handle *h, const ws_advect_params *a, const float *xyz, uint32_t m, float *out_xyz,
                           float *out_velocity, float *out_density)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return advect_points(h, a, xyz, m, out_xyz, out_velocity, out_density);
}

// ======================================================================================
// whitewater: foam, spray and bubbles (include/wsfluid.h defines the stage, the emission and the step)
// ======================================================================================
ws_status ws_default_whitewater_emit_params(ws_whitewater_emit_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    out->tau_trapped[0] = 5.0f;  out->tau_trapped[1] = 50.0f;
    out->tau_crest[0] = 0.5f;    out->tau_crest[1] = 4.0f;
    out->tau_energy[0] = 1.0f;   out->tau_energy[1] = 25.0f;
    out->k_trapped = 400.0f;
    out->k_crest = 400.0f;
    out->crest_align = 0.6f;
    out->dt = 1.0f / 60.0f;
    out->radius = 0.1f;
    out->lifetime[0] = 2.0f;     out->lifetime[1] = 5.0f;
    out->max_per_particle = 8u;
    out->seed = 0u;
    return WS_OK;
}

ws_status ws_default_whitewater_step_params(ws_whitewater_step_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    out->dt = 1.0f / 60.0f;
    out->spray_max = 6u;
    out->bubble_min = 20u;
    out->buoyancy = 2.0f;
    out->drag = 0.5f;
    return WS_OK;
}

ws_status ws_read_whitewater(ws_handle *h, float *out_trapped, float *out_crest, float *out_align, float *out_energy,
                             float *out_normal, uint32_t *out_neighbours)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return read_whitewater(h, out_trapped, out_crest, out_align, out_energy, out_normal, out_neighbours);
}

ws_status ws_emit_whitewater(ws_handle *h, const ws_whitewater_emit_params *e, uint32_t max_emitted, float *out_xyz,
                             float *out_velocity, float *out_life, uint32_t *out_source, uint32_t *n_emitted)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return emit_whitewater(h, e, max_emitted, out_xyz, out_velocity, out_life, out_source, n_emitted);
}

ws_status ws_step_whitewater(ws_handle *h, const ws_whitewater_step_params *p, const float *xyz, const float *velocity,
                             const float *life, uint32_t m, float *out_xyz, float *out_velocity, float *out_life,
                             uint8_t *out_class)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return step_whitewater(h, p, xyz, velocity, life, m, out_xyz, out_velocity, out_life, out_class);
}

// ======================================================================================
// surface tension and XSPH: the read-only stage (ws_apply_cohesion is an edit: ws_api.cpp)
// ======================================================================================
ws_status ws_default_cohesion_params(ws_cohesion_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    out->cohesion = 1.0f;
    out->curvature = 1.0f;
    out->xsph = 0.1f;
    out->rest_density = 0.0f;
    out->reserved = 0u;
    return WS_OK;
}

ws_status ws_read_cohesion(ws_handle *h, const ws_cohesion_params *p, float dt, float *out_normal, float *out_density,
                           float *out_dv, uint32_t *out_neighbours)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return read_cohesion(h, p, dt, out_normal, out_density, out_dv, out_neighbours);
}

// ======================================================================================
// per-particle attributes: paint, mix and sample them (include/wsfluid.h defines every operation)
// ======================================================================================
ws_status ws_default_diffuse_params(ws_diffuse_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    for (float &rate : out->rate) rate = 1.0f;
    out->iterations = 1u;
    out->reserved = 0u;
    return WS_OK;
}

ws_status ws_write_attributes(ws_handle *h, const float *in)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return write_attributes(h, in);
}

ws_status ws_read_attributes(ws_handle *h, float *out)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return read_attributes(h, out);
}

ws_status ws_paint_attributes(ws_handle *h, const ws_brush *b, uint32_t k, uint32_t *out_painted)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return paint_attributes(h, b, k, out_painted);
}

ws_status ws_diffuse_attributes(ws_handle *h, const ws_diffuse_params *p, float dt, uint32_t *out_affected)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return diffuse_attributes(h, p, dt, out_affected);
}

ws_status ws_sample_attribute_grid(ws_handle *h, const float origin[3], const float spacing[3], const uint32_t dims[3],
                                   float *out_value, float *out_density)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_attributes(h, FieldQuery::of_grid(origin, spacing, dims, 1u), out_value, out_density);
}

ws_status ws_sample_attribute_points(ws_handle *h, const float *xyz, uint32_t m, float *out_value, float *out_density)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return sample_attributes(h, FieldQuery::of_points(xyz, m), out_value, out_density);
}

// ======================================================================================
// bodies in the fluid: buoyancy and drag (include/wsfluid.h defines a sample's terms and the order of the sums)
// ======================================================================================
ws_status ws_default_body_params(ws_body_params *out)
{
    if (!out) return WS_ERR_INVALID_ARG;
    out->fluid_density = 1000.0f;
    out->drag = 500.0f;
    out->rest_density = 0.0f;
    out->reserved = 0u;
    return WS_OK;
}

ws_status ws_body_forces(ws_handle *h, const ws_body_params *p, const float *sample_xyz, const float *sample_velocity,
                         const float *sample_volume, uint32_t m, const uint32_t *body_start, const float *body_centre, uint32_t nb,
                         float *out_force, float *out_torque, float *out_volume, uint32_t *out_wet, float *out_sample_force,
                         float *out_sample_fraction)
{
    if (!h) return WS_ERR_INVALID_ARG;
    return body_forces(h, p, sample_xyz, sample_velocity, sample_volume, m, body_start, body_centre, nb, out_force, out_torque,
                       out_volume, out_wet, out_sample_force, out_sample_fraction);
}

}  // extern "C"
