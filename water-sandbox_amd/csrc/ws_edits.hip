// ws_edits.hip -- gfx950 (CDNA4) kernels of the between-step edits: ws_apply_forces, ws_collide_solids,
// ws_collide_volumes and the velocity pass of ws_apply_cohesion.  Never inside ws_step.  Compiled with the flags and
// under the arithmetic contract of ws_kernels.hip.
#include "ws_device.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// ws_apply_forces: the emitters' acceleration as one explicit Euler step on the velocities (never inside ws_step)
//
// include/wsfluid.h pins every operation; IEEE arithmetic whatever the handle's flags.  The emitters are a by-value kernel
// argument (768 B): the loop over them is wave-uniform and reads them through scalar loads -- no LDS, no device buffer.
// Returns whether any emitter saw the particle (v is replaced only then: an unseen particle keeps its bits).  COUNTS: one
// ballot per emitter and wave, one atomic per wave that saw anything.  Every lane of the wave must call.
// ---------------------------------------------------------------------------------
template <bool COUNTS>
__device__ __forceinline__ bool forces_eval(const WsForceSet &fs, uint32_t k, float dt, bool active, const float4 &p, float4 &v,
                                            uint32_t *__restrict__ affected)
{
    float ax = 0.f, ay = 0.f, az = 0.f;
    bool hit = false;
    for (uint32_t e = 0; e < k; e++) {
        const ws_force &f = fs.e[e];
        const float qx = p.x - f.centre[0], qy = p.y - f.centre[1], qz = p.z - f.centre[2];
        const float dst = sqrtf(qx * qx + qy * qy + qz * qz);
        const bool in = active && dst < f.radius;
        if constexpr (COUNTS) {
            const uint32_t c = (uint32_t)__popcll(__ballot(in));
            if (c && (threadIdx.x & 63u) == 0u) atomicAdd(&affected[e], c);
        }
        if (!in) continue;
        hit = true;
        const float w = 1.f - dst / f.radius, s = f.strength * w;
        if (f.kind == WS_FORCE_RADIAL) {
            if (dst > 0.f) {
                ax = ax - (qx / dst) * s;
                ay = ay - (qy / dst) * s;
                az = az - (qz / dst) * s;
            }
        } else if (f.kind == WS_FORCE_JET) {
            ax = ax + f.axis[0] * s;
            ay = ay + f.axis[1] * s;
            az = az + f.axis[2] * s;
        } else {
            const float tx = f.axis[1] * qz - f.axis[2] * qy;
            const float ty = f.axis[2] * qx - f.axis[0] * qz;
            const float tz = f.axis[0] * qy - f.axis[1] * qx;
            ax = ax + tx * s;
            ay = ay + ty * s;
            az = az + tz * s;
        }
        const float g = f.damping * w;
        ax = ax - v.x * g;
        ay = ay - v.y * g;
        az = az - v.z * g;
    }
    if (hit) {
        v.x = v.x + dt * ax;
        v.y = v.y + dt * ay;
        v.z = v.z + dt * az;
    }
    return hit;
}

// ---------------------------------------------------------------------------------
// ws_collide_solids: push the particles out of k solids, respond to the solids' motion, sum the reaction (never inside
// ws_step)
//
// include/wsfluid.h pins every operation; IEEE arithmetic whatever the handle's flags.  The solids are a by-value kernel
// argument (WsSolidSet: 16 x 112 B and one squared reach each): the loop over them is wave-uniform and reads them through
// scalar loads -- no LDS and no device buffer for them.  A wave none of whose lanes lies within a solid's reach skips the
// solid (reach2: wsk_solid_reach2, a bound no contact can lie beyond, so the skip changes no bit; +inf, never skipped,
// for HOLLOW solids, which touch everything outside them).
// REACT: the contact count and the six fixed-point reaction sums of every solid, reduced before they reach memory: across
// the wave with shuffles (only in waves that have a contact), per workgroup in LDS (acc: WS_SOLID_WORDS 64-bit words per
// solid, zeroed by the caller), and from there at most one 64-bit atomic per workgroup, solid and word
// (solids_flush).  Every lane of the wave must call.  Returns whether any solid touched the particle.
// (solids_fixed and wave_sum_i64, step 6's fixed point and its sum across a wave: ws_device.h -- the gauges share them)
// ---------------------------------------------------------------------------------

// Steps 3 to 6 of the definition, shared by every edit that collides (solids_eval, volumes_eval): given the signed distance
// s and the outward unit normal n of one object at the running position -- `hit` = the particle is active and s < margin
// -- the push-out, the response against the object's surface velocity and, with REACT, the object's contact count and six
// fixed-point sums into its row `a` of the workgroup's accumulator.  Every lane of the wave must call.
template <bool REACT>
__device__ __forceinline__ bool contact_respond(bool hit, float s, float nx, float ny, float nz, float margin, const float *centre,
                                                const float *V, const float *W, float restitution, float friction, float4 &p,
                                                float4 &v, unsigned long long *a)
{
    bool kicked = false;
    float dvx = 0.f, dvy = 0.f, dvz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
    if (hit) {
        const float out = margin - s;
        p.x = p.x + out * nx;
        p.y = p.y + out * ny;
        p.z = p.z + out * nz;
        rx = p.x - centre[0]; ry = p.y - centre[1]; rz = p.z - centre[2];
        const float ux = V[0] + (W[1] * rz - W[2] * ry);
        const float uy = V[1] + (W[2] * rx - W[0] * rz);
        const float uz = V[2] + (W[0] * ry - W[1] * rx);
        const float relx = v.x - ux, rely = v.y - uy, relz = v.z - uz;
        const float vn = relx * nx + rely * ny + relz * nz;
        if (vn < 0.f) {
            kicked = true;
            const float j = (1.f + restitution) * (-vn);
            const float tx = relx - vn * nx, ty = rely - vn * ny, tz = relz - vn * nz;
            dvx = j * nx - friction * tx;
            dvy = j * ny - friction * ty;
            dvz = j * nz - friction * tz;
            v.x = v.x + dvx;
            v.y = v.y + dvy;
            v.z = v.z + dvz;
        }
    }
    if constexpr (REACT) {
        const unsigned long long hits = __ballot(hit);
        if (hits) {  // wave-uniform
            const bool lead = (threadIdx.x & 63u) == 0u;
            if (lead) atomicAdd(&a[0], (unsigned long long)__popcll(hits));
            if (__ballot(kicked)) {
                long long w[6] = {0, 0, 0, 0, 0, 0};
                if (kicked) {
                    const float ix = -dvx, iy = -dvy, iz = -dvz;
                    w[0] = solids_fixed(ix);
                    w[1] = solids_fixed(iy);
                    w[2] = solids_fixed(iz);
                    w[3] = solids_fixed(ry * iz - rz * iy);
                    w[4] = solids_fixed(rz * ix - rx * iz);
                    w[5] = solids_fixed(rx * iy - ry * ix);
                }
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const long long sum = wave_sum_i64(w[c]);
                    if (lead && sum) atomicAdd(&a[1 + c], (unsigned long long)sum);
                }
            }
        }
    }
    return hit;
}

// the step's own container rule (force_integrate_bin) on a particle some object touched
__device__ __forceinline__ void contact_container(const WsDev &d, float4 &p, float4 &v)
{
    const float nd = -1.f * d.damping;
    if (p.x < d.ext_min[0]) { v.x *= nd; p.x = d.ext_min[0]; } else if (p.x > d.ext_max[0]) { v.x *= nd; p.x = d.ext_max[0]; }
    if (p.y < d.ext_min[1]) { v.y *= nd; p.y = d.ext_min[1]; } else if (p.y > d.ext_max[1]) { v.y *= nd; p.y = d.ext_max[1]; }
    if (p.z < d.ext_min[2]) { v.z *= nd; p.z = d.ext_min[2]; } else if (p.z > d.ext_max[2]) { v.z *= nd; p.z = d.ext_max[2]; }
}

template <bool REACT>
__device__ __forceinline__ bool solids_eval(const WsDev &d, const WsSolidSet &ss, uint32_t k, bool active, float4 &p, float4 &v,
                                            unsigned long long *acc)
{
    bool touched = false;
    for (uint32_t e = 0; e < k; e++) {
        const ws_solid &S = ss.e[e];
        const float qx = p.x - S.centre[0], qy = p.y - S.centre[1], qz = p.z - S.centre[2];
        const float q2 = qx * qx + qy * qy + qz * qz;
        if (!__ballot(active && q2 <= ss.reach2[e])) continue;  // wave-uniform: nobody can be in contact
        const float *R = S.rot;
        float s, nx, ny, nz;
        if (S.kind == WS_SOLID_SPHERE) {
            const float dst = sqrtf(q2);
            s = dst - S.size[0];
            nx = dst > 0.f ? qx / dst : 0.f;
            ny = dst > 0.f ? qy / dst : 1.f;
            nz = dst > 0.f ? qz / dst : 0.f;
        } else if (S.kind == WS_SOLID_CAPSULE) {
            const float l1 = R[3] * qx + R[4] * qy + R[5] * qz;
            const float t = fminf(fmaxf(l1, -S.size[1]), S.size[1]);
            const float wx = qx - t * R[3], wy = qy - t * R[4], wz = qz - t * R[5];
            const float dst = sqrtf(wx * wx + wy * wy + wz * wz);
            s = dst - S.size[0];
            nx = dst > 0.f ? wx / dst : R[0];
            ny = dst > 0.f ? wy / dst : R[1];
            nz = dst > 0.f ? wz / dst : R[2];
        } else {
            const float l0 = R[0] * qx + R[1] * qy + R[2] * qz;
            const float l1 = R[3] * qx + R[4] * qy + R[5] * qz;
            const float l2 = R[6] * qx + R[7] * qy + R[8] * qz;
            const float a0 = fabsf(l0) - S.size[0], a1 = fabsf(l1) - S.size[1], a2 = fabsf(l2) - S.size[2];
            const float g = fmaxf(fmaxf(a0, a1), a2);
            float m0, m1, m2;
            if (g > 0.f) {
                const float u0 = copysignf(fmaxf(a0, 0.f), l0), u1 = copysignf(fmaxf(a1, 0.f), l1), u2 = copysignf(fmaxf(a2, 0.f), l2);
                const float dst = sqrtf(u0 * u0 + u1 * u1 + u2 * u2);
                s = dst;
                m0 = u0 / dst; m1 = u1 / dst; m2 = u2 / dst;
            } else {
                const int star = a0 == g ? 0 : a1 == g ? 1 : 2;
                s = g;
                m0 = star == 0 ? copysignf(1.f, l0) : 0.f;
                m1 = star == 1 ? copysignf(1.f, l1) : 0.f;
                m2 = star == 2 ? copysignf(1.f, l2) : 0.f;
            }
            nx = (m0 * R[0] + m1 * R[3]) + m2 * R[6];
            ny = (m0 * R[1] + m1 * R[4]) + m2 * R[7];
            nz = (m0 * R[2] + m1 * R[5]) + m2 * R[8];
        }
        if (S.flags & WS_SOLID_HOLLOW) {
            s = -s;
            nx = -nx; ny = -ny; nz = -nz;
        }
        touched |= contact_respond<REACT>(active && s < S.margin, s, nx, ny, nz, S.margin, S.centre, S.velocity, S.angular_velocity,
                                          S.restitution, S.friction, p, v, acc + e * WS_SOLID_WORDS);
    }
    if (touched) contact_container(d, p, v);
    return touched;
}

// the workgroup's sums on their way out: one 64-bit atomic per solid and word, only for the solids the workgroup touched
// (word 0, the contact count, is non-zero exactly then).  Called by every thread, after a barrier.
__device__ __forceinline__ void solids_flush(const unsigned long long *acc, uint32_t k, unsigned long long *__restrict__ sums)
{
    const uint32_t t = threadIdx.x;
    if (t < k * WS_SOLID_WORDS && acc[t - t % WS_SOLID_WORDS] != 0ull && acc[t] != 0ull) atomicAdd(&sums[t], acc[t]);
}

// ---------------------------------------------------------------------------------
// ws_collide_volumes: ws_collide_solids with the solid given as a signed-distance volume (never inside ws_step)
//
// include/wsfluid.h pins every operation; IEEE arithmetic whatever the handle's flags.  The slots' descriptors, the poses
// and one squared reach per pose are a by-value kernel argument (WsVolumeSet), read through scalar loads in the wave-uniform
// loop -- the pose's slot is wave-uniform too, so its descriptor is.  A wave none of whose lanes lies within the pose's
// reach skips it with one ballot (reach2: volumes_reach2, a bound no point of the volume's domain lies beyond; outside the
// domain there is no contact, so the skip changes no bit).
// The eight corner values are the only gathers: every lane of a wave that goes on computes a CLAMPED cell -- a lane outside
// the domain, or an inactive one, reads cell (0, 0, 0) -- so that the eight loads are issued together, before the first
// use and under no divergent branch, through the read-only path.  The distance and the gradient are those of one
// trilinear interpolant; steps 3 to 6 and the reaction are the solids' (contact_respond).  Every lane of the wave must call.
// ---------------------------------------------------------------------------------
template <bool REACT>
__device__ __forceinline__ bool volumes_eval(const WsDev &d, const WsVolumeSet &vs, uint32_t k, bool active, float4 &p, float4 &v,
                                             unsigned long long *acc)
{
    bool touched = false;
    for (uint32_t e = 0; e < k; e++) {
        const ws_volume_pose &P = vs.e[e];
        const float qx = p.x - P.centre[0], qy = p.y - P.centre[1], qz = p.z - P.centre[2];
        const float q2 = qx * qx + qy * qy + qz * qz;
        if (!__ballot(active && q2 <= vs.reach2[e])) continue;  // wave-uniform: nobody can be in the domain
        const WsVolumeDesc &D = vs.vol[P.slot & (WS_MAX_VOLUMES - 1u)];
        const float *R = P.rot;
        const float l0 = R[0] * qx + R[1] * qy + R[2] * qz;
        const float l1 = R[3] * qx + R[4] * qy + R[5] * qz;
        const float l2 = R[6] * qx + R[7] * qy + R[8] * qz;
        const float g0 = (l0 - D.origin[0]) / D.spacing[0];
        const float g1 = (l1 - D.origin[1]) / D.spacing[1];
        const float g2 = (l2 - D.origin[2]) / D.spacing[2];
        const uint32_t n0 = D.dims[0], n1 = D.dims[1], n2 = D.dims[2];
        const bool in = active && g0 >= 0.f && g0 <= (float)(n0 - 1u) && g1 >= 0.f && g1 <= (float)(n1 - 1u) && g2 >= 0.f &&
                        g2 <= (float)(n2 - 1u);
        const float h0 = in ? g0 : 0.f, h1 = in ? g1 : 0.f, h2 = in ? g2 : 0.f;
        const uint32_t i0 = min((uint32_t)h0, n0 - 2u), i1 = min((uint32_t)h1, n1 - 2u), i2 = min((uint32_t)h2, n2 - 2u);
        const float f0 = h0 - (float)i0, f1 = h1 - (float)i1, f2 = h2 - (float)i2;
        const float *__restrict__ c = D.sdf + ((i2 * n1 + i1) * n0 + i0);  // (at most 2^26 nodes)
        const uint32_t sy = n0, sz = n0 * n1;
        const float c000 = c[0], c100 = c[1], c010 = c[sy], c110 = c[sy + 1u];
        const float c001 = c[sz], c101 = c[sz + 1u], c011 = c[sz + sy], c111 = c[sz + sy + 1u];
        const float d00 = c100 - c000, d10 = c110 - c010, d01 = c101 - c001, d11 = c111 - c011;
        const float cx00 = c000 + f0 * d00, cx10 = c010 + f0 * d10, cx01 = c001 + f0 * d01, cx11 = c011 + f0 * d11;
        const float e0 = cx10 - cx00, e1 = cx11 - cx01;
        const float cy0 = cx00 + f1 * e0, cy1 = cx01 + f1 * e1;
        const float hh = cy1 - cy0;
        const float s = cy0 + f2 * hh;
        const float dz0 = d00 + f1 * (d10 - d00), dz1 = d01 + f1 * (d11 - d01);
        const float G0 = (dz0 + f2 * (dz1 - dz0)) / D.spacing[0];
        const float G1 = (e0 + f2 * (e1 - e0)) / D.spacing[1];
        const float G2 = hh / D.spacing[2];
        const float gg = G0 * G0 + G1 * G1 + G2 * G2;
        float m0 = 0.f, m1 = 1.f, m2 = 0.f;
        if (gg > 0.f) {
            const float len = sqrtf(gg);
            m0 = G0 / len; m1 = G1 / len; m2 = G2 / len;
        }
        const float nx = (m0 * R[0] + m1 * R[3]) + m2 * R[6];
        const float ny = (m0 * R[1] + m1 * R[4]) + m2 * R[7];
        const float nz = (m0 * R[2] + m1 * R[5]) + m2 * R[8];
        touched |= contact_respond<REACT>(in && s < P.margin, s, nx, ny, nz, P.margin, P.centre, P.velocity, P.angular_velocity,
                                          P.restitution, P.friction, p, v, acc + e * WS_SOLID_WORDS);
    }
    if (touched) contact_container(d, p, v);
    return touched;
}

// ---------------------------------------------------------------------------------
// the between-step edits (ws_apply_forces, ws_collide_solids, ws_collide_volumes, and whatever comes next): an edit is a
// TYPE, and two kernels serve every edit -- k_edit_current on a single handle's `cur`, k_edit_records on the gathered
// records of slab handles
//
// An edit is a by-value kernel argument (its objects reach the wave-uniform loop through scalar loads) that declares
//   moves      whether eval may change the position (else p comes back as it went in and is not stored);
//   acc_words  the 64-bit LDS words a workgroup accumulates in, at most WS_BLOCK (0: none, and no barrier is taken);
//   eval(d, active, p, v, acc)  the definition on one particle; true if it changed p or v.  EVERY lane of the workgroup
//              calls it (it may ballot and shuffle), inactive lanes with active == false and zeros; d is the handle's
//              grid, on slab handles the global one; acc is zeroed, and other waves add to it;
//   flush(acc) the workgroup's words on their way to memory, called by every thread after a barrier.
// Around it the kernels guarantee: the record read once and written once; an unchanged particle keeps its bits; the
// predicted position is the library's own p + v * WS_LOOKAHEAD, never the edit's; and `cur` is left binned -- cid, the
// record's cell id, the per-cell count and the rank, what bin_current leaves -- so that any number of edits may follow
// one another between two steps.
// ---------------------------------------------------------------------------------
template <bool COUNTS>
struct EditForces {
    static constexpr bool moves = false;
    static constexpr uint32_t acc_words = 0;
    WsForceArgs a;
    __device__ bool eval(const WsDev &, bool active, float4 &p, float4 &v, unsigned long long *) const
    {
        return forces_eval<COUNTS>(a.fs, a.k, a.dt, active, p, v, a.affected);
    }
    __device__ void flush(const unsigned long long *) const {}
};

template <bool REACT>
struct EditSolids {
    static constexpr bool moves = true;
    static constexpr uint32_t acc_words = REACT ? WS_MAX_SOLIDS * WS_SOLID_WORDS : 0u;
    WsSolidArgs a;
    __device__ bool eval(const WsDev &d, bool active, float4 &p, float4 &v, unsigned long long *acc) const
    {
        return solids_eval<REACT>(d, a.ss, a.k, active, p, v, acc);
    }
    __device__ void flush(const unsigned long long *acc) const { solids_flush(acc, a.k, a.sums); }
};

template <bool REACT>
struct EditVolumes {
    static constexpr bool moves = true;
    static constexpr uint32_t acc_words = REACT ? WS_MAX_VOLUME_POSES * WS_SOLID_WORDS : 0u;
    WsVolumeArgs a;
    __device__ bool eval(const WsDev &d, bool active, float4 &p, float4 &v, unsigned long long *acc) const
    {
        return volumes_eval<REACT>(d, a.vs, a.k, active, p, v, acc);
    }
    __device__ void flush(const unsigned long long *acc) const { solids_flush(acc, a.k, a.sums); }
};

// ws_apply_cohesion: the neighbour stage (k_cohesion_normals / k_cohesion_stage, ws_fields.hip) has left dv
// and the contributing-neighbour count c BY ID, as one float4 each; the edit adds dv[id] where c[id] > 0 -- an unaffected particle keeps its
// bits, a -0 included.  The id rides in the w lane of p (cur.pos(i).w; the record's id word).  COUNTS: one ballot per
// wave and at most one atomic, as forces_eval<COUNTS>, into a.affected's slots.
template <bool COUNTS>
struct EditCohesion {
    static constexpr bool moves = false;
    static constexpr uint32_t acc_words = 0;
    WsCohesionArgs a;
    __device__ bool eval(const WsDev &, bool active, float4 &p, float4 &v, unsigned long long *) const
    {
        const uint32_t id = __float_as_uint(p.w);
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);  // {dv, c (bits)}: one 16-byte gather per particle
        if (active && id < a.n) r = a.dvc[id];
        const bool hit = __float_as_uint(r.w) > 0u;
        if constexpr (COUNTS) {
            const uint32_t k = (uint32_t)__popcll(__ballot(hit));
            // (nearly every wave has something to add: to one word that is 65 536 atomics in a row at 4 M particles --
            // measured 757 us, ten times the rest of the pass -- so a wave adds to one of WS_COHESION_SLOTS words, a cache
            // line apart, and the host sums them)
            const uint32_t slot = ((blockIdx.x * WS_BLOCK + threadIdx.x) >> 6) % WS_COHESION_SLOTS;
            if (k && (threadIdx.x & 63u) == 0u) atomicAdd(a.affected + slot * WS_COHESION_SLOT_WORDS, k);
        }
        if (hit) {
            v.x = v.x + r.x;
            v.y = v.y + r.y;
            v.z = v.z + r.z;
        }
        return hit;
    }
    __device__ void flush(const unsigned long long *) const {}
};

// what a launcher's argument struct becomes on the device: WITH = whether the call wants its outputs (COUNTS / REACT)
template <class With>
EditForces<With::value> edit_of(const WsForceArgs &a, With) { return {a}; }
template <class With>
EditSolids<With::value> edit_of(const WsSolidArgs &a, With) { return {a}; }
template <class With>
EditVolumes<With::value> edit_of(const WsVolumeArgs &a, With) { return {a}; }
template <class With>
EditCohesion<With::value> edit_of(const WsCohesionArgs &a, With) { return {a}; }

template <class Edit>
__device__ __forceinline__ void edit_begin(unsigned long long *acc)
{
    static_assert(Edit::acc_words <= (uint32_t)WS_BLOCK, "one thread zeroes and flushes one accumulator word");
    if constexpr (Edit::acc_words != 0u) {
        if (threadIdx.x < Edit::acc_words) acc[threadIdx.x] = 0ull;
        __syncthreads();
    }
}

template <class Edit>
__device__ __forceinline__ void edit_end(const Edit &edit, const unsigned long long *acc)
{
    if constexpr (Edit::acc_words != 0u) {
        __syncthreads();
        edit.flush(acc);
    }
}

// Single-GPU handles: one lane per slot of `cur` in the order the last step left it (two 16-byte loads of consecutive
// records), then what k_refresh_pred and k_bin would do in two more passes: the predicted position in registers, its
// cell, cid[i] and the velocity record's w lane, the per-cell count and the particle's rank in it -- one atomic per run
// of lanes that share a cell, as the force kernel's epilogue draws them.  The record halves go out as 16-byte stores,
// {v, cell id} always and {p, id} for an edit that moves; cur.pred is not stored (k_reorder<true> and k_refresh_pred
// recompute it from the record).
template <class Edit>
__global__ void __launch_bounds__(WS_BLOCK) k_edit_current(WsDev d, WsSoA cur, uint32_t *__restrict__ cid,
                                                           uint32_t *__restrict__ count, Edit edit)
{
    __shared__ unsigned long long acc[Edit::acc_words ? Edit::acc_words : 1u];
    edit_begin<Edit>(acc);
    const uint32_t i = blockIdx.x * WS_BLOCK + threadIdx.x;
    const bool active = i < d.n;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
    if (active) {
        p = cur.pos(i);
        v = cur.vel(i);
    }
    edit.eval(d, active, p, v, acc);
    uint32_t c = 0;
    if (active) {
        c = grid_cell(d, p.x + v.x * WS_LOOKAHEAD, p.y + v.y * WS_LOOKAHEAD, p.z + v.z * WS_LOOKAHEAD);
        cid[i] = c;
        if constexpr (Edit::moves) cur.pos(i) = p;
        cur.vel(i) = make_float4(v.x, v.y, v.z, __uint_as_float(c));
    }
    const uint32_t r = wave_run_atomic_inc(count, c, active);
    if (active && cur.rank) cur.rank[i] = r;
    edit_end(edit, acc);
}

// The gathered state of slab handles (WS_PACK_STATE_H, what k_slab_select<2> reads): per source rank r, stride_words
// apart, min(cnt[4 r], max_n) records of 10 words: {id, pos[3], vel[3], pred[3]}.  The nine floats of record t of rank r:
__device__ __forceinline__ float *state_record(uint32_t *all, size_t stride_words, uint32_t r, uint32_t t)
{
    return reinterpret_cast<float *>(all + (size_t)r * stride_words + (size_t)t * 10u + 1u);
}

// Slab handles: the same definition on the gathered records of every rank (blockIdx.y = source rank), edited in place:
// velocity, position for an edit that moves, and the predicted position by the library's own rule.  d: the GLOBAL grid.
template <class Edit>
__global__ void __launch_bounds__(WS_BLOCK) k_edit_records(WsDev d, uint32_t *__restrict__ all, const uint32_t *__restrict__ cnt,
                                                           uint32_t max_n, size_t stride_words, Edit edit)
{
    __shared__ unsigned long long acc[Edit::acc_words ? Edit::acc_words : 1u];
    edit_begin<Edit>(acc);
    const uint32_t t = blockIdx.x * WS_BLOCK + threadIdx.x, r = blockIdx.y;
    const bool active = t < min(cnt[4 * r], max_n);
    float *f = state_record(all, stride_words, r, t);
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
    if (active) {
        // (w: the record's id word, where cur.pos(i) has it)
        p = make_float4(f[0], f[1], f[2], __uint_as_float(reinterpret_cast<const uint32_t *>(f)[-1]));
        v = make_float4(f[3], f[4], f[5], 0.f);
    }
    const bool changed = edit.eval(d, active, p, v, acc);
    if (active) {
        if (changed) {
            if constexpr (Edit::moves) { f[0] = p.x; f[1] = p.y; f[2] = p.z; }
            f[3] = v.x; f[4] = v.y; f[5] = v.z;
        }
        f[6] = p.x + v.x * WS_LOOKAHEAD; f[7] = p.y + v.y * WS_LOOKAHEAD; f[8] = p.z + v.z * WS_LOOKAHEAD;
    }
    edit_end(edit, acc);
}


template <class Args>
void wsk_edit_current(hipStream_t s, const WsDev &d, WsSoA cur, uint32_t *cid, uint32_t *count, const Args &a)
{
    if (!d.n) return;
    ws_dispatch([&](auto with) {
        using Edit = decltype(edit_of(a, with));
        hipLaunchKernelGGL(k_edit_current<Edit>, dim3(cdiv(d.n, WS_BLOCK)), dim3(WS_BLOCK), 0, s, d, cur, cid, count, edit_of(a, with));
    }, a.outputs());
}
template void wsk_edit_current(hipStream_t, const WsDev &, WsSoA, uint32_t *, uint32_t *, const WsForceArgs &);
template void wsk_edit_current(hipStream_t, const WsDev &, WsSoA, uint32_t *, uint32_t *, const WsSolidArgs &);
template void wsk_edit_current(hipStream_t, const WsDev &, WsSoA, uint32_t *, uint32_t *, const WsVolumeArgs &);
template void wsk_edit_current(hipStream_t, const WsDev &, WsSoA, uint32_t *, uint32_t *, const WsCohesionArgs &);

template <class Args>
void wsk_edit_records(hipStream_t s, const WsDev &d, uint32_t *all, const uint32_t *cnt, uint32_t world, uint32_t max_n,
                      size_t stride_words, const Args &a)
{
    if (!max_n) return;
    ws_dispatch([&](auto with) {
        using Edit = decltype(edit_of(a, with));
        hipLaunchKernelGGL(k_edit_records<Edit>, dim3(cdiv(max_n, WS_BLOCK), world), dim3(WS_BLOCK), 0, s, d, all, cnt, max_n, stride_words,
                           edit_of(a, with));
    }, a.outputs());
}
template void wsk_edit_records(hipStream_t, const WsDev &, uint32_t *, const uint32_t *, uint32_t, uint32_t, size_t, const WsForceArgs &);
template void wsk_edit_records(hipStream_t, const WsDev &, uint32_t *, const uint32_t *, uint32_t, uint32_t, size_t, const WsSolidArgs &);
template void wsk_edit_records(hipStream_t, const WsDev &, uint32_t *, const uint32_t *, uint32_t, uint32_t, size_t, const WsVolumeArgs &);
template void wsk_edit_records(hipStream_t, const WsDev &, uint32_t *, const uint32_t *, uint32_t, uint32_t, size_t, const WsCohesionArgs &);
