// fluid_compute.hpp -- header-only C++17 mirror of the reference's fluid host interface
// (src/fluid_compute.rs, src/fluid_container.rs, src/gravity.rs, src/helpers.rs) over the C ABI
// of include/wsfluid.h.  The reference's host is Rust; no Rust toolchain exists in this image, so
// this is the compiled host side that is built and exercised here (rust/fluid_compute.rs is the
// source-only Bevy shim).  Names and argument meaning follow the reference.
#pragma once

#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "wsfluid.h"

namespace water_sandbox {

struct Vec3 {
    float x, y, z;
};

// src/fluid_compute.rs:41-51,:67-79
struct FluidStaticProps {
    float delta_time = 1.0f / 60.0f;
    float collision_damping = 0.95f;
    float smoothing_radius = 0.25f;
    float target_density = 10.0f;
    float pressure_scalar = 22.0f;
    float near_pressure_scalar = 2.0f;
    float viscosity_strength = 0.1f;

    // :55-63
    ws_smoothing_kernel get_smoothing_kernel() const
    {
        ws_params p{};
        p.smoothing_radius = smoothing_radius;
        ws_smoothing_kernel k{};
        ws_get_smoothing_kernel(&p, &k);
        return k;
    }
};

// src/gravity.rs:9-33
struct Gravity {
    std::array<float, 4> value{0.f, -9.8f, 0.f, 0.f};
    void set_zero() { value = {0.f, 0.f, 0.f, 0.f}; }
    void set_default() { value = {0.f, -9.8f, 0.f, 0.f}; }
};

// src/fluid_container.rs:17-51
struct FluidContainerExt {
    std::array<float, 4> ext_min, ext_max;
};

struct FluidContainer {
    std::array<float, 3> position{0.f, 0.f, 0.f};
    std::array<float, 3> size{16.f, 9.f, 9.f};
    FluidContainerExt get_ext(float padding) const
    {
        FluidContainerExt e{};
        ws_get_ext(position.data(), size.data(), padding, e.ext_min.data(), e.ext_max.data());
        return e;
    }
};

// src/helpers.rs:3-20
inline std::vector<Vec3> cube_fluid(unsigned ni, unsigned nj, unsigned nk, float particle_rad)
{
    std::vector<Vec3> pts((size_t)ni * nj * nk);
    ws_cube_fluid(ni, nj, nk, particle_rad, reinterpret_cast<float *>(pts.data()));
    return pts;
}

using FluidParticle = ws_particle80;  // src/fluid_compute.rs:106-115

struct WsError : std::runtime_error {
    ws_status status;
    WsError(ws_status s, const std::string &what) : std::runtime_error(what), status(s) {}
};

// The role of AppComputeWorker<FluidWorker>, src/fluid_compute.rs:239-366.
class FluidWorker {
   public:
    static constexpr float PARTICLE_RADIUS = 0.1f;  // :20

    // FluidWorker::build, :277-366
    static FluidWorker build(const FluidStaticProps &props, const Gravity &gravity, const FluidContainer &container,
                             const std::vector<Vec3> &points, int device = 0)
    {
        check_abi();
        FluidWorker w;
        w.n_ = (uint32_t)points.size();
        const ws_params p = make_params(props, gravity, container);
        ws_device_cfg cfg{};
        cfg.device = device;
        const ws_status st = ws_create(&p, reinterpret_cast<const float *>(points.data()), w.n_, &cfg, &w.h_);
        if (st != WS_OK) throw WsError(st, ws_last_error(nullptr));
        return w;
    }

    // (a library of another ABI version lays ws_transport / ws_device_cfg out differently: refuse it before any struct crosses)
    static void check_abi()
    {
        if (ws_abi_version() != WS_ABI_VERSION)
            throw WsError(WS_ERR_UNSUPPORTED, "libwsfluid.so speaks another ABI version than include/wsfluid.h of this build");
    }

    // The same worker as ONE x-slab of the domain (multi-GPU: one per GPU; the reference is single-GPU).
    // Every rank is handed ALL points -- FluidParticlesInitial, :82-85 -- and keeps what ws_slab_assign gives it.
    // n_ stays the GLOBAL particle count: read_positions / read_vec / reset / write_slice work on global, id-ordered
    // arrays on a slab handle too (collective calls: every rank makes them at the same point of its frame).
    static FluidWorker build_slab(const FluidStaticProps &props, const Gravity &gravity, const FluidContainer &container,
                                  const std::vector<Vec3> &points, unsigned rank, unsigned world, const ws_transport &transport,
                                  int device = 0, unsigned flags = 0)
    {
        check_abi();
        FluidWorker w;
        w.n_ = (uint32_t)points.size();
        const ws_params p = make_params(props, gravity, container);
        std::vector<uint32_t> owner(points.size());
        ws_status st = ws_slab_assign(&p, reinterpret_cast<const float *>(points.data()), w.n_, world, owner.data());
        if (st != WS_OK) throw WsError(st, ws_last_error(nullptr));
        std::vector<Vec3> mine;
        std::vector<uint32_t> ids;
        for (uint32_t i = 0; i < w.n_; i++)
            if (owner[i] == rank) {
                mine.push_back(points[i]);
                ids.push_back(i);
            }
        ws_device_cfg cfg{};
        cfg.device = device;
        cfg.rank = rank;
        cfg.world_size = world;
        cfg.flags = flags;
        st = ws_slab_create(&p, reinterpret_cast<const float *>(mine.data()), ids.data(), (uint32_t)mine.size(), w.n_, &cfg,
                            &transport, &w.h_);
        if (st != WS_OK) throw WsError(st, ws_last_error(nullptr));
        return w;
    }

    FluidWorker(FluidWorker &&o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = nullptr; }
    FluidWorker &operator=(FluidWorker &&o) noexcept
    {
        if (this != &o) {
            ws_destroy(h_);
            h_ = o.h_;
            n_ = o.n_;
            o.h_ = nullptr;
        }
        return *this;
    }
    FluidWorker(const FluidWorker &) = delete;
    ~FluidWorker() { ws_destroy(h_); }

    // AppComputeWorker::run / ready, :396,:474
    void run() { check(ws_step(h_)); }
    void sync() { check(ws_sync(h_)); }
    bool ready()
    {
        int r = 0;
        check(ws_ready(h_, &r));
        return r != 0;
    }
    // worker.read_vec::<FluidParticle>("particles"), :478
    std::vector<FluidParticle> read_vec()
    {
        std::vector<FluidParticle> out(n_);
        check(ws_read_particles(h_, out.data()));
        return out;
    }
    std::vector<Vec3> read_positions()
    {
        std::vector<Vec3> out(n_);
        check(ws_read_positions(h_, reinterpret_cast<float *>(out.data())));
        return out;
    }
    // the same into a buffer the host keeps (page-locked once with pin()), optionally overlapped with the next
    // step: read_positions_begin(buf); run(); read_positions_end();
    void read_positions_into(std::vector<Vec3> &buf)
    {
        buf.resize(n_);
        check(ws_read_positions(h_, reinterpret_cast<float *>(buf.data())));
    }
    void read_positions_begin(std::vector<Vec3> &buf)
    {
        if (buf.size() != n_) throw WsError(WS_ERR_INVALID_ARG, "read_positions_begin: wrong buffer size");
        check(ws_read_positions_begin(h_, reinterpret_cast<float *>(buf.data())));
    }
    void read_positions_end() { check(ws_read_positions_end(h_)); }
    // ... or into the library's own page-locked double buffer (no buffer of the host's to pin): after _end, view() is the
    // frame just read and stays untouched while the next frame's copy is in flight
    void read_positions_begin_owned() { check(ws_read_positions_begin(h_, nullptr)); }
    const Vec3 *read_positions_view()
    {
        const float *p = nullptr;
        check(ws_read_positions_view(h_, &p));
        return reinterpret_cast<const Vec3 *>(p);
    }
    void pin(std::vector<Vec3> &buf) { check(ws_pin_host_buffer(h_, buf.data(), buf.size() * sizeof(Vec3))); }
    void unpin(std::vector<Vec3> &buf) { check(ws_unpin_host_buffer(h_, buf.data())); }
    // velocities.length() per particle: the input of update_particle_color, :489-502
    // The SPH density field of the current positions at the nodes origin + (i, j, k) * spacing (ws_sample_density_grid):
    // dims[0] * dims[1] * dims[2] values, x fastest; with a gradient vector, 3 floats per node in the same order.
    std::vector<float> sample_density_grid(const Vec3 &origin, const Vec3 &spacing, const uint32_t dims[3],
                                           std::vector<float> *gradient = nullptr)
    {
        const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
        std::vector<float> out(nodes);
        if (gradient) gradient->resize(nodes * 3);
        check(ws_sample_density_grid(h_, reinterpret_cast<const float *>(&origin), reinterpret_cast<const float *>(&spacing),
                                     dims, out.data(), gradient ? gradient->data() : nullptr));
        return out;
    }
    // The surface rho = iso of that field as a triangle mesh (ws_extract_surface): 3 floats per vertex (and normal, when
    // asked for), 3 vertex indices per triangle.  Counts first, then the mesh at exactly that size.
    void extract_surface(const Vec3 &origin, const Vec3 &spacing, const uint32_t dims[3], float iso, std::vector<float> &xyz,
                         std::vector<uint32_t> &tri, std::vector<float> *normals = nullptr)
    {
        const float *o = reinterpret_cast<const float *>(&origin), *s = reinterpret_cast<const float *>(&spacing);
        uint32_t nv = 0, nt = 0;
        check(ws_extract_surface(h_, o, s, dims, iso, 0, 0, nullptr, nullptr, nullptr, &nv, &nt));
        xyz.resize((size_t)nv * 3 + 1);
        tri.resize((size_t)nt * 3 + 1);
        if (normals) normals->resize((size_t)nv * 3 + 1);
        check(ws_extract_surface(h_, o, s, dims, iso, nv, nt, xyz.data(), normals ? normals->data() : nullptr, tri.data(),
                                 &nv, &nt));
        xyz.resize((size_t)nv * 3);
        tri.resize((size_t)nt * 3);
        if (normals) normals->resize((size_t)nv * 3);
    }

    // The anisotropic kernels (include/wsfluid.h ws_aniso_params; ws_default_aniso_params gives the defaults).  The
    // per-particle ellipsoids in original-id order (ws_read_anisotropy): 3 floats of centre, 6 of M (xx yy zz xy xz yz),
    // f = det M and the neighbour count per particle; any output may be null.
    void read_anisotropy(const ws_aniso_params &a, std::vector<float> *centre, std::vector<float> *matrix,
                         std::vector<float> *scale, std::vector<uint32_t> *neighbours)
    {
        const size_t n = ws_num_particles(h_);
        if (centre) centre->resize(n * 3);
        if (matrix) matrix->resize(n * 6);
        if (scale) scale->resize(n);
        if (neighbours) neighbours->resize(n);
        check(ws_read_anisotropy(h_, &a, centre ? centre->data() : nullptr, matrix ? matrix->data() : nullptr,
                                 scale ? scale->data() : nullptr, neighbours ? neighbours->data() : nullptr));
    }
    // sample_density_grid of the anisotropic field (ws_sample_aniso_grid).
    std::vector<float> sample_aniso_grid(const ws_aniso_params &a, const Vec3 &origin, const Vec3 &spacing,
                                         const uint32_t dims[3], std::vector<float> *gradient = nullptr)
    {
        const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
        std::vector<float> out(nodes);
        if (gradient) gradient->resize(nodes * 3);
        check(ws_sample_aniso_grid(h_, &a, reinterpret_cast<const float *>(&origin), reinterpret_cast<const float *>(&spacing),
                                   dims, out.data(), gradient ? gradient->data() : nullptr));
        return out;
    }
    // extract_surface of the anisotropic field (ws_extract_aniso_surface): counts first, then the mesh at that size.
    void extract_aniso_surface(const ws_aniso_params &a, const Vec3 &origin, const Vec3 &spacing, const uint32_t dims[3],
                               float iso, std::vector<float> &xyz, std::vector<uint32_t> &tri,
                               std::vector<float> *normals = nullptr)
    {
        const float *o = reinterpret_cast<const float *>(&origin), *s = reinterpret_cast<const float *>(&spacing);
        uint32_t nv = 0, nt = 0;
        check(ws_extract_aniso_surface(h_, &a, o, s, dims, iso, 0, 0, nullptr, nullptr, nullptr, &nv, &nt));
        xyz.resize((size_t)nv * 3 + 1);
        tri.resize((size_t)nt * 3 + 1);
        if (normals) normals->resize((size_t)nv * 3 + 1);
        check(ws_extract_aniso_surface(h_, &a, o, s, dims, iso, nv, nt, xyz.data(), normals ? normals->data() : nullptr,
                                       tri.data(), &nv, &nt));
        xyz.resize((size_t)nv * 3);
        tri.resize((size_t)nt * 3);
        if (normals) normals->resize((size_t)nv * 3);
    }

    // Where rays first meet the surface field = r.iso (ws_cast_rays; include/wsfluid.h has the march): one hit parameter
    // per ray, +INFINITY on a miss; with a normals vector, 3 floats per ray.  origins / directions: one Vec3 per ray
    // (directions are not normalised: t is in units of their length).  a = nullptr: the density field.
    std::vector<float> cast_rays(const ws_ray_params &r, const std::vector<Vec3> &origins, const std::vector<Vec3> &directions,
                                 std::vector<float> *normals = nullptr, const ws_aniso_params *a = nullptr)
    {
        if (origins.size() != directions.size()) throw std::runtime_error("cast_rays: one direction per origin");
        std::vector<float> t(origins.size());
        if (normals) normals->resize(origins.size() * 3);
        check(ws_cast_rays(h_, a, &r, reinterpret_cast<const float *>(origins.data()),
                           reinterpret_cast<const float *>(directions.data()), (uint32_t)origins.size(), t.data(),
                           normals ? normals->data() : nullptr));
        return t;
    }
    // The same for one ray per pixel of a width x height image (ws_cast_camera), x fastest.
    std::vector<float> cast_camera(const ws_ray_params &r, const ws_camera &cam, uint32_t width, uint32_t height,
                                   std::vector<float> *normals = nullptr, const ws_aniso_params *a = nullptr)
    {
        const uint32_t size[2] = {width, height};
        std::vector<float> t((size_t)width * height);
        if (normals) normals->resize(t.size() * 3);
        check(ws_cast_camera(h_, a, &r, &cam, size, t.data(), normals ? normals->data() : nullptr));
        return t;
    }

    // The velocities in original-id order (ws_read_velocities), read_positions' companion.
    std::vector<Vec3> read_velocities()
    {
        std::vector<Vec3> out(n_);
        check(ws_read_velocities(h_, reinterpret_cast<float *>(out.data())));
        return out;
    }
    // The fluid's velocity field at points (ws_sample_velocity_points): one Vec3 per point, zero in the air; with a
    // density vector also the density field there.
    std::vector<Vec3> sample_velocity_points(const std::vector<Vec3> &points, std::vector<float> *density = nullptr)
    {
        std::vector<Vec3> u(points.size());
        if (density) density->resize(points.size());
        check(ws_sample_velocity_points(h_, reinterpret_cast<const float *>(points.data()), (uint32_t)points.size(),
                                        reinterpret_cast<float *>(u.data()), density ? density->data() : nullptr));
        return u;
    }
    // Tracers (foam, dye, streamline points) carried through the frozen velocity field, in place: `substeps` midpoint
    // steps of dt each (ws_advect_points; include/wsfluid.h has the march).
    void advect_points(std::vector<Vec3> &points, float dt, uint32_t substeps = 1)
    {
        const ws_advect_params a = {dt, substeps};
        float *p = reinterpret_cast<float *>(points.data());
        check(ws_advect_points(h_, &a, p, (uint32_t)points.size(), p, nullptr, nullptr));
    }

    // Whitewater (include/wsfluid.h: Ihmsen et al. 2012).  The host owns the diffuse particles.
    struct Diffuse {
        std::vector<Vec3> xyz, velocity;
        std::vector<float> life;
        std::vector<uint8_t> kind;  // 0 spray, 1 foam, 2 bubble, 3 dead (after step_whitewater)
    };
    // New diffuse particles born from the current state (ws_emit_whitewater), appended to `into`; returns how many.
    uint32_t emit_whitewater(const ws_whitewater_emit_params &e, Diffuse &into)
    {
        uint32_t k = 0;
        check(ws_emit_whitewater(h_, &e, 0, nullptr, nullptr, nullptr, nullptr, &k));
        const size_t at = into.xyz.size();
        into.xyz.resize(at + k);
        into.velocity.resize(at + k);
        into.life.resize(at + k);
        into.kind.resize(at + k, 0);
        if (k)
            check(ws_emit_whitewater(h_, &e, k, reinterpret_cast<float *>(into.xyz.data() + at),
                                     reinterpret_cast<float *>(into.velocity.data() + at), into.life.data() + at, nullptr, &k));
        return k;
    }
    // Classify and move the diffuse particles by one p.dt, in place (ws_step_whitewater); the caller drops kind == 3.
    void step_whitewater(const ws_whitewater_step_params &p, Diffuse &d)
    {
        if (d.xyz.empty()) return;
        d.kind.resize(d.xyz.size());
        float *x = reinterpret_cast<float *>(d.xyz.data()), *v = reinterpret_cast<float *>(d.velocity.data());
        check(ws_step_whitewater(h_, &p, x, v, d.life.data(), (uint32_t)d.xyz.size(), x, v, d.life.data(), d.kind.data()));
    }

    // Things that float (include/wsfluid.h ws_body_forces).  The host owns the bodies: each is a run of sample points --
    // position, the material's velocity there, the share of the body's volume -- and the centre its torque is taken about.
    struct Bodies {
        std::vector<Vec3> xyz, velocity;   // per sample, grouped by body
        std::vector<float> volume;         // per sample
        std::vector<uint32_t> start;       // bodies + 1 entries: body b owns the samples start[b] .. start[b + 1] - 1
        std::vector<Vec3> centre;          // per body
        std::vector<Vec3> force, torque;   // per body, after body_forces
        std::vector<float> submerged;      // per body: the submerged volume
        std::vector<uint32_t> wet;         // per body: samples that touch the fluid
    };
    // Buoyancy and drag of the current fluid state on the bodies: one force and one torque each, for the host to integrate.
    void body_forces(const ws_body_params &p, Bodies &b)
    {
        const size_t nb = b.centre.size();
        if (nb == 0 || b.xyz.empty()) return;
        b.force.resize(nb);
        b.torque.resize(nb);
        b.submerged.resize(nb);
        b.wet.resize(nb);
        check(ws_body_forces(h_, &p, reinterpret_cast<const float *>(b.xyz.data()), reinterpret_cast<const float *>(b.velocity.data()),
                             b.volume.data(), (uint32_t)b.xyz.size(), b.start.data(), reinterpret_cast<const float *>(b.centre.data()),
                             (uint32_t)nb, reinterpret_cast<float *>(b.force.data()), reinterpret_cast<float *>(b.torque.data()),
                             b.submerged.data(), b.wet.data(), nullptr, nullptr));
    }

    // Solid things in the water (include/wsfluid.h ws_collide_solids): the fluid is pushed out of the solids and bounces
    // off their moving surfaces; per solid the contacts and the momentum it took per unit of particle mass -- the other
    // half of body_forces.  react = false: only enqueue, nothing is waited for.
    struct SolidReaction {
        std::vector<uint32_t> contacts;      // per solid
        std::vector<double> impulse, angular;  // per solid x 3; angular about the solid's centre
    };
    SolidReaction collide_solids(const std::vector<ws_solid> &solids, bool react = true)
    {
        SolidReaction r;
        if (solids.empty()) return r;
        if (!react) {
            check(ws_collide_solids(h_, solids.data(), (uint32_t)solids.size(), nullptr, nullptr, nullptr));
            return r;
        }
        r.contacts.resize(solids.size());
        r.impulse.resize(3 * solids.size());
        r.angular.resize(3 * solids.size());
        check(ws_collide_solids(h_, solids.data(), (uint32_t)solids.size(), r.contacts.data(), r.impulse.data(), r.angular.data()));
        return r;
    }

    // Solids given as signed-distance volumes (include/wsfluid.h ws_volume_upload, ws_collide_volumes): a grid of
    // distances per shape, uploaded once into one of WS_MAX_VOLUMES slots (sdf: nx * ny * nz floats, x fastest; empty =
    // release the slot), then any number of poses of the resident volumes per call, with the solids' reaction.
    void upload_volume(uint32_t slot, const float origin[3], const float spacing[3], const uint32_t dims[3],
                       const std::vector<float> &sdf)
    {
        check(ws_volume_upload(h_, slot, origin, spacing, dims, sdf.empty() ? nullptr : sdf.data()));
    }
    SolidReaction collide_volumes(const std::vector<ws_volume_pose> &poses, bool react = true)
    {
        SolidReaction r;
        if (poses.empty()) return r;
        if (!react) {
            check(ws_collide_volumes(h_, poses.data(), (uint32_t)poses.size(), nullptr, nullptr, nullptr));
            return r;
        }
        r.contacts.resize(poses.size());
        r.impulse.resize(3 * poses.size());
        r.angular.resize(3 * poses.size());
        check(ws_collide_volumes(h_, poses.data(), (uint32_t)poses.size(), r.contacts.data(), r.impulse.data(), r.angular.data()));
        return r;
    }

    // Surface tension and XSPH velocity smoothing between two steps (include/wsfluid.h ws_apply_cohesion): one explicit
    // step of dt on the velocities.  Returns the number of particles that had a contributing neighbour.
    uint32_t apply_cohesion(const ws_cohesion_params &p, float dt)
    {
        uint32_t affected = 0;
        check(ws_apply_cohesion(h_, &p, dt, &affected));
        return affected;
    }

    // What the fluid carries (include/wsfluid.h ws_write_attributes .. ws_sample_attribute_points): four floats per
    // particle, by id, kept on the device -- dye, temperature, whatever the host means by them.  Paint them with up to
    // WS_MAX_BRUSHES spheres, mix them between neighbours, sample them where the mesh's vertices are.
    void write_attributes(const std::vector<float> &a) { check(ws_write_attributes(h_, a.empty() ? nullptr : a.data())); }
    std::vector<float> read_attributes()
    {
        std::vector<float> out((size_t)n_ * 4);
        check(ws_read_attributes(h_, out.data()));
        return out;
    }
    std::vector<uint32_t> paint_attributes(const std::vector<ws_brush> &brushes)
    {
        std::vector<uint32_t> painted(brushes.size());
        if (!brushes.empty()) check(ws_paint_attributes(h_, brushes.data(), (uint32_t)brushes.size(), painted.data()));
        return painted;
    }
    uint32_t diffuse_attributes(const ws_diffuse_params &p, float dt)
    {
        uint32_t affected = 0;
        check(ws_diffuse_attributes(h_, &p, dt, &affected));
        return affected;
    }
    // xyz: m * 3 floats; returns m * 4
    std::vector<float> sample_attribute_points(const std::vector<float> &xyz)
    {
        std::vector<float> out(xyz.size() / 3 * 4);
        if (!out.empty()) check(ws_sample_attribute_points(h_, xyz.data(), (uint32_t)(xyz.size() / 3), out.data(), nullptr));
        return out;
    }
    // dims[0] * dims[1] * dims[2] nodes, x fastest; returns 4 floats per node
    std::vector<float> sample_attribute_grid(const float origin[3], const float spacing[3], const uint32_t dims[3])
    {
        std::vector<float> out((size_t)dims[0] * dims[1] * dims[2] * 4);
        check(ws_sample_attribute_grid(h_, origin, spacing, dims, out.data(), nullptr));
        return out;
    }

    std::vector<float> read_speeds()
    {
        std::vector<float> out(n_);
        check(ws_read_speeds(h_, out.data()));
        return out;
    }
    // the three worker.write calls of update(), :479-481
    void write(const FluidStaticProps &props, const Gravity &gravity, const FluidContainer &container)
    {
        const ws_params p = make_params(props, gravity, container);
        check(ws_set_params(h_, &p));
    }
    // worker.write_slice("particles", ..), :521
    void write_slice(const std::vector<FluidParticle> &particles)
    {
        if (particles.size() != n_) throw WsError(WS_ERR_INVALID_ARG, "write_slice: wrong particle count");
        check(ws_write_particles(h_, particles.data()));
    }
    // despawn_liquid's reset, :517-524
    void reset(const std::vector<Vec3> &points)
    {
        if (points.size() != n_) throw WsError(WS_ERR_INVALID_ARG, "reset: wrong particle count");
        check(ws_reset(h_, reinterpret_cast<const float *>(points.data())));
    }
    uint32_t num_particles() const { return n_; }
    ws_handle *raw() { return h_; }

    static ws_params make_params(const FluidStaticProps &props, const Gravity &gravity, const FluidContainer &container)
    {
        ws_params p{};
        p.delta_time = props.delta_time;
        p.collision_damping = props.collision_damping;
        p.smoothing_radius = props.smoothing_radius;
        p.target_density = props.target_density;
        p.pressure_scalar = props.pressure_scalar;
        p.near_pressure_scalar = props.near_pressure_scalar;
        p.viscosity_strength = props.viscosity_strength;
        const FluidContainerExt e = container.get_ext(PARTICLE_RADIUS);  // :302
        for (int i = 0; i < 4; i++) {
            p.gravity[i] = gravity.value[i];
            p.ext_min[i] = e.ext_min[i];
            p.ext_max[i] = e.ext_max[i];
        }
        return p;
    }

   private:
    FluidWorker() = default;
    void check(ws_status st)
    {
        if (st != WS_OK) throw WsError(st, ws_last_error(h_));
    }
    ws_handle *h_ = nullptr;
    uint32_t n_ = 0;
};

}  // namespace water_sandbox
