"""ctypes binding of libwsfluid.so plus a host-side mirror of the reference's fluid
worker interface (src/fluid_compute.rs), used by the tests, bench.py and smoke().

This module is plumbing over the C ABI in include/wsfluid.h.  It never computes physics
itself and has no CPU fallback: if the HIP library is missing or no gfx950 device is
visible, construction raises.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import build as _build

INF = 999999999  # assets/simulation.wgsl:36

# FluidParticle, src/fluid_compute.rs:106-115
PARTICLE_DTYPE = np.dtype(
    [
        ("position", np.float32, 4),
        ("density", np.float32, 2),
        ("pressure", np.float32, 2),
        ("velocity", np.float32, 4),
        ("acceleration", np.float32, 4),
        ("predicted_position", np.float32, 4),
    ]
)
assert PARTICLE_DTYPE.itemsize == 80

WS_FLAG_PROFILE = 1
WS_FLAG_REFERENCE_ORDER = 2
WS_FLAG_IEEE_DIVISION = 4
WS_FLAG_GRAPH = 8
WS_FLAG_EXACT_MESSAGES = 16
WS_FLAG_LAGGED_MESSAGES = 32
WS_FLAG_FIXED_MESSAGES = 64
WS_FLAG_NO_OVERLAP = 128
WS_FLAG_GRAPH_MULTIRANK = 256
WS_ABI_VERSION = 2
KERNEL_IDS = {"cell_scan": 0, "cell_scatter": 1, "reorder": 2, "density": 3, "force_integrate_bin": 4, "bin": 5}

# every symbol include/wsfluid.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "ws_default_params", "ws_get_smoothing_kernel", "ws_cube_fluid", "ws_get_ext",
    "ws_bit_sorter_stage_count", "ws_status_string", "ws_abi_version", "ws_create", "ws_destroy",
    "ws_step", "ws_ready", "ws_sync", "ws_set_params", "ws_read_positions", "ws_read_particles",
    "ws_reset", "ws_write_particles", "ws_pin_host_buffer", "ws_unpin_host_buffer", "ws_read_speeds", "ws_read_positions_begin", "ws_read_positions_end", "ws_read_positions_view", "ws_slab_counters", "ws_rccl_unique_id", "ws_rccl_transport_create",
    "ws_rccl_transport_destroy", "ws_rccl_last_error", "ws_rccl_transport_communicators",
    "ws_local_hub_create", "ws_local_hub_destroy", "ws_local_transport_create", "ws_local_transport_destroy", "ws_read_sort_view", "ws_last_error", "ws_num_particles",
    "ws_steps_done", "ws_kernel_name", "ws_profile_read", "ws_profile_reset", "ws_profile_select",
    "ws_grid_dims", "ws_read_stats", "ws_slab_assign", "ws_slab_create", "ws_slab_read_particles", "ws_slab_rebalance", "ws_slab_balanced_cuts",
    "ws_sample_density_grid", "ws_sample_density_points", "ws_extract_surface",
    "ws_default_aniso_params", "ws_read_anisotropy", "ws_sample_aniso_grid", "ws_sample_aniso_points",
    "ws_extract_aniso_surface", "ws_cast_rays", "ws_cast_camera",
    "ws_read_velocities", "ws_sample_velocity_grid", "ws_sample_velocity_points", "ws_advect_points",
    "ws_default_whitewater_emit_params", "ws_default_whitewater_step_params", "ws_read_whitewater", "ws_emit_whitewater",
    "ws_step_whitewater", "ws_apply_forces", "ws_default_body_params", "ws_body_forces", "ws_collide_solids",
    "ws_volume_upload", "ws_collide_volumes", "ws_default_cohesion_params", "ws_read_cohesion", "ws_apply_cohesion",
    "ws_default_diffuse_params", "ws_write_attributes", "ws_read_attributes", "ws_paint_attributes", "ws_diffuse_attributes",
    "ws_sample_attribute_grid", "ws_sample_attribute_points",
    "ws_reserve_particles", "ws_particle_capacity", "ws_add_particles", "ws_remove_particles", "ws_remove_particle_ids",
    "ws_measure", "ws_select_particles",
]


class WsParams(C.Structure):
    """ws_params: FluidStaticProps + Gravity + FluidContainerExt."""

    _fields_ = [
        ("delta_time", C.c_float),
        ("collision_damping", C.c_float),
        ("smoothing_radius", C.c_float),
        ("target_density", C.c_float),
        ("pressure_scalar", C.c_float),
        ("near_pressure_scalar", C.c_float),
        ("viscosity_strength", C.c_float),
        ("reserved0", C.c_float),
        ("gravity", C.c_float * 4),
        ("ext_min", C.c_float * 4),
        ("ext_max", C.c_float * 4),
    ]


class WsAnisoParams(C.Structure):
    """ws_aniso_params: the anisotropic kernels' lambda, k_r, k_n and N_eps (include/wsfluid.h)."""

    _fields_ = [
        ("smoothing", C.c_float),
        ("max_ratio", C.c_float),
        ("lone_scale", C.c_float),
        ("min_neighbours", C.c_uint32),
    ]


class WsRayParams(C.Structure):
    """ws_ray_params: the march of ws_cast_rays / ws_cast_camera (include/wsfluid.h)."""

    _fields_ = [
        ("t_start", C.c_float),
        ("dt", C.c_float),
        ("steps", C.c_uint32),
        ("refine", C.c_uint32),
        ("iso", C.c_float),
    ]


class WsAdvectParams(C.Structure):
    """ws_advect_params: the march of ws_advect_points (include/wsfluid.h)."""

    _fields_ = [("dt", C.c_float), ("substeps", C.c_uint32)]


class WsWhitewaterEmitParams(C.Structure):
    """ws_whitewater_emit_params: thresholds, rates and the spawn cylinder of ws_emit_whitewater (include/wsfluid.h)."""

    _fields_ = [
        ("tau_trapped", C.c_float * 2),
        ("tau_crest", C.c_float * 2),
        ("tau_energy", C.c_float * 2),
        ("k_trapped", C.c_float),
        ("k_crest", C.c_float),
        ("crest_align", C.c_float),
        ("dt", C.c_float),
        ("radius", C.c_float),
        ("lifetime", C.c_float * 2),
        ("max_per_particle", C.c_uint32),
        ("seed", C.c_uint32),
    ]


class WsWhitewaterStepParams(C.Structure):
    """ws_whitewater_step_params: the classes and forces of ws_step_whitewater (include/wsfluid.h)."""

    _fields_ = [
        ("dt", C.c_float),
        ("spray_max", C.c_uint32),
        ("bubble_min", C.c_uint32),
        ("buoyancy", C.c_float),
        ("drag", C.c_float),
    ]


WS_FORCE_RADIAL, WS_FORCE_JET, WS_FORCE_VORTEX = 0, 1, 2
WS_MAX_FORCES = 16


class WsForce(C.Structure):
    """ws_force: one emitter of ws_apply_forces -- a puller / pusher, a jet or a vortex with a brake (include/wsfluid.h)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("centre", C.c_float * 3),
        ("axis", C.c_float * 3),
        ("radius", C.c_float),
        ("strength", C.c_float),
        ("damping", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


WS_SOLID_SPHERE, WS_SOLID_BOX, WS_SOLID_CAPSULE = 0, 1, 2
WS_SOLID_HOLLOW = 1
WS_MAX_SOLIDS = 16


class WsSolid(C.Structure):
    """ws_solid: one obstacle of ws_collide_solids -- a sphere, a box or a capsule, solid or hollow (include/wsfluid.h)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("flags", C.c_uint32),
        ("centre", C.c_float * 3),
        ("rot", C.c_float * 9),
        ("size", C.c_float * 3),
        ("velocity", C.c_float * 3),
        ("angular_velocity", C.c_float * 3),
        ("restitution", C.c_float),
        ("friction", C.c_float),
        ("margin", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


WS_MAX_VOLUMES = 4
WS_MAX_VOLUME_POSES = 16


class WsVolumePose(C.Structure):
    """ws_volume_pose: one instance of a resident signed-distance volume in ws_collide_volumes (include/wsfluid.h)."""

    _fields_ = [
        ("slot", C.c_uint32),
        ("flags", C.c_uint32),
        ("centre", C.c_float * 3),
        ("rot", C.c_float * 9),
        ("velocity", C.c_float * 3),
        ("angular_velocity", C.c_float * 3),
        ("restitution", C.c_float),
        ("friction", C.c_float),
        ("margin", C.c_float),
        ("reserved", C.c_uint32),
    ]


class WsBodyParams(C.Structure):
    """ws_body_params: buoyancy and drag of ws_body_forces (include/wsfluid.h)."""

    _fields_ = [
        ("fluid_density", C.c_float),
        ("drag", C.c_float),
        ("rest_density", C.c_float),
        ("reserved", C.c_uint32),
    ]


class WsCohesionParams(C.Structure):
    """ws_cohesion_params: the strengths of ws_read_cohesion / ws_apply_cohesion (include/wsfluid.h)."""

    _fields_ = [
        ("cohesion", C.c_float),
        ("curvature", C.c_float),
        ("xsph", C.c_float),
        ("rest_density", C.c_float),
        ("reserved", C.c_uint32),
    ]


WS_BRUSH_MIX, WS_BRUSH_ADD = 0, 1
WS_MAX_BRUSHES = 16


class WsBrush(C.Structure):
    """ws_brush: one brush of ws_paint_attributes -- a sphere that mixes a value into, or adds it to, the painted channels
    of the particles in reach (include/wsfluid.h)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("centre", C.c_float * 3),
        ("radius", C.c_float),
        ("falloff", C.c_float),
        ("strength", C.c_float),
        ("channels", C.c_uint32),
        ("value", C.c_float * 4),
    ]


WS_SINK_SPHERE, WS_SINK_BOX = 0, 1
WS_MAX_SINKS = 16
REMOVED = 0xFFFFFFFF  # out_new_id of a removed particle


class WsSink(C.Structure):
    """ws_sink: a region ws_remove_particles drains (32 bytes)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("reserved", C.c_uint32),
        ("centre", C.c_float * 3),
        ("half", C.c_float * 3),
    ]


WS_MAX_REGIONS = 16
WS_GAUGE_ATTRIBUTES = 1  # ws_measure flags bit 0: also sum the four attributes
GAUGE_FIXED = 24  # the sums are fixed point: sum / 2**24


class WsGauge(C.Structure):
    """ws_gauge: what ws_measure reports of one region (152 bytes)."""

    _fields_ = [
        ("count", C.c_uint64),
        ("sum_pos", C.c_int64 * 3),
        ("sum_vel", C.c_int64 * 3),
        ("sum_ang", C.c_int64 * 3),
        ("sum_speed2", C.c_int64),
        ("sum_attr", C.c_int64 * 4),
        ("min_pos", C.c_float * 3),
        ("max_pos", C.c_float * 3),
        ("max_speed2", C.c_float),
        ("reserved", C.c_uint32),
    ]


GAUGE_DTYPE = np.dtype([("count", np.uint64), ("sum_pos", np.int64, 3), ("sum_vel", np.int64, 3), ("sum_ang", np.int64, 3),
                        ("sum_speed2", np.int64), ("sum_attr", np.int64, 4), ("min_pos", np.float32, 3),
                        ("max_pos", np.float32, 3), ("max_speed2", np.float32), ("reserved", np.uint32)])
assert GAUGE_DTYPE.itemsize == C.sizeof(WsGauge) == 152


class WsDiffuseParams(C.Structure):
    """ws_diffuse_params: the per-channel rates and the iteration count of ws_diffuse_attributes (include/wsfluid.h)."""

    _fields_ = [
        ("rate", C.c_float * 4),
        ("iterations", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class WsCamera(C.Structure):
    """ws_camera: pixel (i, j) looks along forward + u * right + w * up from eye (include/wsfluid.h)."""

    _fields_ = [
        ("eye", C.c_float * 3),
        ("forward", C.c_float * 3),
        ("right", C.c_float * 3),
        ("up", C.c_float * 3),
    ]


class WsSmoothingKernel(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("pow2", "pow2_der", "pow3", "pow3_der", "spikey_pow3")]


class WsDeviceCfg(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("flags", C.c_uint32),
        ("rank", C.c_uint32),
        ("world_size", C.c_uint32),
        ("capacity", C.c_uint32),
        ("ghost_capacity", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
        ("stream", C.c_void_p),
    ]


class WsError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("wsfluid status %d: %s" % (status, text))
        self.status = status


_lib = None


def lib_path():
    return _build.LIB


def load_library():
    """Load libwsfluid.so, building it first if it is stale.  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("WSFLUID_LIBRARY")  # an alternative build of the same ABI (kernel A/B runs)
    if not path:
        if _build.needs_build():
            _build.build_library()
        path = _build.LIB
    _lib = bind_library(path)
    return _lib


def bind_library(path):
    """dlopen a build of the wsfluid ABI and declare its prototypes (the product library, or the test-only
    reference-order build the tests load explicitly)."""
    L = C.CDLL(path)
    vp, u32, fp = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
    L.ws_default_params.argtypes = [C.POINTER(WsParams)]
    L.ws_get_smoothing_kernel.argtypes = [C.POINTER(WsParams), C.POINTER(WsSmoothingKernel)]
    L.ws_cube_fluid.argtypes = [u32, u32, u32, C.c_float, vp]
    L.ws_get_ext.argtypes = [vp, vp, C.c_float, vp, vp]
    L.ws_bit_sorter_stage_count.argtypes = [u32]
    L.ws_bit_sorter_stage_count.restype = u32
    L.ws_status_string.argtypes = [C.c_int]
    L.ws_status_string.restype = C.c_char_p
    L.ws_abi_version.restype = u32
    L.ws_create.argtypes = [C.POINTER(WsParams), vp, u32, C.POINTER(WsDeviceCfg), C.POINTER(vp)]
    L.ws_destroy.argtypes = [vp]
    L.ws_step.argtypes = [vp]
    L.ws_ready.argtypes = [vp, C.POINTER(C.c_int)]
    L.ws_sync.argtypes = [vp]
    L.ws_set_params.argtypes = [vp, C.POINTER(WsParams)]
    L.ws_read_positions.argtypes = [vp, vp]
    L.ws_read_particles.argtypes = [vp, vp]
    L.ws_reset.argtypes = [vp, vp]
    L.ws_pin_host_buffer.argtypes = [vp, vp, C.c_uint64]
    L.ws_read_speeds.argtypes = [vp, vp]
    L.ws_read_positions_begin.argtypes = [vp, vp]
    L.ws_read_positions_end.argtypes = [vp]
    L.ws_read_positions_view.argtypes = [vp, C.POINTER(vp)]
    L.ws_unpin_host_buffer.argtypes = [vp, vp]
    L.ws_write_particles.argtypes = [vp, vp]
    L.ws_read_sort_view.argtypes = [vp, vp, vp, vp]
    L.ws_last_error.argtypes = [vp]
    L.ws_last_error.restype = C.c_char_p
    L.ws_num_particles.argtypes = [vp]
    L.ws_num_particles.restype = u32
    L.ws_steps_done.argtypes = [vp]
    L.ws_steps_done.restype = C.c_uint64
    L.ws_kernel_name.argtypes = [u32]
    L.ws_kernel_name.restype = C.c_char_p
    L.ws_profile_read.argtypes = [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.ws_profile_reset.argtypes = [vp]
    L.ws_profile_select.argtypes = [vp, u32]
    L.ws_grid_dims.argtypes = [vp, vp]
    L.ws_read_stats.argtypes = [vp, vp]
    L.ws_sample_density_grid.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ws_sample_density_points.argtypes = [vp, vp, u32, vp, vp]
    L.ws_extract_surface.argtypes = [vp, vp, vp, vp, C.c_float, u32, u32, vp, vp, vp, vp, vp]
    L.ws_default_aniso_params.argtypes = [vp]
    L.ws_read_anisotropy.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ws_sample_aniso_grid.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ws_sample_aniso_points.argtypes = [vp, vp, vp, u32, vp, vp]
    L.ws_extract_aniso_surface.argtypes = [vp, vp, vp, vp, vp, C.c_float, u32, u32, vp, vp, vp, vp, vp]
    L.ws_cast_rays.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp]
    L.ws_cast_camera.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ws_read_velocities.argtypes = [vp, vp]
    L.ws_sample_velocity_grid.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ws_sample_velocity_points.argtypes = [vp, vp, u32, vp, vp]
    L.ws_advect_points.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.ws_default_whitewater_emit_params.argtypes = [vp]
    L.ws_default_whitewater_step_params.argtypes = [vp]
    L.ws_read_whitewater.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ws_emit_whitewater.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.ws_step_whitewater.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.ws_apply_forces.argtypes = [vp, vp, u32, C.c_float, vp]
    L.ws_default_cohesion_params.argtypes = [vp]
    L.ws_read_cohesion.argtypes = [vp, vp, C.c_float, vp, vp, vp, vp]
    L.ws_apply_cohesion.argtypes = [vp, vp, C.c_float, vp]
    L.ws_default_diffuse_params.argtypes = [vp]
    L.ws_write_attributes.argtypes = [vp, vp]
    L.ws_read_attributes.argtypes = [vp, vp]
    L.ws_paint_attributes.argtypes = [vp, vp, u32, vp]
    L.ws_diffuse_attributes.argtypes = [vp, vp, C.c_float, vp]
    L.ws_sample_attribute_grid.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ws_sample_attribute_points.argtypes = [vp, vp, u32, vp, vp]
    L.ws_default_body_params.argtypes = [vp]
    L.ws_collide_solids.argtypes = [vp, vp, u32, vp, vp, vp]
    L.ws_volume_upload.argtypes = [vp, u32, vp, vp, vp, vp]
    L.ws_collide_volumes.argtypes = [vp, vp, u32, vp, vp, vp]
    L.ws_body_forces.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.ws_reserve_particles.argtypes = [vp, u32]
    L.ws_particle_capacity.argtypes = [vp]
    L.ws_particle_capacity.restype = u32
    L.ws_add_particles.argtypes = [vp, vp, vp, vp, u32]
    L.ws_remove_particles.argtypes = [vp, vp, u32, vp, vp]
    L.ws_remove_particle_ids.argtypes = [vp, vp, u32, vp]
    L.ws_measure.argtypes = [vp, vp, u32, u32, vp]
    L.ws_select_particles.argtypes = [vp, vp, u32, u32, vp, vp]
    return L


def _aniso_args(aniso):
    """The leading arguments an anisotropic call adds after the handle: () for the density sampler, (params,) else."""
    return () if aniso is None else (C.byref(aniso),)


def sample_density_grid(L, h, check, origin, spacing, dims, gradient=False, want=True, aniso=None):
    """ws_sample_density_grid: (density (nz, ny, nx), gradient (nz, ny, nx, 3) or None); dims = (nx, ny, nz).
    want=False (slab handles): contribute to the collective call and return (None, None).  aniso (a WsAnisoParams):
    ws_sample_aniso_grid instead."""
    f = L.ws_sample_density_grid if aniso is None else L.ws_sample_aniso_grid
    a = _aniso_args(aniso)
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    sp = np.ascontiguousarray(spacing, np.float32).reshape(3)
    d = np.ascontiguousarray(dims, np.uint32).reshape(3)
    if not want:
        check(f(h, *a, o.ctypes.data, sp.ctypes.data, d.ctypes.data, None, None))
        return None, None
    nx, ny, nz = (int(v) for v in d)
    rho = np.empty((nz, ny, nx), np.float32)
    grad = np.empty((nz, ny, nx, 3), np.float32) if gradient else None
    check(f(h, *a, o.ctypes.data, sp.ctypes.data, d.ctypes.data, rho.ctypes.data, grad.ctypes.data if gradient else None))
    return rho, grad


def sample_density_points(L, h, check, xyz, gradient=False, want=True, aniso=None):
    """ws_sample_density_points (aniso: ws_sample_aniso_points): (density (m,), gradient (m, 3) or None)."""
    f = L.ws_sample_density_points if aniso is None else L.ws_sample_aniso_points
    a = _aniso_args(aniso)
    q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    m = q.shape[0]
    if not want:
        check(f(h, *a, q.ctypes.data, m, None, None))
        return None, None
    rho = np.empty(m, np.float32)
    grad = np.empty((m, 3), np.float32) if gradient else None
    check(f(h, *a, q.ctypes.data, m, rho.ctypes.data, grad.ctypes.data if gradient else None))
    return rho, grad


def read_anisotropy(L, h, check, aniso, n, want=True):
    """ws_read_anisotropy: (centre (n, 3), matrix (n, 6) xx yy zz xy xz yz, scale (n,), neighbours (n,) uint32)."""
    if not want:
        check(L.ws_read_anisotropy(h, C.byref(aniso), None, None, None, None))
        return None, None, None, None
    c = np.empty((n, 3), np.float32)
    m = np.empty((n, 6), np.float32)
    f = np.empty(n, np.float32)
    nb = np.empty(n, np.uint32)
    check(L.ws_read_anisotropy(h, C.byref(aniso), c.ctypes.data, m.ctypes.data, f.ctypes.data, nb.ctypes.data))
    return c, m, f, nb


def aniso_params(**kw):
    """ws_default_aniso_params, with any field overridden by keyword (smoothing, max_ratio, lone_scale, min_neighbours)."""
    p = WsAnisoParams()
    load_library().ws_default_aniso_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def ray_params(t_start, dt, steps, refine, iso):
    return WsRayParams(float(t_start), float(dt), int(steps), int(refine), float(iso))


def camera(eye, forward, right, up):
    cam = WsCamera()
    for name, v in (("eye", eye), ("forward", forward), ("right", right), ("up", up)):
        for k in range(3):
            getattr(cam, name)[k] = float(v[k])
    return cam


def cast_rays(L, h, check, march, origins, directions, normals=True, want=True, aniso=None):
    """ws_cast_rays: (t (m,) float32, +inf on a miss; normal (m, 3) float32 or None).  march: a WsRayParams; aniso=None:
    the density field, else a WsAnisoParams.  want=False (slab handles): contribute and return (None, None)."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    assert o.shape == v.shape
    m = o.shape[0]
    a = None if aniso is None else C.byref(aniso)
    if not want:
        check(L.ws_cast_rays(h, a, C.byref(march), o.ctypes.data, v.ctypes.data, m, None, None))
        return None, None
    t = np.empty(m, np.float32)
    n = np.empty((m, 3), np.float32) if normals else None
    check(L.ws_cast_rays(h, a, C.byref(march), o.ctypes.data, v.ctypes.data, m, t.ctypes.data, n.ctypes.data if normals else None))
    return t, n


def cast_camera(L, h, check, march, cam, size, normals=True, want=True, aniso=None):
    """ws_cast_camera: (t (H, W) float32, normal (H, W, 3) float32 or None) of a size = (W, H) image; cam: a WsCamera."""
    sz = np.ascontiguousarray(size, np.uint32).reshape(2)
    a = None if aniso is None else C.byref(aniso)
    if not want:
        check(L.ws_cast_camera(h, a, C.byref(march), C.byref(cam), sz.ctypes.data, None, None))
        return None, None
    wd, ht = int(sz[0]), int(sz[1])
    t = np.empty((ht, wd), np.float32)
    n = np.empty((ht, wd, 3), np.float32) if normals else None
    check(L.ws_cast_camera(h, a, C.byref(march), C.byref(cam), sz.ctypes.data, t.ctypes.data, n.ctypes.data if normals else None))
    return t, n


def read_velocities(L, h, check, n, want=True):
    """ws_read_velocities: (n, 3) float32 in original-id order.  want=False (slab handles): contribute, return None."""
    if not want:
        check(L.ws_read_velocities(h, None))
        return None
    out = np.empty((n, 3), np.float32)
    check(L.ws_read_velocities(h, out.ctypes.data))
    return out


def sample_velocity_grid(L, h, check, origin, spacing, dims, density=True, want=True):
    """ws_sample_velocity_grid: (velocity (nz, ny, nx, 3), density (nz, ny, nx) or None); dims = (nx, ny, nz).
    want=False (slab handles): contribute to the collective call and return (None, None)."""
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    sp = np.ascontiguousarray(spacing, np.float32).reshape(3)
    d = np.ascontiguousarray(dims, np.uint32).reshape(3)
    if not want:
        check(L.ws_sample_velocity_grid(h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, None, None))
        return None, None
    nx, ny, nz = (int(v) for v in d)
    u = np.empty((nz, ny, nx, 3), np.float32)
    rho = np.empty((nz, ny, nx), np.float32) if density else None
    check(L.ws_sample_velocity_grid(h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, u.ctypes.data,
                                    rho.ctypes.data if density else None))
    return u, rho


def sample_velocity_points(L, h, check, xyz, density=True, want=True):
    """ws_sample_velocity_points: (velocity (m, 3), density (m,) or None)."""
    q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    m = q.shape[0]
    if not want:
        check(L.ws_sample_velocity_points(h, q.ctypes.data, m, None, None))
        return None, None
    u = np.empty((m, 3), np.float32)
    rho = np.empty(m, np.float32) if density else None
    check(L.ws_sample_velocity_points(h, q.ctypes.data, m, u.ctypes.data, rho.ctypes.data if density else None))
    return u, rho


def advect_params(dt, substeps=1):
    return WsAdvectParams(float(dt), int(substeps))


def advect_points(L, h, check, march, xyz, field=False, want=True):
    """ws_advect_points: the tracers xyz (m, 3) after march.substeps midpoint steps of march.dt through the frozen velocity
    field: (xyz (m, 3), velocity (m, 3) or None, density (m,) or None), the last two -- the field at the final positions --
    with field=True.  march: a WsAdvectParams.  want=False (slab handles): contribute and return (None, None, None)."""
    q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    m = q.shape[0]
    if not want:
        check(L.ws_advect_points(h, C.byref(march), q.ctypes.data, m, None, None, None))
        return None, None, None
    out = np.empty((m, 3), np.float32)
    u = np.empty((m, 3), np.float32) if field else None
    rho = np.empty(m, np.float32) if field else None
    check(L.ws_advect_points(h, C.byref(march), q.ctypes.data, m, out.ctypes.data, u.ctypes.data if field else None,
                             rho.ctypes.data if field else None))
    return out, u, rho


def _whitewater_params(cls, default, fields):
    p = cls()
    status = default(C.byref(p))
    assert status == 0, status
    for k, v in fields.items():
        cur = getattr(p, k)  # (an unknown name raises)
        if isinstance(cur, C.Array):
            for t, x in enumerate(v):
                cur[t] = x
        else:
            setattr(p, k, v)
    return p


def whitewater_emit_params(**fields):
    """ws_default_whitewater_emit_params with the given fields replaced (tau_trapped=(lo, hi), seed=7, ...)."""
    return _whitewater_params(WsWhitewaterEmitParams, load_library().ws_default_whitewater_emit_params, fields)


def whitewater_step_params(**fields):
    """ws_default_whitewater_step_params with the given fields replaced."""
    return _whitewater_params(WsWhitewaterStepParams, load_library().ws_default_whitewater_step_params, fields)


def read_whitewater(L, h, check, n, want=True):
    """ws_read_whitewater: a dict of the stage by id -- trapped, crest, align, energy (n,) float32, normal (n, 3),
    neighbours (n,) uint32.  want=False (slab handles): contribute, return None."""
    if not want:
        check(L.ws_read_whitewater(h, None, None, None, None, None, None))
        return None
    out = {k: np.empty(n, np.float32) for k in ("trapped", "crest", "align", "energy")}
    out["normal"] = np.empty((n, 3), np.float32)
    out["neighbours"] = np.empty(n, np.uint32)
    check(L.ws_read_whitewater(h, *(out[k].ctypes.data for k in ("trapped", "crest", "align", "energy", "normal",
                                                                  "neighbours"))))
    return out


def emit_whitewater(L, h, check, emit, cap=None, want=True):
    """ws_emit_whitewater: a dict of the new diffuse particles -- xyz, velocity (k, 3) float32, life (k,), source (k,)
    uint32 (the emitting particle's id), count = k.  cap: the capacity offered; None asks for the count first.  When the
    count exceeds cap the arrays are None and count says what to offer.  want=False (slab handles): contribute."""
    if not want:
        check(L.ws_emit_whitewater(h, C.byref(emit), 0, None, None, None, None, None))
        return None
    k = C.c_uint32(0)
    if cap is None:
        check(L.ws_emit_whitewater(h, C.byref(emit), 0, None, None, None, None, C.byref(k)))
        cap = k.value
    xyz = np.empty((cap, 3), np.float32)
    vel = np.empty((cap, 3), np.float32)
    life = np.empty(cap, np.float32)
    src = np.empty(cap, np.uint32)
    check(L.ws_emit_whitewater(h, C.byref(emit), cap, xyz.ctypes.data, vel.ctypes.data, life.ctypes.data, src.ctypes.data,
                               C.byref(k)))
    if k.value > cap:
        return dict(xyz=None, velocity=None, life=None, source=None, count=k.value)
    return dict(xyz=xyz[:k.value], velocity=vel[:k.value], life=life[:k.value], source=src[:k.value], count=k.value)


def step_whitewater(L, h, check, step, xyz, velocity, life, in_place=False, want=True):
    """ws_step_whitewater: (xyz (m, 3), velocity (m, 3), life (m,), class (m,) uint8: 0 spray, 1 foam, 2 bubble, 3 dead)
    after one step.dt.  in_place: xyz, velocity and life must be contiguous float32 arrays and are overwritten (and
    returned).  want=False (slab handles): contribute and return None."""
    if in_place:
        for a in (xyz, velocity, life):
            assert a.dtype == np.float32 and a.flags.c_contiguous
        p, v, l = xyz.reshape(-1, 3), velocity.reshape(-1, 3), life.reshape(-1)
    else:
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(velocity, np.float32).reshape(-1, 3)
        l = np.ascontiguousarray(life, np.float32).reshape(-1)
    m = p.shape[0]
    assert v.shape[0] == m and l.shape[0] == m
    if not want:
        check(L.ws_step_whitewater(h, C.byref(step), p.ctypes.data, v.ctypes.data, l.ctypes.data, m, None, None, None, None))
        return None
    op, ov, ol = (p, v, l) if in_place else (np.empty_like(p), np.empty_like(v), np.empty_like(l))
    cls = np.empty(m, np.uint8)
    check(L.ws_step_whitewater(h, C.byref(step), p.ctypes.data, v.ctypes.data, l.ctypes.data, m, op.ctypes.data,
                               ov.ctypes.data, ol.ctypes.data, cls.ctypes.data))
    return op, ov, ol, cls


def force(kind, centre, radius, strength, axis=(0.0, 0.0, 0.0), damping=0.0):
    """One ws_force: kind = WS_FORCE_RADIAL / _JET / _VORTEX (or "radial" / "jet" / "vortex")."""
    kind = {"radial": WS_FORCE_RADIAL, "jet": WS_FORCE_JET, "vortex": WS_FORCE_VORTEX}.get(kind, kind)
    return WsForce(kind, (C.c_float * 3)(*centre), (C.c_float * 3)(*axis), radius, strength, damping, (C.c_uint32 * 2)(0, 0))


def apply_forces(L, h, check, forces, dt, counts=True):
    """ws_apply_forces: one Euler step of the emitters' acceleration on the velocities (include/wsfluid.h has the
    definition).  forces: a WsForce or a sequence of them.  Returns the per-emitter counts of affected particles (k,)
    uint32, or None with counts=False (a single handle then only enqueues)."""
    forces = [forces] if isinstance(forces, WsForce) else list(forces)
    arr = (WsForce * max(len(forces), 1))(*forces)
    out = np.zeros(max(len(forces), 1), np.uint32) if counts else None
    check(L.ws_apply_forces(h, C.byref(arr), len(forces), dt, out.ctypes.data if counts else None))
    return out[:len(forces)] if counts else None


def sink(kind, centre, half):
    """One ws_sink: kind = WS_SINK_SPHERE / _BOX (or "sphere" / "box"); half = the box's three half extents, or the
    sphere's radius (a number, or (R, 0, 0))."""
    kind = {"sphere": WS_SINK_SPHERE, "box": WS_SINK_BOX}.get(kind, kind)
    if np.ndim(half) == 0:
        half = (float(half), 0.0, 0.0)
    return WsSink(kind, 0, (C.c_float * 3)(*(float(x) for x in centre)), (C.c_float * 3)(*(float(x) for x in half)))


def add_particles(L, h, check, positions, velocities=None, attributes=None):
    """ws_add_particles: m new particles with the ids n .. n+m-1 (include/wsfluid.h has the definition).  positions (m, 3);
    velocities (m, 3) or None (at rest); attributes (m, 4) or None (+0).  Returns m."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    m = pos.shape[0]
    vel = None if velocities is None else np.ascontiguousarray(velocities, np.float32).reshape(-1, 3)
    att = None if attributes is None else np.ascontiguousarray(attributes, np.float32).reshape(-1, 4)
    assert vel is None or vel.shape[0] == m, (vel.shape, m)
    assert att is None or att.shape[0] == m, (att.shape, m)
    check(L.ws_add_particles(h, pos.ctypes.data if m else None, None if vel is None else vel.ctypes.data,
                             None if att is None else att.ctypes.data, m))
    return m


def remove_particles(L, h, check, n, sinks, counts=True, new_ids=True):
    """ws_remove_particles: every particle the sinks (a WsSink or a sequence of them) contain; n = the count before the
    call.  Returns (per-sink counts (k,) uint32 or None, new id by old id (n,) uint32 -- REMOVED where the particle is
    gone -- or None)."""
    sinks = [sinks] if isinstance(sinks, WsSink) else list(sinks)
    arr = (WsSink * max(len(sinks), 1))(*sinks)
    removed = np.zeros(max(len(sinks), 1), np.uint32) if counts else None
    ids = np.empty(n, np.uint32) if new_ids else None
    check(L.ws_remove_particles(h, C.byref(arr), len(sinks), removed.ctypes.data if counts else None,
                                ids.ctypes.data if new_ids else None))
    return (removed[:len(sinks)] if counts else None), ids


def remove_particle_ids(L, h, check, n, ids, new_ids=True):
    """ws_remove_particle_ids: the particles named in ids (duplicates count once); n = the count before the call.  Returns
    the new id by old id (n,) uint32 -- REMOVED where the particle is gone -- or None."""
    ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    out = np.empty(n, np.uint32) if new_ids else None
    check(L.ws_remove_particle_ids(h, ids.ctypes.data if ids.size else None, ids.size, out.ctypes.data if new_ids else None))
    return out


region = sink  # a ws_region is a ws_sink by another name: the same 32 bytes, validation and containment


class Gauges(dict):
    """ws_measure's k gauges as numpy arrays with the raw integers: count (k,) uint64; sum_pos, sum_vel, sum_ang (k, 3),
    sum_speed2 (k,), sum_attr (k, 4) int64, fixed point 2**-24; min_pos, max_pos (k, 3), max_speed2 (k,) float32."""

    def total(self, name):
        """The sum `name` ("pos", "vel", "ang", "speed2", "attr") as float64: the integers divided by 2**24."""
        return self["sum_" + name].astype(np.float64) / 2.0 ** GAUGE_FIXED

    def mean(self, name):
        """total(name) / count per region: the centre of mass ("pos"), the mean velocity, ... (NaN for an empty region)."""
        t = self.total(name)
        c = self["count"].astype(np.float64).reshape((-1,) + (1,) * (t.ndim - 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            return t / c


def _regions(regions):
    regions = [regions] if isinstance(regions, WsSink) else list(regions)
    return regions, (WsSink * max(len(regions), 1))(*regions)


def measure(L, h, check, regions, attributes=False, want=True):
    """ws_measure: up to 16 gauges in one pass (include/wsfluid.h has the definition).  regions: a WsSink or a sequence of
    them (region() / sink() builds one).  Returns a Gauges dict; want=False (a slab rank that only contributes): None."""
    regions, arr = _regions(regions)
    out = np.zeros(max(len(regions), 1), GAUGE_DTYPE)
    check(L.ws_measure(h, C.byref(arr), len(regions), WS_GAUGE_ATTRIBUTES if attributes else 0, out.ctypes.data if want else None))
    if not want:
        return None
    out = out[:len(regions)]
    return Gauges((name, np.ascontiguousarray(out[name])) for name in GAUGE_DTYPE.names if name != "reserved")


def select_particles(L, h, check, regions, cap):
    """ws_select_particles: (ids (min(total, cap),) uint32 ascending, total) of the particles at least one region contains."""
    regions, arr = _regions(regions)
    cap = int(cap)
    ids = np.empty(cap, np.uint32)
    total = C.c_uint32(0)
    check(L.ws_select_particles(h, C.byref(arr), len(regions), cap, ids.ctypes.data if cap else None, C.byref(total)))
    return ids[:min(cap, total.value)].copy(), int(total.value)


def cohesion_params(**fields):
    """ws_default_cohesion_params with the given fields replaced (cohesion, curvature, xsph, rest_density)."""
    return _whitewater_params(WsCohesionParams, load_library().ws_default_cohesion_params, fields)


def read_cohesion(L, h, check, n, params, dt, want=True):
    """ws_read_cohesion: a dict of the stage by id -- normal (n, 3) float32, density (n,), dv (n, 3), neighbours (n,)
    uint32 (include/wsfluid.h has the definition).  want=False (slab handles): contribute, return None."""
    if not want:
        check(L.ws_read_cohesion(h, C.byref(params), dt, None, None, None, None))
        return None
    out = dict(normal=np.empty((n, 3), np.float32), density=np.empty(n, np.float32), dv=np.empty((n, 3), np.float32),
               neighbours=np.empty(n, np.uint32))
    check(L.ws_read_cohesion(h, C.byref(params), dt, *(out[k].ctypes.data for k in ("normal", "density", "dv", "neighbours"))))
    return out


def apply_cohesion(L, h, check, params, dt, count=True):
    """ws_apply_cohesion: v += dv of the stage on every particle that has a contributing neighbour.  Returns how many
    particles were affected, or None with count=False (a single handle then only enqueues)."""
    out = C.c_uint32(0)
    check(L.ws_apply_cohesion(h, C.byref(params), dt, C.byref(out) if count else None))
    return int(out.value) if count else None


def brush(kind, centre, radius, value, strength=1.0, falloff=0.0, channels=15):
    """One ws_brush: kind = WS_BRUSH_MIX / _ADD (or "mix" / "add"); value = four floats; channels = a bit mask (bit c =
    channel c is painted) or a sequence of channel numbers."""
    kind = {"mix": WS_BRUSH_MIX, "add": WS_BRUSH_ADD}.get(kind, kind)
    if not isinstance(channels, (int, np.integer)):
        channels = sum(1 << int(c) for c in set(channels))
    return WsBrush(kind, (C.c_float * 3)(*(float(x) for x in centre)), float(radius), float(falloff), float(strength),
                   int(channels), (C.c_float * 4)(*(float(x) for x in value)))


def diffuse_params(**fields):
    """ws_default_diffuse_params with the given fields replaced (rate=(r0, r1, r2, r3), iterations=8)."""
    return _whitewater_params(WsDiffuseParams, load_library().ws_default_diffuse_params, fields)


def write_attributes(L, h, check, n, values):
    """ws_write_attributes: values (n, 4) float32 by id, or None for all +0."""
    if values is None:
        check(L.ws_write_attributes(h, None))
        return
    a = np.ascontiguousarray(values, np.float32)
    assert a.size == n * 4, (a.shape, n)
    check(L.ws_write_attributes(h, a.ctypes.data))


def read_attributes(L, h, check, n, want=True):
    """ws_read_attributes: (n, 4) float32 in original-id order.  want=False (slab handles): return None."""
    if not want:
        check(L.ws_read_attributes(h, None))
        return None
    out = np.empty((n, 4), np.float32)
    check(L.ws_read_attributes(h, out.ctypes.data))
    return out


def paint_attributes(L, h, check, brushes, counts=True):
    """ws_paint_attributes: the brushes (a WsBrush or a sequence of them), in order, on every particle in their reach.
    Returns the per-brush counts of painted particles (k,) uint32, or None with counts=False."""
    brushes = [brushes] if isinstance(brushes, WsBrush) else list(brushes)
    arr = (WsBrush * max(len(brushes), 1))(*brushes)
    out = np.zeros(max(len(brushes), 1), np.uint32) if counts else None
    check(L.ws_paint_attributes(h, C.byref(arr), len(brushes), out.ctypes.data if counts else None))
    return out[:len(brushes)] if counts else None


def diffuse_attributes(L, h, check, params, dt, count=True):
    """ws_diffuse_attributes: params.iterations kernel-weighted exchanges between neighbours at params.rate * dt per
    channel.  Returns how many particles have a contributing neighbour, or None with count=False."""
    out = C.c_uint32(0)
    check(L.ws_diffuse_attributes(h, C.byref(params), dt, C.byref(out) if count else None))
    return int(out.value) if count else None


def sample_attribute_grid(L, h, check, origin, spacing, dims, density=True, want=True):
    """ws_sample_attribute_grid: (value (nz, ny, nx, 4), density (nz, ny, nx) or None); dims = (nx, ny, nz).
    want=False (slab handles): contribute to the collective call and return (None, None)."""
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    sp = np.ascontiguousarray(spacing, np.float32).reshape(3)
    d = np.ascontiguousarray(dims, np.uint32).reshape(3)
    if not want:
        check(L.ws_sample_attribute_grid(h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, None, None))
        return None, None
    nx, ny, nz = (int(v) for v in d)
    val = np.empty((nz, ny, nx, 4), np.float32)
    rho = np.empty((nz, ny, nx), np.float32) if density else None
    check(L.ws_sample_attribute_grid(h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, val.ctypes.data,
                                     rho.ctypes.data if density else None))
    return val, rho


def sample_attribute_points(L, h, check, xyz, density=True, want=True):
    """ws_sample_attribute_points: (value (m, 4), density (m,) or None)."""
    q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    m = q.shape[0]
    if not want:
        check(L.ws_sample_attribute_points(h, q.ctypes.data, m, None, None))
        return None, None
    val = np.empty((m, 4), np.float32)
    rho = np.empty(m, np.float32) if density else None
    check(L.ws_sample_attribute_points(h, q.ctypes.data, m, val.ctypes.data, rho.ctypes.data if density else None))
    return val, rho


def solid(kind, centre, size, rot=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), hollow=False, velocity=(0.0, 0.0, 0.0),
          angular_velocity=(0.0, 0.0, 0.0), restitution=0.0, friction=0.0, margin=0.0):
    """One ws_solid: kind = WS_SOLID_SPHERE / _BOX / _CAPSULE (or "sphere" / "box" / "capsule"); size = a radius, three
    half extents or (radius, half length); rot = the nine floats of the rows R_0 R_1 R_2 (or a 3 x 3 nested sequence)."""
    kind = {"sphere": WS_SOLID_SPHERE, "box": WS_SOLID_BOX, "capsule": WS_SOLID_CAPSULE}.get(kind, kind)
    size = [float(x) for x in np.atleast_1d(np.asarray(size, np.float64))]
    rot = [float(x) for x in np.asarray(rot, np.float64).reshape(-1)]
    return WsSolid(kind, WS_SOLID_HOLLOW if hollow else 0, (C.c_float * 3)(*centre), (C.c_float * 9)(*rot),
                   (C.c_float * 3)(*(size + [0.0] * (3 - len(size)))), (C.c_float * 3)(*velocity), (C.c_float * 3)(*angular_velocity),
                   restitution, friction, margin, (C.c_uint32 * 2)(0, 0))


def collide_solids(L, h, check, solids, reaction=True):
    """ws_collide_solids: push the fluid out of the solids, respond to their motion, sum the reaction (include/wsfluid.h
    has the definition).  solids: a WsSolid or a sequence of them.  Returns (contacts (k,) uint32, impulse (k, 3) float64,
    angular (k, 3) float64) -- per unit of particle mass, angular about each solid's centre -- or None with
    reaction=False (a single handle then only enqueues)."""
    solids = [solids] if isinstance(solids, WsSolid) else list(solids)
    k = len(solids)
    arr = (WsSolid * max(k, 1))(*solids)
    if not reaction:
        check(L.ws_collide_solids(h, C.byref(arr), k, None, None, None))
        return None
    contacts, impulse, angular = np.zeros(max(k, 1), np.uint32), np.zeros((max(k, 1), 3)), np.zeros((max(k, 1), 3))
    check(L.ws_collide_solids(h, C.byref(arr), k, contacts.ctypes.data, impulse.ctypes.data, angular.ctypes.data))
    return contacts[:k], impulse[:k], angular[:k]


def volume_pose(slot, centre=(0.0, 0.0, 0.0), rot=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), velocity=(0.0, 0.0, 0.0),
                angular_velocity=(0.0, 0.0, 0.0), restitution=0.0, friction=0.0, margin=0.0):
    """One ws_volume_pose: an instance of the volume resident in `slot`; centre = where the volume's local origin lies,
    rot = the nine floats of the rows R_0 R_1 R_2 (or a 3 x 3 nested sequence)."""
    rot = [float(x) for x in np.asarray(rot, np.float64).reshape(-1)]
    return WsVolumePose(slot, 0, (C.c_float * 3)(*centre), (C.c_float * 9)(*rot), (C.c_float * 3)(*velocity),
                        (C.c_float * 3)(*angular_velocity), restitution, friction, margin, 0)


def upload_volume(L, h, check, slot, origin, spacing, sdf):
    """ws_volume_upload: sdf (nz, ny, nx) float32 -- x fastest in memory -- or None to release the slot."""
    if sdf is None:
        check(L.ws_volume_upload(h, slot, None, None, None, None))
        return
    sdf = np.ascontiguousarray(sdf, np.float32)
    assert sdf.ndim == 3, "sdf has the shape (nz, ny, nx)"
    dims = (C.c_uint32 * 3)(sdf.shape[2], sdf.shape[1], sdf.shape[0])
    check(L.ws_volume_upload(h, slot, (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), dims, sdf.ctypes.data))


def collide_volumes(L, h, check, poses, reaction=True):
    """ws_collide_volumes: ws_collide_solids against poses of the resident signed-distance volumes (include/wsfluid.h has
    the definition).  poses: a WsVolumePose or a sequence of them.  Returns what collide_solids returns, per pose."""
    poses = [poses] if isinstance(poses, WsVolumePose) else list(poses)
    k = len(poses)
    arr = (WsVolumePose * max(k, 1))(*poses)
    if not reaction:
        check(L.ws_collide_volumes(h, C.byref(arr), k, None, None, None))
        return None
    contacts, impulse, angular = np.zeros(max(k, 1), np.uint32), np.zeros((max(k, 1), 3)), np.zeros((max(k, 1), 3))
    check(L.ws_collide_volumes(h, C.byref(arr), k, contacts.ctypes.data, impulse.ctypes.data, angular.ctypes.data))
    return contacts[:k], impulse[:k], angular[:k]


def body_params(**fields):
    """ws_default_body_params with the given fields replaced (fluid_density, drag, rest_density)."""
    return _whitewater_params(WsBodyParams, load_library().ws_default_body_params, fields)


BodyForces = collections.namedtuple("BodyForces", "force torque volume wet sample_force sample_fraction")


def body_forces(L, h, check, params, xyz, velocity, volume, body_start, centres, samples=False, want=True):
    """ws_body_forces: buoyancy and drag of the fluid on nb host-owned bodies described by m samples -- xyz, velocity
    (m, 3), volume (m,), body_start (nb + 1,) uint32, centres (nb, 3).  A BodyForces of force, torque (nb, 3), volume
    (nb,) float32, wet (nb,) uint32 and, with samples=True, sample_force (m, 3) and sample_fraction (m,), else None.
    params: a WsBodyParams.  want=False (slab handles): contribute and return None."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(velocity, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(volume, np.float32).reshape(-1)
    bs = np.ascontiguousarray(body_start, np.uint32).reshape(-1)
    c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    m, nb = p.shape[0], c.shape[0]
    assert w.shape[0] == m and v.shape[0] == m and bs.shape[0] == nb + 1
    args = (h, C.byref(params), p.ctypes.data, w.ctypes.data, v.ctypes.data, m, bs.ctypes.data, c.ctypes.data, nb)
    if not want:
        check(L.ws_body_forces(*args, None, None, None, None, None, None))
        return None
    out = BodyForces(np.empty((nb, 3), np.float32), np.empty((nb, 3), np.float32), np.empty(nb, np.float32),
                     np.empty(nb, np.uint32), np.empty((m, 3), np.float32) if samples else None,
                     np.empty(m, np.float32) if samples else None)
    check(L.ws_body_forces(*args, *(None if a is None else a.ctypes.data for a in out)))
    return out


def extract_surface(L, h, check, origin, spacing, dims, iso, normals=True, want=True, collective=False, cap=None,
                    aniso=None):
    """ws_extract_surface: (vertices (V, 3) f32, normals (V, 3) f32 or None, triangles (T, 3) uint32).
    cap = (vertices, triangles): a first guess of the capacities, and one retry at the exact counts when it is too small.
    cap=None, and always on slab handles (collective): a counts-only call first (it samples no gradient), then one at the
    exact counts -- every rank makes the same two calls; want=False contributes to both and returns (None, None, None).
    aniso (a WsAnisoParams): ws_extract_aniso_surface instead."""
    f = L.ws_extract_surface if aniso is None else L.ws_extract_aniso_surface
    a = _aniso_args(aniso)
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    sp = np.ascontiguousarray(spacing, np.float32).reshape(3)
    d = np.ascontiguousarray(dims, np.uint32).reshape(3)
    nv, nt = C.c_uint32(0), C.c_uint32(0)

    def call(cap_v, cap_t, xyz=None, nrm=None, tri=None, counts=True):
        check(f(h, *a, o.ctypes.data, sp.ctypes.data, d.ctypes.data, C.c_float(iso), cap_v, cap_t,
                None if xyz is None else xyz.ctypes.data, None if nrm is None else nrm.ctypes.data,
                None if tri is None else tri.ctypes.data, C.byref(nv) if counts else None,
                C.byref(nt) if counts else None))

    if not want:  # a slab rank that only contributes, to both calls
        call(0, 0, counts=False)
        call(0, 0, counts=False)
        return None, None, None
    if collective or cap is None:
        call(0, 0)
        cap_v, cap_t = nv.value, nt.value
    else:
        cap_v, cap_t = (int(c) for c in cap)
    for _ in range(2):
        xyz = np.empty((cap_v, 3), np.float32)
        nrm = np.empty((cap_v, 3), np.float32) if normals else None
        tri = np.empty((cap_t, 3), np.uint32)
        call(cap_v, cap_t, xyz, nrm, tri)
        if nv.value <= cap_v and nt.value <= cap_t:
            return xyz[:nv.value], (nrm[:nv.value] if normals else None), tri[:nt.value]
        if collective:
            break
        cap_v, cap_t = nv.value, nt.value
    raise RuntimeError("%s: the mesh changed between two calls on the same state" % f.__name__)


# ---------------------------------------------------------------------------------------
# host-side mirror of the reference's resources (names follow the reference)
# ---------------------------------------------------------------------------------------
def default_params():
    """FluidStaticProps::default + Gravity::default + FluidContainer::default().get_ext(0.1)."""
    p = WsParams()
    load_library().ws_default_params(C.byref(p))
    return p


def get_smoothing_kernel(params):
    """FluidStaticProps::get_smoothing_kernel, src/fluid_compute.rs:55-63."""
    k = WsSmoothingKernel()
    load_library().ws_get_smoothing_kernel(C.byref(params), C.byref(k))
    return k


def cube_fluid(ni, nj, nk, particle_rad=0.1):
    """helpers::cube_fluid, src/helpers.rs:3-20."""
    out = np.empty((ni * nj * nk, 3), np.float32)
    load_library().ws_cube_fluid(ni, nj, nk, particle_rad, out.ctypes.data)
    return out


def get_ext(position, size, padding=0.1):
    """FluidContainer::get_ext, src/fluid_container.rs:42-50."""
    pos = np.asarray(position, np.float32)
    sz = np.asarray(size, np.float32)
    mn = np.zeros(4, np.float32)
    mx = np.zeros(4, np.float32)
    load_library().ws_get_ext(pos.ctypes.data, sz.ctypes.data, padding, mn.ctypes.data, mx.ctypes.data)
    return mn, mx


def make_params(container_size=(16.0, 9.0, 9.0), container_position=(0.0, 0.0, 0.0), padding=0.1, **overrides):
    p = default_params()
    mn, mx = get_ext(container_position, container_size, padding)
    for i in range(4):
        p.ext_min[i] = float(mn[i])
        p.ext_max[i] = float(mx[i])
    for k, v in overrides.items():
        if k == "gravity":
            for i in range(4):
                p.gravity[i] = float(v[i]) if i < len(v) else 0.0
        else:
            setattr(p, k, v)
    return p


class FluidWorker:
    """The role of AppComputeWorker<FluidWorker> (src/fluid_compute.rs:239-366): owns the
    device buffers, `run()` enqueues one step, `ready()` polls, `read_vec("particles")`
    returns the 80-byte records in original-id order."""

    def __init__(self, positions, params=None, device=0, profile=False, reference_order=False, ieee_division=False,
                 library=None, graph=False):
        self._L = library if library is not None else load_library()
        self._h = C.c_void_p()
        self._surface_cap = None  # extract_surface's first guess of the capacities, from the previous mesh
        self._aniso_cap = None  # the same for extract_aniso_surface
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self.n = positions.shape[0]
        self.params = params if params is not None else default_params()
        cfg = WsDeviceCfg()
        cfg.device = device
        cfg.flags = ((WS_FLAG_PROFILE if profile else 0) | (WS_FLAG_REFERENCE_ORDER if reference_order else 0)
                     | (WS_FLAG_IEEE_DIVISION if ieee_division else 0) | (WS_FLAG_GRAPH if graph else 0))
        st = self._L.ws_create(C.byref(self.params), positions.ctypes.data, self.n, C.byref(cfg), C.byref(self._h))
        if st != 0:
            raise WsError(st, (self._L.ws_last_error(None) or b"").decode())

    @classmethod
    def build(cls, positions, params=None, **kw):
        return cls(positions, params, **kw)

    def _check(self, st):
        if st != 0:
            raise WsError(st, (self._L.ws_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self._L.ws_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # AppComputeWorker::run / ready
    def run(self, steps=1):
        for _ in range(steps):
            self._check(self._L.ws_step(self._h))

    step = run

    def ready(self):
        r = C.c_int(0)
        self._check(self._L.ws_ready(self._h, C.byref(r)))
        return bool(r.value)

    def sync(self):
        self._check(self._L.ws_sync(self._h))

    # worker.write("fluid_props" | "smoothing_kernel" | "gravity", ..)
    def set_params(self, params):
        self._check(self._L.ws_set_params(self._h, C.byref(params)))
        self.params = params

    def read_positions(self):
        out = np.empty((self.n, 3), np.float32)
        self._check(self._L.ws_read_positions(self._h, out.ctypes.data))
        return out

    def read_positions_begin(self, buf):
        """Start an asynchronous id-order position readback into `buf` ((n, 3) float32, ideally pinned); steps
        enqueued afterwards overlap with the copy.  Finish with read_positions_end()."""
        assert buf.dtype == np.float32 and buf.shape == (self.n, 3) and buf.flags.c_contiguous
        self._check(self._L.ws_read_positions_begin(self._h, buf.ctypes.data))

    def read_positions_end(self):
        self._check(self._L.ws_read_positions_end(self._h))

    def read_positions_begin_owned(self):
        """The same into one of the two page-locked buffers the library owns (ws_read_positions_begin(h, NULL))."""
        self._check(self._L.ws_read_positions_begin(self._h, None))

    def read_positions_view(self, n=None):
        """(n, 3) float32 view of the library-owned buffer the last finished readback filled (no copy; valid until
        the second-next read_positions_begin_owned)."""
        p = C.c_void_p()
        self._check(self._L.ws_read_positions_view(self._h, C.byref(p)))
        n = self.n if n is None else n
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n, 3))

    def read_speeds(self):
        """|velocity| per particle in original-id order (the reference's speed colouring input)."""
        out = np.empty(self.n, np.float32)
        self._check(self._L.ws_read_speeds(self._h, out.ctypes.data))
        return out

    def read_positions_into(self, buf):
        """ws_read_positions into a caller-owned (n, 3) float32 array (pin it with pin_host_buffer for PCIe rate)."""
        assert buf.dtype == np.float32 and buf.shape == (self.n, 3) and buf.flags.c_contiguous
        self._check(self._L.ws_read_positions(self._h, buf.ctypes.data))
        return buf

    def pin_host_buffer(self, buf):
        self._check(self._L.ws_pin_host_buffer(self._h, buf.ctypes.data, buf.nbytes))

    def unpin_host_buffer(self, buf):
        self._check(self._L.ws_unpin_host_buffer(self._h, buf.ctypes.data))

    def read_vec(self, name="particles"):
        if name != "particles":
            raise KeyError(name)
        out = np.empty(self.n, PARTICLE_DTYPE)
        self._check(self._L.ws_read_particles(self._h, out.ctypes.data))
        return out

    def write_slice(self, name, data):
        if name != "particles":
            raise KeyError(name)
        data = np.ascontiguousarray(data, PARTICLE_DTYPE)
        assert data.shape[0] == self.n
        self._check(self._L.ws_write_particles(self._h, data.ctypes.data))

    def reset(self, positions):
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        assert positions.shape[0] == self.n
        self._check(self._L.ws_reset(self._h, positions.ctypes.data))

    def sort_view(self):
        """(particle_cell_indicies, particle_indicies, cell_offsets) as the reference holds them."""
        keys = np.empty(self.n, np.uint32)
        perm = np.empty(self.n, np.uint32)
        off = np.empty(self.n, np.uint32)
        self._check(self._L.ws_read_sort_view(self._h, keys.ctypes.data, perm.ctypes.data, off.ctypes.data))
        return keys, perm, off

    def sample_density_grid(self, origin, spacing, dims, gradient=False):
        """The SPH density field of the current positions at the nodes origin + (i, j, k) * spacing, dims = (nx, ny, nz):
        a float32 array of shape (nz, ny, nx) (x fastest), with gradient=True also its gradient, shape (nz, ny, nx, 3)."""
        rho, grad = sample_density_grid(self._L, self._h, self._check, origin, spacing, dims, gradient)
        return (rho, grad) if gradient else rho

    def sample_density_points(self, xyz, gradient=False):
        """The same field at m points (xyz: (m, 3)): shape (m,), with gradient=True also (m, 3)."""
        rho, grad = sample_density_points(self._L, self._h, self._check, xyz, gradient)
        return (rho, grad) if gradient else rho

    def extract_surface(self, origin, spacing, dims, iso, normals=True):
        """The surface rho = iso of the density field on the grid origin + (i, j, k) * spacing, dims = (nx, ny, nz), as a
        mesh: (vertices (V, 3) float32, normals (V, 3) float32 or None, triangles (T, 3) uint32), triangles counter-
        clockwise seen from outside the fluid (include/wsfluid.h ws_extract_surface has the definition)."""
        mesh = extract_surface(self._L, self._h, self._check, origin, spacing, dims, iso, normals, cap=self._surface_cap)
        nv, nt = len(mesh[0]), len(mesh[2])
        self._surface_cap = (nv + nv // 4 + 4096, nt + nt // 4 + 8192)  # (a mesh moves little from one frame to the next)
        return mesh

    # anisotropic kernels (include/wsfluid.h ws_aniso_params): aniso=None takes the defaults, see aniso_params()
    def anisotropy(self, aniso=None):
        """Per particle in original-id order: (centre (n, 3), M (n, 6) as xx yy zz xy xz yz, f = det M (n,),
        neighbour count (n,) uint32) -- the ellipsoids a splatting renderer draws."""
        return read_anisotropy(self._L, self._h, self._check, aniso or aniso_params(), self.n)

    def sample_aniso_grid(self, origin, spacing, dims, gradient=False, aniso=None):
        """sample_density_grid of the anisotropic field."""
        rho, grad = sample_density_grid(self._L, self._h, self._check, origin, spacing, dims, gradient,
                                        aniso=aniso or aniso_params())
        return (rho, grad) if gradient else rho

    def sample_aniso_points(self, xyz, gradient=False, aniso=None):
        """sample_density_points of the anisotropic field."""
        rho, grad = sample_density_points(self._L, self._h, self._check, xyz, gradient, aniso=aniso or aniso_params())
        return (rho, grad) if gradient else rho

    def extract_aniso_surface(self, origin, spacing, dims, iso, normals=True, aniso=None):
        """extract_surface of the anisotropic field (its own first guess of the capacities)."""
        mesh = extract_surface(self._L, self._h, self._check, origin, spacing, dims, iso, normals, cap=self._aniso_cap,
                               aniso=aniso or aniso_params())
        nv, nt = len(mesh[0]), len(mesh[2])
        self._aniso_cap = (nv + nv // 4 + 4096, nt + nt // 4 + 8192)
        return mesh

    def cast_rays(self, march, origins, directions, normals=True, aniso=None):
        """Where each ray origin + t * direction first meets the surface field = march.iso: (t (m,), +inf on a miss;
        unit normal (m, 3) or None).  march = ray_params(t_start, dt, steps, refine, iso); aniso=None casts at the density
        field, a WsAnisoParams at the anisotropic one (include/wsfluid.h ws_cast_rays has the definition)."""
        return cast_rays(self._L, self._h, self._check, march, origins, directions, normals, aniso=aniso)

    def cast_camera(self, march, cam, size, normals=True, aniso=None):
        """The same for one ray per pixel of a size = (W, H) image seen by cam = camera(eye, forward, right, up):
        (t (H, W), normal (H, W, 3) or None)."""
        return cast_camera(self._L, self._h, self._check, march, cam, size, normals, aniso=aniso)

    def read_velocities(self):
        """The velocities in original-id order, (n, 3) float32: read_positions' companion."""
        return read_velocities(self._L, self._h, self._check, self.n)

    def sample_velocity_grid(self, origin, spacing, dims, density=False):
        """The fluid's velocity field (the kernel-weighted mean of the particles' velocities, zero in the air) at the nodes
        origin + (i, j, k) * spacing, dims = (nx, ny, nz): float32 (nz, ny, nx, 3); with density=True also the density
        field (nz, ny, nx), the bits sample_density_grid returns."""
        u, rho = sample_velocity_grid(self._L, self._h, self._check, origin, spacing, dims, density)
        return (u, rho) if density else u

    def sample_velocity_points(self, xyz, density=False):
        """The same field at m points (xyz: (m, 3)): (m, 3), with density=True also (m,)."""
        u, rho = sample_velocity_points(self._L, self._h, self._check, xyz, density)
        return (u, rho) if density else u

    def advect_points(self, march, xyz, field=False):
        """Tracers (foam, dye, streamline points) carried through the frozen velocity field of the current state:
        march = advect_params(dt, substeps).  The final positions (m, 3); with field=True (positions, velocity (m, 3),
        density (m,)) there (include/wsfluid.h ws_advect_points has the definition)."""
        out, u, rho = advect_points(self._L, self._h, self._check, march, xyz, field)
        return (out, u, rho) if field else out

    def read_whitewater(self):
        """The whitewater potentials of every fluid particle, by id (Ihmsen et al. 2012): a dict of trapped (trapped-air
        potential), crest (wave-crest curvature), align (velocity . normal), energy (kinetic, per unit mass), normal
        (n, 3) and neighbours (include/wsfluid.h ws_read_whitewater has the definition)."""
        return read_whitewater(self._L, self._h, self._check, self.n)

    def emit_whitewater(self, emit, cap=None):
        """New diffuse particles born from the current state: emit = whitewater_emit_params(...).  A dict of xyz,
        velocity, life, source and count; with a cap that is too small the arrays are None and count says what to offer."""
        return emit_whitewater(self._L, self._h, self._check, emit, cap)

    def step_whitewater(self, step, xyz, velocity, life, in_place=False):
        """Classify the host's diffuse particles against the current fluid (spray / foam / bubble / dead) and move them by
        step.dt: step = whitewater_step_params(...).  (xyz, velocity, life, class)."""
        return step_whitewater(self._L, self._h, self._check, step, xyz, velocity, life, in_place)

    def apply_forces(self, forces, dt, counts=True):
        """Push, pull, blow on or stir the fluid between two steps: forces = force(...) or a list of up to 16, applied
        to the velocities as one Euler step of dt.  The per-emitter counts of affected particles, or None with
        counts=False (the call then only enqueues)."""
        return apply_forces(self._L, self._h, self._check, forces, dt, counts)

    def read_cohesion(self, params, dt):
        """The surface-tension and XSPH stage of every fluid particle, by id, read-only: params = cohesion_params(...).
        A dict of normal (n, 3), density (n,), dv (n, 3) -- what apply_cohesion would add -- and neighbours (n,)."""
        return read_cohesion(self._L, self._h, self._check, self.n, params, dt)

    def apply_cohesion(self, params, dt, count=True):
        """Surface tension (Akinci et al. 2013) and XSPH velocity smoothing between two steps: params =
        cohesion_params(...), applied to the velocities as one explicit step of dt.  The number of affected particles,
        or None with count=False (the call then only enqueues)."""
        return apply_cohesion(self._L, self._h, self._check, params, dt, count)

    def write_attributes(self, values):
        """Give every particle its four attribute floats -- dye, temperature, whatever the host means by them: values
        (n, 4) by id, or None for all +0.  Nothing of the physics reads them; the steps carry them along."""
        write_attributes(self._L, self._h, self._check, self.n, values)

    def read_attributes(self):
        """The attributes of every particle, (n, 4) float32 by id."""
        return read_attributes(self._L, self._h, self._check, self.n)

    def paint_attributes(self, brushes, counts=True):
        """Paint the particles inside up to 16 spheres: brushes = brush(...) or a list, applied in order.  The per-brush
        counts of painted particles, or None with counts=False."""
        return paint_attributes(self._L, self._h, self._check, brushes, counts)

    def diffuse_attributes(self, params, dt, count=True):
        """Mix the attributes between neighbours: params = diffuse_params(rate=..., iterations=...).  The number of
        particles with a contributing neighbour, or None with count=False."""
        return diffuse_attributes(self._L, self._h, self._check, params, dt, count)

    def sample_attribute_grid(self, origin, spacing, dims, density=False):
        """The attribute field on a grid: value (nz, ny, nx, 4), with density=True (value, density)."""
        val, rho = sample_attribute_grid(self._L, self._h, self._check, origin, spacing, dims, density)
        return (val, rho) if density else val

    def sample_attribute_points(self, xyz, density=False):
        """The attribute field at points -- the vertices of extract_surface, to colour the mesh: value (m, 4), with
        density=True (value, density)."""
        val, rho = sample_attribute_points(self._L, self._h, self._check, xyz, density)
        return (val, rho) if density else val

    def collide_solids(self, solids, reaction=True):
        """Put solid things in the water between two steps: solids = solid(...) or a list of up to 16.  Particles nearer
        than a solid's margin are pushed out and bounce off its moving surface.  (contacts, impulse, angular): per solid
        the contact count and the momentum the solid took per unit of particle mass, linear and about its centre -- or None
        with reaction=False (the call then only enqueues)."""
        return collide_solids(self._L, self._h, self._check, solids, reaction)

    def upload_volume(self, slot, origin, spacing, sdf):
        """Make a signed-distance volume resident in slot 0 .. 3: sdf of shape (nz, ny, nx), negative inside the solid,
        node (i, j, k) at the local coordinates origin + (i, j, k) * spacing.  sdf=None releases the slot."""
        upload_volume(self._L, self._h, self._check, slot, origin, spacing, sdf)

    def collide_volumes(self, poses, reaction=True):
        """Put resident volumes in the water between two steps: poses = volume_pose(...) or a list of up to 16.  What
        collide_solids returns, per pose."""
        return collide_volumes(self._L, self._h, self._check, poses, reaction)

    def body_forces(self, params, xyz, velocity, volume, body_start, centres, samples=False):
        """What the fluid does to things floating in it: buoyancy and drag on nb host-owned bodies, each a group of sample
        points (xyz, the material's velocity there, the share of the body's volume), as one force and one torque about
        centres[b] per body.  params = body_params(...).  A BodyForces (force, torque, volume, wet, sample_force,
        sample_fraction; the last two with samples=True) -- include/wsfluid.h ws_body_forces has the definition."""
        return body_forces(self._L, self._h, self._check, params, xyz, velocity, volume, body_start, centres, samples)

    # the particle count as a variable (include/wsfluid.h "pouring water in and draining it"): self.n follows the handle
    def reserve(self, capacity):
        """ws_reserve_particles: room for `capacity` particles, so that additions up to it allocate nothing."""
        self._check(self._L.ws_reserve_particles(self._h, int(capacity)))

    def capacity(self):
        return int(self._L.ws_particle_capacity(self._h))

    def _count_changed(self):
        self.n = int(self._L.ws_num_particles(self._h))

    def add_particles(self, positions, velocities=None, attributes=None):
        """m new particles with the ids n .. n+m-1; returns the new count."""
        add_particles(self._L, self._h, self._check, positions, velocities, attributes)
        self._count_changed()
        return self.n

    def remove_particles(self, sinks, counts=True, new_ids=True):
        """Drain the sinks; returns (per-sink counts, new id by old id), either None if not asked for."""
        out = remove_particles(self._L, self._h, self._check, self.n, sinks, counts, new_ids)
        self._count_changed()
        return out

    def remove_particle_ids(self, ids, new_ids=True):
        """Remove the particles named in ids; returns the new id by old id, or None."""
        out = remove_particle_ids(self._L, self._h, self._check, self.n, ids, new_ids)
        self._count_changed()
        return out

    # gauges (include/wsfluid.h "gauges"): read-only, synchronous
    def measure(self, regions, attributes=False):
        """Up to 16 gauges in one pass: a Gauges dict of numpy arrays (raw integers; .total() / .mean() divide)."""
        return measure(self._L, self._h, self._check, regions, attributes)

    def select_particles(self, regions, cap=None):
        """(ids ascending, total) of the particles inside the union of the regions; cap defaults to the particle count."""
        return select_particles(self._L, self._h, self._check, regions, self.n if cap is None else cap)

    def steps_done(self):
        return int(self._L.ws_steps_done(self._h))

    def grid_dims(self):
        d = np.zeros(3, np.uint32)
        self._check(self._L.ws_grid_dims(self._h, d.ctypes.data))
        return tuple(int(x) for x in d)

    def stats(self):
        out = np.zeros(16, np.uint32)
        self._check(self._L.ws_read_stats(self._h, out.ctypes.data))
        st = {"mask_overflow": int(out[0]), "cells_merged": tuple(int(x) for x in out[1:4]), "graph_steps": int(out[4]),
              "tile_schedule": bool(out[15])}
        if out[6]:  # a slab handle: peaks of the fixed-capacity messages against their capacities
            st.update(halo_peak=int(out[5]), halo_capacity=int(out[6]), migration_peak=int(out[7]), migration_capacity=int(out[8]), far_peak=int(out[9]), far_capacity=int(out[10]),
                      migration_now=int(out[11]), halo_now=int(out[12]), far_now=int(out[13]))
        return st

    def profile(self):
        """{kernel name: (total_ms, launches)} since the last profile_reset (needs profile=True)."""
        out = {}
        for name, k in KERNEL_IDS.items():
            ms = C.c_double(0)
            cnt = C.c_uint64(0)
            self._check(self._L.ws_profile_read(self._h, k, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, int(cnt.value))
        return out

    def profile_select(self, mask):
        self._check(self._L.ws_profile_select(self._h, mask & 0xFFFFFFFF))

    def profile_reset(self):
        self._check(self._L.ws_profile_reset(self._h))
