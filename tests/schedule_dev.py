"""ctypes bindings of the developer build's three schedule hooks (csrc/ws_api.cpp under WS_DEV_HOOKS: ws_dev_schedule,
ws_dev_plant_schedule, ws_dev_read_tile_costs).  They exist in tests/libwsfluid_dev.so only and are no part of the
product's interface, so they are bound here and not in the package."""
import ctypes as C

import numpy as np

DENSITY_TILE = 64  # particles per K4 tile (ND_P): K4's groups are group_particles / 64 tiles


def bind(devlib):
    vp, u32 = C.c_void_p, C.c_uint32
    devlib.ws_dev_schedule.argtypes = [vp, vp, u32, vp, u32, u32, u32, u32, vp, vp, vp, vp]
    devlib.ws_dev_plant_schedule.argtypes = [vp, vp, vp]
    devlib.ws_dev_read_tile_costs.argtypes = [vp, vp, vp, vp]
    return devlib


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def run_schedule(worker, cost4, cost5, nclasses, G):
    """k_schedule once on the two cost arrays (either may be empty), groups of G tiles in both halves of the launch.
    Returns (split4, perm4, split5, perm5); what the kernel did not write reads 0xFFFFFFFF."""
    cost4, cost5 = _u32(cost4), _u32(cost5)
    split4, split5 = np.zeros(9, np.uint32), np.zeros(9, np.uint32)
    perm4, perm5 = np.zeros(cost4.size, np.uint32), np.zeros(cost5.size, np.uint32)
    ptr = lambda a: a.ctypes.data if a.size else None
    worker._check(worker._L.ws_dev_schedule(worker._h, ptr(cost4), cost4.size, ptr(cost5), cost5.size, nclasses,
                                            G * DENSITY_TILE, DENSITY_TILE, split4.ctypes.data, ptr(perm4), split5.ctypes.data, ptr(perm5)))
    return split4, perm4, split5, perm5


def tile_counts(worker):
    nt = np.zeros(2, np.uint32)
    worker._check(worker._L.ws_dev_read_tile_costs(worker._h, None, None, nt.ctypes.data))
    return int(nt[0]), int(nt[1])


def plant(worker, cost4, cost5):
    """The next step's K4 / K5 run the schedule k_schedule makes of these costs; their own cost arrays start at zero."""
    cost4, cost5 = _u32(cost4), _u32(cost5)
    assert (cost4.size, cost5.size) == tile_counts(worker)
    worker._check(worker._L.ws_dev_plant_schedule(worker._h, cost4.ctypes.data, cost5.ctypes.data))


def read_tile_costs(worker):
    """(cost4, cost5): what K4 and K5 of the last step wrote, one word per tile."""
    t4, t5 = tile_counts(worker)
    cost4, cost5 = np.zeros(t4, np.uint32), np.zeros(t5, np.uint32)
    worker._check(worker._L.ws_dev_read_tile_costs(worker._h, cost4.ctypes.data, cost5.ctypes.data, None))
    return cost4, cost5
