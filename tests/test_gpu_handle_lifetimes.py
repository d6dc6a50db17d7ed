"""Every device and page-locked allocation of a handle has one owner per lifetime (csrc/ws_internal.h WsScratch / WsGroup,
DESIGN.md 2).  One handle is taken through every lifetime -- the lazily allocated buffers, a re-grid that rebuilds the cell
tables and one that keeps them, a dead handle -- and a second handle, created where the first one's memory was, must
compute the same bits; create / step / re-grid / destroy cycles must give the device its memory back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _smaller(ws, size):
    return ws.make_params(container_size=size, smoothing_radius=np.float32(0.15))


def _one_life(ws, lib):
    """Everything a handle can allocate, in one life; returns what it computed."""
    pos, params = ws.workloads.make_workload("c1", "cloud")
    smaller = _smaller(ws, ws.workloads.CONFIGS["c1"][1])
    w = ws.FluidWorker(pos, params, library=lib)
    out = {}
    w.run(2)
    out["keys"], out["perm"], out["offsets"] = w.sort_view()  # the eight sort-view arrays
    for k in range(2):  # both page-locked buffers the library owns, and the readback's device stage
        w.read_positions_begin_owned()
        w.read_positions_end()
        out["view%d" % k] = w.read_positions_view().copy()
        w.run(1)
    centre = [float(x) for x in pos.mean(axis=0)]
    out["affected"] = np.asarray(w.apply_forces([ws.fluid.force(0, centre, 1.5, 4.0)], 1.0 / 60.0, counts=True))  # the counters
    out["rho"] = np.asarray(w.sample_density_points(pos[:257]))  # the field layer's scratch
    w.set_params(smaller)  # more cells: every cell table is rebuilt
    w.run(2)
    w.set_params(params)   # fewer cells: count / cursor are kept, the starts and the scan state rebuilt
    w.run(2)
    out["particles"] = w.read_vec("particles")  # the staging buffer
    w.close()
    return out


def test_a_second_handle_after_the_first_computes_the_same_bits(ws, devlib):
    a = _one_life(ws, devlib)
    b = _one_life(ws, devlib)
    assert a["affected"].sum() > 0 and np.all(np.isfinite(a["rho"])) and a["rho"].max() > 0
    for name in a:
        if name == "particles":
            assert a[name].tobytes() == b[name].tobytes(), name  # the 80-byte records, bit for bit
        else:
            assert np.array_equal(np.asarray(a[name]).view(np.uint32), np.asarray(b[name]).view(np.uint32)), name


def test_a_dead_handle_is_closed_without_error(ws, devlib, monkeypatch):
    pos, params = ws.workloads.make_workload("c1", "cloud")
    w = ws.FluidWorker(pos, params, library=devlib)
    w.run(2)
    monkeypatch.setenv("WS_FAIL_REGRID", "1")
    with pytest.raises(ws.WsError) as e:
        w.set_params(_smaller(ws, ws.workloads.CONFIGS["c1"][1]))
    monkeypatch.delenv("WS_FAIL_REGRID")
    assert "WS_FAIL_REGRID" in str(e.value) and "unusable" in str(e.value)
    with pytest.raises(ws.WsError):
        w.run(1)
    handle, w._h = w._h, C.c_void_p()
    assert devlib.ws_destroy(handle) == 0  # ws_destroy frees what is left
    again = ws.FluidWorker(pos, params, library=devlib)  # ... and the device is as usable as before
    again.run(1)
    again.sync()
    again.close()


def _free_device_bytes():
    try:
        hip = C.CDLL("libamdhip64.so")
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    except OSError:
        import torch

        return torch.cuda.mem_get_info(0)[0]


def _leak_over_eight_cycles(cycle):
    """Free device memory after the first (warm-up) cycle minus free device memory after the ninth."""
    cycle()
    after_first = _free_device_bytes()
    for _ in range(8):
        cycle()
    lost = after_first - _free_device_bytes()
    print("free device memory after cycle 1: %d B; lost over cycles 2..9: %d B" % (after_first, lost))
    return lost


def test_single_handle_cycles_give_the_memory_back(ws):
    """Less than one leaked copy per cycle of the smallest per-particle array (4 B per particle)."""
    pos, params = ws.workloads.make_workload("c2", "cloud")
    smaller = _smaller(ws, ws.workloads.CONFIGS["c2"][1])

    def cycle():
        w = ws.FluidWorker(pos, params)
        w.run(2)
        w.set_params(smaller)
        w.run(1)
        w.sync()
        w.close()

    assert _leak_over_eight_cycles(cycle) < 8 * 4 * pos.shape[0]


def test_slab_cycles_give_the_memory_back(ws):
    """Two loopback slabs with the default capacity: steps, a collective read, a re-grid, a re-cut, destroy.  The bound is
    one 4-byte array of the smaller slab's capacity per cycle."""
    params = ws.make_params(container_size=(16.0, 9.0, 9.0))
    smaller = _smaller(ws, (16.0, 9.0, 9.0))
    pos = ws.workloads.uniform_cloud(32768, 5, list(params.ext_min), list(params.ext_max))
    owned = np.bincount(ws.slab.assign(params, pos, 2), minlength=2)
    cap = 2 * int(owned.min()) + (1 << 20)  # ws_slab_create's default capacity

    def program(s, rank):
        s.run(2)
        s.read_positions()
        s.set_params(smaller)
        s.run(1)
        s.rebalance()
        s.run(1)
        s.sync()
        return True

    def cycle():
        assert ws.slab.run_loopback_program(pos, params, 2, program) == [True, True]

    assert _leak_over_eight_cycles(cycle) < 8 * 4 * cap
