"""ws_read_velocities / ws_sample_velocity_grid / _points / ws_advect_points in the C ABI: exported, bound, declared in
plain C with the struct size the header gives, the ABI version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ws_read_velocities", "ws_sample_velocity_grid", "ws_sample_velocity_points", "ws_advect_points")


def _declared():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text)))


def test_the_four_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        for method in ("read_velocities", "sample_velocity_grid", "sample_velocity_points", "advect_points"):
            assert callable(getattr(cls, method)), (cls, method)


def test_the_struct_size_is_8(ws):
    assert C.sizeof(ws.fluid.WsAdvectParams) == 8
    assert [n for n, _ in ws.fluid.WsAdvectParams._fields_] == ["dt", "substeps"]
    a = ws.fluid.advect_params(-0.25, 8)
    assert a.dt == -0.25 and a.substeps == 8 and ws.fluid.advect_params(1.0).substeps == 1


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "velocity.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    const ws_advect_params a = {0.0625f, 8u};\n"
        "    const float o[3] = {0.f, 0.f, 0.f}, s[3] = {1.f, 1.f, 1.f}, p[3] = {0.f, 1.f, 0.f};\n"
        "    const uint32_t dims[3] = {1u, 1u, 1u};\n"
        "    float u[3], rho[1], q[3];\n"
        "    ws_status (*read)(ws_handle *, float *) = ws_read_velocities;\n"
        "    ws_status (*grid)(ws_handle *, const float[3], const float[3], const uint32_t[3], float *, float *) =\n"
        "        ws_sample_velocity_grid;\n"
        "    ws_status (*points)(ws_handle *, const float *, uint32_t, float *, float *) = ws_sample_velocity_points;\n"
        "    ws_status (*advect)(ws_handle *, const ws_advect_params *, const float *, uint32_t, float *, float *, float *) =\n"
        "        ws_advect_points;\n"
        "    if (sizeof(ws_advect_params) != 8 || offsetof(ws_advect_params, substeps) != 4) return 1;\n"
        "    u[0] = 7.f; rho[0] = 7.f; q[0] = 7.f;\n"
        "    if (read(NULL, u) != WS_ERR_INVALID_ARG) return 2;\n"
        "    if (grid(NULL, o, s, dims, u, rho) != WS_ERR_INVALID_ARG) return 3;\n"
        "    if (points(NULL, p, 1u, u, rho) != WS_ERR_INVALID_ARG) return 4;\n"
        "    if (advect(NULL, &a, p, 1u, q, u, rho) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (advect(NULL, NULL, NULL, 0u, NULL, NULL, NULL) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return u[0] == 7.f && rho[0] == 7.f && q[0] == 7.f ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "velocity"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    a = ws.fluid.advect_params(0.0625, 2)
    p = np.zeros((4, 3), np.float32)
    o = np.zeros(3, np.float32)
    s = np.ones(3, np.float32)
    dims = np.array([2, 2, 1], np.uint32)
    u = np.full((4, 3), 7.0, np.float32)
    rho = np.full(4, 7.0, np.float32)
    out = np.full((4, 3), 7.0, np.float32)
    assert lib.ws_read_velocities(None, u.ctypes.data) == 1
    assert lib.ws_sample_velocity_grid(None, o.ctypes.data, s.ctypes.data, dims.ctypes.data, u.ctypes.data, rho.ctypes.data) == 1
    assert lib.ws_sample_velocity_points(None, p.ctypes.data, 4, u.ctypes.data, rho.ctypes.data) == 1
    assert lib.ws_advect_points(None, C.byref(a), p.ctypes.data, 4, out.ctypes.data, u.ctypes.data, rho.ctypes.data) == 1
    assert lib.ws_advect_points(None, None, None, 0, None, None, None) == 1
    assert np.all(u == 7.0) and np.all(rho == 7.0) and np.all(out == 7.0)
