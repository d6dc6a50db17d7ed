"""ws_default_body_params and ws_body_forces in the C ABI: exported, bound, declared in plain C with the struct layout the
header gives, the ABI version unchanged, the defaults without a device and the NULL handle refused."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bodies_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ws_default_body_params", "ws_body_forces")
FIELDS = ["fluid_density", "drag", "rest_density", "reserved"]
OFFSETS = {"fluid_density": 0, "drag": 4, "rest_density": 8, "reserved": 12}


def _header():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def test_the_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
    assert len(lib.ws_default_body_params.argtypes) == 1 and len(lib.ws_body_forces.argtypes) == 15
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        assert callable(getattr(cls, "body_forces")), cls
    assert ws.fluid.BodyForces._fields == ("force", "torque", "volume", "wet", "sample_force", "sample_fraction")
    hpp = open(os.path.join(ROOT, "water-sandbox_amd", "host", "fluid_compute.hpp")).read()
    assert "ws_body_forces(" in hpp


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsBodyParams
    assert C.sizeof(S) == 16
    body = re.search(r"typedef struct ws_body_params \{(.*?)\} ws_body_params;", _header(), flags=re.S).group(1)
    assert [n for n, _ in S._fields_] == FIELDS == re.findall(r"\b(\w+);", body)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off, name


def test_the_defaults_need_no_device(ws):
    lib = ws.load_library()
    p = ws.fluid.WsBodyParams(-1.0, -1.0, -1.0, 7)
    assert lib.ws_default_body_params(C.byref(p)) == 0
    d = B.defaults()
    assert (p.fluid_density, p.drag, p.rest_density, p.reserved) == (1000.0, 500.0, 0.0, 0)
    assert (p.fluid_density, p.drag, p.rest_density) == (float(d["fluid_density"]), float(d["drag"]), float(d["rest_density"]))
    assert lib.ws_default_body_params(None) == 1
    q = ws.fluid.body_params(drag=0.0, rest_density=5.0)
    assert (q.fluid_density, q.drag, q.rest_density, q.reserved) == (1000.0, 0.0, 5.0, 0)
    with pytest.raises(AttributeError):
        ws.fluid.body_params(buoyancy=1.0)


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "bodies.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_body_params p = {0.f, 0.f, 0.f, 9u};\n"
        "    ws_status (*dp)(ws_body_params *) = ws_default_body_params;\n"
        "    ws_status (*bf)(ws_handle *, const ws_body_params *, const float *, const float *, const float *, uint32_t,\n"
        "                    const uint32_t *, const float *, uint32_t, float *, float *, float *, uint32_t *, float *,\n"
        "                    float *) = ws_body_forces;\n"
        "    float xyz[3] = {0.f, 0.f, 0.f}, vol[1] = {1.f}, out[3] = {7.f, 7.f, 7.f};\n"
        "    uint32_t start[2] = {0u, 1u}, wet[1] = {7u};\n"
        "    if (sizeof p != 16 || offsetof(ws_body_params, fluid_density) != 0 || offsetof(ws_body_params, drag) != 4) return 1;\n"
        "    if (offsetof(ws_body_params, rest_density) != 8 || offsetof(ws_body_params, reserved) != 12) return 2;\n"
        "    if (WS_ABI_VERSION != 2) return 3;\n"
        "    if (dp(&p) != WS_OK || p.fluid_density != 1000.f || p.drag != 500.f || p.rest_density != 0.f || p.reserved != 0u) return 4;\n"
        "    if (dp(NULL) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (bf(NULL, &p, xyz, xyz, vol, 1u, start, xyz, 1u, out, out, vol, wet, NULL, NULL) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return out[0] == 7.f && wet[0] == 7u && vol[0] == 1.f ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "bodies"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    p = ws.fluid.body_params()
    f = np.zeros((4, 3), np.float32)
    v = np.ones(4, np.float32)
    start = np.array([0, 4], np.uint32)
    out = np.full((4, 3), 7, np.float32)
    wet = np.full(1, 7, np.uint32)
    assert lib.ws_body_forces(None, C.byref(p), f.ctypes.data, f.ctypes.data, v.ctypes.data, 4, start.ctypes.data, f.ctypes.data, 1,
                              out.ctypes.data, out.ctypes.data, v.ctypes.data, wet.ctypes.data, out.ctypes.data, v.ctypes.data) == 1
    assert lib.ws_body_forces(None, None, None, None, None, 0, None, None, 0, None, None, None, None, None, None) == 1
    assert np.all(out == 7) and np.all(wet == 7) and np.all(v == 1)
