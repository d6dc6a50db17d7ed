"""ws_cast_rays / ws_cast_camera in the C ABI: exported, bound, declared in plain C with the struct sizes the header
gives, the ABI version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ws_cast_rays", "ws_cast_camera")


def _declared():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text)))


def test_the_two_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays


def test_the_struct_sizes_are_20_and_48(ws):
    assert C.sizeof(ws.fluid.WsRayParams) == 20
    assert C.sizeof(ws.fluid.WsCamera) == 48
    assert [n for n, _ in ws.fluid.WsRayParams._fields_] == ["t_start", "dt", "steps", "refine", "iso"]
    assert [n for n, _ in ws.fluid.WsCamera._fields_] == ["eye", "forward", "right", "up"]


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "rays.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    const ws_ray_params r = {0.f, 0.125f, 160u, 6u, 5.f};\n"
        "    const ws_camera cam = {{0.f, 9.f, 9.f}, {0.f, -1.f, -1.f}, {1.f, 0.f, 0.f}, {0.f, 1.f, -1.f}};\n"
        "    const float o[3] = {0.f, 9.f, 0.f}, v[3] = {0.f, -1.f, 0.f};\n"
        "    const uint32_t size[2] = {4u, 4u};\n"
        "    float t[16], n[48];\n"
        "    ws_status (*rays)(ws_handle *, const ws_aniso_params *, const ws_ray_params *, const float *, const float *,\n"
        "                      uint32_t, float *, float *) = ws_cast_rays;\n"
        "    ws_status (*camera)(ws_handle *, const ws_aniso_params *, const ws_ray_params *, const ws_camera *,\n"
        "                        const uint32_t[2], float *, float *) = ws_cast_camera;\n"
        "    if (sizeof(ws_ray_params) != 20 || sizeof(ws_camera) != 48) return 1;\n"
        "    if (offsetof(ws_ray_params, iso) != 16 || offsetof(ws_camera, up) != 36) return 2;\n"
        "    t[0] = 7.f; n[0] = 7.f;\n"
        "    if (rays(NULL, NULL, &r, o, v, 1u, t, n) != WS_ERR_INVALID_ARG) return 3;\n"
        "    if (camera(NULL, NULL, &r, &cam, size, t, n) != WS_ERR_INVALID_ARG) return 4;\n"
        "    if (rays(NULL, NULL, NULL, NULL, NULL, 0u, NULL, NULL) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (camera(NULL, NULL, NULL, NULL, NULL, NULL, NULL) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return t[0] == 7.f && n[0] == 7.f ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "rays"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    march = ws.fluid.ray_params(0.0, 0.125, 160, 6, 5.0)
    cam = ws.fluid.camera((0, 9, 9), (0, -1, -1), (1, 0, 0), (0, 1, -1))
    o = np.zeros((4, 3), np.float32)
    v = np.ones((4, 3), np.float32)
    size = np.array([2, 2], np.uint32)
    t = np.full(4, 7.0, np.float32)
    n = np.full((4, 3), 7.0, np.float32)
    assert lib.ws_cast_rays(None, None, C.byref(march), o.ctypes.data, v.ctypes.data, 4, t.ctypes.data, n.ctypes.data) == 1
    assert lib.ws_cast_camera(None, None, C.byref(march), C.byref(cam), size.ctypes.data, t.ctypes.data, n.ctypes.data) == 1
    assert lib.ws_cast_rays(None, None, None, None, None, 0, None, None) == 1
    assert lib.ws_cast_camera(None, None, None, None, None, None, None) == 1
    assert np.all(t == 7.0) and np.all(n == 7.0)
