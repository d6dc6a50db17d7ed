"""ws_extract_surface's C ABI: exported, bound, declared in plain C, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text)))


def test_the_product_library_exports_the_surface_symbol(ws):
    assert hasattr(ws.load_library(), "ws_extract_surface")


def test_abi_symbols_track_the_header_including_the_surface(ws):
    assert "ws_extract_surface" in _declared()
    assert "ws_extract_surface" in ws.fluid.ABI_SYMBOLS
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert ws.load_library().ws_abi_version() == 2  # additive change: the version stays


def test_the_surface_prototype_compiles_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "surface.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    const float o[3] = {0.f, 0.f, 0.f}, s[3] = {0.1f, 0.1f, 0.1f};\n"
        "    const uint32_t d[3] = {2u, 2u, 2u};\n"
        "    float xyz[3], nrm[3];\n"
        "    uint32_t tri[3], nv = 0, nt = 0;\n"
        "    ws_status (*f)(ws_handle *, const float[3], const float[3], const uint32_t[3], float, uint32_t, uint32_t,\n"
        "                   float *, float *, uint32_t *, uint32_t *, uint32_t *) = ws_extract_surface;\n"
        "    if (f(NULL, o, s, d, 1.f, 1u, 1u, xyz, nrm, tri, &nv, &nt) != WS_ERR_INVALID_ARG) return 1;\n"
        "    if (f(NULL, NULL, NULL, NULL, 1.f, 0u, 0u, NULL, NULL, NULL, NULL, NULL) != WS_ERR_INVALID_ARG) return 2;\n"
        "    return nv == 0u && nt == 0u ? 0 : 3;\n"
        "}\n")
    exe = tmp_path / "surface"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_without_a_device(ws):
    lib = ws.load_library()
    o = np.zeros(3, np.float32)
    s = np.full(3, 0.1, np.float32)
    d = np.full(3, 4, np.uint32)
    xyz = np.empty((8, 3), np.float32)
    tri = np.empty((8, 3), np.uint32)
    nv, nt = C.c_uint32(7), C.c_uint32(7)
    assert lib.ws_extract_surface(None, o.ctypes.data, s.ctypes.data, d.ctypes.data, C.c_float(1.0), 8, 8, xyz.ctypes.data,
                                  None, tri.ctypes.data, C.byref(nv), C.byref(nt)) == 1
    assert lib.ws_extract_surface(None, None, None, None, C.c_float(1.0), 0, 0, None, None, None, None, None) == 1
    assert nv.value == 7 and nt.value == 7  # nothing written
