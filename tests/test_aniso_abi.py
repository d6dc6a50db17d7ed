"""The anisotropic kernels' C ABI: the five symbols exported, bound and declared in plain C, the defaults, and the NULL
handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ws_default_aniso_params", "ws_read_anisotropy", "ws_sample_aniso_grid", "ws_sample_aniso_points",
         "ws_extract_aniso_surface"]


def _declared():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text)))


def test_the_five_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
    assert lib.ws_abi_version() == 2  # additive change: the version stays


def test_the_defaults(ws):
    p = ws.fluid.WsAnisoParams()
    assert ws.load_library().ws_default_aniso_params(C.byref(p)) == 0
    assert (p.smoothing, p.max_ratio, p.lone_scale, p.min_neighbours) == (np.float32(0.9), 4.0, 0.5, 12)
    assert ws.load_library().ws_default_aniso_params(None) == 1
    q = ws.fluid.aniso_params(min_neighbours=3)
    assert q.min_neighbours == 3 and q.max_ratio == 4.0
    assert C.sizeof(ws.fluid.WsAnisoParams) == 16


def test_the_prototypes_compile_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "aniso.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_aniso_params a;\n"
        "    const float o[3] = {0.f, 0.f, 0.f}, s[3] = {0.1f, 0.1f, 0.1f};\n"
        "    const uint32_t d[3] = {2u, 2u, 2u};\n"
        "    float c[3], m[6], f[1], rho[8], g[24], xyz[3], nrm[3];\n"
        "    uint32_t n[1], tri[3], nv = 0, nt = 0;\n"
        "    if (ws_default_aniso_params(&a) != WS_OK || a.min_neighbours != 12u) return 1;\n"
        "    if (ws_read_anisotropy(NULL, &a, c, m, f, n) != WS_ERR_INVALID_ARG) return 2;\n"
        "    if (ws_sample_aniso_grid(NULL, &a, o, s, d, rho, g) != WS_ERR_INVALID_ARG) return 3;\n"
        "    if (ws_sample_aniso_points(NULL, &a, o, 1u, rho, g) != WS_ERR_INVALID_ARG) return 4;\n"
        "    ws_status (*e)(ws_handle *, const ws_aniso_params *, const float[3], const float[3], const uint32_t[3], float,\n"
        "                   uint32_t, uint32_t, float *, float *, uint32_t *, uint32_t *, uint32_t *) = ws_extract_aniso_surface;\n"
        "    if (e(NULL, &a, o, s, d, 1.f, 1u, 1u, xyz, nrm, tri, &nv, &nt) != WS_ERR_INVALID_ARG) return 5;\n"
        "    return nv == 0u && nt == 0u ? 0 : 6;\n"
        "}\n")
    exe = tmp_path / "aniso"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_without_a_device(ws):
    lib = ws.load_library()
    a = ws.fluid.aniso_params()
    o = np.zeros(3, np.float32)
    s = np.full(3, 0.1, np.float32)
    d = np.full(3, 4, np.uint32)
    out = np.empty(64 * 3, np.float32)
    nv, nt = C.c_uint32(7), C.c_uint32(7)
    assert lib.ws_read_anisotropy(None, C.byref(a), out.ctypes.data, None, None, None) == 1
    assert lib.ws_sample_aniso_grid(None, C.byref(a), o.ctypes.data, s.ctypes.data, d.ctypes.data, out.ctypes.data, None) == 1
    assert lib.ws_sample_aniso_points(None, C.byref(a), o.ctypes.data, 1, out.ctypes.data, None) == 1
    assert lib.ws_extract_aniso_surface(None, C.byref(a), o.ctypes.data, s.ctypes.data, d.ctypes.data, C.c_float(1.0), 8, 8,
                                        out.ctypes.data, None, out.ctypes.data, C.byref(nv), C.byref(nt)) == 1
    assert lib.ws_extract_aniso_surface(None, None, None, None, None, C.c_float(1.0), 0, 0, None, None, None, None, None) == 1
    assert nv.value == 7 and nt.value == 7  # nothing written
