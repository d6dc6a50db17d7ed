"""The density field sampler's C ABI (ws_sample_density_grid / ws_sample_density_points): exported, bound, declared in
plain C, and argument checks that need no device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ws_sample_density_grid", "ws_sample_density_points")


def _declared():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text)))


def test_product_library_exports_both_sampler_symbols(ws):
    lib = ws.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_abi_symbols_track_the_header_including_the_sampler(ws):
    names = _declared()
    for name in NAMES:
        assert name in names
        assert name in ws.fluid.ABI_SYMBOLS
    assert sorted(ws.fluid.ABI_SYMBOLS) == names
    assert ws.load_library().ws_abi_version() == 2  # additive change: the version stays


def test_sampler_prototypes_compile_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "field.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    const float o[3] = {0.f, 0.f, 0.f}, s[3] = {0.1f, 0.1f, 0.1f};\n"
        "    const uint32_t d[3] = {2u, 2u, 2u};\n"
        "    float rho[8];\n"
        "    ws_status (*g)(ws_handle *, const float[3], const float[3], const uint32_t[3], float *, float *) = ws_sample_density_grid;\n"
        "    ws_status (*p)(ws_handle *, const float *, uint32_t, float *, float *) = ws_sample_density_points;\n"
        "    if (g(NULL, o, s, d, rho, NULL) != WS_ERR_INVALID_ARG) return 1;\n"
        "    if (p(NULL, o, 1u, rho, NULL) != WS_ERR_INVALID_ARG) return 2;\n"
        "    return 0;\n"
        "}\n")
    exe = tmp_path / "field"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_null_handle_is_an_invalid_argument_without_a_device(ws):
    lib = ws.load_library()
    o = np.zeros(3, np.float32)
    s = np.full(3, 0.1, np.float32)
    d = np.full(3, 4, np.uint32)
    rho = np.empty(64, np.float32)
    grad = np.empty((64, 3), np.float32)
    assert lib.ws_sample_density_grid(None, o.ctypes.data, s.ctypes.data, d.ctypes.data, rho.ctypes.data, None) == 1
    assert lib.ws_sample_density_grid(None, o.ctypes.data, s.ctypes.data, d.ctypes.data, None, grad.ctypes.data) == 1
    assert lib.ws_sample_density_grid(None, None, None, None, None, None) == 1
    pts = np.zeros((4, 3), np.float32)
    assert lib.ws_sample_density_points(None, pts.ctypes.data, 4, rho.ctypes.data, grad.ctypes.data) == 1
    assert lib.ws_sample_density_points(None, None, 0, None, None) == 1
