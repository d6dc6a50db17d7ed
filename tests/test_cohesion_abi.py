"""ws_default_cohesion_params, ws_read_cohesion and ws_apply_cohesion in the C ABI: exported, bound, declared in plain C
with the struct layout the header gives, the defaults, the ABI version unchanged, and the NULL handle refused without a
device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ws_default_cohesion_params": 1, "ws_read_cohesion": 7, "ws_apply_cohesion": 4}  # and their parameter counts
FIELDS = ["cohesion", "curvature", "xsph", "rest_density", "reserved"]
OFFSETS = {"cohesion": 0, "curvature": 4, "xsph": 8, "rest_density": 12, "reserved": 16}


def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def test_the_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name, k in NAMES.items():
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == k, name
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        for method in ("read_cohesion", "apply_cohesion"):
            assert callable(getattr(cls, method)), (cls, method)


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsCohesionParams
    assert C.sizeof(S) == 20
    text = _header(comments=True)
    body = re.search(r"typedef struct ws_cohesion_params \{(.*?)\} ws_cohesion_params;", text, flags=re.S).group(1)
    assert "/* 20 bytes */" in body.splitlines()[0]
    # every member, in order, with the offset its comment states
    rows = re.findall(r"\b(float|uint32_t)\s+(\w+);\s*/\* offset (\d+):", body)
    assert [n for _, n, _ in rows] == FIELDS == [n for n, _ in S._fields_]
    for ty, name, off in rows:
        assert int(off) == OFFSETS[name] == getattr(S, name).offset, name
        assert dict(S._fields_)[name] is (C.c_float if ty == "float" else C.c_uint32), name


def test_the_defaults(ws):
    lib = ws.load_library()
    p = ws.fluid.WsCohesionParams(9.0, 9.0, 9.0, 9.0, 9)
    assert lib.ws_default_cohesion_params(C.byref(p)) == 0
    assert (p.cohesion, p.curvature, p.xsph, p.rest_density, p.reserved) == (1.0, 1.0, np.float32(0.1), 0.0, 0)
    assert lib.ws_default_cohesion_params(None) == 1
    q = ws.fluid.cohesion_params(xsph=0.5, rest_density=12.0)
    assert (q.cohesion, q.curvature, q.xsph, q.rest_density, q.reserved) == (1.0, 1.0, 0.5, 12.0, 0)
    with pytest.raises(AttributeError):
        ws.fluid.cohesion_params(adhesion=1.0)


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "cohesion.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_cohesion_params p = {9.f, 9.f, 9.f, 9.f, 9u};\n"
        "    uint32_t n = 7u;\n"
        "    float out[3] = {7.f, 7.f, 7.f};\n"
        "    ws_status (*df)(ws_cohesion_params *) = ws_default_cohesion_params;\n"
        "    ws_status (*rd)(ws_handle *, const ws_cohesion_params *, float, float *, float *, float *, uint32_t *) = ws_read_cohesion;\n"
        "    ws_status (*ap)(ws_handle *, const ws_cohesion_params *, float, uint32_t *) = ws_apply_cohesion;\n"
        "    if (sizeof p != 20 || offsetof(ws_cohesion_params, curvature) != 4 || offsetof(ws_cohesion_params, xsph) != 8) return 1;\n"
        "    if (offsetof(ws_cohesion_params, rest_density) != 12 || offsetof(ws_cohesion_params, reserved) != 16) return 2;\n"
        "    if (WS_ABI_VERSION != 2) return 3;\n"
        "    if (df(&p) != WS_OK || p.cohesion != 1.f || p.curvature != 1.f || p.xsph != 0.1f || p.rest_density != 0.f || p.reserved != 0u) return 4;\n"
        "    if (rd(NULL, &p, 0.01f, out, NULL, NULL, &n) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (ap(NULL, &p, 0.01f, &n) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return n == 7u && out[0] == 7.f ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "cohesion"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    p = ws.fluid.cohesion_params()
    n = np.full(4, 7, np.uint32)
    out = np.full(12, 7.0, np.float32)
    assert lib.ws_apply_cohesion(None, C.byref(p), 0.01, n.ctypes.data) == 1
    assert lib.ws_apply_cohesion(None, None, 0.0, None) == 1
    assert lib.ws_read_cohesion(None, C.byref(p), 0.01, out.ctypes.data, out.ctypes.data, out.ctypes.data, n.ctypes.data) == 1
    assert lib.ws_read_cohesion(None, None, 0.0, None, None, None, None) == 1
    assert np.all(n == 7) and np.all(out == 7.0) and p.cohesion == 1.0
