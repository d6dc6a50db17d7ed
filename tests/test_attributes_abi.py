"""The seven attribute entry points in the C ABI: exported, bound, declared in plain C with the struct layouts the header
gives, the defaults, the ABI version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ws_default_diffuse_params": 1, "ws_write_attributes": 2, "ws_read_attributes": 2, "ws_paint_attributes": 4,
         "ws_diffuse_attributes": 4, "ws_sample_attribute_grid": 6, "ws_sample_attribute_points": 5}  # and their parameter counts
BRUSH = {"kind": 0, "centre": 4, "radius": 16, "falloff": 20, "strength": 24, "channels": 28, "value": 32}
DIFFUSE = {"rate": 0, "iterations": 16, "reserved": 20}
METHODS = ("write_attributes", "read_attributes", "paint_attributes", "diffuse_attributes", "sample_attribute_grid",
           "sample_attribute_points")


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
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls, method)
    assert (ws.fluid.WS_MAX_BRUSHES, ws.fluid.WS_BRUSH_MIX, ws.fluid.WS_BRUSH_ADD) == (16, 0, 1)
    for macro, value in (("WS_MAX_BRUSHES", 16), ("WS_BRUSH_MIX", 0), ("WS_BRUSH_ADD", 1)):
        assert re.search(r"#define %s %du\b" % (macro, value), _header()), macro


@pytest.mark.parametrize("cname,pyname,size,offsets", [("ws_brush", "WsBrush", 48, BRUSH),
                                                       ("ws_diffuse_params", "WsDiffuseParams", 24, DIFFUSE)])
def test_the_structs_have_the_headers_layout(ws, cname, pyname, size, offsets):
    S = getattr(ws.fluid, pyname)
    assert C.sizeof(S) == size
    text = _header(comments=True)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, flags=re.S).group(1)
    assert "/* %d bytes */" % size in body.splitlines()[0]
    # every member, in order, with the offset its comment states
    rows = re.findall(r"\b(float|uint32_t)\s+(\w+)(?:\[(\d)\])?;\s*/\* (?:offset )?(\d+)\b", body)
    assert [n for _, n, _, _ in rows] == list(offsets) == [n for n, _ in S._fields_]
    for ty, name, count, off in rows:
        assert int(off) == offsets[name] == getattr(S, name).offset, name
        base = C.c_float if ty == "float" else C.c_uint32
        field = dict(S._fields_)[name]
        assert (field._type_ is base and field._length_ == int(count)) if count else field is base, name


def test_the_defaults_and_the_helpers(ws):
    lib = ws.load_library()
    p = ws.fluid.WsDiffuseParams((C.c_float * 4)(9.0, 9.0, 9.0, 9.0), 9, 9)
    assert lib.ws_default_diffuse_params(C.byref(p)) == 0
    assert (list(p.rate), p.iterations, p.reserved) == ([1.0, 1.0, 1.0, 1.0], 1, 0)
    assert lib.ws_default_diffuse_params(None) == 1
    q = ws.fluid.diffuse_params(rate=(0.5, 0.0, 2.0, 1.0), iterations=8)
    assert (list(q.rate), q.iterations, q.reserved) == ([0.5, 0.0, 2.0, 1.0], 8, 0)
    with pytest.raises(AttributeError):
        ws.fluid.diffuse_params(diffusivity=1.0)
    b = ws.fluid.brush("add", (1.0, 2.0, 3.0), 0.5, (0.1, 0.2, 0.3, 0.4), strength=-2.0, falloff=0.25, channels=(0, 3))
    assert (b.kind, list(b.centre), b.radius, b.falloff, b.strength, b.channels) == (1, [1.0, 2.0, 3.0], 0.5, 0.25, -2.0, 9)
    assert list(b.value) == [float(np.float32(v)) for v in (0.1, 0.2, 0.3, 0.4)]
    d = ws.fluid.brush("mix", (0.0, 0.0, 0.0), 1.0, (1.0, 0.0, 0.0, 0.0))
    assert (d.kind, d.strength, d.falloff, d.channels) == (0, 1.0, 0.0, 15)


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "attributes.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_diffuse_params p = {{9.f, 9.f, 9.f, 9.f}, 9u, 9u};\n"
        "    ws_brush b = {WS_BRUSH_ADD, {0.f, 0.f, 0.f}, 1.f, 0.f, 1.f, 15u, {1.f, 1.f, 1.f, 1.f}};\n"
        "    uint32_t n = 7u, dims[3] = {2u, 2u, 2u};\n"
        "    float out[4] = {7.f, 7.f, 7.f, 7.f}, o[3] = {0.f, 0.f, 0.f}, s[3] = {1.f, 1.f, 1.f};\n"
        "    ws_status (*df)(ws_diffuse_params *) = ws_default_diffuse_params;\n"
        "    ws_status (*wr)(ws_handle *, const float *) = ws_write_attributes;\n"
        "    ws_status (*rd)(ws_handle *, float *) = ws_read_attributes;\n"
        "    ws_status (*pa)(ws_handle *, const ws_brush *, uint32_t, uint32_t *) = ws_paint_attributes;\n"
        "    ws_status (*di)(ws_handle *, const ws_diffuse_params *, float, uint32_t *) = ws_diffuse_attributes;\n"
        "    ws_status (*sg)(ws_handle *, const float[3], const float[3], const uint32_t[3], float *, float *) = ws_sample_attribute_grid;\n"
        "    ws_status (*sp)(ws_handle *, const float *, uint32_t, float *, float *) = ws_sample_attribute_points;\n"
        "    if (sizeof b != 48 || offsetof(ws_brush, centre) != 4 || offsetof(ws_brush, radius) != 16) return 1;\n"
        "    if (offsetof(ws_brush, falloff) != 20 || offsetof(ws_brush, strength) != 24 || offsetof(ws_brush, channels) != 28) return 2;\n"
        "    if (offsetof(ws_brush, value) != 32 || sizeof p != 24 || offsetof(ws_diffuse_params, iterations) != 16) return 3;\n"
        "    if (offsetof(ws_diffuse_params, reserved) != 20 || WS_ABI_VERSION != 2 || WS_MAX_BRUSHES != 16u || WS_BRUSH_MIX != 0u) return 4;\n"
        "    if (df(&p) != WS_OK || p.rate[0] != 1.f || p.rate[3] != 1.f || p.iterations != 1u || p.reserved != 0u) return 5;\n"
        "    if (wr(NULL, out) != WS_ERR_INVALID_ARG || rd(NULL, out) != WS_ERR_INVALID_ARG) return 6;\n"
        "    if (pa(NULL, &b, 1u, &n) != WS_ERR_INVALID_ARG || di(NULL, &p, 0.01f, &n) != WS_ERR_INVALID_ARG) return 7;\n"
        "    if (sg(NULL, o, s, dims, out, NULL) != WS_ERR_INVALID_ARG || sp(NULL, o, 1u, out, NULL) != WS_ERR_INVALID_ARG) return 8;\n"
        "    return n == 7u && out[0] == 7.f ? 0 : 9;\n"
        "}\n")
    exe = tmp_path / "attributes"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    p = ws.fluid.diffuse_params()
    b = ws.fluid.brush("mix", (0.0, 0.0, 0.0), 1.0, (1.0, 1.0, 1.0, 1.0))
    n = np.full(16, 7, np.uint32)
    out = np.full(32, 7.0, np.float32)
    xyz = np.zeros(3, np.float32)
    dims = np.array([2, 2, 2], np.uint32)
    assert lib.ws_write_attributes(None, out.ctypes.data) == 1 and lib.ws_write_attributes(None, None) == 1
    assert lib.ws_read_attributes(None, out.ctypes.data) == 1
    assert lib.ws_paint_attributes(None, C.byref(b), 1, n.ctypes.data) == 1 and lib.ws_paint_attributes(None, None, 0, None) == 1
    assert lib.ws_diffuse_attributes(None, C.byref(p), 0.01, n.ctypes.data) == 1
    assert lib.ws_diffuse_attributes(None, None, 0.0, None) == 1
    assert lib.ws_sample_attribute_grid(None, xyz.ctypes.data, xyz.ctypes.data, dims.ctypes.data, out.ctypes.data, out.ctypes.data) == 1
    assert lib.ws_sample_attribute_points(None, xyz.ctypes.data, 1, out.ctypes.data, out.ctypes.data) == 1
    assert np.all(n == 7) and np.all(out == 7.0) and list(p.rate) == [1.0] * 4 and b.strength == 1.0
