"""ws_default_whitewater_emit_params / _step_params, ws_read_whitewater, ws_emit_whitewater and ws_step_whitewater in the C
ABI: exported, bound, declared in plain C with the struct layouts the header gives, the ABI version unchanged, the
defaults without a device and the NULL handle refused without one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import whitewater_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ws_default_whitewater_emit_params", "ws_default_whitewater_step_params", "ws_read_whitewater",
           "ws_emit_whitewater", "ws_step_whitewater")
EMIT_FIELDS = ["tau_trapped", "tau_crest", "tau_energy", "k_trapped", "k_crest", "crest_align", "dt", "radius", "lifetime",
               "max_per_particle", "seed"]
STEP_FIELDS = ["dt", "spray_max", "bubble_min", "buoyancy", "drag"]


def _header():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    return re.findall(r"\b(\w+)(?:\[\d+\])?;", body)


def test_the_five_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        for method in ("read_whitewater", "emit_whitewater", "step_whitewater"):
            assert callable(getattr(cls, method)), (cls, method)


def test_the_structs_have_the_headers_layout(ws):
    E, S = ws.fluid.WsWhitewaterEmitParams, ws.fluid.WsWhitewaterStepParams
    assert C.sizeof(E) == 60 and C.sizeof(S) == 20
    assert [n for n, _ in E._fields_] == EMIT_FIELDS == _struct_fields("ws_whitewater_emit_params")
    assert [n for n, _ in S._fields_] == STEP_FIELDS == _struct_fields("ws_whitewater_step_params")
    assert E.tau_crest.offset == 8 and E.k_trapped.offset == 24 and E.lifetime.offset == 44 and E.seed.offset == 56
    assert S.spray_max.offset == 4 and S.drag.offset == 16


def test_the_defaults_need_no_device_and_match_the_restatement(ws):
    lib = ws.load_library()
    assert lib.ws_default_whitewater_emit_params(None) == 1 and lib.ws_default_whitewater_step_params(None) == 1
    e, s = ws.fluid.whitewater_emit_params(), ws.fluid.whitewater_step_params()
    for k, want in W.emit_defaults().items():
        got = getattr(e, k)
        got = tuple(got) if isinstance(got, C.Array) else got
        assert np.all(np.float32(got) == np.float32(want)), k
    for k, want in W.step_defaults().items():
        assert np.float32(getattr(s, k)) == np.float32(want), k
    assert e.crest_align == np.float32(0.6) and s.spray_max == 6 and s.bubble_min == 20
    e = ws.fluid.whitewater_emit_params(tau_crest=(1.0, 2.0), seed=7)
    assert tuple(e.tau_crest) == (1.0, 2.0) and e.seed == 7 and e.max_per_particle == 8
    with pytest.raises(AttributeError):
        ws.fluid.whitewater_step_params(no_such_field=1)


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "whitewater.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_whitewater_emit_params e;\n"
        "    ws_whitewater_step_params s;\n"
        "    float f[3] = {7.f, 7.f, 7.f}, l[1] = {7.f};\n"
        "    uint32_t u[1] = {7u}, k = 7u;\n"
        "    uint8_t c[1] = {7u};\n"
        "    ws_status (*de)(ws_whitewater_emit_params *) = ws_default_whitewater_emit_params;\n"
        "    ws_status (*ds)(ws_whitewater_step_params *) = ws_default_whitewater_step_params;\n"
        "    ws_status (*rd)(ws_handle *, float *, float *, float *, float *, float *, uint32_t *) = ws_read_whitewater;\n"
        "    ws_status (*em)(ws_handle *, const ws_whitewater_emit_params *, uint32_t, float *, float *, float *, uint32_t *,\n"
        "                    uint32_t *) = ws_emit_whitewater;\n"
        "    ws_status (*st)(ws_handle *, const ws_whitewater_step_params *, const float *, const float *, const float *,\n"
        "                    uint32_t, float *, float *, float *, uint8_t *) = ws_step_whitewater;\n"
        "    if (sizeof e != 60 || offsetof(ws_whitewater_emit_params, lifetime) != 44) return 1;\n"
        "    if (sizeof s != 20 || offsetof(ws_whitewater_step_params, drag) != 16) return 2;\n"
        "    if (de(&e) != WS_OK || ds(&s) != WS_OK || de(NULL) != WS_ERR_INVALID_ARG || ds(NULL) != WS_ERR_INVALID_ARG) return 3;\n"
        "    if (e.max_per_particle != 8u || e.crest_align != 0.6f || s.spray_max != 6u || s.bubble_min != 20u) return 4;\n"
        "    if (rd(NULL, l, l, l, l, f, u) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (em(NULL, &e, 1u, f, f, l, u, &k) != WS_ERR_INVALID_ARG) return 6;\n"
        "    if (st(NULL, &s, f, f, l, 1u, f, f, l, c) != WS_ERR_INVALID_ARG) return 7;\n"
        "    return f[0] == 7.f && l[0] == 7.f && u[0] == 7u && k == 7u && c[0] == 7u ? 0 : 8;\n"
        "}\n")
    exe = tmp_path / "whitewater"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    e, s = ws.fluid.whitewater_emit_params(), ws.fluid.whitewater_step_params()
    f = np.full((4, 3), 7.0, np.float32)
    l = np.full(4, 7.0, np.float32)
    u = np.full(4, 7, np.uint32)
    c = np.full(4, 7, np.uint8)
    k = C.c_uint32(7)
    assert lib.ws_read_whitewater(None, l.ctypes.data, l.ctypes.data, l.ctypes.data, l.ctypes.data, f.ctypes.data,
                                  u.ctypes.data) == 1
    assert lib.ws_emit_whitewater(None, C.byref(e), 4, f.ctypes.data, f.ctypes.data, l.ctypes.data, u.ctypes.data,
                                  C.byref(k)) == 1
    assert lib.ws_step_whitewater(None, C.byref(s), f.ctypes.data, f.ctypes.data, l.ctypes.data, 4, f.ctypes.data,
                                  f.ctypes.data, l.ctypes.data, c.ctypes.data) == 1
    assert lib.ws_step_whitewater(None, None, None, None, None, 0, None, None, None, None) == 1
    assert np.all(f == 7.0) and np.all(l == 7.0) and np.all(u == 7) and np.all(c == 7) and k.value == 7
