"""The count-changing calls in the C ABI: exported, bound, declared in plain C with the struct layout the header gives, the
ABI version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"ws_reserve_particles": 2, "ws_particle_capacity": 1, "ws_add_particles": 5, "ws_remove_particles": 5,
         "ws_remove_particle_ids": 4}
FIELDS = ["kind", "reserved", "centre", "half"]
OFFSETS = {"kind": 0, "reserved": 4, "centre": 8, "half": 20}


def _header():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def test_the_symbols_are_exported_declared_and_bound(ws):
    lib = ws.load_library()
    for name, argc in CALLS.items():
        assert hasattr(lib, name), name
        assert name in _declared() and name in ws.fluid.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == argc, name
    assert lib.ws_particle_capacity.restype is C.c_uint32
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for method in ("reserve", "capacity", "add_particles", "remove_particles", "remove_particle_ids"):
        assert callable(getattr(ws.FluidWorker, method)), method
    text = _header()
    assert int(re.search(r"#define WS_MAX_SINKS\s+(\d+)u", text).group(1)) == 16 == ws.fluid.WS_MAX_SINKS
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(WS_SINK_[A-Z]+)\s*=\s*(\d+)", text))
    assert enum == {"WS_SINK_SPHERE": 0, "WS_SINK_BOX": 1}
    assert (ws.fluid.WS_SINK_SPHERE, ws.fluid.WS_SINK_BOX) == (0, 1)


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsSink
    assert C.sizeof(S) == 32
    body = re.search(r"typedef struct ws_sink \{(.*?)\} ws_sink;", _header(), flags=re.S).group(1)
    assert [n for n, _ in S._fields_] == FIELDS == re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off, name
    b = ws.fluid.sink("box", (1.0, 2.0, 3.0), (0.5, 0.25, 0.125))
    assert (b.kind, b.reserved, tuple(b.centre), tuple(b.half)) == (1, 0, (1.0, 2.0, 3.0), (0.5, 0.25, 0.125))
    s = ws.fluid.sink(ws.fluid.WS_SINK_SPHERE, (0, 0, 0), 0.75)
    assert (s.kind, tuple(s.half)) == (0, (0.75, 0.0, 0.0))


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "population.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_sink s = {WS_SINK_BOX, 0u, {0.f, 0.f, 0.f}, {1.f, 2.f, 3.f}};\n"
        "    float p[3] = {0.f, 0.f, 0.f};\n"
        "    uint32_t n[WS_MAX_SINKS], id[1] = {0u};\n"
        "    ws_status (*rs)(ws_handle *, uint32_t) = ws_reserve_particles;\n"
        "    uint32_t (*pc)(ws_handle *) = ws_particle_capacity;\n"
        "    ws_status (*ad)(ws_handle *, const float *, const float *, const float *, uint32_t) = ws_add_particles;\n"
        "    ws_status (*rm)(ws_handle *, const ws_sink *, uint32_t, uint32_t *, uint32_t *) = ws_remove_particles;\n"
        "    ws_status (*ri)(ws_handle *, const uint32_t *, uint32_t, uint32_t *) = ws_remove_particle_ids;\n"
        "    n[0] = 7u;\n"
        "    if (sizeof s != 32 || offsetof(ws_sink, reserved) != 4 || offsetof(ws_sink, centre) != 8) return 1;\n"
        "    if (offsetof(ws_sink, half) != 20) return 2;\n"
        "    if (WS_SINK_SPHERE != 0 || WS_SINK_BOX != 1 || WS_MAX_SINKS != 16u || WS_ABI_VERSION != 2) return 3;\n"
        "    if (rs(NULL, 8u) != WS_ERR_INVALID_ARG || pc(NULL) != 0u) return 4;\n"
        "    if (ad(NULL, p, NULL, NULL, 1u) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (rm(NULL, &s, 1u, n, NULL) != WS_ERR_INVALID_ARG || ri(NULL, id, 1u, NULL) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return n[0] == 7u && s.half[2] == 3.f ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "population"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    s = ws.fluid.sink("sphere", (0, 0, 0), 1.0)
    n = np.full(16, 7, np.uint32)
    ids = np.zeros(1, np.uint32)
    pos = np.zeros(3, np.float32)
    assert lib.ws_remove_particles(None, C.byref(s), 1, n.ctypes.data, n.ctypes.data) == 1
    assert lib.ws_remove_particle_ids(None, ids.ctypes.data, 1, n.ctypes.data) == 1
    assert lib.ws_add_particles(None, pos.ctypes.data, None, None, 1) == 1
    assert lib.ws_add_particles(None, None, None, None, 0) == 1
    assert lib.ws_reserve_particles(None, 16) == 1
    assert lib.ws_particle_capacity(None) == 0
    assert np.all(n == 7) and s.half[0] == 1.0
