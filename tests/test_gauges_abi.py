"""The gauges in the C ABI: exported, bound, declared in plain C with the struct layout the header gives, the ABI version
unchanged, and the NULL handle refused without a device and with nothing written."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"ws_measure": 5, "ws_select_particles": 6}
FIELDS = ["count", "sum_pos", "sum_vel", "sum_ang", "sum_speed2", "sum_attr", "min_pos", "max_pos", "max_speed2", "reserved"]
OFFSETS = {"count": 0, "sum_pos": 8, "sum_vel": 32, "sum_ang": 56, "sum_speed2": 80, "sum_attr": 88, "min_pos": 120,
           "max_pos": 132, "max_speed2": 144, "reserved": 148}


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
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for method in ("measure", "select_particles"):
        assert callable(getattr(ws.FluidWorker, method)) and callable(getattr(ws.fluid, method)), method
    assert callable(ws.slab.SlabWorker.measure)
    text = _header()
    assert int(re.search(r"#define WS_MAX_REGIONS\s+(\d+)u", text).group(1)) == 16 == ws.fluid.WS_MAX_REGIONS
    assert int(re.search(r"#define WS_GAUGE_ATTRIBUTES\s+(\d+)u", text).group(1)) == 1 == ws.fluid.WS_GAUGE_ATTRIBUTES
    assert re.search(r"typedef\s+ws_sink\s+ws_region\s*;", text)
    assert ws.fluid.region is ws.fluid.sink


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsGauge
    assert C.sizeof(S) == 152 == ws.fluid.GAUGE_DTYPE.itemsize
    body = re.search(r"typedef struct ws_gauge \{(.*?)\} ws_gauge;", _header(), flags=re.S).group(1)
    assert [n for n, _ in S._fields_] == FIELDS == re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert list(ws.fluid.GAUGE_DTYPE.names) == FIELDS
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off == ws.fluid.GAUGE_DTYPE.fields[name][1], name
    r = ws.fluid.region("box", (1.0, 2.0, 3.0), (0.5, 0.25, 0.125))
    assert isinstance(r, ws.fluid.WsSink) and C.sizeof(r) == 32 and (r.kind, tuple(r.half)) == (1, (0.5, 0.25, 0.125))
    g = ws.fluid.Gauges(count=np.array([2, 0], np.uint64), sum_pos=np.array([[1 << 24, 3 << 24, -(1 << 25)], [0, 0, 0]], np.int64))
    assert g.total("pos").tolist() == [[1.0, 3.0, -2.0], [0.0, 0.0, 0.0]]
    assert g.mean("pos")[0].tolist() == [0.5, 1.5, -1.0] and np.isnan(g.mean("pos")[1]).all()


def test_the_rust_shim_declares_the_struct_with_the_same_fields():
    rust = open(os.path.join(ROOT, "rust", "fluid_compute.rs")).read()
    m = re.search(r"#\[repr\(C\)\][^\n]*\n(?:#\[[^\n]*\]\n)*pub struct WsGauge \{(.*?)\n\}", rust, flags=re.S)
    assert m, "no #[repr(C)] pub struct WsGauge"
    got = re.findall(r"pub\s+(\w+)\s*:\s*(?:\[(\w+);\s*(\d+)\]|(\w+))\s*,", m.group(1))
    want = [("count", "u64", 1), ("sum_pos", "i64", 3), ("sum_vel", "i64", 3), ("sum_ang", "i64", 3), ("sum_speed2", "i64", 1),
            ("sum_attr", "i64", 4), ("min_pos", "f32", 3), ("max_pos", "f32", 3), ("max_speed2", "f32", 1), ("reserved", "u32", 1)]
    assert [(n, a or s, int(k or 1)) for n, a, k, s in got] == want
    size = {"u64": 8, "i64": 8, "f32": 4, "u32": 4}
    assert sum(size[t] * k for _, t, k in want) == 152


def test_the_prototypes_compile_and_run_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "gauges.c"
    checks = " || ".join("offsetof(ws_gauge, %s) != %d" % (n, o) for n, o in OFFSETS.items())
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "#include <string.h>\n"
        "int main(void) {\n"
        "    ws_region r = {WS_SINK_SPHERE, 0u, {0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}};\n"
        "    ws_gauge g[WS_MAX_REGIONS], seven;\n"
        "    uint32_t ids[2] = {7u, 7u}, total = 7u;\n"
        "    ws_status (*me)(ws_handle *, const ws_region *, uint32_t, uint32_t, ws_gauge *) = ws_measure;\n"
        "    ws_status (*se)(ws_handle *, const ws_region *, uint32_t, uint32_t, uint32_t *, uint32_t *) = ws_select_particles;\n"
        "    const ws_sink *same = &r;\n"
        "    memset(g, 7, sizeof g);\n"
        "    memset(&seven, 7, sizeof seven);\n"
        "    if (sizeof(ws_gauge) != 152 || sizeof(ws_region) != 32 || sizeof g != 16 * 152) return 1;\n"
        "    if (" + checks + ") return 2;\n"
        "    if (WS_MAX_REGIONS != 16u || WS_GAUGE_ATTRIBUTES != 1u || WS_ABI_VERSION != 2) return 3;\n"
        "    if (sizeof g[0].count != 8 || sizeof g[0].sum_attr != 32 || sizeof g[0].min_pos != 12) return 4;\n"
        "    if (me(NULL, &r, 1u, 0u, g) != WS_ERR_INVALID_ARG) return 5;\n"
        "    if (se(NULL, same, 1u, 2u, ids, &total) != WS_ERR_INVALID_ARG) return 6;\n"
        "    return memcmp(&g[0], &seven, sizeof seven) == 0 && ids[0] == 7u && ids[1] == 7u && total == 7u ? 0 : 7;\n"
        "}\n")
    exe = tmp_path / "gauges"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    r = ws.fluid.region("sphere", (0, 0, 0), 1.0)
    out = np.full(16 * 152, 7, np.uint8)
    ids = np.full(4, 7, np.uint32)
    total = C.c_uint32(7)
    assert lib.ws_measure(None, C.byref(r), 1, 0, out.ctypes.data) == 1
    assert lib.ws_measure(None, C.byref(r), 1, 1, out.ctypes.data) == 1
    assert lib.ws_measure(None, None, 0, 0, None) == 1
    assert lib.ws_select_particles(None, C.byref(r), 1, 4, ids.ctypes.data, C.byref(total)) == 1
    assert lib.ws_select_particles(None, C.byref(r), 1, 0, None, None) == 1
    assert np.all(out == 7) and np.all(ids == 7) and total.value == 7 and r.half[0] == 1.0
