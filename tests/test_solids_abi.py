"""ws_collide_solids in the C ABI: exported, bound, declared in plain C with the struct layout the header gives, the ABI
version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["kind", "flags", "centre", "rot", "size", "velocity", "angular_velocity", "restitution", "friction", "margin", "reserved"]
OFFSETS = {"kind": 0, "flags": 4, "centre": 8, "rot": 20, "size": 56, "velocity": 68, "angular_velocity": 80,
           "restitution": 92, "friction": 96, "margin": 100, "reserved": 104}


def _raw():
    return open(os.path.join(ROOT, "include", "wsfluid.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def test_the_symbol_is_exported_declared_and_bound(ws):
    lib = ws.load_library()
    assert hasattr(lib, "ws_collide_solids")
    assert "ws_collide_solids" in _declared() and "ws_collide_solids" in ws.fluid.ABI_SYMBOLS
    assert lib.ws_collide_solids.argtypes is not None and len(lib.ws_collide_solids.argtypes) == 6
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        assert callable(getattr(cls, "collide_solids")), cls
    text = _header()
    for name, value in (("WS_SOLID_SPHERE", 0), ("WS_SOLID_BOX", 1), ("WS_SOLID_CAPSULE", 2), ("WS_SOLID_HOLLOW", 1),
                        ("WS_MAX_SOLIDS", 16)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, text).group(1)) == value == getattr(ws.fluid, name)
    hpp = open(os.path.join(ROOT, "water-sandbox_amd", "host", "fluid_compute.hpp")).read()
    assert "ws_collide_solids(h_" in hpp


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsSolid
    assert C.sizeof(S) == 112
    raw = re.search(r"typedef struct ws_solid \{(.*?)\} ws_solid;", _raw(), flags=re.S).group(1)
    assert int(re.search(r"(\d+) bytes", raw).group(1)) == 112
    body = re.search(r"typedef struct ws_solid \{(.*?)\} ws_solid;", _header(), flags=re.S).group(1)
    assert [n for n, _ in S._fields_] == FIELDS == re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    # the offsets the header's comments pin, against the binding and against the table above
    pinned = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(\w+)(?:\[\d+\])?;\s*/\* offset (\d+)", raw))
    assert pinned == OFFSETS
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off, name
    s = ws.fluid.solid("box", (1.0, 2.0, 3.0), (0.5, 0.25, 0.125), rot=[[0, 1, 0], [-1, 0, 0], [0, 0, 1]], hollow=True,
                       velocity=(1, 0, 0), angular_velocity=(0, 2, 0), restitution=0.5, friction=0.25, margin=0.0625)
    assert (s.kind, s.flags) == (1, 1) and tuple(s.centre) == (1.0, 2.0, 3.0) and tuple(s.size) == (0.5, 0.25, 0.125)
    assert tuple(s.rot) == (0, 1, 0, -1, 0, 0, 0, 0, 1) and tuple(s.velocity) == (1, 0, 0) and tuple(s.angular_velocity) == (0, 2, 0)
    assert (s.restitution, s.friction, s.margin, tuple(s.reserved)) == (0.5, 0.25, 0.0625, (0, 0))
    g = ws.fluid.solid(ws.fluid.WS_SOLID_SPHERE, (0, 0, 0), 0.75)
    assert (g.kind, g.flags) == (0, 0) and tuple(g.size) == (0.75, 0.0, 0.0) and tuple(g.rot) == (1, 0, 0, 0, 1, 0, 0, 0, 1)
    c = ws.fluid.solid("capsule", (0, 0, 0), (0.25, 1.0))
    assert c.kind == 2 and tuple(c.size) == (0.25, 1.0, 0.0)


def test_the_prototype_compiles_and_runs_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "solids.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_solid s = {WS_SOLID_BOX, WS_SOLID_HOLLOW, {0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f},\n"
        "                  {0.5f, 0.5f, 0.5f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.5f, 0.1f, 0.01f, {0u, 0u}};\n"
        "    uint32_t n[WS_MAX_SOLIDS];\n"
        "    double imp[3 * WS_MAX_SOLIDS], ang[3 * WS_MAX_SOLIDS];\n"
        "    ws_status (*cs)(ws_handle *, const ws_solid *, uint32_t, uint32_t *, double *, double *) = ws_collide_solids;\n"
        "    n[0] = 7u; imp[0] = 7.0; ang[0] = 7.0;\n"
        "    if (sizeof s != 112 || offsetof(ws_solid, flags) != 4 || offsetof(ws_solid, centre) != 8) return 1;\n"
        "    if (offsetof(ws_solid, rot) != 20 || offsetof(ws_solid, size) != 56 || offsetof(ws_solid, velocity) != 68) return 2;\n"
        "    if (offsetof(ws_solid, angular_velocity) != 80 || offsetof(ws_solid, restitution) != 92) return 3;\n"
        "    if (offsetof(ws_solid, friction) != 96 || offsetof(ws_solid, margin) != 100 || offsetof(ws_solid, reserved) != 104) return 3;\n"
        "    if (WS_SOLID_SPHERE != 0u || WS_SOLID_CAPSULE != 2u || WS_MAX_SOLIDS != 16u || WS_ABI_VERSION != 2) return 4;\n"
        "    if (cs(NULL, &s, 1u, n, imp, ang) != WS_ERR_INVALID_ARG) return 5;\n"
        "    return n[0] == 7u && imp[0] == 7.0 && ang[0] == 7.0 && s.margin == 0.01f ? 0 : 6;\n"
        "}\n")
    exe = tmp_path / "solids"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    s = ws.fluid.solid("sphere", (0, 0, 0), 1.0)
    n = np.full(16, 7, np.uint32)
    imp, ang = np.full((16, 3), 7.0), np.full((16, 3), 7.0)
    assert lib.ws_collide_solids(None, C.byref(s), 1, n.ctypes.data, imp.ctypes.data, ang.ctypes.data) == 1
    assert lib.ws_collide_solids(None, None, 0, None, None, None) == 1
    assert np.all(n == 7) and np.all(imp == 7.0) and np.all(ang == 7.0) and tuple(s.size) == (1.0, 0.0, 0.0)
