"""ws_apply_forces in the C ABI: exported, bound, declared in plain C with the struct layout the header gives, the ABI
version unchanged, and the NULL handle refused without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["kind", "centre", "axis", "radius", "strength", "damping", "reserved"]
OFFSETS = {"kind": 0, "centre": 4, "axis": 16, "radius": 28, "strength": 32, "damping": 36, "reserved": 40}


def _header():
    text = open(os.path.join(ROOT, "include", "wsfluid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", _header())))


def test_the_symbol_is_exported_declared_and_bound(ws):
    lib = ws.load_library()
    assert hasattr(lib, "ws_apply_forces")
    assert "ws_apply_forces" in _declared() and "ws_apply_forces" in ws.fluid.ABI_SYMBOLS
    assert lib.ws_apply_forces.argtypes is not None and len(lib.ws_apply_forces.argtypes) == 5
    assert sorted(ws.fluid.ABI_SYMBOLS) == _declared()
    assert lib.ws_abi_version() == 2 == ws.fluid.WS_ABI_VERSION  # additive change: the version stays
    for cls in (ws.FluidWorker, ws.slab.SlabWorker):
        assert callable(getattr(cls, "apply_forces")), cls
    text = _header()
    for name, value in (("WS_FORCE_RADIAL", 0), ("WS_FORCE_JET", 1), ("WS_FORCE_VORTEX", 2), ("WS_MAX_FORCES", 16)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, text).group(1)) == value == getattr(ws.fluid, name)


def test_the_struct_has_the_headers_layout(ws):
    S = ws.fluid.WsForce
    assert C.sizeof(S) == 48
    body = re.search(r"typedef struct ws_force \{(.*?)\} ws_force;", _header(), flags=re.S).group(1)
    assert [n for n, _ in S._fields_] == FIELDS == re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    for name, off in OFFSETS.items():
        assert getattr(S, name).offset == off, name
    f = ws.fluid.force("vortex", (1.0, 2.0, 3.0), 0.5, -4.0, axis=(0.0, 1.0, 0.0), damping=0.25)
    assert f.kind == 2 and tuple(f.centre) == (1.0, 2.0, 3.0) and tuple(f.axis) == (0.0, 1.0, 0.0)
    assert (f.radius, f.strength, f.damping, tuple(f.reserved)) == (0.5, -4.0, 0.25, (0, 0))
    g = ws.fluid.force(ws.fluid.WS_FORCE_RADIAL, (0, 0, 0), 1.0, 2.0)
    assert g.kind == 0 and tuple(g.axis) == (0.0, 0.0, 0.0) and g.damping == 0.0


def test_the_prototype_compiles_and_runs_as_plain_c(ws, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "forces.c"
    src.write_text(
        '#include "wsfluid.h"\n'
        "#include <stddef.h>\n"
        "int main(void) {\n"
        "    ws_force f = {WS_FORCE_JET, {0.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, 0.5f, 2.f, 0.f, {0u, 0u}};\n"
        "    uint32_t n[WS_MAX_FORCES];\n"
        "    ws_status (*ap)(ws_handle *, const ws_force *, uint32_t, float, uint32_t *) = ws_apply_forces;\n"
        "    n[0] = 7u;\n"
        "    if (sizeof f != 48 || offsetof(ws_force, centre) != 4 || offsetof(ws_force, axis) != 16) return 1;\n"
        "    if (offsetof(ws_force, radius) != 28 || offsetof(ws_force, strength) != 32) return 2;\n"
        "    if (offsetof(ws_force, damping) != 36 || offsetof(ws_force, reserved) != 40) return 3;\n"
        "    if (WS_FORCE_RADIAL != 0u || WS_FORCE_VORTEX != 2u || WS_MAX_FORCES != 16u || WS_ABI_VERSION != 2) return 4;\n"
        "    if (ap(NULL, &f, 1u, 0.01f, n) != WS_ERR_INVALID_ARG) return 5;\n"
        "    return n[0] == 7u && f.radius == 0.5f ? 0 : 6;\n"
        "}\n")
    exe = tmp_path / "forces"
    lib = ws.fluid.lib_path()
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_handle_is_an_invalid_argument_and_writes_nothing(ws):
    lib = ws.load_library()
    f = ws.fluid.force("radial", (0, 0, 0), 1.0, 1.0)
    n = np.full(16, 7, np.uint32)
    assert lib.ws_apply_forces(None, C.byref(f), 1, 0.01, n.ctypes.data) == 1
    assert lib.ws_apply_forces(None, None, 0, 0.0, None) == 1
    assert np.all(n == 7) and f.radius == 1.0
