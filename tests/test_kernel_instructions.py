"""What the compiler picks inside the two neighbour kernels, read from a device-only cross-compile of csrc/ws_kernels.hip
with the build's own flag list (no GPU needed; a few seconds; skipped when there is no hipcc).  Both kernels are bound by
VALU issue cycles in the settled state, and two kinds of instruction cost them more than their count says:

 * packed f32 arithmetic (v_pk_add / mul / fma_f32), which the SLP vectoriser and vector-typed expressions produce and
   which costs more here than the two scalar instructions each replaces -- none anywhere in either kernel;
 * quarter-rate integer multiplies (v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32) for mask-row addresses that are running
   sums -- none inside any loop of either kernel (a loop = the span from a label to the last branch back to it; the
   prologues and the mask-less sweep's straight-line parts may keep theirs).

Plus the register / LDS budgets the occupancy of the kernels rests on (7 waves per SIMD for K5's plain arithmetic, 8 for
K4), for every instantiation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PACKED_F32 = re.compile(r"\bv_pk_(?:add|mul|fma)_f32\b")
SLOW_MUL = re.compile(r"\bv_(?:mul_lo_u32|mul_hi_u32|mad_u64_u32)\b")
LINK_ONLY = {"-fPIC", "-shared"}  # of the build's flags, the ones that make no sense with -S


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{demangled kernel name: (assembly of its body, {.amdhsa_* key: value})} of K4's and K5's instantiations."""
    import water_sandbox_amd as ws

    hipcc = ws.build.hipcc()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)) or not shutil.which("c++filt"):
        pytest.skip("no hipcc / c++filt on this machine")
    out = str(tmp_path_factory.mktemp("asm") / "ws_kernels.s")
    flags = [f for f in ws.build.HIPCC_FLAGS if f not in LINK_ONLY]
    assert "-fno-slp-vectorize" in flags and "-ffp-contract=off" in flags and "-O3" in flags
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", ws.build.CSRC,
                                             "-o", out, os.path.join(ws.build.CSRC, "ws_kernels.hip")])
    txt = open(out).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M)}
    meta = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, flags=re.S)}
    names = [n for n in meta if "k_density_listed" in n or "k_force_listed" in n]
    short = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    found = {s.split("(")[0].replace("void ", ""): (body[n], meta[n]) for n, s in zip(names, short)}
    assert len([k for k in found if k.startswith("k_density_listed")]) == 6, sorted(found)    # IEEE x {plain, CUT, SCHED}
    assert len([k for k in found if k.startswith("k_force_listed")]) == 24, sorted(found)  # ... x ACCEL_ONLY x tile
    return found


def loop_lines(body):
    """The instruction lines inside loops: every span from a basic-block label to a later branch back to it."""
    lines = body.split("\n")
    label = {}
    for n, line in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            label[m.group(1)] = n
    inside = set()
    for n, line in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", line)
        if m and label.get(m.group(1), n + 1) <= n:
            inside.update(range(label[m.group(1)], n + 1))
    return [lines[n] for n in sorted(inside)]


def template_args(name):
    return [a.strip() for a in name[name.index("<") + 1:name.rindex(">")].split(",")]


def test_the_loop_finder_sees_loops(kernels):
    """K4 walks nine runs in two forms each, K5 has the walk, the iterator and the sweep: a parser that found no loop
    would pass the multiply check for nothing."""
    for name, (body, _) in kernels.items():
        inside = loop_lines(body)
        assert any("global_load_dwordx4" in line for line in inside), name  # the candidate loads / the gathers
        assert len(inside) > 200, (name, len(inside))


def test_no_packed_f32_in_the_neighbour_kernels(kernels):
    for name, (body, _) in kernels.items():
        assert not PACKED_F32.findall(body), (name, PACKED_F32.findall(body)[:4])


def test_no_integer_multiplies_inside_the_loops(kernels):
    for name, (body, _) in kernels.items():
        bad = [line.strip() for line in loop_lines(body) if SLOW_MUL.search(line)]
        assert not bad, (name, bad[:4])


def test_register_and_lds_budgets(kernels):
    for name, (_, meta) in kernels.items():
        vgpr, lds = int(meta["next_free_vgpr"]), int(meta["group_segment_fixed_size"])
        assert int(meta["private_segment_fixed_size"]) == 0, (name, "scratch")
        args = template_args(name)
        if name.startswith("k_density_listed"):
            assert vgpr <= 64 and lds == 4864, (name, vgpr, lds)  # 8 waves per SIMD
        else:
            ieee, sched, tile = args[0] == "true", args[3] == "true", int(args[4])
            limit = 80 if ieee else 74 if sched else 72  # 72: 7 waves per SIMD
            assert vgpr <= limit, (name, vgpr, limit)
            assert lds == 19 * 4 * tile, (name, lds)  # 9 728 B at tile 128
