"""The VALU instructions of one K4 phase-1 trip, read from a device-only cross-compile of csrc/ws_kernels.hip with the
build's own flag list (no GPU needed; skipped when there is no hipcc).  The settled K4 is bound by VALU issue, a wave
makes 83 trips of 4 candidates there, so the instructions of a trip are its time.

Method: in each of the six instantiations, every group of three `global_load_dwordx4 ..., s[..]` (the x / y / z planes of
one trip) sits in loops; the innermost one -- the shortest span from a basic-block label to a branch back to it that
holds the three loads -- is that trip's loop, and the `v_*` lines inside it are counted.  Nine runs come out as three
copies of each loop.

The parent of this change (commit f047763), counted the same way: 65 VALU in the wave-uniform walk's loop, 63 in the
plain walk's, and about 10 more in the blocks a wave-uniform trip passed through before it came back (two votes that
went through a VGPR, `more` carried as a bool).  The shipped walk keeps its trips in loops of their own and votes on the
scalar unit; no loop may hold more than the parent's did.

Two further parts were built, measured and not adopted (HISTORY.md round 7; they win in the settled state at 2^22
particles and up and lose at 2^16 .. 2^18): tools/ab/patches/k4_masked_push.patch (store, advance and mark in the lanes
that accept a candidate only) and k4_whole_trips.patch (trips without validity tests while every lane has four
candidates left).  With them the trip without validity tests has to stay at least 12 VALU below the parent's 65 -- the
four validity compares, four v_cndmask, three v_addc and an address formation: the bound is kept on the patched build,
so the patches stay honest for whoever takes them up again."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_ONLY = {"-fPIC", "-shared"}

PARENT_UNIFORM, PARENT_PLAIN = 65, 63  # commit f047763, same method
UNIFORM, PLAIN = 59, 60                # achieved, shipped: 32 distance arithmetic + 27 / 28
PATCHED_WHOLE, PATCHED_PARTIAL, PATCHED_PLAIN = 49, 53, 54  # achieved with k4_masked_push + k4_whole_trips + k4_uicmp_votes
PARTS = ["k4_masked_push", "k4_whole_trips", "k4_uicmp_votes"]


def k4_bodies(csrc, out):
    """{mangled name: assembly of the body} of K4's six instantiations, compiled from the sources in `csrc`."""
    import water_sandbox_amd as ws

    hipcc = ws.build.hipcc()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    flags = [f for f in ws.build.HIPCC_FLAGS if f not in LINK_ONLY]
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                                             "-o", out, os.path.join(csrc, "ws_kernels.hip")])
    txt = open(out).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M)}
    found = {n: b for n, b in body.items() if "k_density_listed" in n}
    assert len(found) == 6, sorted(found)
    return found


def trip_loops(body):
    """[VALU count of the innermost loop around each group of three plane loads], in program order."""
    lines = body.split("\n")
    label = {}
    for n, line in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            label[m.group(1)] = n
    loops = []
    for n, line in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", line)
        if m and label.get(m.group(1), n + 1) <= n:
            loops.append((label[m.group(1)], n))
    loads = [n for n, line in enumerate(lines) if re.search(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", line)]
    assert loads and len(loads) % 3 == 0, len(loads)
    counts = []
    for g in range(0, len(loads), 3):
        first, last = loads[g], loads[g + 2]
        assert last - first == 2, "the three plane loads of a trip are issued together"
        around = [(b - a, a, b) for a, b in loops if a <= first and last <= b]
        assert around, "a trip outside every loop"
        _, a, b = min(around)
        counts.append(sum(1 for line in lines[a:b + 1] if re.match(r"\s+v_", line)))
    return counts


def test_valu_instructions_per_trip(tmp_path):
    import water_sandbox_amd as ws

    for name, body in k4_bodies(ws.build.CSRC, str(tmp_path / "ws_kernels.s")).items():
        counts = trip_loops(body)
        print(name, counts)
        assert sorted(counts) == sorted([UNIFORM, PLAIN] * 3), (name, counts)
    assert UNIFORM <= PARENT_UNIFORM and PLAIN <= PARENT_PLAIN


@pytest.mark.skipif(shutil.which("patch") is None, reason="no patch(1)")
def test_valu_instructions_per_trip_with_the_parts_that_were_not_adopted(tmp_path):
    import water_sandbox_amd as ws

    work = tmp_path / "water-sandbox_amd"
    work.mkdir()
    shutil.copytree(ws.build.CSRC, str(work / "csrc"))
    for part in PARTS:
        with open(os.path.join(ROOT, "tools", "ab", "patches", part + ".patch")) as p:
            subprocess.run(["patch", "-s", "-p1", "-d", str(tmp_path)], stdin=p, check=True)
    for name, body in k4_bodies(str(work / "csrc"), str(tmp_path / "ws_kernels_parts.s")).items():
        counts = trip_loops(body)
        print(name, counts)
        assert sorted(counts) == sorted([PATCHED_WHOLE, PATCHED_PARTIAL, PATCHED_PLAIN] * 3), (name, counts)
    assert PATCHED_WHOLE <= PARENT_UNIFORM - 12  # the issue's bound on the trip without validity tests
    assert PATCHED_PARTIAL <= PARENT_UNIFORM and PATCHED_PLAIN <= PARENT_PLAIN
