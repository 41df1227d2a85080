"""The lean form of the walk cache's lists on the host build of the per-ray code (no GPU needed).

tests/cpu_harness/walk_lean_harness.cpp takes the scenes, tables and kinds of rays of the walk-cache harness and asserts
for each ray: the list recorded with vrc_frame::walkLean set equals the other form in its count and its node, tNear and
tFar planes, and its second plane unpacks to the node's own slotInfoIndex and to an n that equals the trip count of
`for( ; travel > 0; travel -= stepSize )` run on the dist the other form recorded; the count pass says "every visit
packs" for the power-of-two steps and "not" for 1/75; and vrc_pixel_walk_replay_lean leaves the pixel bits and the sample
count of vrc_pixel_walk_replay under alpha 0.05 and 1.0, grey and coloured tables, and onto a pixel that is not cleared
first.  Once per run: the lean uniform march against vrc_march_segment_as<..., UNIFORM> for every n from 0 to 70 and
4095, entries from transparent to opaque and starting alphas on both sides of the early-exit threshold, in two and four
floats; and the pack limits (4095 / 4096 steps, index 2^20 - 1 / 2^20).  3 grids x 2 variants x 7 kinds x 100 rays =
4200 rays.  Run plain, and a tenth of it as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_lean_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_lean_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_lean_san")
DEPS = [SRC, os.path.join(HERE, "cpu_harness", "walk_cache_harness.cpp")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

RAYS, LISTS, VISITS, UNIFORM, NOTLEAN, MARCHES, BAD = range(7)
PER = 100
MARCH_CASES = 72 * 8 * 6 * 2  # n x entry alphas x starting alphas x (two floats, four floats)


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _check(t, per):
    assert t[BAD] == 0, t
    assert t[RAYS] == per * 3 * 2 * 7  # every generated ray ran
    assert 0 < t[LISTS] < t[RAYS], t  # rays with and without a list
    assert t[VISITS] > t[LISTS], t  # lists of more than one visit, compared word for word
    assert 0 < t[UNIFORM] < t[VISITS], t  # uniform and mixed bricks
    assert 0 < t[NOTLEAN] < t[LISTS], t  # the step of 1/75 was refused, the others were not
    assert t[MARCHES] == MARCH_CASES, t


def test_lean_lists_unpack_to_slot_and_step_count_and_replay_equals_the_other_form():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_lean_run.restype = C.c_uint64
    H.walk_lean_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 7)()
    bad = H.walk_lean_run(2025, PER, out)
    t = list(out)
    print("rays %d lists %d visits %d uniform %d not lean %d marches %d mismatches %d" % tuple(t))
    assert bad == 0, t
    _check(t, PER)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_LEAN_MAIN"])
    r = subprocess.run([exe, str(PER // 10)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    _check([int(words[0][i]) for i in (1, 3, 5, 7, 9, 11, 13)], PER // 10)
