"""The uniform-only form of the lean replay on the host build of the per-ray code (no GPU needed).

tests/cpu_harness/walk_uniform_only_harness.cpp takes the grids, tables and kinds of rays of the lean harness, makes every
brick uniform, and asserts for each ray: the count pass reports no visit that gathers; vrc_pixel_walk_replay_lean<...,
true> -- handed no node table and no atlas -- leaves the pixel bits and the sample count of vrc_pixel_walk_replay_lean
from the same list, under alpha 0.05 and 1.0, grey and coloured tables, onto a pixel that is not cleared first, and from
planes that hold fewer visits than the ray has; a word that does not hold one value, planted on one visit, ends the
list at that visit (the lean replay of the visits before it) and a slot index past slotInfo is clamped, neither with a
read outside slotInfo's own allocation.  Lists of no visit, one visit and several are all met.  3 grids x 2 variants x
7 kinds x 100 rays = 4200 rays.  Run plain, and a tenth of it as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_uniform_only_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_uniform_only_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_uniform_only_san")
DEPS = [SRC] + [os.path.join(HERE, "cpu_harness", n) for n in ("walk_lean_harness.cpp", "walk_cache_harness.cpp")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

RAYS, NONE, ONE, MORE, REPLAYS, PLANTED, BAD = range(7)
PER = 100


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _check(t, per):
    assert t[BAD] == 0, t
    assert t[RAYS] == per * 3 * 2 * 7  # every generated ray ran
    assert t[NONE] > 0 and t[ONE] > 0 and t[MORE] > 0, t  # lists of 0, 1 and K visits
    assert t[NONE] + t[ONE] + t[MORE] == t[RAYS], t
    lists = t[ONE] + t[MORE]
    assert t[PLANTED] == 6 * lists, t  # a word planted under every table set-up of every ray that has a list
    assert t[REPLAYS] == 12 * t[RAYS] + 6 * lists, t  # whole planes, planes of one visit, an index past slotInfo


def test_the_uniform_only_replay_leaves_the_lean_replays_pixels_and_counts():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_uniform_only_run.restype = C.c_uint64
    H.walk_uniform_only_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 7)()
    bad = H.walk_uniform_only_run(2025, PER, out)
    t = list(out)
    print("rays %d none %d one %d more %d replays %d planted %d mismatches %d" % tuple(t))
    assert bad == 0, t
    _check(t, PER)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_UNIFORM_ONLY_MAIN"])
    r = subprocess.run([exe, str(PER // 10)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    _check([int(words[0][i]) for i in (1, 3, 5, 7, 9, 11, 13)], PER // 10)
