"""The resolved visit words of the uniform-only replay on the host build of the per-ray code (no GPU needed).

tests/cpu_harness/walk_resolved_harness.cpp holds
  - vrc_walk_resolved_word (vrc_core.h) to vrc_lean_slot_word + vrc_slot_holds_one_value over one word of slotInfo: every
    known/mixed bit pattern x 256 values, a list word whose index is none, 1, the last word and past walkSlots, with
    slotInfo and without it, the visit below, at and above the ray's count;
  - vrc_pixel_walk_replay_lean<false, ..., true> with the resolved planes to the same function without them, memcmp of
    the pixel: the generated rays of the uniform-only harness (lists of no visit, one visit and walkK visits, and planes
    of one visit under a longer count), grey and four-float tables, alpha 0.05 and 1.0, a pixel that is not cleared,
    the first-visit table and the free march on and off, and a word that does not hold one value planted on a visit;
  - vrc_plan_walk_resolved (vrc_plan.h) over all its inputs;
  - the replay's tile decode (vrc_replay_tile_origin, vrc_replay_lane_pixel) to the one it replaced, for every lane of
    every tile of 1 x 1 up to 9 x 7 tiles.
Run plain, and with fewer rays as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_resolved_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_resolved_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_resolved_san")
DEPS = [SRC] + [os.path.join(HERE, "cpu_harness", n) for n in ("walk_uniform_only_harness.cpp", "walk_lean_harness.cpp",
                                                                "walk_cache_harness.cpp")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h", "vrc_plan.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

RAYS, NONE, ONE, MORE, REPLAYS, PLANTED, BAD = range(7)
PER = 40
# patterns x values x indices x step counts x counts 0 .. walkK, with slotInfo and without
WORDS = 2 * 4 * 256 * 5 * 4 * 4
# 6 table set-ups x (first-visit table, free march) on and off
SETUPS = 6 * 4


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _lib():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_resolved_words.restype = C.c_uint64
    H.walk_resolved_words.argtypes = [C.POINTER(C.c_uint64)]
    H.walk_resolved_run.restype = C.c_uint64
    H.walk_resolved_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    H.walk_resolved_tiles.restype = C.c_uint64
    H.walk_resolved_tiles.argtypes = [C.POINTER(C.c_uint64)]
    H.walk_resolved_default.restype = C.c_int64
    H.walk_resolved_plan.restype = C.c_int
    H.walk_resolved_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int]
    return H


def _check_words(t):
    assert t[2] == 0, t
    assert t[0] == WORDS, t
    # the bit: with slotInfo, an index that is not none (4 of 5), the known-and-not-mixed pattern (1 of 4), and the
    # visit (1) below the count (counts 2 and 3 of 0 .. 3)
    assert t[1] == 256 * 4 * 4 * 2, t


def _check_run(t, per):
    assert t[BAD] == 0, t
    assert t[RAYS] == per * 3 * 2 * 7  # every generated ray ran
    assert t[NONE] > 0 and t[ONE] > 0 and t[MORE] > 0, t  # counts 0, 1 and walkK
    assert t[NONE] + t[ONE] + t[MORE] == t[RAYS], t
    lists = t[ONE] + t[MORE]
    assert t[PLANTED] == lists, t
    assert t[REPLAYS] == SETUPS * (2 * t[RAYS] + lists), t  # whole planes, planes of one visit, a planted word


def test_the_resolved_word_is_the_slot_words_rule():
    t = (C.c_uint64 * 3)()
    bad = _lib().walk_resolved_words(t)
    print("words %d set %d mismatches %d" % tuple(t))
    assert bad == 0, list(t)
    _check_words(list(t))


def test_the_replay_from_resolved_planes_leaves_the_same_pixels():
    out = (C.c_uint64 * 7)()
    bad = _lib().walk_resolved_run(2025, PER, out)
    t = list(out)
    print("rays %d none %d one %d more %d replays %d planted %d mismatches %d" % tuple(t))
    assert bad == 0, t
    _check_run(t, PER)


def test_the_plan_over_all_its_inputs():
    H = _lib()
    assert H.walk_resolved_default() == 1
    for option in (0, 1):
        for count in (0, 1):
            for uniform in (0, 1):
                for fits in (0, 1):
                    want = int(option == 1 and count == 0 and uniform == 1 and fits == 1)
                    assert H.walk_resolved_plan(option, count, uniform, fits) == want, (option, count, uniform, fits)


def test_the_tile_decode_is_the_one_it_replaced():
    t = (C.c_uint64 * 1)()
    bad = _lib().walk_resolved_tiles(t)
    assert bad == 0
    assert t[0] == 64 * sum(x * y for x in range(1, 10) for y in range(1, 8))


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_RESOLVED_MAIN"])
    per = PER // 10
    r = subprocess.run([exe, str(per)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    _check_words([int(lines["words"][i]) for i in (1, 3, 5)])
    _check_run([int(lines["rays"][i]) for i in (1, 3, 5, 7, 9, 11, 13)], per)
    assert int(lines["pixels"][3]) == 0 and int(lines["plan"][2]) == 0, r.stdout
