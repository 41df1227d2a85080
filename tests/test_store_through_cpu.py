"""The pixel store of the replay and the decision behind VRC_OPT_STORE_THROUGH, on the host (no GPU needed).

tests/cpu_harness/store_through_harness.cpp holds two things to what they replaced or state:
  - vrc_plan_store_through (vrc_plan.h) over all its inputs: the option, what the walk cache did with the pass (0 ... 4,
    only 4 is a replay) and the frame's size, with the 4 GiB edge -- 16384 x 16384 pixels are exactly 2^32 bytes and
    keep the plain stores, one pixel row less takes the write-through ones;
  - the host build of vrc_store_pixel: with vrc_frame::storeThrough at 0 and at 1, vrc_pixel_walk_replay,
    vrc_pixel_walk_replay_lean and its uniform-only form leave, byte for byte, the pixel, the sample count and the
    untouched neighbours that the walk (vrc_pixel_grid_dda, whose stores are plain assignments) leaves for the same ray --
    the grids, tables and kinds of rays of the lean harness, as they are and with every brick uniform.  Rays without
    visits are met, and leave zeros where the frame clears.  3 grids x 2 scene forms x 2 variants x 7 kinds x 40 rays.
Run plain, and a quarter of it as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "store_through_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libstore_through_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "store_through_san")
DEPS = [SRC] + [os.path.join(HERE, "cpu_harness", n) for n in ("walk_uniform_only_harness.cpp", "walk_lean_harness.cpp",
                                                                "walk_cache_harness.cpp")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h", "vrc_plan.h")] + [
    os.path.join(orc.ROOT, "include", "vrc_hip.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

RAYS, NONE, LISTS, REPLAYS, UNIFORM, CLEARED, BAD = range(7)
PER = 40


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _lib():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.store_through_run.restype = C.c_uint64
    H.store_through_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    H.store_through_plan.restype = C.c_int
    H.store_through_plan.argtypes = [C.c_int64, C.c_int64, C.c_uint32, C.c_uint32]
    H.store_through_default.restype = C.c_int64
    return H


def _check(t, per):
    assert t[BAD] == 0, t
    assert t[RAYS] == per * 3 * 2 * 2 * 7  # every generated ray ran
    assert t[NONE] > 0 and t[LISTS] > 0 and t[NONE] + t[LISTS] == t[RAYS], t
    # six table set-ups x two values of the word x (two replay functions, and the uniform-only form on half the scenes)
    assert t[REPLAYS] == 6 * 2 * (2 * t[RAYS] + t[RAYS] // 2), t
    assert t[UNIFORM] == 6 * 2 * (t[RAYS] // 2), t
    assert t[CLEARED] == 4 * t[NONE], t  # the four set-ups that clear, for every ray without visits


def test_the_decision_over_all_its_inputs():
    H = _lib()
    assert H.store_through_default() == 1
    sizes = [(0, 0), (1, 1), (40, 24), (1024, 1024), (16384, 16383), (16383, 16384), (16384, 16384), (16385, 16384),
             (65535, 4096), (65536, 4096), (65536, 4095), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF), (1 << 28, 1),
             ((1 << 28) - 1, 1), (1, 1 << 28), (1 << 31, 2),
             (1 << 31, 1 << 29), (1 << 30, 1 << 30), (1 << 16, 1 << 16)]  # (bytes of 2^64 and more: no wrap to a small number)
    for option, used, (w, h) in itertools.product((0, 1), (0, 1, 2, 3, 4), sizes):
        want = option == 1 and used == 4 and w * h * 16 < 2 ** 32
        assert H.store_through_plan(option, used, w, h) == int(want), (option, used, w, h)
    # the edge the kernel's 32-bit byte offset sets: exactly 4 GiB is refused, one pixel row less is taken
    assert 16384 * 16384 * 16 == 2 ** 32
    assert H.store_through_plan(1, 4, 16384, 16384) == 0
    assert H.store_through_plan(1, 4, 16384, 16383) == 1


def test_the_host_store_leaves_the_bytes_of_the_assignment_it_replaced():
    H = _lib()
    out = (C.c_uint64 * 7)()
    bad = H.store_through_run(2026, PER, out)
    t = list(out)
    print("rays %d none %d lists %d replays %d uniform %d cleared %d mismatches %d" % tuple(t))
    assert bad == 0, t
    _check(t, PER)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DSTORE_THROUGH_MAIN"])
    r = subprocess.run([exe, str(PER // 4)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    _check([int(words[0][i]) for i in (1, 3, 5, 7, 9, 11, 13)], PER // 4)
    assert words[0][14:16] == ["plan", "0"]
