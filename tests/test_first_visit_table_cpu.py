"""The first-visit table of the lean replay and the decisions behind VRC_OPT_FIRST_VISIT_TABLE, on the host (no GPU needed).

tests/cpu_harness/first_visit_harness.cpp holds three things to what they state:
  - the host build of the row builder (vrc_core.h: vrc_first_visit_row) against vrc_march_uniform_lean from zero, for all
    256 entries x every n in 0 .. ROWS - 1, in the grey and the four-float form, over classified tables of alpha 0.05,
    0.3 and 1.0 (the last with an entry whose w is 1, which crosses at sample 1, and one more with the opacity
    correction at 8): colours with memcmp, `done` with the march's return value, the counted march's samples with
    min(n, crossing);
  - vrc_pixel_walk_replay_lean with the table against without it, both lean forms, at n = 0, 1, 31, 32, 33, 63, 64,
    150, ROWS - 1 (looked up) and ROWS, ROWS + 1 (marched); a pass that does not clear, and a first visit whose word does
    not hold one value, are handed a table of NaNs and leave the pixel of the run without one;
  - vrc_plan_first_visit and vrc_plan_first_visit_build (vrc_plan.h) over all their inputs.
Run plain, and all of it as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "first_visit_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libfirst_visit_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "first_visit_san")
DEPS = [SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_plan.h")] + [
    os.path.join(orc.ROOT, "include", "vrc_hip.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

CELLS, EARLY, CROSSING, BAD = range(4)
CALLED_OUT = (0, 1, 31, 32, 33, 63, 64)


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _lib():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.first_visit_run.restype = C.c_uint64
    H.first_visit_run.argtypes = [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint64)]
    H.first_visit_replay.restype = C.c_uint64
    H.first_visit_replay.argtypes = [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    H.first_visit_rows.restype = C.c_uint32
    H.first_visit_default.restype = C.c_int64
    H.first_visit_plan.restype = C.c_int
    H.first_visit_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32] + [C.c_int] * 4
    return H


@pytest.mark.parametrize("grey", (1, 0), ids=("grey", "four-float"))
@pytest.mark.parametrize("alpha,correction", ((0.05, 1.0), (0.3, 1.0), (1.0, 1.0), (1.0, 8.0)))
def test_a_row_is_the_march_from_zero(alpha, correction, grey):
    H = _lib()
    rows = H.first_visit_rows()
    assert rows >= 152 and all(n < rows for n in CALLED_OUT)  # every n of the issue's list is a row of the table
    t = (C.c_uint64 * 4)()
    bad = H.first_visit_run(alpha, correction, grey, t)
    print("alpha %g correction %g grey %d: cells %d ended early %d entries crossing %d mismatches %d" % (
        alpha, correction, grey, t[CELLS], t[EARLY], t[CROSSING], t[BAD]))
    assert bad == 0 and t[BAD] == 0
    assert t[CELLS] == 256 * rows
    if alpha == 1.0:
        # entry 255 has w = 1: every n >= 1 of it ends early, and the table freezes it from row 1 on
        assert t[CROSSING] >= 1 and t[EARLY] >= rows - 1
    if alpha == 0.05 and correction == 1.0:
        assert t[CROSSING] > 0 and t[EARLY] > 0  # 0.95^135 < 0.001: the largest entries cross inside the rows


@pytest.mark.parametrize("uniform_only", (1, 0), ids=("uniform-only", "lean"))
@pytest.mark.parametrize("grey", (1, 0), ids=("grey", "four-float"))
@pytest.mark.parametrize("alpha", (0.05, 1.0))
def test_the_replay_with_the_table_leaves_the_pixel_of_the_replay_without(alpha, grey, uniform_only):
    H = _lib()
    t = (C.c_uint64 * 4)()
    bad = H.first_visit_replay(alpha, grey, uniform_only, t)
    assert bad == 0 and t[BAD] == 0
    assert t[CELLS] == 256 * 11 * 4


def test_the_decisions_over_all_their_inputs():
    H = _lib()
    assert H.first_visit_default() == 1
    seen = set()
    for option, count, used, lean, clear, classify, current, prev in itertools.product(
            (0, 1), (0, 1), (0, 1, 2, 3, 4), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)):
        wanted = option == 1 and count == 0 and used == 4 and lean != 0 and clear == 1 and classify == 0
        want = (1 if wanted and current else 0) | (2 if wanted and not current and prev else 0)
        got = H.first_visit_plan(option, count, used, lean, clear, classify, current, prev)
        assert got == want, (option, count, used, lean, clear, classify, current, prev)
        seen.add(got)
    assert seen == {0, 1, 2}  # never both: a pass that builds is handed `current` by the caller, then asked again
    # the edit sequence: a new table every frame never builds; the second frame with one table does, and is then current
    assert H.first_visit_plan(1, 0, 4, 2, 1, 0, 0, 0) == 0
    assert H.first_visit_plan(1, 0, 4, 2, 1, 0, 0, 1) == 2
    assert H.first_visit_plan(1, 0, 4, 2, 1, 0, 1, 1) == 1


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DFIRST_VISIT_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cells ")]
    assert len(words) == 1
    rows = _lib().first_visit_rows()
    assert int(words[0][1]) == 7 * 256 * rows and int(words[0][3]) == 12 * 256 * 11 * 4 and int(words[0][5]) == 960
    assert words[0][6:] == ["mismatches", "0", "plan", "0"]
