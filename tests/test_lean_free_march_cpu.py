"""The free body of the lean march and the decision behind VRC_OPT_LEAN_FREE_MARCH, on the host (no GPU needed).

tests/cpu_harness/lean_free_harness.cpp holds vrc_march_uniform_lean with the frame's word set (vrc_core.h:
vrc_march_uniform_free behind vrc_lean_free_visit) to the march it stood in for, exhaustively:
  - against vrc_march_uniform_counted and against the text of the lean march before the free body, with memcmp on the
    colour, and on return value and count; both colour forms; n = 0 .. 300 and 4095; entries over a grid of alpha from 0
    to 1 with 0, -0, denormals, 1.0, a negative value and NaN; start alpha 0 .. 0.9995, a negative value, NaN, and
    0.99 - n * e.w with its neighbours one ulp either way (the pre-test's own edge);
  - the free body is taken exactly where the pre-test passes (a hook counter), never with the word clear and never by a
    counted march;
  - the bound's premise: wherever the pre-test passes, the tested march returns false;
  - vrc_plan_lean_free_march (vrc_plan.h) over all its inputs.
Run plain, and all of it as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "lean_free_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "liblean_free_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "lean_free_san")
DEPS = [SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_plan.h")] + [
    os.path.join(orc.ROOT, "include", "vrc_hip.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

CASES, PASSED, EARLY, BAD, FREED, PREMISE, STRAY = range(7)
N_COUNTS = 302  # 0 .. 300 and 4095
N_ENTRIES = 27
N_STARTS = 14   # and three more around the pre-test's edge where that lies in [0, 1)


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _lib():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.lean_free_run.restype = C.c_uint64
    H.lean_free_run.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    H.lean_free_group.restype = C.c_uint32
    H.lean_free_default.restype = C.c_int64
    H.lean_free_plan.restype = C.c_int
    H.lean_free_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
    return H


@pytest.fixture(scope="module")
def tallies():
    H = _lib()
    out = {}
    for grey in (1, 0):
        t = (C.c_uint64 * 7)()
        out[grey] = (H.lean_free_run(grey, t), list(t))
    return out


@pytest.mark.parametrize("grey", (1, 0), ids=("grey", "four-float"))
def test_the_free_march_is_the_tested_march_bit_for_bit(tallies, grey):
    bad, t = tallies[grey]
    print("grey %d: cases %d passed the pre-test %d ended early %d mismatches %d" % (grey, t[CASES], t[PASSED], t[EARLY], t[BAD]))
    assert bad == 0 and t[BAD] == 0
    lo = N_COUNTS * N_ENTRIES * N_STARTS
    assert lo < t[CASES] <= lo + 3 * N_COUNTS * N_ENTRIES
    # both bodies are well exercised, and so is the early exit of the tested one
    assert t[PASSED] > t[CASES] // 10 and t[CASES] - t[PASSED] > t[CASES] // 10 and t[EARLY] > t[CASES] // 20


@pytest.mark.parametrize("grey", (1, 0), ids=("grey", "four-float"))
def test_the_free_body_is_taken_where_the_pre_test_passes_and_nowhere_else(tallies, grey):
    _, t = tallies[grey]
    assert t[FREED] == t[PASSED] > 0
    assert t[STRAY] == 0  # not with the frame's word clear, not by a counted march


@pytest.mark.parametrize("grey", (1, 0), ids=("grey", "four-float"))
def test_the_premise_of_the_bound_no_passing_case_reaches_the_threshold(tallies, grey):
    _, t = tallies[grey]
    assert t[PREMISE] == 0


def test_the_group_is_a_power_of_two():
    g = _lib().lean_free_group()
    assert g >= 4 and g & (g - 1) == 0


def test_the_decision_over_all_its_inputs():
    H = _lib()
    assert H.lean_free_default() == 1
    seen = set()
    for option, count, used, lean, classify in itertools.product((0, 1), (0, 1), (0, 1, 2, 3, 4), (0, 1, 2), (0, 1)):
        want = 1 if option == 1 and count == 0 and used == 4 and lean != 0 and classify == 0 else 0
        assert H.lean_free_plan(option, count, used, lean, classify) == want, (option, count, used, lean, classify)
        seen.add(want)
    assert seen == {0, 1}


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DLEAN_FREE_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cases ")]
    assert len(words) == 1
    w = dict(zip(words[0][0::2], words[0][1::2]))
    assert int(w["cases"]) > 2 * N_COUNTS * N_ENTRIES * N_STARTS and int(w["freed"]) == int(w["passed"]) > 0
    assert (w["premise"], w["stray"], w["plans"], w["mismatches"], w["plan"]) == ("0", "0", "120", "0", "0")
