"""vrc_brick_segment in two parts, on the host build of the per-ray code (no GPU needed).

The grid walk takes a brick's interval first (vrc_core.h: vrc_brick_interval) and completes the segment where the march
needs it: the uniform march reads the distance alone (vrc_segment_dist), every other march the whole segment
(vrc_segment_complete).  tests/cpu_harness/segment_split_harness.cpp keeps a verbatim copy of the function as it was in
one piece; over generated cases -- axis-parallel rays, intervals of one ulp, brick corners, bricks behind the eye, 0, 1
and 3 clip planes, both variants, tNear beyond tFarGlobal -- interval plus completion must return the same bool, the same
`stop` and the same bits of pos, step, dist and tNear, and the distance-only form the same bits of dist.  Run plain, and
as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "segment_split_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libsegment_split_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "segment_split_san")
DEPS = [SRC, os.path.join(orc.ROOT, "libre_amd", "csrc", "vrc_core.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]

KINDS = ["random", "axis-parallel", "one ulp", "corner", "behind the eye", "past tFarGlobal"]
CASES, SEGMENTS, STOP, ONE_ULP, BAD = range(5)


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _check(tallies):
    for kind, t in zip(KINDS, tallies):
        assert t[BAD] == 0, (kind, t)
        if kind != "behind the eye":
            assert t[CASES] > 0 and 0 < t[SEGMENTS] < t[CASES], (kind, t)  # bricks hit and bricks missed
    by = dict(zip(KINDS, tallies))
    assert by["behind the eye"][CASES] > 0 and by["behind the eye"][SEGMENTS] == 0  # never marched, by either variant
    assert by["past tFarGlobal"][STOP] > 0  # the reference's break
    assert by["one ulp"][ONE_ULP] > 0 and by["corner"][ONE_ULP] > 0


def test_interval_plus_completion_is_the_segment_it_was():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.segment_split_run.restype = C.c_uint64
    H.segment_split_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    assert H.segment_split_kinds() == len(KINDS)
    out = (C.c_uint64 * (5 * len(KINDS)))()
    per = 30000  # x 6 kinds x 2 variants x 3 plane counts = 1.08e6 cases
    bad = H.segment_split_run(2024, per, out)
    tallies = [list(out[5 * k:5 * k + 5]) for k in range(len(KINDS))]
    assert sum(t[CASES] for t in tallies) == per * 36 >= 10 ** 6
    assert bad == 0, tallies
    _check(tallies)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DSEGMENT_SPLIT_MAIN"])
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=300)  # 1.08e5 cases
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("kind ")]
    tallies = [[int(ln[3]), int(ln[5]), int(ln[7]), int(ln[9]), int(ln[11])] for ln in lines]
    assert len(tallies) == len(KINDS)
    _check(tallies)
