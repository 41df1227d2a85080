"""The walk cache on the host build of the per-ray code (no GPU needed).

tests/cpu_harness/walk_cache_harness.cpp generates rays over grids of 1x1x1, 4x4x4 and 4x3x2 bricks (every third brick
constant and marked uniform) -- axis-parallel rays through brick faces, along brick edges and through brick corners
exactly, oblique rays, an eye inside the volume, the near plane inside a brick, cut global intervals and per-brick clip
planes, both variants -- and asserts for each: the recorded list (vrc_pixel_walk_record: count pass and record pass)
equals the sequence of visits the walk hands to vrc_march_brick, node for node and bit for bit in tNear, tFar and the
vrc_segment_dist of them, with no word written outside the ray's column or beyond walkK visits; and the pixel and the
sample count replayed from the list recorded ONCE (vrc_pixel_walk_replay) equal the walk's under alpha 0.05 and 1.0,
grey and coloured tables, and onto a pixel that is not cleared first.  No generated case is skipped: 3 grids x 2
variants x 7 kinds x 200 rays = 8400 cases, six table set-ups each.  Run plain, and a tenth of it as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_cache_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_cache_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_cache_san")
DEPS = [SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(orc.ROOT, "include")]

KINDS = ["axis through a face", "axis along an edge", "through a corner", "oblique", "eye inside", "near plane inside",
         "clipped"]
CASES, LISTS, VISITS, EARLY, UNIFORM, BAD = range(6)
PER = 200


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _check(tallies, per):
    assert sum(t[CASES] for t in tallies) == per * 3 * 2 * len(KINDS)  # every generated case ran
    for kind, t in zip(KINDS, tallies):
        assert t[BAD] == 0, (kind, t)
        assert t[CASES] == per * 6 and t[LISTS] > 0, (kind, t)
        assert t[VISITS] > t[LISTS], (kind, t)  # lists of more than one visit
        assert 0 < t[UNIFORM] < t[VISITS], (kind, t)  # uniform and mixed bricks
        assert t[EARLY] > 0, (kind, t)  # rays an opaque table ended before the list did
    by = dict(zip(KINDS, tallies))
    assert by["oblique"][LISTS] < by["oblique"][CASES] or by["clipped"][LISTS] < by["clipped"][CASES]  # rays without a list


def test_recorded_lists_are_the_walks_visits_and_replay_equals_the_walk():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_cache_run.restype = C.c_uint64
    H.walk_cache_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    assert H.walk_cache_kinds() == len(KINDS)
    out = (C.c_uint64 * (6 * len(KINDS)))()
    bad = H.walk_cache_run(2025, PER, out)
    tallies = [list(out[6 * k:6 * k + 6]) for k in range(len(KINDS))]
    print("cases %d, lists %d, visits %d" % tuple(sum(t[i] for t in tallies) for i in (CASES, LISTS, VISITS)))
    assert bad == 0, tallies
    _check(tallies, PER)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_CACHE_MAIN"])
    r = subprocess.run([exe, str(PER // 10)], capture_output=True, text=True, timeout=300)  # 840 cases
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("kind ")]
    tallies = [[int(ln[i]) for i in (3, 5, 7, 9, 11, 13)] for ln in lines]
    assert len(tallies) == len(KINDS)
    _check(tallies, PER // 10)
