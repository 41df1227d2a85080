"""The host logic of the walk cache and the ray cache (libre_amd/csrc/vrc_plan.h), no GPU needed.

vrc_walk_open / vrc_walk_decide / vrc_walk_commit / vrc_walk_launched / vrc_walk_forget and vrc_plan_ray_cache replaced
render_walk_cache and render_ray_cache of vrc_api.hip, the three transitions render_march made behind its launches, and
the hand-written resets.  tests/cpu_harness/walk_plan_harness.cpp keeps verbatim copies of that text and drives both
sides through the same generated SEQUENCES of renders -- the state machine is the subject -- with option changes,
outside resets, failed allocations and failed launches between and inside them.  After every step old and new must agree
on the return code, the seven walk read-backs and the ray cache's, the polls, allocations (and their words) and launches
(and the walk fields they found in the frame), and the whole remembered state; after every step that returned VRC_OK
also on every frame field either side writes.  The tallies prove, as conditions, what the sequences reached.  Run plain,
and as a stand-alone program under the address and undefined-behaviour sanitizers on a tenth of the sequences."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_plan_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_plan_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_plan_san")
API = os.path.join(orc.ROOT, "libre_amd", "csrc", "vrc_api.hip")
DEPS = [SRC, os.path.join(orc.ROOT, "libre_amd", "csrc", "vrc_plan.h"), os.path.join(orc.ROOT, "include", "vrc_hip.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]

SEED, SEQUENCES, STEPS = 2024, 40000, 64

# lines of the copied blocks, counted in vrc_api.hip as it stood before the rules moved to vrc_plan.h
OLD_LINES = {"STRUCTS": 55, "RAY": 30, "WALK": 152, "MARCH": 24, "STORED": 2, "STREAM": 4, "OPTION": 19, "ROWMAP": 3,
             "NODES": 1}
NEW_BLOCKS = ["render_ray_cache", "walk_poll", "walk_allocate", "render_walk_cache", "march", "stored"]
# tallies that count trouble or bulk, not coverage
NOT_COVERAGE = {"steps", "bad", "refused"}


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _block(begin, end):
    body = open(SRC).read().split("/* %s */\n" % begin)[1].split("/* %s */" % end)[0]
    return body[:body.rindex("\n") + 1]  # (without the indentation in front of the END marker)


def _check_coverage(t):
    """Every condition the sequences must have reached, by name."""
    missing = [name for name, v in t.items() if name not in NOT_COVERAGE and v == 0]
    assert not missing, missing


def test_the_copied_text_has_the_lines_counted_before_the_move():
    assert {b: _block("BEGIN %s BLOCK" % b, "END %s BLOCK" % b).count("\n") for b in OLD_LINES} == OLD_LINES


def test_the_callers_under_test_are_the_text_of_vrc_api_hip():
    api = open(API).read()
    for name in NEW_BLOCKS:
        body = _block("BEGIN NEW %s" % name, "END NEW %s" % name)
        assert body.strip() and body in api, name
    # ... and beside the plan's own helpers nothing in vrc_api.hip assigns the caches' states
    for word in ("walk.state =", ".s.state =", "rayCacheValid", "rayPrevSet", "ray.valid =", "ray.prevSet =", "resolvedValid ="):
        assert word not in api, word


def test_walk_and_ray_cache_decide_over_sequences_what_the_text_they_replaced_decided():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_plan_run.restype = C.c_uint64
    H.walk_plan_run.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    H.walk_plan_tally_name.restype = C.c_char_p
    n = H.walk_plan_tallies()
    out = (C.c_uint64 * n)()
    bad = H.walk_plan_run(SEED, SEQUENCES, STEPS, out)
    t = {H.walk_plan_tally_name(i).decode(): int(out[i]) for i in range(n)}
    assert bad == 0 and t["bad"] == 0, t
    assert t["steps"] == SEQUENCES * STEPS
    assert 0 < t["refused"] < t["steps"]
    _check_coverage(t)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_PLAN_MAIN"])
    r = subprocess.run([exe, str(SEQUENCES // 10), str(STEPS)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    t = {ln.split()[0]: int(ln.split()[1]) for ln in r.stdout.splitlines()}
    assert t["bad"] == 0 and t["steps"] == SEQUENCES // 10 * STEPS and 0 < t["refused"] < t["steps"]
    _check_coverage(t)
