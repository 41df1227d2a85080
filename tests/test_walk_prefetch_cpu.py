"""The unconditional reads of the lean replay on the host build of the per-ray code (no GPU needed).

vrc_pixel_walk_replay_lean asks for the list word of visit min(k + 2, walkK - 1) and for the slot word of visit k + 1 in
every visit k, and for the words of its first two visits before it has looked at the ray's count: no load of the uniform
path stands under a branch, so that the compiled loop can leave them in flight across the march.  That is only right
if every such read stays inside what the host allocates.  tests/cpu_harness/walk_prefetch_harness.cpp replays lists
whose allocation is exactly (1 + 4 K) P words over a slotInfo of exactly walkSlots words, for K = 1, 2, 3, every count
from 0 to K (so rays whose count equals K, and lists with unrecorded words behind the count), and the slot index as
recorded, 0, on the last word of slotInfo, beyond walkSlots, and without slotInfo; each replay is compared, colour bits
and sample count, with vrc_pixel_walk_replay from the other form of the same list.  Run plain, and as a stand-alone
program under the address and undefined-behaviour sanitizers: that run is what proves the reads stay inside the
allocations."""
import ctypes as C
import os
import subprocess

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "walk_prefetch_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libwalk_prefetch_harness.so")
SAN = os.path.join(HERE, "cpu_harness", "walk_prefetch_san")
DEPS = [SRC] + [os.path.join(HERE, "cpu_harness", n) for n in ("walk_lean_harness.cpp", "walk_cache_harness.cpp")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", n) for n in ("vrc_core.h", "vrc_tables.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I",
         os.path.join(orc.ROOT, "include")]

LISTS, REPLAYS, FULL, EMPTY, LAST, BEYOND, BAD = range(7)
PER = 20


def _build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def _check(t, per):
    assert t[BAD] == 0, t
    assert 0 < t[LISTS] <= per * 3 * 2 * 7, t  # rays that met a brick
    # per list at least: K = 1, counts 0 and 1, two and five set-ups of the index, three tables
    assert t[REPLAYS] >= t[LISTS] * (2 + 5) * 3, t
    assert t[FULL] > 0 and t[EMPTY] > 0 and t[FULL] + t[EMPTY] < t[REPLAYS], t  # count = K, 0, and in between
    assert t[LAST] > 0 and t[BEYOND] == t[LAST], t


def test_reads_past_the_count_and_clamped_slot_indices_leave_the_replay_what_it_was():
    H = C.CDLL(_build(OUT, ["-fPIC", "-shared"]))
    H.walk_prefetch_run.restype = C.c_uint64
    H.walk_prefetch_run.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 7)()
    bad = H.walk_prefetch_run(2025, PER, out)
    t = list(out)
    print("lists %d replays %d full %d empty %d last %d beyond %d mismatches %d" % tuple(t))
    assert bad == 0, t
    _check(t, PER)


def test_the_same_as_a_stand_alone_program_under_the_sanitizers():
    exe = _build(SAN, ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-DWALK_PREFETCH_MAIN"])
    r = subprocess.run([exe, str(PER // 2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("lists ")]
    assert len(words) == 1
    _check([int(words[0][i]) for i in (1, 3, 5, 7, 9, 11, 13)], PER // 2)
