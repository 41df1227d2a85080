"""The per-slot words without a GPU: the key functions of libre_amd/csrc/vrc_core.h in a host build
(tests/cpu_harness/slot_words_harness.cpp) against NumPy, and the conditions under which the sample counts of
tests/test_slot_words.py, and the count windows tests/test_mip.py, test_fold.py and test_iso.py assert for the scenes
"skip" and "skip16", say what they claim to say (tests/slot_words.py, tests/skip_window.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import skip_window
import slot_words as sw

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "slot_words_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libslot_words_harness.so")
RAISE, LOWER, REACH_MAX, REACH_MIN = range(4)
_H = None


def harness():
    global _H
    if _H is None:
        deps = [SRC, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (OUT, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, OUT)
        _H = C.CDLL(OUT)
        _H.slot_words_ask_integer.restype = C.c_int
        _H.slot_words_ask_float.restype = C.c_int
    return _H


def float_keys(v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    kmax, kmin = np.zeros(v.size, dtype=np.uint32), np.zeros(v.size, dtype=np.uint32)
    bmax, bmin = np.zeros(v.size, dtype=np.float32), np.zeros(v.size, dtype=np.float32)
    harness().slot_words_float_keys(C.c_void_p(v.ctypes.data), C.c_uint32(v.size), C.c_void_p(kmax.ctypes.data),
                                    C.c_void_p(kmin.ctypes.data), C.c_void_p(bmax.ctypes.data), C.c_void_p(bmin.ctypes.data))
    return kmax, kmin, bmax, bmin


def ask_integer(question, atlas_bytes, word, m):
    r = harness().slot_words_ask_integer(C.c_int(question), C.c_uint32(atlas_bytes), C.c_uint32(int(word)), C.c_uint32(int(m)))
    assert r in (0, 1)
    return bool(r)


def ask_float(question, atlas_bytes, trilinear, word, m):
    r = harness().slot_words_ask_float(C.c_int(question), C.c_uint32(atlas_bytes), C.c_int(int(trilinear)),
                                       C.c_uint32(int(word)), C.c_float(float(m)))
    assert r in (0, 1)
    return bool(r)


F = np.float32
DEN = F(1e-45)
#: sorted: every float order a key has to keep, the zeros and the denormals included
SORTED = np.array([-np.inf, -sw.FLT_MAX, -1.0, -DEN, -0.0, 0.0, DEN, 1.0, sw.FLT_MAX, np.inf], dtype=np.float32)


# ---- the keys -------------------------------------------------------------------------------------------------------------
def test_the_maximum_key_orders_as_the_floats_do_and_is_never_zero():
    kmax, _, _, _ = float_keys(SORTED)
    assert (np.diff(kmax.astype(np.int64)) > 0).all(), kmax  # strictly: -0.0 lies below +0.0, as their bits do
    assert (kmax != 0).all()
    assert (kmax == sw.max_key(SORTED)).all()
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = v[~np.isnan(v)]
    k = float_keys(v)[0]
    assert (k != 0).all() and (k == sw.max_key(v)).all()
    order = np.argsort(k, kind="stable")
    assert (np.diff(v[order].astype(np.float64)) >= 0).all()  # sorted by key = sorted as numbers (float64 holds a float32)
    # (only a number has such a key: the all-ones NaN maps to 0 and the positive NaNs above +infinity's key, which is why
    # the upload leaves a NaN out before it asks -- vrc_voxel_max_key; tests/test_slot_words.py has the bricks for it)
    assert k.max() <= float_keys([np.inf])[0][0] and k.min() >= float_keys([-np.inf])[0][0]


def test_the_inverse_gives_the_float_back_bit_for_bit():
    rng = np.random.default_rng(2)
    v = np.concatenate([SORTED, rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    v = v[~np.isnan(v)]
    _, _, bmax, bmin = float_keys(v)
    assert np.array_equal(bmax.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(bmin.view(np.uint32), v.view(np.uint32))


def test_the_minimum_key_is_the_mirror():
    kmax, kmin, _, _ = float_keys(SORTED)
    assert (np.diff(kmin.astype(np.int64)) < 0).all()  # the smallest float has the largest key
    assert (kmin != 0).all()
    assert (kmin == float_keys(-SORTED)[0]).all()  # the key of the negated voxel
    stored = np.arange(65536, dtype=np.uint32)
    key, back = np.zeros_like(stored), np.zeros_like(stored)
    harness().slot_words_stored_keys(C.c_void_p(stored.ctypes.data), C.c_uint32(stored.size), C.c_void_p(key.ctypes.data),
                                     C.c_void_p(back.ctypes.data))
    assert (key == (0xFFFFFFFF - stored.astype(np.uint64)).astype(np.uint32)).all()
    assert (key != 0).all() and (np.diff(key.astype(np.int64)) < 0).all() and (back == stored).all()


# ---- the three questions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atlas_bytes,top", [(1, 255), (2, 65535)])
def test_an_integer_maximum_answers_as_the_header_says(atlas_bytes, top):
    """word = the largest stored value + 1.  No sample can raise M iff M >= the largest; none can reach M iff M > it."""
    for largest in (0, 1, 100, top - 1, top):
        word = largest + 1
        for m in (largest - 1, largest, largest + 1):
            if m < 0:
                continue
            assert ask_integer(RAISE, atlas_bytes, word, m) == (m >= largest), (largest, m)
            assert ask_integer(REACH_MAX, atlas_bytes, word, m) == (m > largest), (largest, m)
            for tri in (0, 1):  # a float M of the same atlas; trilinear: the margin max + |max| * 1e-6, float32
                bound = F(largest) + np.abs(F(largest)) * F(1e-6) if tri else F(largest)
                for fm in (F(m), np.nextafter(bound, F(-np.inf)), bound, np.nextafter(bound, F(np.inf))):
                    assert ask_float(RAISE, atlas_bytes, tri, word, fm) == bool(fm >= bound), (largest, fm, tri)
                    assert ask_float(REACH_MAX, atlas_bytes, tri, word, fm) == bool(fm > bound), (largest, fm, tri)
                assert 0.0 <= float(bound) - largest <= 1e-6 * largest + float(np.spacing(F(largest)))  # (the margin, rounded once)


@pytest.mark.parametrize("atlas_bytes,top", [(1, 255), (2, 65535)])
def test_an_integer_minimum_answers_as_the_header_says(atlas_bytes, top):
    """word = the complement of the smallest stored value.  No sample can lower M iff M <= the smallest; none can reach
    M iff M < it."""
    for smallest in (0, 1, 100, top - 1, top):
        word = 0xFFFFFFFF - smallest
        for m in (smallest - 1, smallest, smallest + 1):
            if m < 0:
                continue
            assert ask_integer(LOWER, atlas_bytes, word, m) == (m <= smallest), (smallest, m)
            assert ask_integer(REACH_MIN, atlas_bytes, word, m) == (m < smallest), (smallest, m)
            for tri in (0, 1):
                bound = F(smallest) - np.abs(F(smallest)) * F(1e-6) if tri else F(smallest)
                for fm in (F(m), np.nextafter(bound, F(-np.inf)), bound, np.nextafter(bound, F(np.inf))):
                    assert ask_float(LOWER, atlas_bytes, tri, word, fm) == bool(fm <= bound), (smallest, fm, tri)
                    assert ask_float(REACH_MIN, atlas_bytes, tri, word, fm) == bool(fm < bound), (smallest, fm, tri)


@pytest.mark.parametrize("trilinear", [0, 1])
def test_a_float_word_answers_as_the_header_says(trilinear):
    """The float atlas: the words are keys, the comparisons are made on the floats they stand for -- at the word's own
    float, at the floats whose keys are word - 1 and word + 1, and around the trilinear margin."""
    values = [v for v in SORTED if np.isfinite(v)] + [F(-0.5), F(0.3), F(123456.0)]
    for x in values:
        x = F(x)
        kmax, kmin = float_keys([x])[0][0], float_keys([x])[1][0]
        with np.errstate(over="ignore"):  # (the margin of FLT_MAX is +infinity, and so is the float after it)
            up = F(x) + np.abs(x) * F(1e-6) if trilinear else x   # float32 throughout, each operation rounded
            down = F(x) - np.abs(x) * F(1e-6) if trilinear else x
            around = {x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf)), up, down,
                      np.nextafter(up, F(np.inf)), np.nextafter(up, F(-np.inf)),
                      np.nextafter(down, F(np.inf)), np.nextafter(down, F(-np.inf)), F(-np.inf), F(np.inf)}
        for m in around:
            what = (float(x), float(m), trilinear)
            assert ask_float(RAISE, 4, trilinear, kmax, m) == bool(m >= up), what
            assert ask_float(REACH_MAX, 4, trilinear, kmax, m) == bool(m > up), what
            assert ask_float(LOWER, 4, trilinear, kmin, m) == bool(m <= down), what
            assert ask_float(REACH_MIN, 4, trilinear, kmin, m) == bool(m < down), what
    # the zeros are one number: a maximum of -0.0 is reached by an M of +0.0 and the other way round
    for a, b in ((F(-0.0), F(0.0)), (F(0.0), F(-0.0))):
        assert ask_float(RAISE, 4, 0, float_keys([a])[0][0], b) and not ask_float(REACH_MAX, 4, 0, float_keys([a])[0][0], b)
    # an all-NaN brick leaves the key of -infinity (of +infinity for the minimum): every M, finite or not, settles it
    ninf = float_keys([F(-np.inf)])[0][0]
    assert ask_float(RAISE, 4, 0, ninf, F(-3e38)) and ask_float(REACH_MAX, 4, 0, ninf, F(-3e38))
    assert ask_float(RAISE, 4, 0, ninf, F(-np.inf)) and not ask_float(REACH_MAX, 4, 0, ninf, F(-np.inf))


# ---- the scenes of tests/slot_words.py -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sw.GEOMETRIES))
def test_the_reference_leaves_no_sample_in_doubt_and_reads_no_extremum(name):
    g = sw.geometry(name)
    for what, r in [("all", g.ref)] + [("node %d" % k, g.per_node[nid]) for k, nid in enumerate(g.ids)]:
        assert (r.counts_lo == r.counts_hi).all() and (r.counts == r.counts_lo).all(), (name, what)
        # the mask brick is 1 where a test puts an extremum: no sample reads such a voxel, not even a doubtful one
        assert r.m[r.certain].max() == 0.0 and not r.extra, (name, what)
        assert not (r.maybe & ~r.certain).any()
    n, rays = int(g.ref.counts.sum()), int((g.ref.counts > 0).sum())
    print("%s: %d samples on %d rays of %d" % (name, n, rays, g.W * g.H))
    assert rays >= 100 and n >= 3000
    if len(g.ids) == 2:
        front, back = (g.per_node[nid].counts for nid in g.ids)
        assert (front + back == g.ref.counts).all()
        # front then back along EVERY ray: no ray meets the back brick without a sample in the front one
        assert not ((front == 0) & (back > 0)).any() and (back > 0).sum() >= 100
        assert sw.expected_two(g, False) == int(front.sum()) < sw.expected_two(g, True) == n


@pytest.mark.parametrize("name", ["whole", "two_whole"])
def test_no_trilinear_tap_reads_an_extremum_either(name):
    """The one trilinear case per probe (tests/test_slot_words.py): the same counts, and with an overlap of 4 the taps,
    half a voxel further out, stay clear of the planted voxels too."""
    g = sw.geometry(name)
    r, per_node = sw.trilinear_ref(name)
    assert (r.counts_lo == r.counts_hi).all() and (r.counts == g.ref.counts).all()
    assert r.m[r.certain].max() == 0.0 and not r.extra
    for nid in g.ids:
        assert (per_node[nid].counts == g.per_node[nid].counts).all() and per_node[nid].m[per_node[nid].certain].max() == 0.0


@pytest.mark.parametrize("name", sorted(sw.GEOMETRIES))
def test_every_extremum_lies_in_the_overlap(name):
    g = sw.geometry(name)
    ov = [g.vi.overlap[a] for a in range(3)]
    for nid in g.ids:
        sz, sy, sx = g.shape[nid]
        for x, y, z in sw.positions(g.shape[nid], True).values():
            assert x < sx and y < sy and z < sz
            assert any(p < ov[a] or p >= n - ov[a] for a, (p, n) in enumerate(((x, sx), (y, sy), (z, sz))))
    lanes = [p for k, p in sw.positions(g.shape[g.ids[0]], True).items() if k.startswith("lane")]
    assert sorted(p[0] % 8 for p in lanes) == list(range(8)) and len({p[0] // 8 for p in lanes}) == 1


def test_the_big_brick_needs_the_grid_stride_tail():
    """grid_for caps the repack's grid at 2048 * 4 workgroups of 256 threads: the last voxel of a 136^3 brick is moved
    by a thread's second trip."""
    g = sw.geometry("big")
    sz, sy, sx = g.shape[g.ids[0]]
    assert (sx, sy, sz) == (136, 136, 136) == tuple(g.slot_dim)
    assert sx * sy * sz > 2048 * 4 * 256


@pytest.mark.parametrize("tname", sorted(sw.TYPES))
def test_the_planted_values_stand_clear_of_the_noise(tname):
    shape = (6, 5, 4)
    hi = sw.max_noise(tname, shape).astype(np.float64).max()
    for v in sw.maxima(tname):
        assert float(sw.stored_float(tname, v)) > hi
        assert sw.next_above(tname, v) > sw.iso_of(tname, v)
    for fold in (sw.vrc.MIP_FOLD_MAX, sw.vrc.MIP_FOLD_MIN):
        noise = sw.back_noise(tname, shape, fold).astype(np.float64)
        for a, ext, marched in sw.fold_cases(tname, fold):
            a, ext = float(sw.stored_float(tname, a)), float(sw.stored_float(tname, ext))
            if fold == sw.vrc.MIP_FOLD_MIN:
                assert noise.min() > ext or noise.min() >= a >= ext
                assert marched == (ext < a)
            else:
                assert noise.max() < ext or noise.max() <= a <= ext
                assert marched == (ext > a)
    if tname == "uint32":
        assert sw.iso_of(tname, 2 ** 32 - 1) == 2.0 ** 32 and sw.iso_of(tname, 16777217) == 16777216.0


# ---- the count windows of tests/skip_window.py -----------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [skip_window.DDA, skip_window.REFORDER])
@pytest.mark.parametrize("fold", [skip_window.MAX, skip_window.MIN, "iso"])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_the_predicted_window_is_honest(name, fold, loop):
    """A window proves something only if it is narrow and lies below the count without skipping; and the rays on which
    float64 is in doubt -- a sample it cannot call taken, two bricks entered at one distance -- stay within mip_ref's
    cap of 5 % of the hit rays."""
    w = skip_window.iso_of(name, loop) if fold == "iso" else skip_window.of(name, fold, loop)
    saving = w.off_lo - w.hi
    print("%s %s %s: %d .. %d with skipping (width %d), %d .. %d without; saving at least %d; %d doubtful rays of %d hit" % (
        name, fold, loop, w.lo, w.hi, w.hi - w.lo, w.off_lo, w.off_hi, saving, int(w.doubtful.sum()), int(w.hit.sum())))
    assert w.hi < w.off_lo
    assert w.hi - w.lo <= 0.1 * saving
    assert int(w.doubtful.sum()) <= 0.05 * int(w.hit.sum())
    if fold != "iso":  # (an isosurface ray that hits has a window of its own: the group it leaves behind)
        assert ((w.ray_lo == w.ray_hi) | w.doubtful).all()


@pytest.mark.parametrize("loop", [skip_window.DDA, skip_window.REFORDER])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_the_host_build_counts_inside_the_window_ray_by_ray(name, loop):
    """The kernels' own per-ray code, built for the host over words that are right by construction: every ray's count
    lies in the ray's window, with uniform bricks folded and marched; the minimum's frame total in its window."""
    import fold_ref
    import mip_scenes
    s = mip_scenes.get(name)
    form = (mip_scenes.GRID | mip_scenes.FIXED) if loop == skip_window.DDA else 0
    w = skip_window.of(name, skip_window.MAX, loop)
    for extra in (mip_scenes.SKIP, mip_scenes.SKIP | mip_scenes.UNIFORM):
        each = np.zeros((s.H, s.W), dtype=np.int64)
        _, n = mip_scenes.harness_render(s, form | extra, per_pixel=each)
        assert ((w.ray_lo <= each) & (each <= w.ray_hi)).all() and w.lo <= n <= w.hi
    w = skip_window.of(name, skip_window.MIN, loop)
    n = fold_ref.harness_render(fold_ref.complemented_scene(name), form | mip_scenes.SKIP | mip_scenes.UNIFORM, fold_ref.FOLD_MIN)[1]
    assert w.lo <= n <= w.hi
    import iso_ref
    w = skip_window.iso_of(name, loop)
    for extra in (mip_scenes.SKIP, mip_scenes.SKIP | mip_scenes.UNIFORM):
        n = iso_ref.harness_render(iso_ref.scene(name), form | extra, iso_ref.ISO[name])[1]
        assert w.lo <= n <= w.hi
