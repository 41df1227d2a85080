"""The lean form of the walk cache's lists on the GPU (VRC_OPT_WALK_LEAN_USED; include/vrc_hip.h).

Where the step size is a power of two, the pool has fewer than 2^20 slots and no visit takes 4096 samples or more, the
record pass stores `n << 20 | slotInfoIndex` where the other form stores the segment's length, and the replay is the
lean instance (vrc_last_kernel: vrc_k_raycast_replay<...,lean>).  Nothing of the result may change: every frame here --
on the way to the replay and in it -- and every sample count equals, bit for bit, the frame of a context with
VRC_OPT_WALK_CACHE = 0, which tests/test_ray_cache.py and tests/test_gpu_parity.py hold to the oracle.  No tolerance
appears.  Every frame also asserts what VRC_OPT_WALK_LEAN_USED reads: 1 exactly on the replayed frames of a lean-able
view (and then the kernel's name says lean), 0 everywhere else.

Shapes and helpers are those of tests/test_walk_cache.py: a viewport of 13 x 10 tiles with partial tiles on both edges,
64^3 voxels in bricks of 16^3 (two groups of 32 samples across a brick at 256 samples per ray, four at 512, and every
remainder where a ray clips a brick's corner).  What crosses the early-exit threshold where -- inside a group, inside a
remainder, on a group's last sample -- is enumerated sample by sample on the host build (tests/test_walk_lean_cpu.py);
here opaque and half-opaque tables over two camera angles put crossings into both."""
import copy

import numpy as np
import pytest

import orc
from test_uniform_bricks_cpu import assert_split
from test_walk_cache import FRESH, RESTART, VIEWPORT, VOXELS, _get, _gpu, _opt, frame, off, scene, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu


def lean_used(vrc, g):
    return _get(vrc, g, vrc.OPT_WALK_LEAN_USED)


def same(got, want, what, counted):
    (fb, n), (wfb, wn) = got, want
    assert np.array_equal(fb, wfb), "%s: %d pixels differ" % (what, int((fb != wfb).any(axis=-1).sum()))
    assert n == wn and (n > 0) == counted, (what, n, wn)


def steady(vrc, g, ref, what, expect=FRESH, lean=1, **kw):
    """Frames of g reading the modes of `expect` (None: whatever it reads), each equal to the frame of ref (option off);
    the lean option reads `lean` on the replayed frames and 0 on the others, and the kernel's name agrees."""
    want, m, _ = frame(vrc, ref, **kw)
    assert m == 0 and lean_used(vrc, ref) == 0, what
    for i, e in enumerate(expect):
        got, m, _ = frame(vrc, g, **kw)
        assert e is None or m == e, "%s: frame %d read mode %d, expected %r" % (what, i, m, expect)
        name = g.L.vrc_last_kernel()
        assert (b"vrc_k_raycast_replay<" in name) == (m == 4), (what, m, name)
        if e is not None:
            assert lean_used(vrc, g) == (lean if m == 4 else 0), (what, i, m, lean_used(vrc, g))
        assert name.endswith(b",lean>") == (lean_used(vrc, g) == 1), (what, m, name)
        same(got, want, "%s frame %d (mode %d)" % (what, i, m), kw.get("count", True))
    return want


def banded_volume():
    """Slabs across z, the axis the default camera looks along: two noise bricks, two uniform ones, two noise, two
    uniform (overlap included), so a ray's list alternates between runs that gather and runs that do not."""
    vol = orc.hash_volume(*VOXELS)
    vol[28:52, :, :] = 90
    vol[:20, :, :] = 200
    return vol


# cases 1 and 2: every brick uniform; the counted and the uncounted instances, four-float and grey
@pytest.mark.parametrize("count", [False, True])
@pytest.mark.parametrize("spr", [256, 512])
def test_a_uniform_volume_replays_lean(vrc, spr, count):
    s = scene("mem", (0.5, 0.35), spr)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)  # (g keeps the default, 1)
        expect = FRESH
        for coloured in (False, True):
            g.s.tf = ref.s.tf = table(0.05, coloured)
            what = "mem spr %d count %d coloured %d" % (spr, count, coloured)
            fb, _ = steady(vrc, g, ref, what, expect=expect, count=count)
            assert fb[..., 3].max() > 0.05 and (fb[..., 3] == 0.0).any(), what  # rays that hit and rays that miss
            assert (b"<%s,%d," % (b"true" if count else b"false", 0 if coloured else 3)) in g.L.vrc_last_kernel()
            expect = (4, 4)  # the transfer function changes nothing of the lists


# case 3: runs of uniform bricks and runs of noise in one list, and noise alone
@pytest.mark.parametrize("spin", [(0.0, 0.0), (0.5, 0.35)])
@pytest.mark.parametrize("volume", ["banded", "hash"])
def test_gather_runs_and_uniform_runs_in_one_list(vrc, volume, spin):
    if volume == "banded":
        s = orc.build_scene(voxels=VOXELS, block=16, viewport=VIEWPORT, volume=banded_volume(), spin=spin, spr=256)
        assert_split(s)
    else:
        s = scene(volume, spin, 256)
    with _gpu(s) as g, _gpu(s) as ref:
        off(vrc, ref, g)
        expect = FRESH
        for alpha, coloured in ((0.05, False), (1.0, True), (0.3, False)):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            what = "%s spin %r alpha %g coloured %d" % (volume, spin, alpha, coloured)
            steady(vrc, g, ref, what, expect=expect)
            steady(vrc, g, ref, what + " uncounted", expect=(4,), count=False)
            expect = (4, 4)


# case 4: a step that is no power of two keeps the other form
def test_300_samples_per_ray_is_not_lean(vrc):
    s = scene("mem", (0.5, 0.35), 300)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        for coloured in (False, True):
            g.s.tf = ref.s.tf = table(0.3, coloured)
            steady(vrc, g, ref, "spr 300 coloured %d" % coloured, expect=(4, 4) if coloured else FRESH, lean=0)


# case 5: a visit of 4096 samples or more does not fit the word
def test_a_visit_of_4096_samples_or_more_is_not_lean(vrc):
    s = orc.build_scene(voxels=(32, 32, 32), block=32, viewport=VIEWPORT, volume="mem", spin=(0.5, 0.35), spr=4096)
    assert s.n_nodes == 1 and s.render.samplesPerRay == 4096
    s.tf = table(0.05, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        # (the eye is 1.5 from the middle of a cube of side 1: a ray through the middle travels at least 1 = 4096 steps)
        steady(vrc, g, ref, "one brick, 4096 samples per ray", lean=0)
    # ... and the same brick at 2048 samples per ray does
    s = orc.build_scene(voxels=(32, 32, 32), block=32, viewport=VIEWPORT, volume="mem", spin=(0.5, 0.35), spr=2048)
    s.tf = table(0.05, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        steady(vrc, g, ref, "one brick, 2048 samples per ray", lean=1)


# case 6: early ray termination inside whole groups and inside remainders
@pytest.mark.parametrize("spin", [(0.0, 0.0), (0.5, 0.35)])
def test_opaque_tables_end_rays_inside_groups_and_remainders(vrc, spin):
    s = scene("mem", spin, 256)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        expect = FRESH
        for alpha in (1.0, 0.5, 0.2):
            for coloured in (False, True):
                g.s.tf = ref.s.tf = table(alpha, coloured)
                what = "spin %r alpha %g coloured %d" % (spin, alpha, coloured)
                fb, _ = steady(vrc, g, ref, what, expect=expect)
                if alpha == 1.0:
                    assert fb[..., 3].max() > 0.999, what  # early ray termination
                expect = (4,)


# case 7: the lists do not depend on what ended the rays of the frame they were recorded in
@pytest.mark.parametrize("first,then", [(1.0, 0.05), (0.05, 1.0)])
def test_lists_recorded_under_one_table_serve_the_other(vrc, first, then):
    s = scene("mem")
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        g.s.tf = ref.s.tf = table(first, False)
        fb, _ = steady(vrc, g, ref, "recorded under alpha %g" % first)
        assert (fb[..., 3].max() > 0.999) == (first == 1.0)
        for coloured in (False, True):
            g.s.tf = ref.s.tf = table(then, coloured)
            fb, _ = steady(vrc, g, ref, "replayed under alpha %g coloured %d" % (then, coloured), expect=(4, 4))
            assert (fb[..., 3].max() > 0.999) == (then == 1.0)


# case 8: row bands, and two renderer slots over one pool
def test_row_bands(vrc):
    s = scene("mem")
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        whole = steady(vrc, g, ref, "whole frame")
        for x in (g, ref):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows.ctypes.data, len(rows)))
            x.s = copy.copy(banded)
        part = steady(vrc, g, ref, "row bands")
        assert np.array_equal(part[0], whole[0][rows])


def test_two_renderer_slots_over_one_pool(vrc):
    from libre_amd import driver as drv
    drv.load_library()
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    spins = [(0.5, 0.35), (0.2, 0.1)]
    want = []
    for spin in spins:
        with drv.App("mem://#64,64,64,16", 100, 76, **kw) as one:
            one.set_camera(spin=spin)
            one.set_option(vrc.OPT_WALK_CACHE, 0)
            fb, _ = one.render_frame()
            assert one.get_option(vrc.OPT_WALK_CACHE_USED) == 0 and one.get_option(vrc.OPT_WALK_LEAN_USED) == 0
            want.append(fb)
    with drv.App("mem://#64,64,64,16", 100, 76, **kw) as app:
        app.set_frames_in_flight(2)
        for i in range(12):  # the slots alternate; each is a context with lists of its own
            k = i % 2
            app.select_slot(k)
            app.set_camera(spin=spins[k])
            got, _ = app.render_frame()
            m, lean = app.get_option(vrc.OPT_WALK_CACHE_USED), app.get_option(vrc.OPT_WALK_LEAN_USED)
            assert lean == (1 if m == 4 else 0), (i, m, lean)
            assert np.array_equal(got, want[k]), "frame %d" % i
        assert m == 4 and lean == 1


# case 9: an upload turns a uniform brick into a mixed one between two frames
@pytest.mark.parametrize("option", [1, 2])
def test_an_upload_that_makes_a_uniform_brick_mixed(vrc, option):
    s = scene("mem")
    s.tf = table(0.3, False)
    nid = s.sorted_ids[len(s.sorted_ids) // 2]
    noise = np.random.default_rng(7).integers(30, 230, size=s.bricks[nid].shape, dtype=np.uint8)
    assert noise.shape == s.bricks[nid].shape and noise.dtype == s.bricks[nid].dtype and noise.min() != noise.max()
    size = vrc.u32x3(noise.shape[2], noise.shape[1], noise.shape[0])
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_CACHE, option)
        before = steady(vrc, g, ref, "before the upload")
        for x in (g, ref):
            slot = vrc.f32x3()
            vrc.check(x.L, x.L.vrc_pool_release_slot(x.pool, vrc.f32x3(*x.slots[nid])))
            vrc.check(x.L, x.L.vrc_pool_copy_to_slot(x.pool, noise.ctypes.data, size, slot))
            assert (slot[0], slot[1], slot[2]) == x.slots[nid]
        # at 1 the view is counted again; at 2 the lean lists stay and the visits of that brick gather
        after = steady(vrc, g, ref, "after the upload", expect=(None,) * 5 if option == 1 else (4,) * 3)
        assert not np.array_equal(before[0], after[0])
        assert frame(vrc, g)[1] == 4 and lean_used(vrc, g) == 1


# case 10: lists that do not fit the planes the budget allows are neither lean nor replayed
def test_lists_over_the_budget_stay_on_the_walk(vrc):
    s = scene("mem")
    s.tf = table(0.3, False)
    plane = 13 * 10 * 64 * 4  # bytes of one plane: whole tiles
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, 5 * plane)  # one visit per ray; the longest list has more
        steady(vrc, g, ref, "one visit fits", expect=(0, 0, 1, 0, 0, 0), lean=0)
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) == 0
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, 512 << 20)
        steady(vrc, g, ref, "default budget", expect=RESTART)
