"""VRC_OPT_WALK_CACHE on the GPU: a view that stands still over an unchanged node list walks the brick grid once.  Frames
that load their rays (VRC_OPT_RAY_CACHE_USED = 2) count the longest list (mode 1), record every ray's visits (mode 3;
mode 2 while the count is on its way) and from then on march from the lists (mode 4) with vrc_k_raycast_replay;
VRC_OPT_WALK_CACHE_USED says which the last vrc_render did.  The replayed march receives the same bricks, intervals and
distances in the same order, so every frame and sample count equals the frame of a context with the option off, bit for
bit -- no tolerance appears here.  Every comparison of a replayed frame first asserts that mode 4 was reached: a run that
never replays fails.  The option-0 frames are what tests/test_ray_cache.py and tests/test_gpu_parity.py hold to the
oracle.  (GpuScene.render ends in a synchronising read-back, so the count has always arrived by the next frame: from a
fresh view the modes read 0, 0, 1, 3, 4, 4; mode 2 is seen by the one test that renders without reading back.)

With the option at 1 a view most of whose visits gather voxels is counted and then left on the walk, because the replay
gains nothing there; the contexts of the tests that hold the replay to the walk on such volumes (hash, mixed) therefore
set VRC_WALK_CACHE_ALWAYS, and the tests at the end are about the choice at 1."""
import copy
import ctypes as C

import numpy as np
import pytest

import orc
from test_uniform_bricks_cpu import assert_split, mixed_volume

pytestmark = pytest.mark.gpu

VOXELS, BLOCK = (64, 64, 64), 16
VIEWPORT = (100, 76)  # 13 x 10 tiles of 8 x 8: partial tiles on both edges
FRESH = (0, 0, 1, 3, 4, 4)  # rays computed, rays stored, rays loaded + count pass, record pass, replayed, replayed
RESTART = (1, 3, 4)  # the rays stay loaded, only the lists start over
NEW_NODES = (0, 1, 3, 4)  # ... and a node list has to repeat before it is counted


@pytest.fixture(scope="module")
def vrc():
    from libre_amd import vrc as v
    v.load_library()  # fails loudly when the HIP extension is missing
    return v


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    return h


def _gpu(s):
    from gpu_run import GpuScene
    return GpuScene(s)


def _opt(vrc, g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _get(vrc, g, option):
    v = C.c_int64(-1)
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, option, C.byref(v)))
    return int(v.value)


def mode(vrc, g):
    return _get(vrc, g, vrc.OPT_WALK_CACHE_USED)


def table(alpha, coloured):
    tf = orc.linear_ramp_tf(alpha)
    if coloured:  # red, green and blue differ: the four-float table and colours
        tf[:, 1] = tf[::-1, 1]
        tf[:, 2] *= np.float32(0.5)
    return np.ascontiguousarray(tf)


_scenes = {}


def scene(volume="mem", spin=(0.5, 0.35), spr=256, **kw):
    key = (volume, spin, spr, repr(sorted(kw.items())))
    if key not in _scenes:
        vol = mixed_volume() if volume == "mixed" else volume
        _scenes[key] = orc.build_scene(voxels=VOXELS, block=BLOCK, viewport=VIEWPORT, volume=vol, spin=spin, spr=spr, **kw)
    return copy.copy(_scenes[key])  # (tf, planes and view are replaced, never written in place)


def same(got, want, what, counted=True):
    (fb, n), (wfb, wn) = got, want
    assert np.array_equal(fb, wfb), "%s: %d pixels differ" % (what, int((fb != wfb).any(axis=-1).sum()))
    if counted:
        assert n == wn and n > 0, (what, n, wn)


def frame(vrc, g, **kw):
    fb, n, st = g.render(**kw)
    return (fb, n), mode(vrc, g), st


def steady(vrc, g, ref, what, expect=FRESH, **kw):
    """Frames of g (option on) reading the modes of `expect`, each equal to the frame of ref (option off)."""
    want, m, st_ref = frame(vrc, ref, **kw)
    assert m == 0, what
    seen = []
    for i, e in enumerate(expect):
        got, m, st = frame(vrc, g, **kw)
        seen.append(m)
        assert m == e, "%s: frame %d read mode %d, modes so far %r, expected %r" % (what, i, m, seen, expect)
        assert st.kernel_variant == st_ref.kernel_variant and (m == 0 or st.kernel_variant == vrc.KERNEL_GRID_DDA), what
        replayed = b"vrc_k_raycast_replay<" in g.L.vrc_last_kernel()
        assert replayed == (m == 4), (what, m, g.L.vrc_last_kernel())
        same(got, want, "%s frame %d (mode %d)" % (what, i, m), counted=kw.get("count", True))
    return want


def always(vrc, g):
    _opt(vrc, g, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS)


def off(vrc, ref, g):
    """ref walks every frame; g replays whatever the bricks hold."""
    _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
    always(vrc, g)


def start_over(vrc, g):
    _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
    always(vrc, g)


@pytest.mark.parametrize("spr", [256, 300])  # the counted form of the uniform march, and its float chain
@pytest.mark.parametrize("spin", [(0.0, 0.0), (0.5, 0.35)])
@pytest.mark.parametrize("volume", ["mem", "hash", "mixed"])
def test_every_frame_on_the_way_to_the_replay_and_after_is_the_walked_one(vrc, volume, spin, spr):
    s = scene(volume, spin, spr)
    assert s.render.samplesPerRay == spr
    if volume == "mixed":
        assert_split(s)
    with _gpu(s) as g, _gpu(s) as ref:
        off(vrc, ref, g)
        expect = FRESH
        for alpha in (0.05, 1.0):
            for coloured in (False, True):
                g.s.tf = ref.s.tf = table(alpha, coloured)
                what = "%s spin %r spr %d alpha %g coloured %d" % (volume, spin, spr, alpha, coloured)
                (fb, _n) = steady(vrc, g, ref, what, expect=expect)
                assert fb[..., 3].max() > 0.05 and (fb[..., 3] == 0.0).any(), what  # rays that hit and rays that miss
                if alpha == 1.0:
                    assert fb[..., 3].max() > 0.999, what  # early ray termination
                # without the sample counter: another kernel instance, the same lists
                steady(vrc, g, ref, what + " uncounted", expect=(4, 4), count=False)
                start_over(vrc, g)
                expect = RESTART
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) > 0
        assert _get(vrc, ref, vrc.OPT_WALK_CACHE_BYTES) == 0


@pytest.mark.parametrize("volume", ["mem", "hash", "mixed"])
@pytest.mark.parametrize("first,then", [(1.0, 0.05), (0.05, 1.0)])
def test_lists_recorded_under_one_transfer_function_serve_another(vrc, volume, first, then):
    # the test this design exists for: a list is complete whatever ended the rays of the frame it was recorded in
    s = scene(volume)
    with _gpu(s) as g, _gpu(s) as ref:
        off(vrc, ref, g)
        g.s.tf = ref.s.tf = table(first, False)
        fb, _ = steady(vrc, g, ref, "%s recorded under alpha %g" % (volume, first))
        assert (fb[..., 3].max() > 0.999) == (first == 1.0)
        for coloured in (False, True):
            g.s.tf = ref.s.tf = table(then, coloured)
            fb, _ = steady(vrc, g, ref, "%s replayed under alpha %g coloured %d" % (volume, then, coloured), expect=(4, 4))
            assert (fb[..., 3].max() > 0.999) == (then == 1.0)
            steady(vrc, g, ref, "%s ... uncounted" % volume, expect=(4,), count=False)


def test_what_changes_the_lists_starts_over_and_what_does_not_keeps_them(vrc, hip):
    s = scene("mixed")
    s.tf = table(0.3, False)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    with _gpu(s) as g, _gpu(s) as ref:
        off(vrc, ref, g)
        steady(vrc, g, ref, "start")

        def both(fn):
            fn(g)
            fn(ref)

        # a camera move: mode 0 (and nothing but the walk), then the sequence again
        moved = scene("mixed", spin=(0.2, 0.1))
        moved.tf = s.tf
        both(lambda x: setattr(x, "s", copy.copy(moved)))
        a = steady(vrc, g, ref, "camera")
        # clip planes (the rays change with them)
        clipped = copy.copy(moved)
        clipped.planes = np.ascontiguousarray([[0.6, 0.0, 0.8, 0.2], [0.0, 1.0, 0.0, 0.3]], dtype=np.float32)
        both(lambda x: setattr(x, "s", copy.copy(clipped)))
        b = steady(vrc, g, ref, "clip planes")
        assert not np.array_equal(a[0], b[0])
        # a changed node list (the same bricks in another order): the rays stay loaded, the lists start over
        shuffled = copy.copy(clipped)
        n = shuffled.n_nodes
        nodes = (type(shuffled.nodes[0]) * n)(*[shuffled.nodes[(i + 5) % n] for i in range(n)])
        shuffled.nodes = nodes
        both(lambda x: setattr(x, "s", copy.copy(shuffled)))
        steady(vrc, g, ref, "node list", expect=NEW_NODES)
        both(lambda x: setattr(x, "s", copy.copy(clipped)))
        steady(vrc, g, ref, "node list back", expect=NEW_NODES)
        # node lists that alternate (passes over different subsets, bricks streaming in) never repeat: nothing is
        # counted, nothing recorded, until one of them stays
        for i in range(3):
            for scn in (shuffled, clipped):
                both(lambda x: setattr(x, "s", copy.copy(scn)))
                steady(vrc, g, ref, "alternating node lists, round %d" % i, expect=(0,))
        steady(vrc, g, ref, "the node list stays", expect=RESTART)
        # row bands
        rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
        banded = copy.copy(clipped)
        banded.H = len(rows)

        def bands(x):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows.ctypes.data, len(rows)))
            x.s = copy.copy(banded)
        both(bands)
        d = steady(vrc, g, ref, "row bands")
        assert np.array_equal(d[0], b[0][rows])

        def unbanded(x):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, None, 0))
            x.s = copy.copy(clipped)
        both(unbanded)
        steady(vrc, g, ref, "no row bands")
        # another stream
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, stream))
        steady(vrc, g, ref, "stream")
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, None))
        steady(vrc, g, ref, "own stream")
        # each option
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        steady(vrc, g, ref, "option off", expect=(0, 0, 0))
        always(vrc, g)
        steady(vrc, g, ref, "option on", expect=RESTART)
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_CACHE, 3) == vrc.VRC_EINVAL
        _opt(vrc, g, vrc.OPT_RAY_CACHE, 0)
        steady(vrc, g, ref, "ray cache off", expect=(0, 0, 0))
        _opt(vrc, g, vrc.OPT_RAY_CACHE, 1)
        steady(vrc, g, ref, "ray cache on")
        # what the lists do not depend on keeps mode 4: the transfer function, VRC_OPT_UNIFORM_BRICKS (this context
        # replays whatever the bricks hold), the grey table
        for alpha, coloured in ((0.3, True), (1.0, False)):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            steady(vrc, g, ref, "transfer function alpha %g coloured %d" % (alpha, coloured), expect=(4, 4))
        for v in (0, 1):
            both(lambda x: _opt(vrc, x, vrc.OPT_UNIFORM_BRICKS, v))
            steady(vrc, g, ref, "uniform bricks %d" % v, expect=(4, 4))
        for v in (0, 1):
            both(lambda x: _opt(vrc, x, vrc.OPT_GREY_TABLE, v))
            steady(vrc, g, ref, "grey table %d" % v, expect=(4, 4))
        # the GL variant: its own intervals (lattice snap, clip planes per brick), its own lists
        steady(vrc, g, ref, "gl variant", variant=1)
        steady(vrc, g, ref, "cuda variant again", variant=0)
        # frames outside the instance set walk, and read 0
        for kw in (dict(filter_mode=1, kernel=vrc.KERNEL_GRID_DDA), dict(stepping=0), dict(kernel=vrc.KERNEL_REFERENCE_ORDER),
                   dict(kernel=vrc.KERNEL_LDS)):
            steady(vrc, g, ref, "not eligible: %r" % kw, expect=(0, 0, 0, 0), **kw)
        steady(vrc, g, ref, "eligible again")
    assert hip.hipStreamDestroy(stream) == 0


def test_a_budget_too_small_stays_on_the_walk_for_good(vrc):
    s = scene("hash")
    s.tf = table(0.3, False)
    plane = 13 * 10 * 64 * 4  # bytes of one plane: whole tiles
    with _gpu(s) as g, _gpu(s) as ref:
        off(vrc, ref, g)
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BUDGET) == 512 << 20
        # not even one visit per ray fits: nothing is counted
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, 5 * plane - 1)
        steady(vrc, g, ref, "no visit fits", expect=(0,) * 6)
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) == 0
        # one visit fits, the longest list does not: counted once, then the walk for good
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, 5 * plane)
        steady(vrc, g, ref, "one visit fits", expect=(1, 0, 0, 0))
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) == 0
        # the default again
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, 512 << 20)
        steady(vrc, g, ref, "default budget", expect=RESTART)
        used = _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES)
        assert used % plane == 0 and (used // plane - 1) % 4 == 0 and used // plane >= 9, used  # 1 + 4 K planes, K >= 2
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_CACHE_BUDGET, -1) == vrc.VRC_EINVAL


def test_a_frame_that_does_not_clear_first(vrc):
    # two vrc_render calls over the same node list in one frame: the second composites onto the first (its pixels are
    # loaded, and the rays the first pass ended stay ended)
    s = scene("mixed")
    passes = [(0, s.n_nodes), (0, s.n_nodes)]
    for alpha in (0.05, 1.0):
        s.tf = table(alpha, False)
        with _gpu(s) as g, _gpu(s) as ref:
            off(vrc, ref, g)
            want, m, _ = frame(vrc, ref, passes=passes)
            once, _, _ = frame(vrc, ref)
            assert m == 0 and (alpha == 1.0 or not np.array_equal(want[0], once[0]))
            seen = []
            for i in range(4):
                got, m, _ = frame(vrc, g, passes=passes)
                seen.append(m)
                same(got, want, "alpha %g frame %d" % (alpha, i))
            assert seen == [0, 3, 4, 4], seen  # (the mode of the frame's second pass: computed + stored, counted + recorded)


def test_two_slots_with_different_cameras_through_the_plugin(vrc):
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
            assert one.get_option(vrc.OPT_WALK_CACHE_USED) == 0 and fb[..., 3].max() > 0.0
            want.append(fb)
    assert not np.array_equal(want[0], want[1])
    with drv.App("mem://#64,64,64,16", 100, 76, **kw) as app:
        app.set_frames_in_flight(2)
        seen = {0: [], 1: []}
        for i in range(12):  # the slots alternate; each is a context with lists of its own
            k = i % 2
            app.select_slot(k)
            app.set_camera(spin=spins[k])
            got, _ = app.render_frame()
            seen[k].append(app.get_option(vrc.OPT_WALK_CACHE_USED))
            assert np.array_equal(got, want[k]), "frame %d" % i
        for k in (0, 1):
            assert seen[k][-1] == 4 and sorted(seen[k]) == seen[k] and seen[k][0] == 0, seen
        # the option reaches every slot
        app.set_option(vrc.OPT_WALK_CACHE, 0)
        for k in (0, 1):
            app.select_slot(k)
            app.set_camera(spin=spins[k])
            got, _ = app.render_frame()
            assert app.get_option(vrc.OPT_WALK_CACHE_USED) == 0 and np.array_equal(got, want[k])


def test_the_count_that_has_not_arrived_reads_2_and_the_frame_walks(vrc, hip):
    # vrc_render never waits for the count: a host function holds the context's stream while three frames are queued, the
    # one that counts and two that ask for the count (GpuScene.render would read back in between)
    import threading
    s = scene("mem")
    s.tf = table(0.3, False)
    gate, entered = threading.Event(), threading.Event()

    @C.CFUNCTYPE(None, C.c_void_p)
    def hold(_):
        entered.set()
        gate.wait(20.0)

    hip.hipLaunchHostFunc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        want, _, _ = frame(vrc, ref)
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, stream))
        steady(vrc, g, ref, "everything allocated")  # (nothing in the held frames may wait for the device)
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 1)
        seen = []
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        assert hip.hipLaunchHostFunc(stream, C.cast(hold, C.c_void_p), None) == 0
        try:
            for _ in range(3):
                vrc.check(L, L.vrc_pre_render(g.ctx, view))
                vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
                seen.append(mode(vrc, g))
        finally:
            gate.set()
        fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
        vrc.check(L, L.vrc_post_render(g.ctx, fb.ctypes.data))
        assert entered.is_set() and seen == [1, 2, 2], seen
        assert np.array_equal(fb, want[0])
        steady(vrc, g, ref, "after the count arrived", expect=(3, 4, 4))
        vrc.check(L, L.vrc_ctx_set_stream(g.ctx, None))
    assert hip.hipStreamDestroy(stream) == 0


def test_at_1_a_view_that_gathers_stays_on_the_walk_and_a_uniform_one_replays(vrc):
    # hash: every brick is mixed, every visit gathers -- counted once, nothing recorded, nothing allocated
    s = scene("hash")
    s.tf = table(0.3, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        assert _get(vrc, g, vrc.OPT_WALK_CACHE) == 1
        steady(vrc, g, ref, "hash at 1", expect=(0, 0, 1, 0, 0, 0))
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) == 0
        always(vrc, g)
        steady(vrc, g, ref, "hash, always", expect=RESTART)
        assert _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES) > 0
    # mem: every brick is uniform -- replayed; with VRC_OPT_UNIFORM_BRICKS = 0 the same bricks gather, and the view is
    # counted again and left on the walk; back at 1 it is counted again and replays
    s = scene("mem")
    s.tf = table(0.3, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        steady(vrc, g, ref, "mem at 1")
        for v, expect in ((0, (1, 0, 0, 0)), (1, RESTART)):
            _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, v)
            _opt(vrc, ref, vrc.OPT_UNIFORM_BRICKS, v)
            steady(vrc, g, ref, "mem at 1, uniform bricks %d" % v, expect=expect)
        # a brick upload into the pool may change what gathers: the view is counted again once the pool is quiet
        # (here the last brick goes into its own slot again)
        nid = s.ids[-1]
        brick = np.ascontiguousarray(s.bricks[nid])
        size = vrc.u32x3(brick.shape[2], brick.shape[1], brick.shape[0])
        for x in (g, ref):
            slot = vrc.f32x3()
            vrc.check(x.L, x.L.vrc_pool_release_slot(x.pool, vrc.f32x3(*x.slots[nid])))
            vrc.check(x.L, x.L.vrc_pool_copy_to_slot(x.pool, brick.ctypes.data, size, slot))
            assert (slot[0], slot[1], slot[2]) == x.slots[nid]
        steady(vrc, g, ref, "mem at 1, after an upload", expect=NEW_NODES)
