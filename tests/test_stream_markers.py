"""VRC_OPT_STREAM_MARKERS on the GPU.  0 (the default): the dispatch of a timed march that is one launch carries the
second timing event, which is also the render fence, and the stream waits for the pool's uploads once per upload; 1: a wait, two recorded events and a
recorded fence around every march.  Frames and counts are equal bit for bit, the statistics keep their contract, and the
ordering between marches and uploads holds where the per-frame wait and the recorded fence are gone."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vrc():
    from libre_amd import vrc as v
    v.load_library()  # fails loudly when the HIP extension is missing
    return v


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")  # the HIP runtime libvrc_hip.so itself is linked against
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    return h


def _gpu(s):
    from gpu_run import GpuScene
    return GpuScene(s)


def _opt(vrc, g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def scene(**kw):
    kw.setdefault("spin", (0.5, 0.35))
    return orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(64, 64), **kw)


def both(vrc, g, what, count=True, launches=1, **kw):
    """The frame with the markers (1) and without (0): equal frames, counts, kernel form and timed launches."""
    _opt(vrc, g, vrc.OPT_STREAM_MARKERS, 1)
    want, n_want, st_want = g.render(count=count, **kw)
    _opt(vrc, g, vrc.OPT_STREAM_MARKERS, 0)
    got, n_got, st_got = g.render(count=count, **kw)
    assert st_got.kernel_variant == st_want.kernel_variant, what
    assert st_got.kernel_launches == st_want.kernel_launches == launches, what
    assert np.array_equal(got, want), "%s: %d pixels differ" % (what, int((got != want).any(axis=-1).sum()))
    assert n_got == n_want, (what, n_got, n_want)
    if count:
        assert n_got > 0, what
    assert got[..., 3].max() > 0.0, what
    return got


def test_the_option_reads_back_and_defaults_to_off(vrc):
    L = vrc.load_library()
    ctx = C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    v = C.c_int64(-1)
    vrc.check(L, L.vrc_get_option(ctx, vrc.OPT_STREAM_MARKERS, C.byref(v)))
    assert v.value == 0
    vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_STREAM_MARKERS, 1))
    vrc.check(L, L.vrc_get_option(ctx, vrc.OPT_STREAM_MARKERS, C.byref(v)))
    assert v.value == 1
    L.vrc_ctx_destroy(ctx)


@pytest.mark.parametrize("timing", [1, 0])
def test_composite_forms(vrc, timing):
    # (timing 0: nothing is timed, and the pool's own fence is recorded behind the march under either option)
    with _gpu(scene()) as g:
        _opt(vrc, g, vrc.OPT_KERNEL_TIMING, timing)

        def run(what, **kw):
            both(vrc, g, what, launches=1 if timing else 0, **kw)

        for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                for count in (True, False):  # VRC_OPT_COUNT_SAMPLES on and off
                    run("kernel %d grey %d count %d" % (kernel, grey, count), kernel=kernel, count=count)
        _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
        run("trilinear", filter_mode=vrc.FILTER_TRILINEAR)
        run("trilinear by gathers", kernel=vrc.KERNEL_GRID_DDA, filter_mode=vrc.FILTER_TRILINEAR)
        run("LDS", kernel=vrc.KERNEL_LDS)
        run("LDS trilinear", kernel=vrc.KERNEL_LDS, filter_mode=vrc.FILTER_TRILINEAR)
        # the marches of several launches keep their recorded pair
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 4)
        run("ray compaction")
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 0)
        _opt(vrc, g, vrc.OPT_DEPTH_SPLIT, 1)  # (alpha 0.05: early termination cannot occur, the split is taken)
        run("depth split")
        assert "vrc_k_raycast_split" in g.L.vrc_last_kernel().decode()


def test_per_ray_lod(vrc):
    vi = orc.mem_volume_info(64, 64, 64, 16)
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(64, 64), spin=(0.5, 0.35),
                        ids=orc.all_level_ids(vi, None))
    lod = (1.5, orc.world_space_per_pixel(s))
    with _gpu(s) as g:
        both(vrc, g, "per-ray LOD, gathers", kernel=vrc.KERNEL_GRID_DDA, ray_lod=lod)
        both(vrc, g, "per-ray LOD, trilinear", filter_mode=vrc.FILTER_TRILINEAR, ray_lod=lod)


@pytest.mark.parametrize("fold", [0, 1, 2])
def test_mip_with_each_fold(vrc, fold):
    with _gpu(scene(volume="hash")) as g:
        _opt(vrc, g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        _opt(vrc, g, vrc.OPT_MIP_FOLD, fold)
        both(vrc, g, "MIP fold %d" % fold)
        both(vrc, g, "MIP fold %d trilinear" % fold, filter_mode=vrc.FILTER_TRILINEAR)
        if fold != vrc.MIP_FOLD_MEAN:
            _opt(vrc, g, vrc.OPT_MIP_DEPTH, 1)
            both(vrc, g, "MIP fold %d with depth" % fold)


def _frames(vrc, g, n):
    """n frames without reading the statistics in between; the wall time of the synchronised loop in ms."""
    L, s = g.L, g.s
    view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
    render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
    nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
    vrc.check(L, L.vrc_synchronize(g.ctx))
    t0 = time.perf_counter()
    for _ in range(n):
        vrc.check(L, L.vrc_pre_render(g.ctx, view))
        vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
    vrc.check(L, L.vrc_synchronize(g.ctx))
    wall = (time.perf_counter() - t0) * 1e3
    st = vrc.Stats()
    vrc.check(L, L.vrc_get_stats(g.ctx, C.byref(st)))
    return st, wall


def test_statistics_keep_their_contract(vrc):
    with _gpu(scene()) as g:
        g.render(count=False)  # options, transfer function, tile schedule; reads the statistics
        got = {}
        for markers in (1, 0):
            _opt(vrc, g, vrc.OPT_STREAM_MARKERS, markers)
            st, wall = _frames(vrc, g, 5)
            print("markers %d: kernel_ms_sum %.6f over %d launches, wall %.6f ms" % (markers, st.kernel_ms_sum,
                                                                                    st.kernel_launches, wall))
            assert st.kernel_launches == 5
            assert math.isfinite(st.kernel_ms_sum) and 0.0 < st.kernel_ms_sum <= wall
            assert math.isfinite(st.kernel_ms) and 0.0 < st.kernel_ms <= st.kernel_ms_sum
            got[markers] = st
        assert got[0].kernel_variant == got[1].kernel_variant
        assert got[0].kernel_launches == got[1].kernel_launches


def _constant_scene(values):
    """32^3 in eight 16^3 bricks, brick k holding values[k] everywhere."""
    s = orc.build_scene(voxels=(32, 32, 32), block=16, viewport=(48, 48), spin=(0.5, 0.35), alpha=0.3)
    assert len(s.ids) == 8
    for k, nid in enumerate(s.ids):
        s.bricks[nid] = np.full_like(s.bricks[nid], values[k])
    return s


def _replace_brick(vrc, g, t, nid):
    """Release nid's slot and upload scene t's brick into it, with no synchronisation of the caller's own."""
    vrc.check(g.L, g.L.vrc_pool_release_slot(g.pool, vrc.f32x3(*g.slots[nid])))
    brick = t.bricks[nid]
    slot = vrc.f32x3()
    vrc.check(g.L, g.L.vrc_pool_copy_to_slot(g.pool, brick.ctypes.data,
                                            vrc.u32x3(brick.shape[2], brick.shape[1], brick.shape[0]), slot))
    assert tuple(slot) == g.slots[nid]
    g.s = t


@pytest.mark.parametrize("own_stream", [False, True])
def test_uploads_into_a_recycled_slot_stay_ordered(vrc, hip, own_stream):
    values = [40 + 20 * k for k in range(8)]
    stream = C.c_void_p()
    with _gpu(_constant_scene(values)) as g:
        assert g.info()["free"] == 0  # a pool of exactly eight slots: the new brick can only take the released one
        if own_stream:
            assert hip.hipStreamCreate(C.byref(stream)) == 0
            vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, stream))
        first, n_first, _ = g.render()
        for rnd in range(3):
            k = (3 * rnd + 1) % 8
            nid = g.s.ids[k]
            values[k] = 255 - 30 * rnd
            t = _constant_scene(values)
            # no synchronisation between the march and the upload: the library's events alone order them
            _replace_brick(vrc, g, t, nid)
            got, n_got, _ = g.render()
            with _gpu(t) as fresh:
                want, n_want, _ = fresh.render()
            assert np.array_equal(got, want) and n_got == n_want, "round %d" % rnd
            assert (got != first).any()
        if own_stream:
            vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, None))
    if own_stream:
        assert hip.hipStreamDestroy(stream) == 0


def test_a_new_stream_waits_for_the_uploads_again(vrc, hip):
    # frames on one stream, then a new stream and an upload of OTHER voxels that no stream has waited for: a first march
    # on the new stream that skipped its wait would read the slot's old constant and differ from a fresh context's frame
    values = [40 + 20 * k for k in range(8)]
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    with _gpu(_constant_scene(values)) as g:
        before, _, _ = g.render()
        g.render()
        for i, stream in enumerate(streams + [None]):  # two new streams, then back to the context's own
            vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, stream))
            k = (3 * i + 1) % 8  # (bricks that the frame shows, as above)
            values[k] = 255 - 30 * i
            t = _constant_scene(values)
            _replace_brick(vrc, g, t, g.s.ids[k])
            got, n_got, _ = g.render()
            with _gpu(t) as fresh:
                want, n_want, _ = fresh.render()
            assert (want != before).any()
            assert np.array_equal(got, want) and n_got == n_want, "stream %d" % i
            got, n_got, _ = g.render()  # ... and a frame that has nothing to wait for
            assert np.array_equal(got, want) and n_got == n_want, "stream %d, second frame" % i
            before = want
    for st in streams:
        assert hip.hipStreamDestroy(st) == 0


def test_two_renderer_slots_on_two_streams_over_one_pool(vrc, hip):
    from libre_amd import driver as drv
    drv.load_library()
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", 64, 64, **kw) as one:
        one.set_camera(spin=(0.5, 0.35))
        want, _ = one.render_frame()
    assert want[..., 3].max() > 0.0
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    with drv.App("mem://#64,64,64,16", 64, 64, **kw) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_frames_in_flight(2)
        for k in range(2):
            app.select_slot(k)
            app.set_stream(streams[k])
        for frame in range(6):  # the slots alternate; the first frame of slot 0 uploads every brick
            app.select_slot(frame % 2)
            got, _ = app.render_frame()
            assert np.array_equal(got, want), "frame %d" % frame
        for k in range(2):
            app.select_slot(k)
            app.set_stream(None)
    for st in streams:
        assert hip.hipStreamDestroy(st) == 0
