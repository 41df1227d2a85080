"""VRC_OPT_RAY_CACHE on the GPU: a view that stands still computes its rays once (mode 0), stores them the first time it
repeats (mode 1) and loads them from then on (mode 2); VRC_OPT_RAY_CACHE_USED says which the last vrc_render did.  The
loaded ray is the stored bits, so every frame and sample count equals the frame of a context with the option off, bit
for bit -- no tolerance appears here.  Every comparison of a cached frame first asserts that mode 2 was reached: a run
that never touches the cache fails.  The option-0 frames are what tests/test_gpu_parity.py holds to the oracle."""
import copy
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

VOXELS, BLOCK = (64, 64, 64), 16
VIEWPORT = (100, 76)  # 13 x 10 tiles of 8 x 8: partial tiles on both edges


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


def mode(vrc, g):
    v = C.c_int64(-1)
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_RAY_CACHE_USED, C.byref(v)))
    return int(v.value)


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
        _scenes[key] = orc.build_scene(voxels=VOXELS, block=BLOCK, viewport=VIEWPORT, volume=volume, spin=spin, spr=spr,
                                       **kw)
    return copy.copy(_scenes[key])  # (tf, planes and view are replaced, never written in place)


def same(got, want, what):
    (fb, n), (wfb, wn) = got, want
    assert np.array_equal(fb, wfb), "%s: %d pixels differ" % (what, int((fb != wfb).any(axis=-1).sum()))
    assert n == wn and n > 0, (what, n, wn)


def frame(vrc, g, **kw):
    fb, n, st = g.render(**kw)
    return (fb, n), mode(vrc, g), st


def steady(vrc, g, ref, what, expect=(0, 1, 2, 2), **kw):
    """Frames of g (option on) until the last of `expect`, each equal to the frame of ref (option off)."""
    want, m, st_ref = frame(vrc, ref, **kw)
    assert m == 0, what
    seen = []
    for i, e in enumerate(expect):
        got, m, st = frame(vrc, g, **kw)
        seen.append(m)
        assert m == e, "%s: frame %d read mode %d, modes so far %r, expected %r" % (what, i, m, seen, expect)
        assert st.kernel_variant == st_ref.kernel_variant, what
        same(got, want, "%s frame %d (mode %d)" % (what, i, m))
    return want


@pytest.mark.parametrize("spr", [256, 300])  # the counted form of the uniform march, and its float chain
@pytest.mark.parametrize("spin", [(0.0, 0.0), (0.5, 0.35)])
@pytest.mark.parametrize("volume", ["mem", "hash"])
def test_steady_state_reads_0_1_2_2_and_every_frame_is_the_uncached_one(vrc, volume, spin, spr):
    s = scene(volume, spin, spr)
    assert s.render.samplesPerRay == spr
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_RAY_CACHE, 0)
        first = True
        for alpha in (0.05, 1.0):
            for coloured in (False, True):
                g.s.tf = ref.s.tf = table(alpha, coloured)
                if not first:  # start over: a new transfer function alone would keep mode 2
                    _opt(vrc, g, vrc.OPT_RAY_CACHE, 0)
                    _opt(vrc, g, vrc.OPT_RAY_CACHE, 1)
                first = False
                what = "%s spin %r spr %d alpha %g coloured %d" % (volume, spin, spr, alpha, coloured)
                (fb, _n) = steady(vrc, g, ref, what)
                assert fb[..., 3].max() > 0.05 and (fb[..., 3] == 0.0).any(), what  # rays that hit and rays that miss
                if alpha == 1.0:
                    assert fb[..., 3].max() > 0.999, what  # early ray termination
                # without the sample counter: another kernel instance, the same rays
                _opt(vrc, g, vrc.OPT_RAY_CACHE, 0)
                _opt(vrc, g, vrc.OPT_RAY_CACHE, 1)
                want, m0, _ = frame(vrc, ref, count=False)
                for e in (0, 1, 2):
                    got, m, _ = frame(vrc, g, count=False)
                    assert m == e, what
                    assert np.array_equal(got[0], want[0]), what + " uncounted"


def test_what_changes_the_rays_starts_over_and_what_does_not_keeps_the_cache(vrc, hip):
    s = scene("hash")
    s.tf = table(0.3, False)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_RAY_CACHE, 0)
        steady(vrc, g, ref, "start")

        def both(fn):
            fn(g)
            fn(ref)

        def restarted(what):
            return steady(vrc, g, ref, what, expect=(0, 1, 2))

        # a camera change (the same bricks in the same slots, another view and list order)
        moved = scene("hash", spin=(0.2, 0.1))
        moved.tf = s.tf
        both(lambda x: setattr(x, "s", copy.copy(moved)))
        a = restarted("camera")
        # clip planes: 0 -> 2
        clipped = copy.copy(moved)
        clipped.planes = np.ascontiguousarray([[0.6, 0.0, 0.8, 0.2], [0.0, 1.0, 0.0, 0.3]], dtype=np.float32)
        both(lambda x: setattr(x, "s", copy.copy(clipped)))
        b = restarted("clip planes")
        assert not np.array_equal(a[0], b[0])
        # the viewport's offset
        shifted = copy.copy(clipped)
        shifted.view = orc.ViewData.from_buffer_copy(clipped.view)
        shifted.view.glViewport[0], shifted.view.glViewport[1] = 3, 5
        both(lambda x: setattr(x, "s", copy.copy(shifted)))
        c = restarted("viewport offset")
        assert not np.array_equal(b[0], c[0])
        # row bands
        rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
        banded = copy.copy(shifted)
        banded.H = len(rows)

        def bands(x):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows.ctypes.data, len(rows)))
            x.s = copy.copy(banded)
        both(bands)
        d = restarted("row bands")
        assert np.array_equal(d[0], c[0][rows])
        # other bands of the same number of rows: the same pixel buffer, other rays
        rows2 = np.ascontiguousarray(rows + 2, dtype=np.uint32)
        both(lambda x: vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows2.ctypes.data, len(rows2))))
        d2 = restarted("other row bands")
        assert np.array_equal(d2[0], c[0][rows2])

        def unbanded(x):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, None, 0))
            x.s = copy.copy(shifted)
        both(unbanded)
        restarted("no row bands")
        # a pixel buffer of another size
        small = orc.with_viewport(clipped, 60, 44)
        small.tf, small.planes = clipped.tf, clipped.planes
        both(lambda x: setattr(x, "s", copy.copy(small)))
        restarted("smaller pixel buffer")
        both(lambda x: setattr(x, "s", copy.copy(clipped)))
        restarted("larger pixel buffer")
        # another stream
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, stream))
        restarted("stream")
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, None))
        restarted("own stream")
        # the option itself
        _opt(vrc, g, vrc.OPT_RAY_CACHE, 0)
        steady(vrc, g, ref, "option off", expect=(0, 0, 0))
        _opt(vrc, g, vrc.OPT_RAY_CACHE, 1)
        restarted("option on")

        # what the rays do not depend on keeps mode 2: the transfer function (grey -> coloured -> opaque grey) ...
        for alpha, coloured in ((0.3, True), (1.0, False)):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            steady(vrc, g, ref, "transfer function alpha %g coloured %d" % (alpha, coloured), expect=(2, 2))
        # ... and VRC_OPT_UNIFORM_BRICKS
        for v in (0, 1):
            both(lambda x: _opt(vrc, x, vrc.OPT_UNIFORM_BRICKS, v))
            steady(vrc, g, ref, "uniform bricks %d" % v, expect=(2, 2))
    assert hip.hipStreamDestroy(stream) == 0


def test_passes_of_a_multi_pass_frame(vrc):
    # four vrc_render calls per frame (CudaRaycastPipeline.cpp:149-185): the first computes, the second stores, the
    # third and fourth load -- in the frame's first pass order; the next frame loads from its first pass on
    s = scene("hash")
    s.tf = table(1.0, False)
    q = s.n_nodes // 4
    passes = [(0, q), (q, 2 * q), (2 * q, 3 * q), (3 * q, s.n_nodes)]
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_RAY_CACHE, 0)
        want, m, _ = frame(vrc, ref, passes=passes)
        assert m == 0
        whole, _, _ = frame(vrc, ref)
        assert np.array_equal(want[0], whole[0]) and want[1] == whole[1]  # the synchronous frame
        got, m, _ = frame(vrc, g, passes=passes[:2])
        assert m == 1  # the second pass stored
        got, m, _ = frame(vrc, g, passes=passes)
        assert m == 2
        same(got, want, "multi-pass, loaded from the first pass on")
    with _gpu(s) as g:
        got, m, _ = frame(vrc, g, passes=passes)  # a fresh context: 0, 1, 2, 2 inside one frame
        assert m == 2
        same(got, want, "multi-pass, first frame")
        assert (got[0][..., 3] > 0.999).any()


def test_multi_pass_frame_through_the_plugin_and_two_slots_on_two_streams(vrc, hip):
    from libre_amd import driver as drv
    drv.load_library()
    # 64 leaf bricks of 40^3 through a 1 MB atlas (16 slots): 4 passes (tests/test_gpu_host.py)
    frames = {}
    for on in (0, 1):
        with drv.App("hash://#128,128,128,32", 100, 76, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=1) as app:
            app.set_camera(spin=(0.5, 0.35))
            app.set_colormap(table(0.05, False))
            app.set_option(vrc.OPT_RAY_CACHE, on)
            for i in range(2):
                fb, st = app.render_frame()
                assert st.n_passes == 4 and st.n_available == 64
                assert app.get_option(vrc.OPT_RAY_CACHE_USED) == (2 if on else 0)  # the frame's last pass
                frames[(on, i)] = fb
    for i in range(2):
        assert np.array_equal(frames[(1, i)], frames[(0, i)]), i
    assert frames[(0, 0)][..., 3].max() > 0.05

    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", 100, 76, **kw) as one:
        one.set_camera(spin=(0.5, 0.35))
        one.set_option(vrc.OPT_RAY_CACHE, 0)
        want, _ = one.render_frame()
        assert one.get_option(vrc.OPT_RAY_CACHE_USED) == 0
    assert want[..., 3].max() > 0.0
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    with drv.App("mem://#64,64,64,16", 100, 76, **kw) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_frames_in_flight(2)
        for k in range(2):
            app.select_slot(k)
            app.set_stream(streams[k])
        seen = {0: [], 1: []}
        for i in range(8):  # the slots alternate; each has a ray cache of its own
            k = i % 2
            app.select_slot(k)
            got, _ = app.render_frame()
            seen[k].append(app.get_option(vrc.OPT_RAY_CACHE_USED))
            assert np.array_equal(got, want), "frame %d" % i
        assert seen == {0: [0, 1, 2, 2], 1: [0, 1, 2, 2]}, seen
        # the option reaches every slot
        app.set_option(vrc.OPT_RAY_CACHE, 0)
        for k in range(2):
            app.select_slot(k)
            got, _ = app.render_frame()
            assert app.get_option(vrc.OPT_RAY_CACHE_USED) == 0 and np.array_equal(got, want)
        for k in range(2):
            app.select_slot(k)
            app.set_stream(None)
    for st in streams:
        assert hip.hipStreamDestroy(st) == 0


def test_supersampled_gl_variant_always_computes_its_rays(vrc):
    s = scene("hash", spr=128)
    s.tf = table(0.3, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_RAY_CACHE, 0)
        # one ray per pixel: the GLSL twin's rays through the pixel centres are cached like any other
        steady(vrc, g, ref, "gl variant", variant=1)
        s4 = copy.copy(s)
        s4.render = orc.RenderData.from_buffer_copy(s.render)
        s4.render.samplesPerPixel = 4
        g.s, ref.s = copy.copy(s4), copy.copy(s4)
        steady(vrc, g, ref, "gl variant, 4 jittered rays per pixel", expect=(0, 0, 0), variant=1)
        g.s, ref.s = copy.copy(s), copy.copy(s)
        steady(vrc, g, ref, "gl variant again", expect=(0, 1, 2), variant=1)


def test_trilinear_filter_and_the_forms_that_compute_their_rays(vrc):
    s = scene("hash")
    s.tf = table(0.3, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_RAY_CACHE, 0)
        # the gather form of the trilinear filter is a vrc_k_raycast instance: the same vrc_pixel_grid_dda
        steady(vrc, g, ref, "trilinear, grid walk", kernel=vrc.KERNEL_GRID_DDA, filter_mode=1)
        # whatever AUTO picks for it, the frame is the uncached one: the tap-packed atlas is another instance of the
        # same kernel and goes on loading the rays the gather form stored; the LDS-staged kernel computes its own
        want, _, _ = frame(vrc, ref, filter_mode=1)
        for i in range(3):
            got, m, st = frame(vrc, g, filter_mode=1)
            assert st.kernel_variant in (vrc.KERNEL_PACKED, vrc.KERNEL_LDS)
            assert m == (2 if st.kernel_variant == vrc.KERNEL_PACKED else 0), (i, m, st.kernel_variant)
            same(got, want, "trilinear, auto, frame %d" % i)
        # the reference-order loop and the LDS-staged kernel never read the cache
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_LDS):
            steady(vrc, g, ref, "kernel %d" % kernel, expect=(0, 0, 0), kernel=kernel)
        # ... and neither do ray compaction and the depth split
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 4)
        _opt(vrc, ref, vrc.OPT_ERT_COMPACTION, 4)
        steady(vrc, g, ref, "ray compaction", expect=(0, 0, 0))
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 0)
        _opt(vrc, ref, vrc.OPT_ERT_COMPACTION, 0)
        steady(vrc, g, ref, "grid walk again", expect=(0, 1, 2))
