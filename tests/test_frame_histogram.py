"""Per-frame histogram of the rendered brick set (lvh_app_set_histogram / lvh_app_frame_histogram; the reference's
HistogramFilter, livre/lib/pipeline/HistogramFilter.cpp:77-132, and SendHistogramFilter, livre/eq/Channel.cpp:92-125).
Every expectation is built on the CPU from the data source's bricks (numpy bincount of each brick's interior times
8^(depth-1-level)) and compared exactly."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


_BRICKS = {}


def _brick_hist(drv, uri, nid):
    """(histogram of the brick's interior, bin count) -- cached per (uri, id)"""
    key = (uri, nid)
    if key not in _BRICKS:
        info = drv.datasource_info(uri)
        ov = info["overlap"]
        bs = drv.datasource_node(uri, nid)["block_size"]
        raw = drv.datasource_brick(uri, nid)
        u16 = raw.size == 2 * np.prod([bs[a] + 2 * ov[a] for a in range(3)])
        a = raw.view(np.uint16 if u16 else np.uint8).reshape(bs[2] + 2 * ov[2], bs[1] + 2 * ov[1], bs[0] + 2 * ov[0])
        inner = a[ov[2]:ov[2] + bs[2], ov[1]:ov[1] + bs[1], ov[0]:ov[0] + bs[0]].ravel()
        bins = 1024 if u16 else 256
        vals = (inner.astype(np.int64) >> 6) if u16 else inner.astype(np.int64)
        _BRICKS[key] = (np.bincount(vals, minlength=bins).astype(np.uint64), bins)
    return _BRICKS[key]


def expected(drv, uri, ids):
    depth = drv.datasource_info(uri)["depth"]
    out = None
    for nid in set(ids):
        h, bins = _brick_hist(drv, uri, nid)
        level = orc.unpack(nid)[0]
        term = h * np.uint64(8 ** (depth - 1 - level))
        out = term if out is None else out + term
    if out is None:
        out = np.zeros(1024 if "uint16" in uri else 256, dtype=np.uint64)
    return out


def _app(drv, uri, W=48, H=48, spin=(0.5, 0.35), **kw):
    kw.setdefault("synchronous", True)
    kw.setdefault("gpu_cache_mb", 64)
    app = drv.App(uri, W, H, **kw)
    app.set_camera(spin=spin)
    app.set_colormap(orc.linear_ramp_tf(0.05))
    app.set_histogram(True)
    return app


def test_mem_known_answer_mixed_levels(drv):
    # tests/lib/cache.cpp:97-119 extended to a frame: every interior voxel of a mem:// brick holds one value, so the
    # frame histogram is a set of spikes value(node) += 8^(d-1-l) * 32^3
    uri = "mem://#128,128,128,32"
    with _app(drv, uri, 64, 64, sse=1.0) as app:
        app.render_frame()
        bins, rng, area, fid = app.frame_histogram()
        ids = app.visible_set()
        levels = {orc.unpack(i)[0] for i in ids}
        assert len(levels) > 1, "a mixed-level cut"
        depth = drv.datasource_info(uri)["depth"]
        want = np.zeros(256, dtype=np.uint64)
        for nid in ids:
            want[orc.lib().orc_mem_brick_value_u8(nid)] += np.uint64(8 ** (depth - 1 - orc.unpack(nid)[0]) * 32 ** 3)
        assert (bins == want).all()
        assert rng == (0.0, 255.0) and area == 1.0 and fid == 0
        app.render_frame()
        assert app.frame_histogram()[3] == 1


def test_mem_known_answer_at_c2_size(drv):
    uri = "mem://#1024,1024,1024,128"
    with _app(drv, uri, 256, 256, min_lod=3, max_lod=3, gpu_cache_mb=2048) as app:
        app.render_frame()
        bins = app.frame_histogram()[0]
        ids = app.visible_set()
        assert len(ids) > 300
        want = np.zeros(256, dtype=np.uint64)
        for nid in ids:
            want[orc.lib().orc_mem_brick_value_u8(nid)] += np.uint64(128 ** 3)
        assert (bins == want).all()


def test_noise_volume_sse_cut_and_uint16_raw(drv, tmp_path):
    uri = "hash://#128,128,128,32"
    with _app(drv, uri, 64, 64, sse=1.0) as app:
        app.render_frame()
        assert (app.frame_histogram()[0] == expected(drv, uri, app.visible_set())).all()
    rng = np.random.default_rng(11)
    path = tmp_path / "v16.raw"
    rng.integers(0, 65536, size=(64, 64, 64), dtype=np.uint16).tofile(str(path))
    uri16 = "raw://%s#64,64,64,uint16,16" % path
    with _app(drv, uri16, 40, 40, sse=1.0) as app:
        app.render_frame()
        bins, r, _, _ = app.frame_histogram()
        assert bins.size == 1024 and r == (0.0, 65535.0)
        assert (bins == expected(drv, uri16, app.visible_set())).all()


def test_multipass_frame_counts_every_visible_brick_once(drv):
    uri = "hash://#128,128,128,32"
    with _app(drv, uri, 40, 40, min_lod=2, max_lod=2, gpu_cache_mb=1) as app:
        _, st = app.render_frame()
        assert st.n_passes == 4
        assert (app.frame_histogram()[0] == expected(drv, uri, app.visible_set())).all()


def _window(mv, proj, W, H, box):
    c = np.array([(box[0] + box[3]) / 2, (box[1] + box[4]) / 2, (box[2] + box[5]) / 2, 1.0])
    clip = np.array(proj, dtype=np.float64).reshape(4, 4).T @ (np.array(mv, dtype=np.float64).reshape(4, 4).T @ c)
    return (clip[0] / clip[3] * 0.5 + 0.5) * W, (clip[1] / clip[3] * 0.5 + 0.5) * H


def test_tiles_and_bands_partition_the_frame(drv):
    uri, W, H = "hash://#128,128,128,32", 64, 64
    kw = dict(min_lod=2, max_lod=2, spin=(0.3, 0.2))
    with _app(drv, uri, W, H, **kw) as full:
        full.render_frame()
        want = full.frame_histogram()[0]
        assert (want == expected(drv, uri, full.visible_set())).all()
        mv, proj = full.view_matrices()
        centres = [_window(mv, proj, W, H, drv.datasource_node(uri, i)["world_box"]) for i in full.visible_set()]
    # no centre lies on an edge used below (else the split would depend on rounding)
    for px, py in centres:
        for e in (32.0, 16.0, 48.0):
            assert abs(px - e) > 1e-3 and abs(py - e) > 1e-3
    total, area = np.zeros_like(want), 0.0
    for tile in ((0, 0, 32, 32), (32, 0, 32, 32), (0, 32, 32, 32), (32, 32, 32, 32)):
        with _app(drv, uri, W, H, tile=tile, **kw) as t:
            t.render_frame()
            bins, _, a, _ = t.frame_histogram()
            total += bins
            area += a
    assert (total == want).all() and area == 1.0
    total, area = np.zeros_like(want), 0.0
    for bands in (((0, 16), (32, 16)), ((16, 16), (48, 16))):
        with _app(drv, uri, W, H, **kw) as b:
            b.set_bands(bands)
            b.render_frame()
            bins, _, a, _ = b.frame_histogram()
            total += bins
            area += a
    assert (total == want).all() and area == 1.0


def test_per_ray_lod_counts_the_sse_cut(drv):
    uri = "hash://#128,128,128,32"
    for cache in (64, 2):  # one pass; slabs (the hierarchy does not fit the atlas)
        with _app(drv, uri, 64, 64, sse=1.0, gpu_cache_mb=cache) as app:
            app.set_ray_lod(True)
            _, st = app.render_frame()
            assert (app.frame_histogram()[0] == expected(drv, uri, app.visible_set())).all(), cache


def test_async_mode_counts_the_rendering_set(drv):
    uri = "hash://#128,128,128,32"
    with _app(drv, uri, 48, 48, min_lod=2, max_lod=2) as sync:
        sync.render_frame()
        want = sync.frame_histogram()[0]
    with _app(drv, uri, 48, 48, min_lod=2, max_lod=2, synchronous=False) as app:
        app.render_frame()
        assert (app.frame_histogram()[0] == expected(drv, uri, app.node_order())).all()
        app.wait_uploads()
        app.render_frame()
        assert (app.frame_histogram()[0] == want).all()


def test_cache_behaviour_kept_list_recycled_slots_and_frames_in_flight(drv):
    uri = "hash://#128,128,128,32"
    with _app(drv, uri, 48, 48, sse=1.0) as app:
        app.render_frame()
        first = app.frame_histogram()[0]
        app.render_frame()  # the kept list
        assert (app.frame_histogram()[0] == first).all()
    # a camera sweep through a small atlas: slots are recycled between frames, every frame matches its own set
    with _app(drv, uri, 48, 48, min_lod=2, max_lod=2, gpu_cache_mb=3) as app:
        for k in range(6):
            app.set_camera(spin=(0.4 * k, 0.25 * k))
            app.render_frame()
            assert (app.frame_histogram()[0] == expected(drv, uri, app.visible_set())).all(), k
    with _app(drv, uri, 48, 48, sse=1.0) as app:
        app.set_frames_in_flight(2)
        app.select_slot(0)
        app.set_camera(spin=(0.1, 0.0))
        app.render_frame()
        ids0 = app.visible_set()
        app.select_slot(1)
        app.set_camera(spin=(1.2, 0.7))
        app.render_frame()
        ids1 = app.visible_set()
        assert (app.frame_histogram()[0] == expected(drv, uri, ids1)).all()
        app.select_slot(0)
        h0, _, _, fid0 = app.frame_histogram()
        assert (h0 == expected(drv, uri, ids0)).all() and fid0 == 0


def test_default_off_frame_is_bit_identical_and_asking_is_an_error(drv):
    from libre_amd import driver
    uri = "hash://#128,128,128,32"
    with drv.App(uri, 48, 48, synchronous=True, sse=1.0, gpu_cache_mb=64) as off:
        off.set_camera(spin=(0.5, 0.35))
        off.set_colormap(orc.linear_ramp_tf(0.05))
        fb_off, _ = off.render_frame()
        with pytest.raises(driver.DriverError, match="off"):
            off.frame_histogram()
    with _app(drv, uri, 48, 48, sse=1.0) as on:
        fb_on, _ = on.render_frame()
    assert (fb_on == fb_off).all()


def test_pool_histogram_any_divisor_bin_count_and_region(drv):
    # vrc_pool_histogram runs on the new binning kernel: constant and noise bricks, bin counts that divide the range,
    # regions that do not start or end on micro-block faces
    from libre_amd import vrc
    L = vrc.load_library()
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    rng = np.random.default_rng(3)
    for dtype, bpv, range_ in ((np.uint8, 1, 256), (np.uint16, 2, 65536)):
        vrc.check(L, L.vrc_pool_create(ctx, bpv, 0, 0, 1, vrc.u32x3(37, 29, 45), 4 * bpv * 48 ** 3, C.byref(pool)))
        slot = vrc.f32x3()
        for brick in (np.full((45, 29, 37), 77, dtype=dtype), rng.integers(0, range_, size=(45, 29, 37), dtype=dtype)):
            brick = np.ascontiguousarray(brick)
            vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(37, 29, 45), slot))
            for bins_n in (1, 2, 16, 64, 256) + ((1024, 4096) if bpv == 2 else ()):
                for org, size in (((0, 0, 0), (37, 29, 45)), ((3, 5, 7), (30, 17, 9)), ((9, 1, 0), (1, 1, 1))):
                    bins = np.zeros(bins_n, dtype=np.uint64)
                    vrc.check(L, L.vrc_pool_histogram(pool, slot, vrc.u32x3(*org), vrc.u32x3(*size), bins_n, 3,
                                                      bins.ctypes.data))
                    sub = brick[org[2]:org[2] + size[2], org[1]:org[1] + size[1], org[0]:org[0] + size[0]]
                    want = np.bincount(sub.ravel().astype(np.int64) // (range_ // bins_n), minlength=bins_n) * 3
                    assert (bins == want.astype(np.uint64)).all(), (dtype, bins_n, org)
            vrc.check(L, L.vrc_pool_release_slot(pool, slot))
        L.vrc_pool_destroy(pool)
    L.vrc_ctx_destroy(ctx)


def test_pool_rows_follow_uploads_and_releases(drv):
    # the C ABI directly: enable with resident bricks (batched binning), uploads after it, release invalidates
    from libre_amd import vrc
    L = vrc.load_library()
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    vrc.check(L, L.vrc_pool_create(ctx, 1, 0, 0, 1, vrc.u32x3(24, 24, 24), 8 * 24 ** 3, C.byref(pool)))
    rng = np.random.default_rng(9)
    bricks = [rng.integers(0, 256, size=(24, 24, 24), dtype=np.uint8) for _ in range(4)]
    slots = [vrc.f32x3() for _ in bricks]
    for b, s in zip(bricks[:2], slots[:2]):
        vrc.check(L, L.vrc_pool_copy_to_slot(pool, b.ctypes.data, vrc.u32x3(24, 24, 24), s))
    vrc.check(L, L.vrc_pool_enable_histograms(pool, 256, vrc.u32x3(4, 4, 4)))
    for b, s in zip(bricks[2:], slots[2:]):
        vrc.check(L, L.vrc_pool_copy_to_slot(pool, b.ctypes.data, vrc.u32x3(24, 24, 24), s))
    flat = (C.c_float * 12)(*[v for s in slots for v in s])
    scales = (C.c_uint64 * 4)(1, 8, 64, 1)
    vrc.check(L, L.vrc_frame_histogram(ctx, pool, flat, scales, 4, 0))
    out = np.zeros(256, dtype=np.uint64)
    vrc.check(L, L.vrc_get_frame_histogram(ctx, out.ctypes.data, 256))
    want = sum(np.bincount(b[4:20, 4:20, 4:20].ravel(), minlength=256).astype(np.uint64) * np.uint64(k)
               for b, k in zip(bricks, (1, 8, 64, 1)))
    assert (out == want).all()
    vrc.check(L, L.vrc_frame_histogram(ctx, pool, flat, scales, 4, 1))  # accumulate
    vrc.check(L, L.vrc_get_frame_histogram(ctx, out.ctypes.data, 256))
    assert (out == 2 * want).all()
    vrc.check(L, L.vrc_pool_release_slot(pool, slots[0]))
    assert L.vrc_frame_histogram(ctx, pool, flat, scales, 4, 0) == vrc.VRC_EINVAL  # a released slot's row is gone
    assert L.vrc_get_frame_histogram(ctx, out.ctypes.data, 1024) == vrc.VRC_EINVAL
    vrc.check(L, L.vrc_pool_enable_histograms(pool, 0, None))
    assert L.vrc_frame_histogram(ctx, pool, flat, scales, 1, 0) == vrc.VRC_EINVAL
    L.vrc_pool_destroy(pool)
    L.vrc_ctx_destroy(ctx)
