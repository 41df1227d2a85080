"""GPU tests of the C++ host plugin (RenderPipeline("hip") through the flat driver API):
frames against the oracle, synchronous / asynchronous / multipass behaviour, sort-first tiles."""
import ctypes as C
import os

import numpy as np
import pytest

import nongrid
import orc
import scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _oracle_for(app, uri_voxels, block, viewport, spin=(0.0, 0.0), alpha=0.05, volume="mem",
                planes=None, tile=None):
    ids = app.visible_set()
    s = orc.build_scene(voxels=uri_voxels, block=block, viewport=viewport, spin=spin, alpha=alpha,
                        volume=volume, ids=ids, planes=planes, tile=tile)
    fb, n = orc.oracle_render(s, threads=8)
    return s, fb, n


def test_sync_frame_leaves_only_matches_oracle(drv):
    from libre_amd import vrc
    with drv.App("mem://#64,64,64,16", 48, 48, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        info = app.volume_info()
        assert info["depth"] == 3 and info["max_block"] == [24, 24, 24] and info["overlap"] == [4, 4, 4]
        assert sorted(app.visible_set()) == sorted(orc.leaf_ids(orc.mem_volume_info(64, 64, 64, 16)))
        mv, proj = app.view_matrices()
        assert np.allclose(mv, list(orc.default_mv((0.5, 0.35))), atol=1e-7)
        assert np.allclose(proj, list(orc.default_proj()), atol=1e-7)
        fb, st = app.render_frame()
        st2 = app.stats()
        assert st.n_available == 64 and st.n_not_available == 0 and st.n_passes == 1
        assert st.samples_per_ray == 512
        s, want, n_want = _oracle_for(app, (64, 64, 64), 16, (48, 48), spin=(0.5, 0.35))
        scenes.assert_parity(fb, want, "host sync")
        assert abs(int(st2.samples) - n_want) <= 2e-4 * n_want + 8
        # second frame: everything is a cache hit, same bits
        fb2, _ = app.render_frame()
        assert (fb2 == fb).all()
        tex, data = app.cache_stats()
        assert tex["count"] == 64 and tex["misses"] == 64 and data["count"] == 64


def test_hash_volume_with_clip_planes(drv):
    planes = [[-1, 0, 0, 0.2], [0, 1, 0, 0.3], [0.6, 0, 0.8, 0.35]]
    with drv.App("hash://#64,64,64,16", 48, 48, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_clip_planes(planes)
        fb, st = app.render_frame()
        # clip planes also cull bricks in the visible-set generator (ClipPlanes::isClipped)
        assert 0 < st.n_available < 64
        s, want, _ = _oracle_for(app, (64, 64, 64), 16, (48, 48), spin=(0.5, 0.35), volume="hash",
                                 planes=planes)
        scenes.assert_parity(fb, want, "host clip")


def test_lod_cut_mixed_levels_matches_oracle(drv):
    # default SSE on a small window selects coarse and fine bricks together
    with drv.App("mem://#128,128,128,16", 64, 64, synchronous=True, sse=1.0, gpu_cache_mb=16) as app:
        app.set_camera(position=(0.2, 0.1, 0.9), spin=(0.3, 0.2))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        ids = app.visible_set()
        levels = {i & 0xF for i in ids}
        assert len(levels) >= 2, levels
        fb, st = app.render_frame()
        assert st.n_available == len(ids)
        s = orc.build_scene(voxels=(128, 128, 128), block=16, viewport=(64, 64), ids=ids,
                            spin=(0.3, 0.2), eye=(0.2, 0.1, 0.9), order=app.node_order())
        # the driver applies spin after look-at like the oracle helper does
        want, _ = orc.oracle_render(s, threads=8)
        assert st.samples_per_ray == s.render.samplesPerRay
        # AUTO composites a list of mixed brick sizes in the reference's (centre-distance) order
        from libre_amd import vrc
        scenes.assert_parity(fb, want, "host lod cut")
        # the grid walk takes the same samples along the ray instead: the same frame up to the pairs of brick
        # segments the reference's order swaps (quirk Q6; not a parity statement)
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_GRID_DDA)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        dda, _ = app.render_frame()
        n_dda = int(app.stats().samples)
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_AUTO)
        ref, _ = app.render_frame()
        assert int(app.stats().samples) == n_dda
        scenes.assert_close_frames(dda, ref, "grid walk vs reference order on a mixed cut")


def test_multipass_when_atlas_is_smaller_than_the_frame(drv):
    # CudaRaycastPipeline.cpp:149-185: 64 bricks through a pool of a few slots
    # 64 leaf bricks of 40^3 = 4 MB through a 1 MB atlas (16 slots): 4 passes
    with drv.App("hash://#128,128,128,32", 40, 40, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=1) as small:
        small.set_camera(spin=(0.5, 0.35))
        small.set_colormap(orc.linear_ramp_tf(0.05))
        fb_small, st = small.render_frame()
        assert st.n_passes == 4 and st.n_available == 64
        tex, _ = small.cache_stats()
        assert tex["count"] <= 16  # never more texture objects than slots
    with drv.App("hash://#128,128,128,32", 40, 40, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as big:
        big.set_camera(spin=(0.5, 0.35))
        big.set_colormap(orc.linear_ramp_tf(0.05))
        fb_big, st2 = big.render_frame()
        assert st2.n_passes == 1
    scenes.assert_same_frame(fb_small, fb_big, "multipass vs single pass")


def test_async_mode_converges_to_sync_frame(drv):
    # CudaRaycastPipeline.cpp:236-301: render what is resident, upload in the background
    with drv.App("mem://#64,64,64,16", 40, 40, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as sync:
        sync.set_camera(spin=(0.2, 0.1))
        sync.set_colormap(orc.linear_ramp_tf(0.05))
        want, _ = sync.render_frame()
    with drv.App("mem://#64,64,64,16", 40, 40, synchronous=False, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.2, 0.1))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        fb0, st0 = app.render_frame()
        assert st0.n_not_available > 0  # nothing resident yet: the first frame is incomplete
        app.wait_uploads()
        fb1, st1 = app.render_frame()
        assert st1.n_not_available == 0 and st1.n_available == 64
        assert (fb1 == want).all()


def test_sort_first_tile_apps_assemble_the_full_frame(drv):
    W = H = 48
    full_app = drv.App("hash://#64,64,64,16", W, H, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    full_app.set_camera(spin=(0.5, 0.35))
    full_app.set_colormap(orc.linear_ramp_tf(0.05))
    full, _ = full_app.render_frame()
    full_app.close()
    out = np.zeros_like(full)
    for (y0, h) in ((0, 12), (12, 12), (24, 12), (36, 12)):
        with drv.App("hash://#64,64,64,16", W, H, tile=(0, y0, W, h), synchronous=True, min_lod=2,
                     max_lod=2, gpu_cache_mb=8) as t:
            t.set_camera(spin=(0.5, 0.35))
            t.set_colormap(orc.linear_ramp_tf(0.05))
            fb, st = t.render_frame()
            assert fb.shape == (h, W, 4)
            out[y0:y0 + h] = fb
    scenes.assert_close_frames(out, full, "tile apps vs full frame")  # sub-frustum matrices differ in rounding


def test_unknown_renderer_and_volume_are_reported(drv):
    with pytest.raises(drv.DriverError, match="No plugin implementation available"):
        drv.App("mem://#64,64,64,16", 8, 8, renderer="cuda")
    with pytest.raises(drv.DriverError, match="No plugin implementation available"):
        drv.App("nosuch://x", 8, 8)
    # the reference kernel only handles uint8 (quirk Q2); uint16 is an extension here, the other
    # types are refused, not mis-rendered
    with pytest.raises(drv.DriverError):
        a = drv.App("mem://?datatype=float#64,64,64,16", 8, 8, synchronous=True)
        a.render_frame()


def test_uint16_volume_through_the_plugin(drv):
    # mem:// computes the brick value in the volume's type (MemoryDataSource.cpp:54-57), so a
    # uint16 volume with the data range (0,255) must give the uint8 volume's frame
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", 40, 40, **kw) as a8:
        a8.set_camera(spin=(0.4, 0.2))
        f8, _ = a8.render_frame()
    with drv.App("mem://?datatype=uint16#64,64,64,16", 40, 40, **kw) as a16:
        assert a16.volume_info()["bytes_per_voxel"] == 2 if "bytes_per_voxel" in a16.volume_info() else True
        a16.set_camera(spin=(0.4, 0.2))
        a16.set_data_range(0.0, 255.0)
        f16, st = a16.render_frame()
    assert f8[..., 3].max() > 0.01
    assert np.abs(f8 - f16).max() < 1e-5


def test_row_bands_in_one_launch_are_rows_of_the_full_frame(drv):
    # sort-first bands of one rank rendered by a single kernel launch (vrc_set_row_map): the
    # rays are the full frame's, so the stacked bands equal the frame rows bit for bit
    W, H = 48, 64
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("hash://#64,64,64,16", W, H, **kw) as full_app:
        full_app.set_camera(spin=(0.5, 0.35))
        full_app.set_colormap(orc.linear_ramp_tf(0.05))
        full, _ = full_app.render_frame()
    bands = [(8, 8), (40, 16), (24, 8)]
    with drv.App("hash://#64,64,64,16", W, H, **kw) as app:
        app.set_bands(bands)
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        fb, st = app.render_frame()
        assert fb.shape == (32, W, 4) and st.n_passes == 1
        want = np.concatenate([full[y0:y0 + h] for (y0, h) in bands], axis=0)
        assert (fb == want).all()
        # and back to the whole frame
        app.set_bands([])
        app.height = H
        fb2, _ = app.render_frame()
        assert (fb2 == full).all()


def test_frames_in_flight_share_one_atlas(drv):
    # K renderer instances over one pipeline (RenderPipelinePlugin::render takes the Renderer):
    # every slot produces the same frame, bricks are uploaded once
    with drv.App("hash://#64,64,64,16", 40, 40, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_frames_in_flight(3)
        frames = []
        for k in (0, 1, 2, 1, 0):
            app.select_slot(k)
            fb, st = app.render_frame()
            frames.append(fb)
        for fb in frames[1:]:
            assert (fb == frames[0]).all()
        tex, data = app.cache_stats()
        assert tex["misses"] == 64 and tex["count"] == 64  # one upload per brick in total
        with pytest.raises(drv.DriverError):
            app.select_slot(3)


def test_out_of_core_raw_uint16_volume_matches_oracle(drv, tmp_path):
    # BASELINE C3 in small: raw:// uint16 file, bricked on demand with an LOD tree (extension),
    # asynchronous upload, then the same frame as the synchronous mode and as the oracle
    from libre_amd import vrc
    vol = (orc.hash_volume(64, 64, 64).astype(np.uint16) * np.uint16(200)) + np.uint16(7)
    path = str(tmp_path / "vol16.raw")
    vol.tofile(path)
    uri = "raw://%s#64,64,64,uint16,16" % path
    kw = dict(min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App(uri, 48, 40, synchronous=True, **kw) as app:
        assert app.volume_info()["depth"] == 3
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(0.0, 51007.0)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        fb, st = app.render_frame()
        ids = app.visible_set()
        s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(48, 40), spin=(0.5, 0.35), volume=vol,
                            dtype="u16", ids=ids, data_range=(0.0, 51007.0))
        want, n_want = orc.oracle_render(s, threads=8)
        assert want[..., 3].max() > 0.05
        scenes.assert_parity(fb, want, "raw u16 sync")
        assert abs(int(app.stats().samples) - n_want) <= 2e-4 * n_want + 8
        app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR)
        lin, _ = app.render_frame()
        want_lin, _ = orc.oracle_render(s, threads=8, filter_mode=1)
        scenes.assert_parity(lin, want_lin, "raw u16 trilinear")
    with drv.App(uri, 48, 40, synchronous=False, **kw) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(0.0, 51007.0)
        for _ in range(200):
            out, st = app.render_frame()
            app.wait_uploads()
            if st.n_not_available == 0:
                break
        assert st.n_not_available == 0
        out, _ = app.render_frame()
        assert (out == fb).all()


def test_c3_shape_out_of_core_uint16_136_cubed_slots_async_upload_and_lod_cut(drv, tmp_path):
    # BASELINE C3 at a size a test can afford, in C3's shapes: a 512^3 uint16 raw:// file (256 MB) bricked on demand
    # with block 128 -> slots of 136^3 two-byte voxels, LOD octree (depth 3), 512^2 viewport.  (i) synchronous,
    # leaves only: every 32nd row against the oracle, sample counts equal; (ii) asynchronous upload overlapped
    # with the march, screen-space-error LOD cut (mixed levels): converges to the frame the synchronous
    # pipeline renders for the same cut, and that frame matches the oracle.  The full 2048^3 run (17 GB file,
    # 22.6 GB atlas of more than 2^32 voxels) is tools/dev_c3.py (profiles/r1_c3_out_of_core_uint16_2048.txt).
    from libre_amd import vrc
    vol = (orc.hash_volume(512, 512, 512).astype(np.uint16) * np.uint16(257)) ^ np.uint16(0x0155)
    path = str(tmp_path / "vol512_u16.raw")
    vol.tofile(path)
    uri = "raw://%s#512,512,512,uint16,128" % path
    rng_ = (0.0, 65535.0)
    with drv.App(uri, 512, 512, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=1024, cpu_cache_mb=2048) as app:
        assert app.volume_info()["depth"] == 3 and app.volume_info()["max_block"] == [136, 136, 136]
        app.set_camera(spin=(0.3, 0.2))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(*rng_)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        fb, st = app.render_frame()
        assert st.n_available == 64 and st.n_passes == 1
        n_gpu = int(app.stats().samples)
        s = orc.build_scene(voxels=(512, 512, 512), block=128, viewport=(512, 512), spin=(0.3, 0.2), volume=vol,
                            dtype="u16", ids=app.visible_set(), data_range=rng_, order=app.node_order())
        assert s.slot_dim == [136, 136, 136]
        want, n_rows = orc.oracle_render(s, threads=16, rows=(0, 512, 32))
        scenes.assert_parity(fb[::32], want[::32], "C3 shape, leaves, synchronous")
        full, n_want = orc.oracle_render(s, threads=16)
        assert n_gpu == n_want
    kw = dict(sse=2.0, gpu_cache_mb=1024, cpu_cache_mb=2048)
    with drv.App(uri, 512, 512, synchronous=True, **kw) as app:
        app.set_camera(spin=(0.3, 0.2))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(*rng_)
        cut, st = app.render_frame()
        ids = app.visible_set()
        assert len({i & 0xF for i in ids}) >= 2  # the cut mixes levels
        s2 = orc.build_scene(voxels=(512, 512, 512), block=128, viewport=(512, 512), spin=(0.3, 0.2), volume=vol,
                             dtype="u16", ids=ids, data_range=rng_, order=app.node_order())
        want2, _ = orc.oracle_render(s2, threads=16, rows=(0, 512, 32))
        scenes.assert_parity(cut[::32], want2[::32], "C3 shape, LOD cut, synchronous")
    with drv.App(uri, 512, 512, synchronous=False, **kw) as app:
        app.set_camera(spin=(0.3, 0.2))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(*rng_)
        frames = 0
        for frames in range(1, 400):
            out, st = app.render_frame()  # marches what is resident while the loaders work
            assert np.isfinite(out).all()
            if st.n_not_available == 0:
                break
            app.wait_uploads()
        assert st.n_not_available == 0 and frames >= 2  # the first frame had bricks missing
        out, _ = app.render_frame()
        scenes.assert_same_frame(out, cut, "C3 shape, asynchronous upload converged")


def test_glraycaster_variant_through_the_plugin(drv):
    # VRC_OPT_VARIANT on the renderer plugin: GLSL-twin semantics + RGBA8 transfer function
    from libre_amd import vrc
    with drv.App("hash://#64,64,64,16", 48, 48, synchronous=True, min_lod=2, max_lod=2,
                 gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        tf = orc.linear_ramp_tf(0.3)
        app.set_colormap(tf)
        app.set_option(vrc.OPT_VARIANT, vrc.VARIANT_GLRAYCASTER)
        fb, _ = app.render_frame()
        ids = app.visible_set()
        s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(48, 48), spin=(0.5, 0.35), alpha=0.3,
                            volume="hash", ids=ids)
        s.tf = (np.floor(np.clip(s.tf, 0, 1) * 255.0 + 0.5) / 255.0).astype(np.float32)
        want, _ = orc.oracle_render(s, threads=8, variant=1)
        scenes.assert_parity(fb, want, "gl variant via plugin")


def test_async_mode_under_cache_pressure_stays_consistent(drv):
    # texture cache far smaller than the visible set: the LRU keeps evicting bricks whose slots
    # are reused while earlier frames may still be marching (release -> reuse is ordered after the
    # marches by render fences in the pool).  Every frame must be finite, bounded by the full
    # frame's opacity, and the camera-still sequence must settle.
    kw = dict(min_lod=3, max_lod=3)
    with drv.App("hash://#128,128,128,16", 64, 64, synchronous=True, gpu_cache_mb=16, **kw) as full:
        full.set_camera(spin=(0.4, 0.2))
        full.set_colormap(orc.linear_ramp_tf(0.05))
        want, st = full.render_frame()
        assert st.n_available == 512
    with drv.App("hash://#128,128,128,16", 64, 64, synchronous=False, gpu_cache_mb=2, **kw) as app:
        app.set_colormap(orc.linear_ramp_tf(0.05))
        tex, _ = None, None
        for i in range(40):
            app.set_camera(spin=(0.4 + 0.05 * (i % 7), 0.2))
            for _ in range(3):  # marches left in flight while the loaders reuse released slots
                app.render_frame(readback=False)
            fb, st = app.render_frame()
            assert np.isfinite(fb).all() and fb.min() >= 0.0 and fb[..., 3].max() <= 1.0
            # (the LRU only evicts bricks no frame holds: let the loaders run between frames)
            app.wait_uploads()
        tex, data = app.cache_stats()
        assert tex["used"] <= tex["max"] and tex["count"] < 512  # never more than the budget
        assert tex["misses"] > tex["count"]  # bricks were evicted and reloaded
    # multipass synchronous rendering with the same small cache gives the full frame
    with drv.App("hash://#128,128,128,16", 64, 64, synchronous=True, gpu_cache_mb=2, **kw) as app:
        app.set_camera(spin=(0.4, 0.2))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        got, st = app.render_frame()
        assert st.n_passes > 1
        scenes.assert_same_frame(got, want, "multipass under cache pressure")


def test_uvf_volume_through_the_plugin_matches_oracle(drv):
    # the reference's UVF fixture (a 75x75x138 PET scan, zlib bricks of 28^3 + overlap 2, an
    # octree that is not a power of two): leaves only, then the coarser level
    import os
    from libre_amd import vrc
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_reduced.uvf")
    uri = "uvf://" + path
    for lod in (1, 0):
        with drv.App(uri, 56, 48, synchronous=True, min_lod=lod, max_lod=lod, gpu_cache_mb=8) as app:
            app.set_camera(spin=(0.6, 0.3))
            app.set_colormap(orc.linear_ramp_tf(0.3))
            app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
            fb, st = app.render_frame()
            ids = app.visible_set()
            assert len(ids) == (45 if lod == 1 else 12) and st.n_available == len(ids)
            s = orc.scene_from_datasource(drv, uri, ids, (56, 48), spin=(0.6, 0.3), alpha=0.3)
            assert s.render.samplesPerRay == st.samples_per_ray
            want, n_want = orc.oracle_render(s, threads=8)
            assert want[..., 3].max() > 0.3
            scenes.assert_parity(fb, want, "uvf lod %d" % lod)
            assert abs(int(app.stats().samples) - n_want) <= 2e-4 * n_want + 8
            app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR)
            lin, _ = app.render_frame()
            want_lin, _ = orc.oracle_render(s, threads=8, filter_mode=1)
            scenes.assert_parity(lin, want_lin, "uvf lod %d trilinear" % lod)


@pytest.mark.parametrize("seed", range(16 * scenes.FUZZ_SCALE))
def test_random_lod_cuts_through_the_plugin_match_the_oracle(drv, seed):
    # random camera (also close to / inside the volume), screen-space error and volume: the
    # plugin's visible set (mixed levels, holes where bricks are culled), its brick order and
    # the kernel AUTO picks against the oracle rendering the same node list
    from libre_amd import vrc
    rng = np.random.default_rng(7000 + seed)
    vox = int(rng.choice([64, 128]))
    block = 16
    volume = str(rng.choice(["mem", "hash"]))
    W, H = int(rng.integers(24, 64)), int(rng.integers(24, 64))
    eye = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.3, 1.8)))
    spin = (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.2, 1.2)))
    sse = float(rng.choice([0.5, 1.0, 2.0, 4.0]))
    uri = "%s://#%d,%d,%d,%d" % (volume, vox, vox, vox, block)
    with drv.App(uri, W, H, synchronous=True, sse=sse, gpu_cache_mb=32) as app:
        app.set_camera(position=eye, spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.3))
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        ids = app.visible_set()
        fb, st = app.render_frame()
        assert st.n_available == len(ids)
        if not ids:
            assert (fb == 0).all()
            return
        # the oracle renders the plugin's own front-to-back list (checked to be one): with bricks of mixed
        # sizes the order is part of the result (quirk Q6), and the order of bricks at nearly equal centre
        # distance hangs on the last bit of the host's transform
        s = orc.build_scene(voxels=(vox, vox, vox), block=block, viewport=(W, H), ids=ids, spin=spin, eye=eye,
                            volume=volume, alpha=0.3, order=app.node_order())
        want, n_want = orc.oracle_render(s, threads=8)
        assert st.samples_per_ray == s.render.samplesPerRay
        scenes.assert_parity(fb, want, "seed %d %s eye %r spin %r sse %g levels %r" % (
            seed, uri, eye, spin, sse, sorted({i & 0xF for i in ids})))
        # (the transfer function saturates: a ray may cross the early-exit threshold a sample earlier or later)
        assert abs(int(app.stats().samples) - n_want) <= 1e-5 * n_want + 8


@pytest.mark.parametrize("seed", range(8 * scenes.FUZZ_SCALE))
def test_random_sort_first_layouts_reassemble_the_frame(drv, seed):
    # every rank of a random sort-first layout renders its bands in one launch; the assembled
    # frame must be the full frame bit for bit -- point sampled, trilinear (LDS kernel) and with
    # the glRaycaster rules
    from libre_amd import sortfirst, vrc
    rng = np.random.default_rng(9000 + seed)
    W, H = int(rng.integers(16, 56)), int(rng.integers(24, 72))
    world = int(rng.choice([2, 3, 4, 8]))
    bpr = int(rng.choice([1, 2, 4]))
    spin = (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.2, 1.2)))
    mode = int(rng.integers(0, 3))  # 0 point, 1 trilinear, 2 glRaycaster
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)

    def setup(app):
        app.set_camera(spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.3))
        if mode == 1:
            app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR)
        if mode == 2:
            app.set_option(vrc.OPT_VARIANT, vrc.VARIANT_GLRAYCASTER)

    with drv.App("hash://#64,64,64,16", W, H, **kw) as full_app:
        setup(full_app)
        full, _ = full_app.render_frame()
    assert full[..., 3].max() > 0.05
    layout = sortfirst.band_layout(H, world, bpr)
    out = np.full_like(full, -1.0)
    with drv.App("hash://#64,64,64,16", W, H, **kw) as app:
        setup(app)
        for bands in layout:
            if not bands:
                continue
            app.set_bands(bands)
            fb, _ = app.render_frame()
            off = 0
            for (y0, h) in bands:
                out[y0:y0 + h] = fb[off:off + h]
                off += h
    if mode == 1:
        # the LDS-staged kernel takes a sample from the staged box or by gathers depending on the lanes that
        # share its wave; the two code paths contract their multiply-adds differently: the last bit may differ
        assert np.abs(out - full).max() <= 5e-7, (seed, W, H, world, bpr, mode)
    else:
        assert (out == full).all(), (seed, W, H, world, bpr, mode)


def _with_ancestors(ids):
    seen, out = set(), []
    for nid in ids:
        cur = int(nid)
        while cur not in seen:
            seen.add(cur)
            out.append(cur)
            if (cur & 0xF) == 0:
                break
            cur = int(orc.lib().orc_nodeid_parent(C.c_uint64(cur)))
    return out


@pytest.mark.parametrize("seed", range(10 * scenes.FUZZ_SCALE))
def test_per_ray_lod_through_the_plugin_matches_the_oracle(drv, seed):
    # EXTENSION (BASELINE C5): the pipeline makes the ancestors of the SelectVisibles cut resident and
    # the renderer applies the screen-space-error rule along every ray; the oracle renders the
    # same hierarchy with the same rule
    from libre_amd import vrc
    rng = np.random.default_rng(7300 + seed)
    vox = int(rng.choice([64, 128]))
    volume = str(rng.choice(["mem", "hash"]))
    W, H = int(rng.integers(40, 120)), int(rng.integers(40, 120))
    eye = (float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(0.6, 1.8)))
    spin = (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.2, 1.2)))
    sse = float(rng.choice([0.5, 1.0, 2.0, 3.0])) * vox / 64.0 * 48.0 / H
    uri = "%s://#%d,%d,%d,16" % (volume, vox, vox, vox)
    with drv.App(uri, W, H, synchronous=bool(seed % 2 == 0), sse=sse, gpu_cache_mb=64) as app:
        app.set_camera(position=eye, spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.3))
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        app.set_ray_lod(True)
        ids = app.visible_set()
        fb, st = app.render_frame()
        for _ in range(200):  # asynchronous mode: until the whole hierarchy is resident
            if st.n_not_available == 0:
                break
            app.wait_uploads()
            fb, st = app.render_frame()
        assert st.n_not_available == 0
        if not ids:
            assert (fb == 0).all()
            return
        assert st.ray_lod == 1 and st.n_passes <= 1
        hierarchy = _with_ancestors(ids)
        assert st.n_available == len(hierarchy)
        s = orc.build_scene(voxels=(vox, vox, vox), block=16, viewport=(W, H), ids=hierarchy, spin=spin, eye=eye,
                            volume=volume, alpha=0.3)
        assert st.samples_per_ray == s.render.samplesPerRay
        want, n_want = orc.oracle_render(s, threads=8, ray_lod=(sse, orc.world_space_per_pixel(s)))
        scenes.assert_parity(fb, want, "seed %d %s eye %r spin %r sse %g levels %r" % (
            seed, uri, eye, spin, sse, sorted({i & 0xF for i in hierarchy})), allow_frac=scenes.RAY_LOD_ALLOW)
        assert abs(int(app.stats().samples) - n_want) <= 5e-4 * n_want + 16
        # fewer samples than the per-brick cut of the same frame costs
        app.set_ray_lod(False)
        _, st2 = app.render_frame()
        assert st2.ray_lod == 0
        assert int(app.stats().samples) >= n_want - 16


def test_per_ray_lod_falls_back_when_the_hierarchy_does_not_fit(drv):
    from libre_amd import vrc
    with drv.App("hash://#128,128,128,16", 64, 64, synchronous=True, sse=0.5, gpu_cache_mb=1) as app:
        app.set_colormap(orc.linear_ramp_tf(0.3))
        ref, st_ref = app.render_frame()
        assert st_ref.n_passes > 1
        app.set_ray_lod(True)
        fb, st = app.render_frame()
        assert st.ray_lod == 0 and st.n_passes == st_ref.n_passes
        assert np.abs(fb - ref).max() <= 1e-6


def test_per_ray_lod_on_the_uvf_fixture(drv):
    # BASELINE C5's input format: a ragged UVF tree (75x75x138 voxels, 28^3 bricks, two levels whose brick
    # grids do not align) rendered with per-ray LOD + early ray termination through the plugin
    from libre_amd import vrc
    uri = "uvf://" + os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_reduced.uvf")
    for sse, alpha in ((1.0, 0.3), (1.6, 1.0), (0.4, 0.3)):
        with drv.App(uri, 112, 96, synchronous=True, sse=sse, gpu_cache_mb=8) as app:
            app.set_camera(spin=(0.6, 0.3))
            app.set_colormap(orc.linear_ramp_tf(alpha))
            app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
            app.set_ray_lod(True)
            ids = app.visible_set()
            fb, st = app.render_frame()
            assert st.ray_lod == 1
            hierarchy = _with_ancestors(ids)
            assert st.n_available == len(hierarchy)
            s = orc.scene_from_datasource(drv, uri, hierarchy, (112, 96), spin=(0.6, 0.3), alpha=alpha)
            assert s.render.samplesPerRay == st.samples_per_ray
            want, n_want = orc.oracle_render(s, threads=8, ray_lod=(sse, orc.world_space_per_pixel(s)))
            assert want[..., 3].max() > 0.3
            scenes.assert_parity(fb, want, "uvf per-ray lod sse %g" % sse, allow_frac=scenes.RAY_LOD_ALLOW)
            assert abs(int(app.stats().samples) - n_want) <= 5e-4 * n_want + 16


def test_repeated_frames_take_the_kept_brick_list_and_stay_correct(drv):
    # a frame whose visible-set inputs repeat is rendered from the kept brick list and the kept sorted
    # node table (no tree traversal, no cache look-ups, no sort); anything that changes the frame
    # must still change it: transfer function (not part of the key: applied per frame), camera,
    # screen-space error, clip planes, per-ray LOD
    from libre_amd import vrc

    def fresh(setup):
        with drv.App("hash://#64,64,64,16", 96, 80, synchronous=True, sse=1.0) as a:
            setup(a)
            return a.render_frame()[0]

    with drv.App("hash://#64,64,64,16", 96, 80, synchronous=True, sse=1.0) as app:
        app.set_colormap(orc.linear_ramp_tf(0.3))
        first, st = app.render_frame()
        for _ in range(3):
            again, st2 = app.render_frame()
            assert (again == first).all() and st2.n_available == st.n_available
        app.set_colormap(orc.linear_ramp_tf(1.0))
        got, _ = app.render_frame()
        assert np.abs(got - first).max() > 0.05
        assert (got == fresh(lambda a: a.set_colormap(orc.linear_ramp_tf(1.0)))).all()
        app.set_camera(spin=(0.4, 0.2))
        got, _ = app.render_frame()
        assert (got == fresh(lambda a: (a.set_colormap(orc.linear_ramp_tf(1.0)), a.set_camera(spin=(0.4, 0.2))))).all()
        app.set_clip_planes([[0.0, 0.0, 1.0, 0.2]])
        got, _ = app.render_frame()
        assert (got == fresh(lambda a: (a.set_colormap(orc.linear_ramp_tf(1.0)), a.set_camera(spin=(0.4, 0.2)),
                                        a.set_clip_planes([[0.0, 0.0, 1.0, 0.2]])))).all()
        app.set_clip_planes([])
        app.set_ray_lod(True)
        lod, st3 = app.render_frame()
        assert st3.ray_lod == 1
        lod2, st4 = app.render_frame()  # kept path keeps the mode
        assert st4.ray_lod == 1 and (lod2 == lod).all()
        app.set_ray_lod(False)
        back, st5 = app.render_frame()
        assert st5.ray_lod == 0
        assert (back == fresh(lambda a: (a.set_colormap(orc.linear_ramp_tf(1.0)), a.set_camera(spin=(0.4, 0.2))))).all()


def test_per_ray_lod_row_bands_are_rows_of_the_full_frame(drv):
    # BASELINE C5 is sort-first over 8 GPUs: a rank's bands rendered with per-ray LOD in one launch
    # equal those rows of the full per-ray-LOD frame bit for bit (the level choice depends on the
    # ray alone), also on the ragged UVF tree
    uvf = "uvf://" + os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_reduced.uvf")
    for uri, sse in (("hash://#128,128,128,16", 1.5), (uvf, 1.2)):
        W, H = 72, 64
        kw = dict(synchronous=True, sse=sse, gpu_cache_mb=64)
        with drv.App(uri, W, H, **kw) as full_app:
            full_app.set_camera(spin=(0.5, 0.35))
            full_app.set_colormap(orc.linear_ramp_tf(0.3))
            full_app.set_ray_lod(True)
            full, st = full_app.render_frame()
            assert st.ray_lod == 1 and full[..., 3].max() > 0.1
        bands = [(8, 8), (40, 16), (24, 8)]
        with drv.App(uri, W, H, **kw) as app:
            app.set_bands(bands)
            app.set_camera(spin=(0.5, 0.35))
            app.set_colormap(orc.linear_ramp_tf(0.3))
            app.set_ray_lod(True)
            fb, st = app.render_frame()
            assert st.ray_lod == 1 and fb.shape == (32, W, 4)
            want = np.concatenate([full[y0:y0 + h] for (y0, h) in bands], axis=0)
            assert (fb == want).all()


def test_moving_camera_keeps_the_brick_list_and_stays_correct(drv):
    # a camera that moves a little sees the same bricks: the pipeline keeps the brick list and the renderer
    # its node table (the grid kernels do not care for the order of the list); every frame must be the
    # frame a fresh application renders from that camera, and the reference-order kernel must get
    # its sorted list back the moment it is asked for
    from libre_amd import vrc
    uri = "hash://#64,64,64,16"

    def fresh(spin, kernel):
        with drv.App(uri, 80, 64, synchronous=True, sse=1.0) as a:
            a.set_colormap(orc.linear_ramp_tf(0.3))
            a.set_option(vrc.OPT_KERNEL, kernel)
            a.set_camera(spin=spin)
            return a.render_frame()[0]

    with drv.App(uri, 80, 64, synchronous=True, sse=1.0) as app:
        app.set_colormap(orc.linear_ramp_tf(0.3))
        for i, spin in enumerate([(0.0, 0.0), (0.05, 0.02), (0.4, 0.3), (1.7, -0.6), (1.72, -0.6), (3.0, 1.0)]):
            app.set_camera(spin=spin)
            got, st = app.render_frame()
            assert (got == fresh(spin, vrc.KERNEL_AUTO)).all(), spin
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_REFERENCE_ORDER)
        for spin in [(3.0, 1.0), (2.9, 0.9), (0.3, -1.0)]:
            app.set_camera(spin=spin)
            got, _ = app.render_frame()
            assert (got == fresh(spin, vrc.KERNEL_REFERENCE_ORDER)).all(), spin
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_AUTO)
        app.set_ray_lod(True)
        for spin in [(0.3, -1.0), (0.32, -1.0), (1.0, 0.5)]:
            app.set_camera(spin=spin)
            got, st = app.render_frame()
            assert st.ray_lod == 1
            with drv.App(uri, 80, 64, synchronous=True, sse=1.0) as a:
                a.set_colormap(orc.linear_ramp_tf(0.3))
                a.set_ray_lod(True)
                a.set_camera(spin=spin)
                assert (got == a.render_frame()[0]).all(), spin


def test_moving_camera_on_a_list_that_is_not_a_grid_with_the_trilinear_filter(drv):
    # the renderer keeps its sorted node list across a camera move only while the last frame found its bricks through
    # the brick grid.  On a list that is not a grid (the ragged UVF tree) the tap-packed kernel, which AUTO takes for the
    # trilinear filter, marches the list in its order like the reference-order kernel: a camera that reorders the same
    # bricks must get a freshly sorted list -- with the packed atlas, without it (gathers) and with the reference-order
    # kernel asked for
    from libre_amd import vrc
    W, H = 56, 48
    kw = dict(synchronous=True, min_lod=1, max_lod=1, gpu_cache_mb=8)
    spins = [(0.0, 0.0), (0.05, 0.02), (3.14, 0.0), (1.57, 0.3)]

    def setup(a, options, spin):
        a.set_colormap(orc.linear_ramp_tf(0.3))
        for o, v in options:
            a.set_option(o, v)
        a.set_camera(spin=spin)

    L = vrc.load_library()
    leaves = None
    # (options besides the filter, the list-order instance the frames must come from: vrc_k_raycast<false,...>)
    for extra, instance in (([], ",6,unsigned int,12,"), ([(vrc.OPT_PACKED_ATLAS, 0)], ",1,unsigned char,"),
                            ([(vrc.OPT_KERNEL, vrc.KERNEL_REFERENCE_ORDER)], ",1,unsigned char,")):
        options = [(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR)] + extra
        with drv.App(nongrid.UVF, W, H, **kw) as app:
            for spin in spins:
                setup(app, options, spin)
                got, st = app.render_frame()
                ran = L.vrc_last_kernel().decode()
                assert ran.startswith("vrc_k_raycast<false,") and instance in ran, (extra, ran)
                assert st.n_available == 45 and st.n_passes == 1
                visible = sorted(app.visible_set())
                leaves = leaves or visible
                assert visible == leaves and len(leaves) == 45  # the same bricks in every view
                with drv.App(nongrid.UVF, W, H, **kw) as ref:
                    setup(ref, options, spin)
                    want, _ = ref.render_frame()
                    order = ref.node_order()
                assert (got == want).all(), (extra, spin, float(np.abs(got - want).max()))
                assert app.node_order() == order, (extra, spin)


@pytest.mark.parametrize("seed", range(6 * scenes.FUZZ_SCALE))
def test_random_frame_sequences_equal_fresh_applications(drv, seed):
    # the pipeline and the renderer keep state between frames (brick list, node table, tile schedule,
    # classified tables): after any sequence of changes a frame must be the frame a fresh application
    # renders with the same settings -- bit for bit with the gather kernels.  Every third seed on the ragged UVF tree
    # (a list that is not a grid: every kernel marches it in list order)
    from libre_amd import vrc
    rng = np.random.default_rng(11000 + seed)
    volume = str(rng.choice(["hash", "mem"]))
    uri = nongrid.UVF if seed % 3 == 2 else "%s://#64,64,64,16" % volume
    W, H = int(rng.integers(24, 72)), int(rng.integers(24, 72))
    sync = bool(rng.random() < 0.8)
    state = dict(spin=(0.0, 0.0), eye=(0.0, 0.0, 1.5), alpha=0.3, planes=[], ray_lod=False, kernel=vrc.KERNEL_AUTO,
                 flt=vrc.FILTER_NEAREST, bands=[])
    sse = float(rng.choice([0.5, 1.0, 2.0]))

    def apply(app, st):
        app.set_camera(position=st["eye"], spin=st["spin"])
        app.set_colormap(orc.linear_ramp_tf(st["alpha"]))
        app.set_clip_planes(st["planes"])
        app.set_ray_lod(st["ray_lod"])
        app.set_option(vrc.OPT_KERNEL, st["kernel"])
        app.set_option(vrc.OPT_FILTER, st["flt"])
        app.set_bands(st["bands"])
        if not st["bands"]:
            app.height = H

    def settle(app):
        fb, st = app.render_frame()
        for _ in range(200):
            if st.n_not_available == 0:
                break
            app.wait_uploads()
            fb, st = app.render_frame()
        assert st.n_not_available == 0
        return fb

    with drv.App(uri, W, H, synchronous=sync, sse=sse, gpu_cache_mb=16) as app:
        for step in range(8):
            what = int(rng.integers(0, 9))
            if what == 0:    # small camera move
                state["spin"] = (state["spin"][0] + float(rng.uniform(-0.03, 0.03)), state["spin"][1] + float(rng.uniform(-0.03, 0.03)))
            elif what == 1:  # big camera move
                state["spin"] = (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.2, 1.2)))
                state["eye"] = (float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(0.7, 1.8)))
            elif what == 2:
                state["alpha"] = float(rng.choice([0.05, 0.3, 1.0]))
            elif what == 3:
                state["planes"] = [] if state["planes"] else [[0.0, 0.6, 0.8, float(rng.uniform(0.1, 0.3))]]
            elif what == 4:
                state["ray_lod"] = not state["ray_lod"]
            elif what == 5:
                state["kernel"] = int(rng.choice([vrc.KERNEL_AUTO, vrc.KERNEL_REFERENCE_ORDER]))
            elif what == 6:
                state["bands"] = [] if state["bands"] else [(8, 8), (H - 12, 8)]
            elif what == 8:
                state["flt"] = vrc.FILTER_TRILINEAR if state["flt"] == vrc.FILTER_NEAREST else vrc.FILTER_NEAREST
            # what == 7: the same frame again
            if state["ray_lod"]:
                state["kernel"] = vrc.KERNEL_AUTO  # per-ray LOD has its own kernel
            apply(app, state)
            got = settle(app)
            with drv.App(uri, W, H, synchronous=True, sse=sse, gpu_cache_mb=16) as ref:
                apply(ref, state)
                want = ref.render_frame()[0]
            assert got.shape == want.shape and (got == want).all(), (seed, step, what, state, sync)


def test_nrrd_volume_through_the_plugin_matches_the_oracle(drv):
    # the reference's NRRD fixture (tests/lib/nucleon.nrrd -> nucleon.raw, 41^3 uint8, one brick, overlap 0)
    # through data source, caches, upload and kernel, against the oracle's render of the same brick
    import os
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    s = scenes.nucleon_scene(viewport=(48, 48), spin=(0.4, 0.3), alpha=0.3)
    want, n_want = orc.oracle_render(s, threads=8)
    from libre_amd import vrc
    with drv.App("raw://" + os.path.join(gdir, "nucleon.nrrd"), 48, 48, synchronous=True, gpu_cache_mb=16) as app:
        app.set_camera(spin=(0.4, 0.3))
        app.set_colormap(orc.linear_ramp_tf(0.3))
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        fb, st = app.render_frame()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        scenes.assert_parity(fb, want, "nucleon.nrrd through the plugin")
        assert abs(int(app.stats().samples) - n_want) <= 8


def _fake_rccl():
    """tests/host_san/fake_rccl.cpp built next to its source (atomic rename: parallel workers)."""
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_san")
    src, out = os.path.join(here, "fake_rccl.cpp"), os.path.join(here, "libfake_rccl.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-shared", "-fPIC",
                        "--offload-arch=gfx950", "-o", tmp, src], check=True, capture_output=True, timeout=300)
        os.replace(tmp, out)
    return out


@pytest.mark.parametrize("world,bands,batch", [(2, 1, 1), (2, 3, 2), (3, 2, 2), (4, 5, 1)])
def test_abi_gather_with_several_ranks_on_one_gpu(drv, world, bands, batch):
    # vrc_gather_tiles with world > 1: the ranks are threads with a plugin instance each, RCCL is replaced by a
    # test double that moves the bands with device copies and fails on any unmatched send / receive
    # (tests/gpu_fake_rccl_gather.py): bands land at their rows, frames bit-identical to the one-rank frames
    import subprocess
    import sys
    env = dict(os.environ, VRC_RCCL_LIBRARY=_fake_rccl())
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_fake_rccl_gather.py")
    r = subprocess.run([sys.executable, script, str(world), str(bands), str(batch)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_reference_order_tile_culling_with_row_bands_and_mixed_levels(drv):
    # the reference-order kernel first culls the brick list per 8x8 tile (vrc_core.h, "tile culling").  Row bands
    # whose heights are not multiples of 8 put rows of two bands -- frame rows far apart -- into one tile: the tile's
    # pyramid must span them.  Mixed brick sizes (an LOD cut) make AUTO take that kernel; the stacked bands equal
    # the rows of the full frame bit for bit, and the full frame matches the oracle
    from libre_amd import vrc
    W, H = 56, 72
    kw = dict(synchronous=True, sse=2.0, gpu_cache_mb=16)
    eye, spin = (0.15, -0.1, 0.9), (0.7, -0.4)
    with drv.App("hash://#128,128,128,16", W, H, **kw) as app:
        app.set_camera(position=eye, spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.3))
        ids = app.visible_set()
        assert len({i & 0xF for i in ids}) > 1 and len(ids) > 64  # several levels, more bricks than one culling step
        auto, _ = app.render_frame()  # AUTO: the reference-order kernel for a list of mixed brick sizes
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_REFERENCE_ORDER)
        full, st = app.render_frame()
        assert (auto == full).all()
        s = orc.build_scene(voxels=(128, 128, 128), block=16, viewport=(W, H), ids=ids, spin=spin, eye=eye,
                            volume="hash", alpha=0.3, order=app.node_order())
        want, _ = orc.oracle_render(s, threads=8)
        scenes.assert_parity(full, want, "LOD cut, reference order with tile culling")
        bands = [(3, 5), (50, 13), (21, 7), (64, 8)]
        app.set_bands(bands)
        fb, _ = app.render_frame()
        stacked = np.concatenate([full[y0:y0 + h] for (y0, h) in bands], axis=0)
        assert fb.shape == stacked.shape and (fb == stacked).all()
        app.set_bands([])
        app.height = H
        again, _ = app.render_frame()
        assert (again == full).all()


def test_layout_bands_are_checked_in_64_bits(drv):
    # lvh_app_set_layout: y0 + h must not wrap (y0 = 0xFFFFFFFF, h = 2 passed the 32-bit sum and became an
    # out-of-bounds device write on the display rank; round-2 advisor finding)
    with drv.App("mem://#64,64,64,16", 48, 40, device=0, synchronous=True) as app:
        app.set_layout([[(0, 20), (20, 20)]])
        for bad in ([(39, 2)], [(0xFFFFFFFF, 2)], [(40, 0xFFFFFFFF)], [(1, 40)]):
            with pytest.raises(RuntimeError):
                app.set_layout([bad])


@pytest.mark.parametrize("spin", [(0.0, 0.0), (0.5, 0.35), (1.5, 0.2)])
def test_per_ray_lod_in_slabs_when_the_hierarchy_exceeds_the_atlas(drv, spin):
    # per-ray LOD with an atlas of a fraction of the hierarchy: round 2 fell back to the per-brick cut (stats.ray_lod = 0);
    # now the frame is rendered in slabs of space across the view's main axis (renderRayLodInSlabs), every level's bricks
    # of a slab resident, front to back into the accumulating pixel buffer.  It equals the single-pass per-ray LOD frame
    # of a large atlas up to the sampling restarts at the slab faces.
    from libre_amd import vrc
    uri, W, H, sse = "hash://#128,128,128,16", 96, 80, 0.6
    frames = {}
    for mb in (256, 2):  # 13824-byte slots: 2 MiB hold ~150 of the hierarchy's 512 + 64 + 8 + 1 bricks
        with drv.App(uri, W, H, synchronous=True, sse=sse, gpu_cache_mb=mb) as app:
            app.set_camera(spin=spin)
            app.set_colormap(orc.linear_ramp_tf(0.1))
            app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
            app.set_ray_lod(True)
            fb, st = app.render_frame()
            assert st.ray_lod == 1, "atlas of %d MiB" % mb
            frames[mb] = (fb, int(app.stats().samples), st.n_passes, st.n_available)
            again, st2 = app.render_frame()   # and the same frame again, slots re-used
            assert st2.ray_lod == 1 and (again == fb).all()
    (whole, n_whole, p_whole, avail_whole), (slabbed, n_slab, p_slab, avail_slab) = frames[256], frames[2]
    assert p_whole <= 1 and p_slab >= 3 and avail_slab == avail_whole
    # (noise data: a restart at a slab face shifts that run's samples by a fraction of a step -- isolated pixels differ
    # by a few 1e-2, the frame mean by a few 1e-4)
    scenes.assert_close_frames(slabbed, whole, "slabs of a small atlas against the single pass", max_abs=SLAB_MAX_ABS, mean_abs=SLAB_MEAN_ABS)
    assert 0 < n_slab < n_whole  # (the counter is the last launch's: the last slab)


def test_per_ray_lod_in_slabs_in_asynchronous_mode(drv):
    # Round 3's slabs were for --synchronous only; in asynchronous mode (CudaRaycastPipeline.cpp:236-301: render what is
    # resident, load the rest in the background, ask for a redraw) a hierarchy larger than the atlas fell back to the
    # per-brick cut.  Now a frame renders the front-to-back prefix of slabs whose bricks have reached the CPU cache:
    # the first frame has nothing, later frames grow from the front, and the settled frame is the synchronous one.
    uri, W, H, sse, spin = "hash://#128,128,128,16", 96, 80, 0.6, (0.5, 0.35)
    with drv.App(uri, W, H, synchronous=True, sse=sse, gpu_cache_mb=2) as sync:
        sync.set_camera(spin=spin)
        sync.set_colormap(orc.linear_ramp_tf(0.4))
        sync.set_ray_lod(True)
        want, st = sync.render_frame()
        assert st.ray_lod == 1 and st.n_passes >= 3
        n_slabs = st.n_passes
    with drv.App(uri, W, H, synchronous=False, sse=sse, gpu_cache_mb=2) as app:
        app.set_camera(spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.4))
        app.set_ray_lod(True)
        fb0, st0 = app.render_frame()
        assert st0.n_not_available > 0 and st0.n_passes == 0 and not fb0.any()  # nothing has arrived: no slab yet
        app.wait_uploads()
        fb1, st1 = app.render_frame()
        assert st1.ray_lod == 1 and st1.n_not_available == 0 and st1.n_passes == n_slabs
        assert (fb1 == want).all()
    # a partial frame is the front of the volume: with the CPU cache holding only the bricks of the first slabs, the
    # frame equals the synchronous frame wherever the rays end inside them (opaque transfer function: early exits)
    # -- here simply: monotone growth, every partial frame's opacity is bounded by the full frame's
    with drv.App(uri, W, H, synchronous=False, sse=sse, gpu_cache_mb=2) as app:
        app.set_camera(spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.4))
        app.set_ray_lod(True)
        last, grew = None, 0
        import time
        for _ in range(2000):  # (the loader fills the CPU cache meanwhile, slab by slab from the front)
            time.sleep(0.002)
            fb, st = app.render_frame()
            assert (st.ray_lod == 1 or st.n_passes == 0) and np.isfinite(fb).all()
            assert (fb[..., 3] <= want[..., 3] + 1e-6).all()  # a prefix of the slabs: never more opaque than the whole
            if last is not None:
                assert (fb[..., 3] >= last[..., 3] - 1e-6).all()  # the camera stands still: frames only grow
                grew += int((fb[..., 3] > last[..., 3] + 1e-6).any())
            last = fb
            if st.n_not_available == 0:
                break
        assert st.n_not_available == 0 and (fb == want).all()
        assert grew >= 2, "the frame filled in slab by slab (%d growth steps)" % grew
    # a CPU cache too small for the hierarchy: the per-brick cut, as before
    with drv.App(uri, W, H, synchronous=False, sse=sse, gpu_cache_mb=2, cpu_cache_mb=1) as app:
        app.set_camera(spin=spin)
        app.set_colormap(orc.linear_ramp_tf(0.4))
        app.set_ray_lod(True)
        fb, st = app.render_frame()
        assert st.ray_lod == 0


#: what the sampling restarts at slab faces cost against the single pass: isolated pixels / the frame mean.  Measured on
#: MI355X with the slabs in the rays' order: max 1.8e-2, mean 8.0e-4 (the axis-aligned view of the 128^3 scene: eight
#: slabs, every coarse-level run cut seven times, transfer function of alpha 0.1); what a wrong ORDER costs is measured
#: in test_per_ray_lod_slabs_are_ordered_along_the_rays
SLAB_MAX_ABS, SLAB_MEAN_ABS = 2.5e-2, 1e-3


@pytest.mark.parametrize("case", ["eye inside, looking across centre - eye", "flat volume, eye beside it on another axis",
                                  "eye inside, looking along the diagonal"])
def test_per_ray_lod_slabs_are_ordered_along_the_rays(drv, case):
    # Round 3 took the slab axis and direction from (centre of the hierarchy - eye).  With the eye inside the hierarchy's
    # extent along that axis there are rays of both signs; the ones that run the other way crossed into a slab that had
    # been composited already -- back to front (advisor).  Now an axis serves only if every ray that meets
    # the hierarchy runs one way along it (eye outside the extent on that axis, or the four corner rays of the frustum
    # agree); none: per-brick cut.  Reference passes are front to back by the sorted list: CudaRaycastPipeline.cpp:107-127, :149-185.
    from libre_amd import vrc
    if case == "eye inside, looking across centre - eye":
        # centre - eye = (-0.1, 0, -0.2): round 3 sliced across z, front = high z; the view looks along +x
        uri, mb, cam = "hash://#256,256,256,32", 2, dict(position=(0.1, 0.0, 0.2), lookat=(1.0, 0.0, 0.2))
    elif case.startswith("flat"):
        # 192 x 128 x 64 voxels: world box (+-0.5, +-0.333, +-0.167); the eye is outside in z only; |centre - eye| is the
        # same along x and z and round 3's tie went to x, along which the rays run both ways
        uri, mb, cam = "hash://#192,128,64,16", 1, dict(position=(0.3, 0.0, 0.3), lookat=(0.3, 0.0, -1.0))
    else:
        # eye inside on every axis, the view along the diagonal: only the corner rays can tell which axes serve
        uri, mb, cam = "hash://#128,128,128,16", 1, dict(position=(-0.2, -0.1, -0.25), lookat=(1.0, 1.0, 1.0))
    W, H, sse = 96, 80, 0.6
    # Transfer functions under which the ORDER matters (at alpha 0.1 compositing nearly commutes and a reversed order
    # only doubles the restart error).  Measured on MI355X, slabs in the rays' order / reversed on purpose:
    #   alpha 0.4: max <= 9.9e-3, mean <= 7.0e-4  /  max >= 3.1e-2, mean >= 5.9e-3
    #   alpha 1.0: max <= 1.0e-3, mean <= 1.8e-5  /  max >= 9.1e-2, mean >= 1.5e-2   (rays end before most slab faces)
    for alpha, max_abs, mean_abs in ((0.4, SLAB_MAX_ABS, SLAB_MEAN_ABS), (1.0, 2.5e-3, 1e-4)):
        frames = {}
        for cache in (256, mb):  # an atlas for the whole visible hierarchy / for a part of it (at least one layer of bricks)
            with drv.App(uri, W, H, synchronous=True, sse=sse, gpu_cache_mb=cache) as app:
                app.set_camera(**cam)
                app.set_colormap(orc.linear_ramp_tf(alpha))
                app.set_ray_lod(True)
                fb, st = app.render_frame()
                frames[cache] = (fb, st.ray_lod, st.n_passes)
        (whole, lod_whole, p_whole), (small, lod_small, p_small) = frames[256], frames[mb]
        assert lod_whole == 1 and p_whole <= 1 and whole[..., 3].max() > 0.05
        assert lod_small == 1 and p_small >= 2, (lod_small, p_small)
        mx, mean = scenes.assert_close_frames(small, whole, "%s, alpha %g" % (case, alpha), max_abs=max_abs, mean_abs=mean_abs)
        print("slab order, %s, alpha %g: %d slabs, max|d| %.3g mean|d| %.3g" % (case, alpha, p_small, mx, mean))
