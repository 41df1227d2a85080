"""Maximum-intensity projection through the plugin surface (libre_amd.driver.App) on the GPU: the option reaches the
renderers through lvh_app_set_option, multi-pass frames meet in the context's running maxima, row bands are rows of the
full frame.  Frames are held to tests/mip_ref.py by its acceptance rule."""
import numpy as np
import pytest

import mip_ref
import mip_scenes
import orc
from libre_amd import vrc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _mip_app(app, spin=(0.5, 0.35), alpha=0.8):
    app.set_camera(spin=spin)
    app.set_colormap(orc.linear_ramp_tf(alpha))
    app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
    app.set_option(vrc.OPT_COUNT_SAMPLES, 1)


def test_mem_volume_in_synchronous_mode(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        _mip_app(app)
        fb, st = app.render_frame()
        ids = app.visible_set()
        assert st.n_passes == 1 and len(ids) == 64
        # the scene whose ambiguity tests/test_mip_cpu.py caps: the same bricks and step
        assert sorted(ids) == sorted(orc.leaf_ids(mip_scenes.host_mem_scene().vi))
        assert int(st.samples_per_ray) == mip_scenes.host_mem_scene().render.samplesPerRay
        s = mip_scenes.host_mem_scene(ids=ids, spr=int(st.samples_per_ray))
        r = mip_ref.render(s)
        bad, worst, amb = mip_ref.check_frame(s, r, fb)
        print("mem:// through the plugin: %d failing pixels (worst excess %.3g), %d ambiguous" % (bad, worst, amb))
        assert bad == 0
        # per-ray LOD asked for: the plugin renders its per-brick cut -- the same frame
        app.set_ray_lod(True)
        lod, _ = app.render_frame()
        assert not app.stats().ray_lod
        assert np.array_equal(lod, fb)
        # and composite again is the frame of an app that never heard of the option
        app.set_ray_lod(False)
        app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        comp, _ = app.render_frame()
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as plain:
        plain.set_camera(spin=(0.5, 0.35))
        plain.set_colormap(orc.linear_ramp_tf(0.8))
        want, _ = plain.render_frame()
    assert np.array_equal(comp, want)


def test_nucleon_single_brick_without_overlap(drv):
    import os
    # the reference's NRRD fixture (nucleon.nrrd -> nucleon.raw, 41^3 uint8, one brick, overlap 0)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nucleon.nrrd")
    s = mip_scenes.host_nucleon_scene()  # (tests/test_mip_cpu.py caps its ambiguous pixels)
    r = mip_ref.render(s)
    with drv.App("raw://" + path, 44, 36, synchronous=True, gpu_cache_mb=16) as app:
        _mip_app(app, spin=(0.4, 0.3))
        fb, st = app.render_frame()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        bad, worst, amb = mip_ref.check_frame(s, r, fb)
        print("nucleon through the plugin: %d failing pixels (worst excess %.3g), %d ambiguous" % (bad, worst, amb))
        assert bad == 0


def test_a_pool_smaller_than_the_brick_set_takes_several_passes(drv):
    frames = {}
    for mb in (1, 8):
        with drv.App("hash://#128,128,128,32", 40, 40, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=mb) as app:
            _mip_app(app)
            frames[mb], st = app.render_frame()
            assert st.n_passes == (4 if mb == 1 else 1) and st.n_available == 64
    assert frames[8][..., 3].max() > 0.3
    assert np.array_equal(frames[1], frames[8]), "the passes meet in the running maximum: the same frame, bit for bit"


def test_two_bands_are_rows_of_the_full_frame(drv):
    W, H = 48, 64
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("hash://#64,64,64,16", W, H, **kw) as full_app:
        _mip_app(full_app)
        full, _ = full_app.render_frame()
    bands = [(8, 8), (40, 16)]
    with drv.App("hash://#64,64,64,16", W, H, **kw) as app:
        app.set_bands(bands)
        _mip_app(app)
        fb, st = app.render_frame()
        assert fb.shape == (24, W, 4) and st.n_passes == 1
        assert np.array_equal(fb, np.concatenate([full[y0:y0 + h] for (y0, h) in bands], axis=0))
