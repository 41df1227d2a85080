"""A shaded composite frame through the plugin surface (libre_amd.driver.App) on the GPU: lvh_app_set_option hands
VRC_OPT_SHADING and VRC_OPT_SHADING_AMBIENT to every renderer of the app; a mem:// volume, whose bricks hold one value
each, renders the unshaded frame; the nucleon brick passes the rule of tests/shade_ref.py."""
import os

import numpy as np
import pytest

import orc
import shade_ref
from libre_amd import vrc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def test_mem_volume_is_the_unshaded_frame(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.8))
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        plain, st0 = app.render_frame()
        assert plain[..., 3].max() > 0.3
        for uniform in (1, 0):
            app.set_option(vrc.OPT_UNIFORM_BRICKS, uniform)
            app.set_shading(True, 0.1)
            assert app.get_option(vrc.OPT_SHADING) == 1 and app.get_option(vrc.OPT_SHADING_AMBIENT) == 100
            lit, st = app.render_frame()
            assert b"vrc_k_raycast_shade<" in vrc.load_library().vrc_last_kernel()
            assert np.array_equal(lit, plain) and st.samples == st0.samples, uniform
            app.set_shading(False)
        for bad in (2, -1):
            with pytest.raises(drv.DriverError) as e:
                app.set_option(vrc.OPT_SHADING, bad)
            assert "VRC_OPT_SHADING" in str(e.value)
        with pytest.raises(drv.DriverError) as e:
            app.set_option(vrc.OPT_SHADING_AMBIENT, 1001)
        assert "VRC_OPT_SHADING_AMBIENT" in str(e.value)
        assert np.array_equal(app.render_frame()[0], plain)


def test_nucleon_passes_the_rule(drv):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nucleon.nrrd")
    s, r = shade_ref.scene("nucleon"), shade_ref.ref("nucleon", 0)
    with drv.App("raw://" + path, 44, 36, synchronous=True, gpu_cache_mb=16) as app:
        app.set_camera(spin=(0.4, 0.3))
        app.set_colormap(s.tf)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        plain, st0 = app.render_frame()
        app.set_shading(True, shade_ref.AMBIENT)
        fb, st = app.render_frame()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        shade_ref.check(s, fb, r, "nucleon through the plugin")
        assert np.array_equal(fb[..., 3], plain[..., 3]) and st.samples == st0.samples
        assert not np.array_equal(fb, plain)


def test_both_options_reach_every_renderer(drv):
    with drv.App("hash://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.3))
        app.set_frames_in_flight(2)
        plain = app.render_frame()[0]
        app.set_shading(True, 0.4)
        frames = []
        for slot in (0, 1):
            app.select_slot(slot)
            assert app.get_option(vrc.OPT_SHADING) == 1 and app.get_option(vrc.OPT_SHADING_AMBIENT) == 400, slot
            frames.append(app.render_frame()[0])
            assert b"vrc_k_raycast_shade<" in vrc.load_library().vrc_last_kernel()
        assert np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], plain)
        assert np.array_equal(frames[0][..., 3], plain[..., 3])
        # ... and a renderer made afterwards
        app.set_frames_in_flight(3)
        app.select_slot(2)
        assert app.get_option(vrc.OPT_SHADING) == 1 and app.get_option(vrc.OPT_SHADING_AMBIENT) == 400
        assert np.array_equal(app.render_frame()[0], frames[0])
        # a change of the ambient share reaches all three
        app.set_option(vrc.OPT_SHADING_AMBIENT, 1000)
        for slot in (0, 1, 2):
            app.select_slot(slot)
            assert np.array_equal(app.render_frame()[0], plain), slot
