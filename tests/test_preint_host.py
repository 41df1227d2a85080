"""A pre-integrated composite frame through the plugin surface (libre_amd.driver.App) on the GPU: lvh_app_set_option hands
VRC_OPT_PREINTEGRATION to every renderer of the app, those made later included; the nucleon brick passes the rule of
tests/preint_ref.py; setting the option back to 0 restores the plain frame bit for bit."""
import os

import numpy as np
import pytest

import orc
import preint_ref
from libre_amd import vrc

pytestmark = pytest.mark.gpu
NAME = b"vrc_k_raycast_preint<"


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def test_nucleon_passes_the_rule_and_zero_restores_the_plain_frame(drv):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nucleon.nrrd")
    s, r = preint_ref.scene("nucleon"), preint_ref.ref("nucleon", 0)
    with drv.App("raw://" + path, 44, 36, synchronous=True, gpu_cache_mb=16) as app:
        app.set_camera(spin=(0.4, 0.3))
        app.set_colormap(s.tf)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        plain, _ = app.render_frame()
        n_plain = int(app.stats().samples)
        assert NAME not in vrc.load_library().vrc_last_kernel() and n_plain > 0
        app.set_preintegration(1)
        assert app.get_option(vrc.OPT_PREINTEGRATION) == 1
        fb, st = app.render_frame()
        assert NAME in vrc.load_library().vrc_last_kernel()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        preint_ref.check(s, fb, r, "nucleon through the plugin")
        assert abs(int(app.stats().samples) - r.samples) <= 1e-4 * r.samples + 8
        assert not np.array_equal(fb, plain)
        app.set_preintegration(0)
        assert app.get_option(vrc.OPT_PREINTEGRATION) == 0
        again, _ = app.render_frame()
        assert NAME not in vrc.load_library().vrc_last_kernel()
        assert np.array_equal(again, plain) and int(app.stats().samples) == n_plain
        for bad in (2, -1):
            with pytest.raises(drv.DriverError) as e:
                app.set_option(vrc.OPT_PREINTEGRATION, bad)
            assert "VRC_OPT_PREINTEGRATION" in str(e.value)
        assert np.array_equal(app.render_frame()[0], plain)


def test_the_option_reaches_every_renderer(drv):
    with drv.App("hash://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.3))
        app.set_frames_in_flight(2)
        plain = app.render_frame()[0]
        app.set_preintegration(1)
        frames = []
        for slot in (0, 1):
            app.select_slot(slot)
            assert app.get_option(vrc.OPT_PREINTEGRATION) == 1, slot
            frames.append(app.render_frame()[0])
            assert NAME in vrc.load_library().vrc_last_kernel()
        assert np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], plain)
        # ... and a renderer made afterwards
        app.set_frames_in_flight(3)
        app.select_slot(2)
        assert app.get_option(vrc.OPT_PREINTEGRATION) == 1
        assert np.array_equal(app.render_frame()[0], frames[0])
        # back to 0: the plain frame on all three, bit for bit
        app.set_preintegration(0)
        for slot in (0, 1, 2):
            app.select_slot(slot)
            assert app.get_option(vrc.OPT_PREINTEGRATION) == 0
            assert np.array_equal(app.render_frame()[0], plain), slot
            assert NAME not in vrc.load_library().vrc_last_kernel()
