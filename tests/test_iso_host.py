"""An isosurface frame through the plugin surface (libre_amd.driver.App) on the GPU: App.set_isosurface reaches every
renderer as the projection options do, the frame is the C ABI's frame of the same scene, and App.pick answers with the
surface under the pixel -- (hit, V, D, xyz) of the C ABI's read-backs -- or with no hit where the ray misses it."""
import numpy as np
import pytest

import mip_scenes
import orc
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

ISO, AMBIENT = 48.0, 0.25  # (the mem:// volume's bricks hold one value each, 18 to 78: about half of them reach 48)


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _abi(s):
    """(frame, V, counts, D, xyz, G) of the scene through the C ABI"""
    with GpuScene(s) as g:
        vrc.set_isosurface(g.L, g.ctx, ISO, AMBIENT)
        vrc.check(g.L, g.L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO))
        fb, _, _ = g.render()
        v = np.zeros((s.H, s.W), dtype=np.float32)
        c = np.zeros((s.H, s.W), dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
        return (fb, v, c) + vrc.projection_depths(g.L, g.ctx, s.W, s.H) + (vrc.projection_gradients(g.L, g.ctx, s.W, s.H),)


def test_set_isosurface_and_pick_on_the_mem_volume(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.8))
        with pytest.raises(drv.DriverError) as e:  # no isosurface yet: the device layer names the function
            app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
        assert "vrc_set_isosurface" in str(e.value)
        for bad in ((float("nan"), 0.5), (ISO, 1.5)):
            with pytest.raises(drv.DriverError):
                app.set_isosurface(*bad)
        app.set_isosurface(ISO, AMBIENT)
        app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
        fb, st = app.render_frame()
        ids = app.visible_set()
        s = mip_scenes.host_mem_scene(ids=ids, spr=int(st.samples_per_ray))
        afb, av, ac, at, ap, ag = _abi(s)
        assert np.array_equal(fb, afb)
        hit = ac == 1
        assert hit.sum() >= 100 and (~hit).sum() >= 100
        assert (av[hit] >= ISO).all() and np.isfinite(at[hit]).all() and np.isposinf(at[~hit]).all() and (ag[~hit] == 0).all()
        # a pick on every fourth pixel: the matching entry of the read-backs
        hits = misses = 0
        for y in range(0, 36, 2):
            for x in range(0, 44, 2):
                h, v, t, p = app.pick(x, y)
                assert h == bool(hit[y, x])
                if h:
                    hits += 1
                    assert v == av[y, x] and t == at[y, x] and p == tuple(float(a) for a in ap[y, x])
                else:
                    misses += 1
                    assert np.isposinf(t)
        assert hits >= 25 and misses >= 25
        with pytest.raises(drv.DriverError) as e:
            app.pick(44, 0)
        assert "outside the window" in str(e.value)
        # the isosurface reaches a renderer made after it was set
        app.set_frames_in_flight(2)
        app.select_slot(1)
        assert np.array_equal(app.render_frame()[0], fb)
        y, x = [int(a[0]) for a in np.nonzero(hit)]
        assert app.pick(x, y) == (True, float(av[y, x]), float(at[y, x]), tuple(float(a) for a in ap[y, x]))
        # ... and a change reaches every one
        app.set_isosurface(ISO, 1.0)
        flat = app.render_frame()[0]
        assert (flat[hit] == flat[hit][0]).all() and np.array_equal(flat[~hit], fb[~hit])
        app.select_slot(0)
        assert np.array_equal(app.render_frame()[0], flat)
