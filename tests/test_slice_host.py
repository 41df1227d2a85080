"""A slice frame through the plugin surface (libre_amd.driver.App) on the GPU: App.set_slice reaches every renderer as
the isosurface does, before and after a renderer is made; the frame is the C ABI's frame of the same scene, and App.pick
answers (hit, value, t, xyz) of the C ABI's read-backs -- the voxel under the cursor and the point on the plane."""
import numpy as np
import pytest

import mip_scenes
import orc
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

POINT, NORMAL = (0.02, -0.01, 0.03), (0.31, -0.42, 0.85)
PROJECTION_SLICE = getattr(vrc, "PROJECTION_SLICE", 4)


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _plane(point=POINT, normal=NORMAL):
    """what App.set_slice hands down: (n, d = -n . point), formed in double and rounded once"""
    d = -sum(float(a) * float(b) for a, b in zip(normal, point))
    return np.array([normal[0], normal[1], normal[2], d], dtype=np.float32)


def _abi(s, plane):
    """(frame, V, counts, D, xyz) of the scene through the C ABI"""
    with GpuScene(s) as g:
        vrc.set_slice(g.L, g.ctx, plane)
        vrc.check(g.L, g.L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, PROJECTION_SLICE))
        fb, _, _ = g.render()
        v = np.zeros((s.H, s.W), dtype=np.float32)
        c = np.zeros((s.H, s.W), dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
        return (fb, v, c) + vrc.projection_depths(g.L, g.ctx, s.W, s.H)


def test_set_slice_and_pick_on_the_mem_volume(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.8))
        with pytest.raises(drv.DriverError) as e:  # no plane yet: the device layer names the function
            app.set_option(vrc.OPT_PROJECTION, PROJECTION_SLICE)
        assert "vrc_set_slice" in str(e.value)
        for point, normal in ((POINT, (0.0, 0.0, 0.0)), (POINT, (float("nan"), 0.0, 1.0)), ((float("inf"), 0.0, 0.0), NORMAL)):
            with pytest.raises(drv.DriverError) as e:
                app.set_slice(point, normal)
            assert "plane" in str(e.value)
        app.set_slice(POINT, NORMAL)
        app.set_option(vrc.OPT_PROJECTION, PROJECTION_SLICE)
        fb, st = app.render_frame()
        ids = app.visible_set()
        s = mip_scenes.host_mem_scene(ids=ids, spr=int(st.samples_per_ray))
        afb, av, ac, at, ap = _abi(s, _plane())
        assert np.array_equal(fb, afb)
        hit = ac == 1
        assert hit.sum() >= 100 and (~hit).sum() >= 100
        consts = {float(b.flat[0]) for b in s.bricks.values()}
        assert set(np.unique(av[hit]).tolist()) <= consts  # mem://: the brick's constant under the cursor
        assert np.isfinite(at[hit]).all() and np.isposinf(at[~hit]).all() and not fb[~hit].any()
        n = np.array(NORMAL)
        assert np.abs(ap[hit].astype(np.float64) @ n - float(n @ np.array(POINT))).max() <= 1e-5
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
        # the plane and the projection reach a renderer made after they were set
        app.set_frames_in_flight(2)
        app.select_slot(1)
        assert np.array_equal(app.render_frame()[0], fb)
        y, x = [int(a[0]) for a in np.nonzero(hit)]
        assert app.pick(x, y) == (True, float(av[y, x]), float(at[y, x]), tuple(float(a) for a in ap[y, x]))
        # ... and a change reaches every one
        app.set_slice((0.0, 0.0, 0.2), (0.0, 0.0, 1.0))
        moved = app.render_frame()[0]
        assert not np.array_equal(moved, fb)
        assert np.array_equal(moved, _abi(s, _plane((0.0, 0.0, 0.2), (0.0, 0.0, 1.0)))[0])
        app.select_slot(0)
        assert np.array_equal(app.render_frame()[0], moved)
        # a bad plane leaves the one before
        with pytest.raises(drv.DriverError):
            app.set_slice(POINT, (0.0, 0.0, 0.0))
        assert np.array_equal(app.render_frame()[0], moved)
