"""Picking in a composite frame through the plugin surface (libre_amd.driver.App.pick) on the GPU:
App.set_composite_depth reaches every renderer through lvh_app_set_option, a pick is the matching entry of the C ABI's
read-back of the same scene, a ray that stays below the threshold is no hit, and with the option at 0 the pick refuses a
composite frame as it did."""
import os

import numpy as np
import pytest

import mip_scenes
import orc
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

K = 500


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _app(app, spin=(0.5, 0.35), k=K):
    app.set_camera(spin=spin)
    app.set_colormap(orc.linear_ramp_tf(0.8))
    app.set_composite_depth(k)


def _abi(s, k=K):
    """(frame, values, counts, depths, xyz) of the scene through the C ABI"""
    with GpuScene(s) as g:
        vrc.check(g.L, g.L.vrc_set_option(g.ctx, vrc.OPT_COMPOSITE_DEPTH, k))
        fb, _, _ = g.render()
        assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_cdepth<")
        v = np.zeros((s.H, s.W), dtype=np.float32)
        c = np.zeros((s.H, s.W), dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
        return (fb, v, c) + vrc.projection_depths(g.L, g.ctx, s.W, s.H)


def _pick_all(app, w, h, rows=None):
    hit = np.zeros((h, w), dtype=bool)
    v, t, p = np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
    for y in (range(h) if rows is None else rows):
        for x in range(w):
            hit[y, x], v[y, x], t[y, x], p[y, x] = app.pick(x, y)
    return hit, v, t, p


def _compare(picked, abi, rows=None):
    hit, v, t, p = picked
    fb, av, ac, at, ap = abi
    sel = np.zeros(hit.shape, dtype=bool)
    sel[slice(None) if rows is None else rows] = True
    assert np.array_equal(hit[sel], (ac > 0)[sel])
    on = sel & hit
    assert on.sum() > 100
    assert np.array_equal(v[on], av[on]) and np.array_equal(t[on], at[on]) and np.array_equal(p[on], ap[on])
    # a ray that stays below the threshold: no hit, D = +infinity
    below = sel & ~hit
    assert below.sum() > 50 and np.isposinf(t[below]).all()
    assert (fb[..., 3][below] < np.float32(K) / np.float32(1000)).all() and (fb[..., 3][on] >= np.float32(K) / np.float32(1000)).all()


def test_pick_on_the_mem_volume(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        _app(app)
        assert app.get_option(vrc.OPT_COMPOSITE_DEPTH) == K
        fb, st = app.render_frame()
        ids = app.visible_set()
        s = mip_scenes.host_mem_scene(ids=ids, spr=int(st.samples_per_ray))
        abi = _abi(s)
        assert np.array_equal(fb, abi[0])
        picked = _pick_all(app, 44, 36)
        _compare(picked, abi)
        with pytest.raises(drv.DriverError) as e:
            app.pick(44, 0)
        assert "outside the window" in str(e.value)
        # the option reaches a renderer made after it was set
        app.set_frames_in_flight(2)
        app.select_slot(1)
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "no frame rendered in this slot" in str(e.value)
        assert np.array_equal(app.render_frame()[0], fb)
        assert app.pick(20, 18) == tuple(x[18, 20] if x.ndim == 2 else tuple(x[18, 20]) for x in picked)
        # with the option at 0 the frame is the same and the pick refuses it, as before
        app.set_composite_depth(0)
        assert np.array_equal(app.render_frame()[0], fb)
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "lvh_app_pick" in str(e.value) and "VRC_OPT_PROJECTION" in str(e.value)
        # a slot keeps its own last frame
        app.select_slot(0)
        assert app.pick(20, 18)[2] == float(picked[2][18, 20])


def test_pick_in_band_mode(drv):
    W, H = 44, 36
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", W, H, **kw) as full_app:
        _app(full_app)
        full_app.render_frame()
        bands = [(4, 8), (20, 6)]
        rows = np.concatenate([np.arange(y0, y0 + h) for (y0, h) in bands])
        full = _pick_all(full_app, W, H, rows=rows)
    with drv.App("mem://#64,64,64,16", W, H, **kw) as app:
        app.set_bands(bands)
        _app(app)
        app.render_frame()
        mine = _pick_all(app, W, H, rows=rows)  # in window coordinates
        for a, b in zip(full, mine):
            assert np.array_equal(a[rows], b[rows], equal_nan=True)
        assert mine[0][rows].sum() > 100
        with pytest.raises(drv.DriverError) as e:
            app.pick(10, 12)
        assert "row 12" in str(e.value) and "bands" in str(e.value)


def test_pick_on_the_nucleon(drv):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nucleon.nrrd")
    s = mip_scenes.host_nucleon_scene()
    with drv.App("raw://" + path, 44, 36, synchronous=True, gpu_cache_mb=16) as app:
        _app(app, spin=(0.4, 0.3))
        fb, st = app.render_frame()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        abi = _abi(s)
        assert np.array_equal(fb, abi[0])
        _compare(_pick_all(app, 44, 36), abi)
