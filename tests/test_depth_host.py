"""Picking in a MIP frame through the plugin surface (libre_amd.driver.App.pick) on the GPU: VRC_OPT_MIP_DEPTH and
VRC_OPT_MIP_DEPTH_CUE reach every renderer through lvh_app_set_option, a pick is the matching entry of the C ABI's
read-back of the same scene, and frames without a depth refuse it with a message."""
import os

import numpy as np
import pytest

import depth_ref
import mip_scenes
import orc
from depth_ref import FOLD_MAX, FOLD_MIN
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

FOLDS = {"max": FOLD_MAX, "min": FOLD_MIN}


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _depth_app(app, fold, spin=(0.5, 0.35), depth=1, cue=0):
    app.set_camera(spin=spin)
    app.set_colormap(orc.linear_ramp_tf(0.8))
    app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
    app.set_option(vrc.OPT_MIP_FOLD, fold)
    app.set_option(vrc.OPT_MIP_DEPTH, depth)
    app.set_option(vrc.OPT_MIP_DEPTH_CUE, cue)


def _abi(s, fold):
    """(frame, values, counts, depths, xyz) of the scene through the C ABI"""
    with GpuScene(s) as g:
        for o, v in ((vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), (vrc.OPT_MIP_FOLD, fold), (vrc.OPT_MIP_DEPTH, 1)):
            vrc.check(g.L, g.L.vrc_set_option(g.ctx, o, v))
        fb, _, _ = g.render()
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
    _, av, ac, at, ap = abi
    sel = np.zeros(hit.shape, dtype=bool)
    sel[slice(None) if rows is None else rows] = True
    assert np.array_equal(hit[sel], (ac > 0)[sel])
    on = sel & hit
    assert on.sum() > 100
    assert np.array_equal(v[on], av[on]) and np.array_equal(t[on], at[on]) and np.array_equal(p[on], ap[on])
    assert np.isposinf(t[sel & ~hit]).all()


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_pick_on_the_mem_volume(drv, fold):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        _depth_app(app, FOLDS[fold])
        fb, st = app.render_frame()
        ids = app.visible_set()
        assert sorted(ids) == sorted(orc.leaf_ids(mip_scenes.host_mem_scene().vi))
        s = mip_scenes.host_mem_scene(ids=ids, spr=int(st.samples_per_ray))
        abi = _abi(s, FOLDS[fold])
        assert np.array_equal(fb, abi[0])
        picked = _pick_all(app, 44, 36)
        _compare(picked, abi)
        r = depth_ref.render(s, fold=FOLDS[fold])
        assert depth_ref.multi_share(r) <= depth_ref.MULTI_CAP
        assert depth_ref.check(r, picked[1], picked[0].astype(np.uint32), picked[2])[0] == 0
        with pytest.raises(drv.DriverError) as e:
            app.pick(44, 0)
        assert "outside the window" in str(e.value)
        # the two options reach a renderer made after they were set
        app.set_frames_in_flight(2)
        app.select_slot(1)
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "no frame rendered in this slot" in str(e.value)
        assert np.array_equal(app.render_frame()[0], fb)
        assert app.pick(20, 18) == tuple(x[18, 20] if x.ndim == 2 else tuple(x[18, 20]) for x in picked)
        app.set_option(vrc.OPT_MIP_DEPTH, 0)
        app.set_option(vrc.OPT_MIP_DEPTH_CUE, 500)
        app.set_frames_in_flight(3)
        app.select_slot(2)
        cued, _ = app.render_frame()
        assert app.pick(20, 18) == app.pick(20, 18) and app.pick(20, 18)[1:3] == (float(picked[1][18, 20]), float(picked[2][18, 20]))
        hit = picked[0]
        assert (cued[hit] <= fb[hit]).all() and (cued[hit] < fb[hit]).any() and np.array_equal(cued[~hit], fb[~hit])
        # a slot keeps its own last frame
        app.select_slot(0)
        assert app.pick(20, 18)[2] == float(picked[2][18, 20])


def test_frames_without_a_depth_refuse_the_pick(drv):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.8))
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "no frame" in str(e.value)
        app.render_frame()  # composite
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "lvh_app_pick" in str(e.value) and "VRC_OPT_PROJECTION" in str(e.value)
        _depth_app(app, FOLD_MAX, depth=0)
        app.render_frame()  # MIP without depth
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "VRC_OPT_MIP_DEPTH" in str(e.value)
        _depth_app(app, 2, depth=1)
        app.render_frame()  # the mean
        with pytest.raises(drv.DriverError) as e:
            app.pick(20, 18)
        assert "VRC_MIP_FOLD_MEAN" in str(e.value)
        _depth_app(app, FOLD_MAX)
        app.render_frame()
        assert app.pick(20, 18)[0]


def test_pick_in_band_mode(drv):
    W, H = 44, 36
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", W, H, **kw) as full_app:
        _depth_app(full_app, FOLD_MAX)
        full_app.render_frame()
        bands = [(4, 8), (20, 6)]
        rows = np.concatenate([np.arange(y0, y0 + h) for (y0, h) in bands])
        full = _pick_all(full_app, W, H, rows=rows)
    with drv.App("mem://#64,64,64,16", W, H, **kw) as app:
        app.set_bands(bands)
        _depth_app(app, FOLD_MAX)
        app.render_frame()
        mine = _pick_all(app, W, H, rows=rows)  # in window coordinates
        for a, b in zip(full, mine):
            assert np.array_equal(a[rows], b[rows])
        assert mine[0][rows].sum() > 100
        with pytest.raises(drv.DriverError) as e:
            app.pick(10, 12)
        assert "row 12" in str(e.value) and "bands" in str(e.value)


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_pick_on_the_nucleon(drv, fold):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nucleon.nrrd")
    s = mip_scenes.host_nucleon_scene()
    with drv.App("raw://" + path, 44, 36, synchronous=True, gpu_cache_mb=16) as app:
        _depth_app(app, FOLDS[fold], spin=(0.4, 0.3))
        fb, st = app.render_frame()
        assert st.n_available == 1 and st.samples_per_ray == s.render.samplesPerRay
        abi = _abi(s, FOLDS[fold])
        assert np.array_equal(fb, abi[0])
        _compare(_pick_all(app, 44, 36), abi)
