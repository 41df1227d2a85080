"""The minimum and mean folds of a MIP frame through the plugin surface (libre_amd.driver.App) on the GPU: VRC_OPT_MIP_FOLD
reaches every renderer through lvh_app_set_option, multi-pass frames meet in the context's running state, row bands are
rows of the full frame.  Frames are held to tests/fold_ref.py by its acceptance rules (the plugin surface has no
read-back of the projected values: the mean's frame is held to the classification of its reference interval)."""
import numpy as np
import pytest

import fold_ref
import mip_scenes
import orc
from fold_ref import FOLD_MEAN, FOLD_MIN
from libre_amd import vrc

pytestmark = pytest.mark.gpu

FOLDS = {"min": FOLD_MIN, "mean": FOLD_MEAN}


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _fold_app(app, fold, spin=(0.5, 0.35), alpha=0.8):
    app.set_camera(spin=spin)
    app.set_colormap(orc.linear_ramp_tf(alpha))
    app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
    app.set_option(vrc.OPT_MIP_FOLD, fold)
    app.set_option(vrc.OPT_COUNT_SAMPLES, 1)


#: the plugin scenes (tests/test_fold_cpu.py caps the ambiguous pixels and asks for the settled share of all three)
BANDS_MEM, PASSES_MEM = fold_ref.BANDS_MEM, fold_ref.PASSES_MEM


def _scene(app, st, kw):
    """The scene the app rendered, rebuilt from its visible set: the one whose reference conditions the CPU tests assert."""
    ids = app.visible_set()
    default = orc.build_scene(**kw)
    assert sorted(ids) == sorted(orc.leaf_ids(default.vi))
    assert int(st.samples_per_ray) == default.render.samplesPerRay
    return orc.build_scene(ids=ids, spr=int(st.samples_per_ray), **kw)


def _reference(s, fold):
    r = fold_ref.min_render(s) if fold == "min" else fold_ref.mean_render(s)
    if fold == "min":
        assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    else:
        assert int(r.settled.sum()) >= 0.75 * int(r.hit().sum())
    return r


def _hold(s, r, fold, fb, what):
    if fold == "min":
        bad, worst, amb = fold_ref.check_min_frame(s, r, fb)
        print("%s: %d failing pixels (worst excess %.3g), %d ambiguous of %d hit" % (what, bad, worst, amb, int(r.hit().sum())))
    else:
        bad, worst = fold_ref.check_mean_frame(s, r, fb, exact=True)
        print("%s: %d failing pixels (worst excess %.3g), %d settled of %d hit" % (what, bad, worst, int(r.settled.sum()), int(r.hit().sum())))
    assert bad == 0, what


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_mem_volume_in_synchronous_mode(drv, fold):
    with drv.App("mem://#64,64,64,16", 44, 36, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8) as app:
        _fold_app(app, FOLDS[fold])
        fb, st = app.render_frame()
        assert st.n_passes == 1 and len(app.visible_set()) == 64
        s = _scene(app, st, mip_scenes.HOST_MEM)
        _hold(s, _reference(s, fold), fold, fb, "mem:// %s through the plugin" % fold)
        # the maximum of the same app is another frame, and the fold reaches a renderer made later
        app.set_option(vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MAX)
        assert not np.array_equal(app.render_frame()[0], fb)
        app.set_option(vrc.OPT_MIP_FOLD, FOLDS[fold])
        app.set_frames_in_flight(2)
        app.select_slot(1)
        assert np.array_equal(app.render_frame()[0], fb)
        app.select_slot(0)
        # per-ray LOD asked for: every fold renders the per-brick cut -- the same frame
        app.set_ray_lod(True)
        lod, _ = app.render_frame()
        assert not app.stats().ray_lod
        assert np.array_equal(lod, fb)


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_a_pool_smaller_than_the_brick_set_takes_several_passes(drv, fold):
    frames = {}
    for mb in (1, 8):
        with drv.App("mem://#128,128,128,32", 40, 40, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=mb) as app:
            _fold_app(app, FOLDS[fold])
            frames[mb], st = app.render_frame()
            assert st.n_passes == (4 if mb == 1 else 1) and st.n_available == 64
            s = _scene(app, st, PASSES_MEM)
    r = _reference(s, fold)
    # minimum and mean do not depend on how the bricks are dealt to passes (no clip plane: no brick ends a ray early)
    _hold(s, r, fold, frames[1], "mem:// 128^3 %s in four passes" % fold)
    _hold(s, r, fold, frames[8], "mem:// 128^3 %s in one pass" % fold)
    # the minimum does not depend on the order; the mean's integer sums and counts are exact whatever the passes
    assert np.array_equal(frames[1], frames[8]), "the passes meet in the running state: the same frame, bit for bit"


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_two_bands_are_rows_of_the_full_frame(drv, fold):
    W, H = BANDS_MEM["viewport"]
    kw = dict(synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=8)
    with drv.App("mem://#64,64,64,16", W, H, **kw) as full_app:
        _fold_app(full_app, FOLDS[fold])
        full, st = full_app.render_frame()
        s = _scene(full_app, st, BANDS_MEM)
    r = _reference(s, fold)
    _hold(s, r, fold, full, "mem:// %s, full frame" % fold)
    bands = [(8, 8), (40, 16)]
    rows = np.concatenate([np.arange(y0, y0 + h) for (y0, h) in bands])
    with drv.App("mem://#64,64,64,16", W, H, **kw) as app:
        app.set_bands(bands)
        _fold_app(app, FOLDS[fold])
        fb, st = app.render_frame()
        assert fb.shape == (24, W, 4) and st.n_passes == 1
        _hold(s, fold_ref.band_rows(r, rows), fold, fb, "mem:// %s, two bands" % fold)
        assert np.array_equal(fb, full[rows])
