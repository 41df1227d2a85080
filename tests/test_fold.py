"""The minimum and mean folds of a MIP frame (VRC_OPT_MIP_FOLD) and vrc_get_projection_values through the C ABI on the GPU,
held to the float64 references of tests/fold_ref.py by their acceptance rules; tests/test_fold_cpu.py checks the rules,
the scenes and the host build on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library under test loads its HIP runtime: both then share one (a later import finds no device)

import fold_ref
import mip_ref
import mip_scenes
import nongrid
import orc
import scenes
import skip_window
import voxel_types
from fold_ref import FOLD_MAX, FOLD_MEAN, FOLD_MIN
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

FOLDS = {"min": FOLD_MIN, "mean": FOLD_MEAN}


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _fold(g, fold, skip=1, uniform=1, on=True):
    _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP if on else vrc.PROJECTION_COMPOSITE)
    _opt(g, vrc.OPT_MIP_FOLD, fold)
    _opt(g, vrc.OPT_MIP_SKIP, skip)
    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)


def _values(g, h=None):
    """vrc_get_projection_values of the frame just rendered: (values, counts), H x W."""
    h = g.s.H if h is None else h
    v = np.full((h, g.s.W), np.nan, dtype=np.float32)
    c = np.full((h, g.s.W), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    return v, c


def _range(s):
    return float(s.render.dataSourceRange[1]) - float(s.render.dataSourceRange[0])


def _check_min(s, r, fb, v, c, inexact, what, to_q=lambda x: x):
    """The minimum's rules: the frame against the candidates, the read-back against them (inexact: trilinear samples or a
    float atlas, to E0 x range; else to the bit), the frame against the read-back."""
    bad, worst, amb = fold_ref.check_min_frame(s, r, fb)
    print("%s: %d failing pixels (worst excess %.3g), %d ambiguous of %d hit" % (what, bad, worst, amb, int(r.hit().sum())))
    assert bad == 0, what
    q = to_q(v.astype(np.float64))
    tol = scenes.E0 * _range(s) if inexact else 0.0
    bad = fold_ref.check_candidates(r, q, c, tol=tol)
    print("%s: %d read-back values outside their candidates (tolerance %.3g)" % (what, bad, tol))
    assert bad == 0, what
    bad, worst = fold_ref.check_frame_against_values(s, fb, q, c)
    assert bad == 0, (what, worst)


def _check_mean(s, r, fb, v, c, exact, what, to_q=lambda x: x):
    q = to_q(v.astype(np.float64))
    bad, worst, settled = fold_ref.check_mean_values(s, r, q, c, exact=exact)
    print("%s: %d failing values (worst excess %.3g), %d settled of %d hit" % (what, bad, worst, settled, int(r.hit().sum())))
    assert bad == 0, what
    bad, worst = fold_ref.check_frame_against_values(s, fb, q, c)
    print("%s: %d pixels off the classification of their read-back value (worst excess %.3g)" % (what, bad, worst))
    assert bad == 0, what


def _max_samples(g, **kw):
    """|S| of the scene in this process: the maximum with skipping off."""
    _fold(g, FOLD_MAX, skip=0)
    return g.render(**kw)[1]


@pytest.mark.parametrize("stepping", [1, 0])
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
@pytest.mark.parametrize("name", ["spin", "inside", "clip"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_every_served_form_passes_the_rule(fold, name, kernel, filter_mode, stepping):
    what = "%s %s kernel %d filter %d stepping %d" % (fold, name, kernel, filter_mode, stepping)
    s = mip_scenes.get(name) if fold == "min" else fold_ref.mean_scene(name)
    with GpuScene(s) as g:
        _fold(g, FOLDS[fold], skip=0)
        fb, n, stats = g.render(kernel=kernel, filter_mode=filter_mode, stepping=stepping)
        assert stats.kernel_variant == kernel
        assert b"vrc_k_raycast_mip" in g.L.vrc_last_kernel()
        v, c = _values(g)
        if fold == "min":
            _check_min(s, fold_ref.min_ref(name, filter_mode), fb, v, c, filter_mode, what)
        else:
            _check_mean(s, fold_ref.mean_ref(name, filter_mode), fb, v, c, not filter_mode, what)
            assert n == int(c.astype(np.int64).sum())
        # the sample set is the maximum's
        assert n == _max_samples(g, kernel=kernel, filter_mode=filter_mode, stepping=stepping)


def _to_q(image):
    if image == "uint16":
        return lambda x: x
    im = voxel_types.IMAGES[image]
    return lambda x: (x - im.a) / im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_voxel_types(fold, image, filter_mode):
    """Minimum and mean commute with the affine image v = a + b q (b > 0): the references of the q scene are those of the
    typed volume, whose read-back comes in its own units (a signed type un-shifted)."""
    q, t, _ = mip_scenes.typed(image)
    what = "%s %s filter %d" % (fold, image, filter_mode)
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        _fold(g, FOLDS[fold], skip=0)
        fb, n, _ = g.render(filter_mode=filter_mode)
        v, c = _values(g)
        if fold == "min":
            r = fold_ref.min_render(q, filter_mode=filter_mode)
            _check_min(q, r, fb, v, c, filter_mode or image == "float", what, _to_q(image))
            _fold(g, FOLD_MIN, skip=1)
            fb1, n1, _ = g.render(filter_mode=filter_mode)
            v1, c1 = _values(g)
            assert np.array_equal(fb, fb1) and np.array_equal(v, v1) and np.array_equal(c, c1) and n1 <= n
        else:
            r = fold_ref.mean_render(q, filter_mode=filter_mode)
            _check_mean(q, r, fb, v, c, not filter_mode and image != "float", what, _to_q(image))
            assert n == int(c.astype(np.int64).sum())
        assert n == _max_samples(g, filter_mode=filter_mode)


def test_minimum_of_a_float_atlas_with_an_all_nan_brick():
    """tests/nonfinite.py's volume with one brick, and two voxels around it, all NaN: NaN samples drop out of the minimum,
    and a ray that takes nothing else has M = +infinity.  The reference reads the NaN voxels as the largest q there is,
    which loses every comparison and classifies as +infinity does (both lie above r1)."""
    import copy
    import nonfinite
    case = nonfinite.case("allnan_brick")
    q = copy.copy(case.mq)
    q.bricks = {k: np.where(b == nonfinite.Q_NAN, np.uint16(65535), b).astype(np.uint16) for k, b in case.mq.bricks.items()}
    assert not any((b >= 65534).any() for b in case.mq.bricks.values())
    r = fold_ref.min_render(q)
    all_nan = r.certain & (r.m == 65535.0) & ~r.ambiguous()
    assert all_nan.sum() > 50
    im = nonfinite.IMAGE
    with voxel_types.typed_gpu_scene(case.mt) as g:
        frames = {}
        for skip in (0, 1):
            _fold(g, FOLD_MIN, skip=skip)
            fb, n, _ = g.render()
            frames[skip] = (fb, n) + _values(g)
        fb, n, v, c = frames[0]
        assert np.isposinf(v[all_nan]).all() and (c[all_nan] == 1).all()
        assert not np.isnan(v[c > 0]).any()
        qv = np.where(np.isposinf(v), 65535.0, (v.astype(np.float64) - im.a) / im.b)
        _check_min(q, r, fb, qv.astype(np.float32), c, 1, "all-NaN brick")
        assert np.array_equal(fb, frames[1][0]) and np.array_equal(v, frames[1][2]) and frames[1][1] <= n


@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
@pytest.mark.parametrize("name", mip_scenes.COUNT)
def test_mean_samples_are_the_sample_set(name, kernel):
    """vrc_stats.samples of the mean is |S|: the maximum's with skipping off, the sum of the read-back counts, and on
    scenes in which float64 leaves no sample in doubt (the count depends on the geometry alone) mip_ref's count."""
    s, r = fold_ref.mean_scene(name), mip_scenes.ref(name)
    assert (r.counts_lo == r.counts_hi).all()
    with GpuScene(s) as g:
        for filter_mode in (0, 1):
            for skip, uniform in ((1, 1), (0, 0)):  # (neither changes what the mean samples)
                _fold(g, FOLD_MEAN, skip=skip, uniform=uniform)
                _, n, _ = g.render(kernel=kernel, filter_mode=filter_mode)
                _, c = _values(g)
                print("%s filter %d: samples %d, read-back counts %d, mip_ref %d" % (name, filter_mode, n, int(c.sum()), int(r.counts.sum())))
                assert n == int(c.astype(np.int64).sum()) == int(r.counts.sum())
                assert np.array_equal(c, r.counts)
            assert n == _max_samples(g, kernel=kernel, filter_mode=filter_mode)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "clip"])
def test_complement_identity(name, filter_mode):
    """The face-matched volume and its complement in the same slots: the sample positions are the same, so no tie can
    excuse a miss -- mean(v) + mean(255 - v) = 255 within 2 ulp, pixel by pixel, and the counts are identical."""
    a, b = fold_ref.mean_scene(name), fold_ref.mean_scene(name, complement=True)
    assert a.slot_of == b.slot_of
    out = []
    for s in (a, b):
        with GpuScene(s) as g:
            _fold(g, FOLD_MEAN)
            g.render(filter_mode=filter_mode)
            out.append(_values(g))
    (va, ca), (vb, cb) = out
    assert np.array_equal(ca, cb) and (ca > 0).sum() > 100
    has = ca > 0
    total = va[has].astype(np.float64) + vb[has].astype(np.float64)
    ulp = np.spacing(np.maximum(va[has], vb[has])).astype(np.float64)
    worst = float((np.abs(total - 255.0) / ulp).max())
    print("%s filter %d: |mean(v) + mean(255 - v) - 255| at most %.2f ulp over %d pixels" % (name, filter_mode, worst, int(has.sum())))
    assert worst <= 2.0


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_minimum_skipping_and_uniform_bricks_change_no_pixel(name, filter_mode):
    """The complement of mip_scenes.skip_volume: constant bricks next to noise, one dark brick nearest the eye."""
    s = fold_ref.complemented_scene(name)
    r = fold_ref.min_render(s, filter_mode=filter_mode)
    with GpuScene(s) as g:
        frames = {}
        for skip in (0, 1):
            for uniform in (0, 1):
                _fold(g, FOLD_MIN, skip=skip, uniform=uniform)
                fb, n, _ = g.render(kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode)
                frames[skip, uniform] = (fb, n) + _values(g)
        fb, n, v, c = frames[0, 0]
        _check_min(s, r, fb, v, c, filter_mode, name)
        for key, (fb1, n1, v1, c1) in frames.items():
            assert np.array_equal(fb1, fb) and np.array_equal(v1, v) and np.array_equal(c1, c), key
        assert frames[0, 1][1] == n, "uniform bricks: the same count"
        print("%s filter %d: samples %d, with skipping %d / %d" % (name, filter_mode, n, frames[1, 0][1], frames[1, 1][1]))
        assert frames[1, 0][1] < n and frames[1, 1][1] < n
        if not filter_mode:
            # how many, not only fewer (tests/skip_window.py: the window predicted from mip_ref and the smallest voxel
            # NumPy finds in every uploaded brick), for the grid walk and for the loop in list order
            w = skip_window.of(name, skip_window.MIN, skip_window.DDA)
            for uniform in (0, 1):
                skip_window.check(w, frames[1, uniform][1], "%s minimum, grid walk, uniform bricks %d" % (name, uniform))
            for uniform in (0, 1):
                _fold(g, FOLD_MIN, skip=1, uniform=uniform)
                fb1, n1, st = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
                assert st.kernel_variant == vrc.KERNEL_REFERENCE_ORDER and np.array_equal(fb1, fb)
                skip_window.check(skip_window.of(name, skip_window.MIN, skip_window.REFORDER), n1,
                                  "%s minimum, reference order, uniform bricks %d" % (name, uniform))


@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_three_passes_equal_one(fold, kernel):
    s = mip_scenes.get("spin") if fold == "min" else fold_ref.mean_scene("spin")
    n = s.n_nodes
    passes = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    with GpuScene(s) as g:
        _fold(g, FOLDS[fold], skip=0)
        one, n1, _ = g.render(kernel=kernel)
        v1, c1 = _values(g)
        three, n3, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=passes)
        v3, c3 = _values(g)
        # the minimum is bit-identical; the mean's integer sums and counts are exact, whatever the order
        assert np.array_equal(one, three) and n1 == n3 and np.array_equal(v1, v3) and np.array_equal(c1, c3)
        if fold == "min":
            _fold(g, FOLD_MIN, skip=1)
            skipped, _, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=passes)
            assert np.array_equal(one, skipped)
            _check_min(s, fold_ref.min_ref("spin"), three, v3, c3, 0, "three passes")
        else:
            _check_mean(s, fold_ref.mean_ref("spin"), three, v3, c3, True, "three passes")
            # trilinear: a float64 sum in another order, inside the read-back tolerance
            t1 = g.render(kernel=kernel, filter_mode=1)
            w1, d1 = _values(g)
            t3 = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=1, passes=passes)
            w3, d3 = _values(g)
            assert t1[1] == t3[1] and np.array_equal(d1, d3)
            _check_mean(s, fold_ref.mean_ref("spin", 1), t3[0], w3, d3, False, "three trilinear passes")
            assert np.abs(w1.astype(np.float64) - w3)[d1 > 0].max() <= scenes.E0 * _range(s)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_a_brick_without_overlap_takes_the_clamped_sampler(fold, filter_mode):
    s = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    if fold == "min":
        r = fold_ref.min_render(s, filter_mode=filter_mode)
        assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    else:
        r = fold_ref.mean_render(s, filter_mode=filter_mode)
    with GpuScene(s) as g:
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA):
            _fold(g, FOLDS[fold], skip=0)
            fb, n, _ = g.render(kernel=kernel, filter_mode=filter_mode)
            v, c = _values(g)
            what = "nucleon %s kernel %d filter %d" % (fold, kernel, filter_mode)
            if fold == "min":
                _check_min(s, r, fb, v, c, filter_mode, what)
                _fold(g, FOLD_MIN, skip=1)
                fb1, n1, _ = g.render(kernel=kernel, filter_mode=filter_mode)
                assert np.array_equal(fb, fb1) and n1 <= n
            else:
                _check_mean(s, r, fb, v, c, not filter_mode, what)
                assert n == int(c.astype(np.int64).sum())


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_a_non_grid_lod_cut(fold):
    s = nongrid.overlapping_scene("hash_parents_some_children", viewport=(36, 28))
    s.tf = orc.linear_ramp_tf(0.8)
    with GpuScene(s) as g:
        _fold(g, FOLDS[fold], skip=0)
        fb, n, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
        v, c = _values(g)
        if fold == "min":
            r = fold_ref.min_render(s)
            assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
            _check_min(s, r, fb, v, c, 0, "non-grid cut")
            _fold(g, FOLD_MIN, skip=1)
            fb1, n1, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
            assert np.array_equal(fb, fb1) and n1 <= n
        else:
            _check_mean(s, fold_ref.mean_render(s), fb, v, c, True, "non-grid cut")
            assert n == int(c.astype(np.int64).sum())


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_row_map_and_caller_owned_framebuffer(fold):
    s = mip_scenes.get("spin") if fold == "min" else fold_ref.mean_scene("spin")
    with GpuScene(s) as g:
        _fold(g, FOLDS[fold])
        full, _, _ = g.render()
        vfull, cfull = _values(g)
        rows = np.array([3, 4, 5, 17, 18, 30, 35], dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        saved = g.s.H
        try:
            g.s.H = len(rows)  # the buffer GpuScene reads back
            band, _, _ = g.render()
            vband, cband = _values(g)  # W x H entries of the row-mapped buffer
        finally:
            g.s.H = saved
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        assert np.array_equal(band, full[rows])
        assert np.array_equal(vband, vfull[rows]) and np.array_equal(cband, cfull[rows])
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full)
            v, c = _values(g)
            assert np.array_equal(v, vfull) and np.array_equal(c, cfull)
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))
        if fold == "min":
            _check_min(s, fold_ref.min_ref("spin"), full, vfull, cfull, 0, "full frame")
        else:
            _check_mean(s, fold_ref.mean_ref("spin"), full, vfull, cfull, True, "full frame")


def test_refusals_name_the_option_and_leave_the_context_usable():
    s = mip_scenes.get("spin")
    with GpuScene(s) as g:
        v = np.zeros((s.H, s.W), dtype=np.float32)
        # nothing to read before any MIP render, nor after a composite frame
        assert g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, None) == vrc.VRC_EINVAL
        g.render()
        assert g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, None) == vrc.VRC_EINVAL
        assert b"vrc_get_projection_values" in g.L.vrc_last_error()
        _fold(g, FOLD_MIN)
        good, _, _ = g.render()
        vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, None))  # counts may be NULL
        assert np.array_equal(v, _values(g)[0])
        with pytest.raises(vrc.VrcError) as e:
            _opt(g, vrc.OPT_MIP_FOLD, 3)
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_MIP_FOLD" in str(e.value)
        with pytest.raises(vrc.VrcError):
            _opt(g, vrc.OPT_MIP_FOLD, -1)
        got = C.c_int64(-1)
        vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_MIP_FOLD, C.byref(got)))
        assert got.value == FOLD_MIN
        # the refusals of a MIP frame hold for every fold
        for kw, word in ((dict(kernel=vrc.KERNEL_LDS), "VRC_OPT_KERNEL"), (dict(variant=vrc.VARIANT_GLRAYCASTER), "VRC_OPT_VARIANT"),
                         (dict(ray_lod=(1.0, orc.world_space_per_pixel(s))), "vrc_set_ray_lod")):
            for fold in (FOLD_MIN, FOLD_MEAN):
                _fold(g, fold)
                with pytest.raises(vrc.VrcError) as e:
                    g.render(**kw)
                assert e.value.code == vrc.VRC_EINVAL and word in str(e.value), (kw, str(e.value))
        # the fold may not change inside a frame
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        vrc.check(g.L, g.L.vrc_set_ray_lod(g.ctx, 0, 0.0, 0.0))
        for o, val in ((vrc.OPT_KERNEL, vrc.KERNEL_AUTO), (vrc.OPT_VARIANT, 0), (vrc.OPT_FILTER, 0)):
            _opt(g, o, val)
        _fold(g, FOLD_MIN)
        vrc.check(g.L, g.L.vrc_pre_render(g.ctx, view))
        assert g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, None) == vrc.VRC_EINVAL  # a new frame: nothing yet
        vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
        _opt(g, vrc.OPT_MIP_FOLD, FOLD_MEAN)
        assert g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
        assert b"VRC_OPT_MIP_FOLD" in g.L.vrc_last_error()
        _opt(g, vrc.OPT_MIP_FOLD, FOLD_MIN)
        vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
        vrc.check(g.L, g.L.vrc_post_render(g.ctx, None))
        # VRC_OPT_PROJECTION = 2 stays refused: the folds are an option of their own
        with pytest.raises(vrc.VrcError):
            _opt(g, vrc.OPT_PROJECTION, 2)
        # a fold set under the composite projection is not read
        _fold(g, FOLD_MEAN, on=False)
        composite, _, _ = g.render()
        _fold(g, FOLD_MAX, on=False)
        assert np.array_equal(composite, g.render()[0])
        _fold(g, FOLD_MIN)
        again, _, _ = g.render()
        assert np.array_equal(good, again)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_the_maximum_is_unchanged(filter_mode):
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin", filter_mode)
    with GpuScene(s) as g:
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        before, n0, _ = g.render(filter_mode=filter_mode)
        _fold(g, FOLD_MIN)
        g.render(filter_mode=filter_mode)
        _fold(g, FOLD_MAX)
        after, n1, _ = g.render(filter_mode=filter_mode)
        assert np.array_equal(before, after) and n0 == n1
        assert mip_ref.check_frame(s, r, after)[0] == 0
        v, c = _values(g)
        assert fold_ref.check_candidates(r, v, c, tol=scenes.E0 * _range(s) if filter_mode else 0.0) == 0
        assert fold_ref.check_frame_against_values(s, after, v, c)[0] == 0
