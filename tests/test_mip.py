"""Maximum-intensity projection through the C ABI on the GPU (include/vrc_hip.h, "A MIP frame"), held to the float64
restatement tests/mip_ref.py by its acceptance rule; tests/test_mip_cpu.py checks the rule and the scenes on the CPU."""
import ctypes as C

import numpy as np
import pytest

import mip_ref
import mip_scenes
import nongrid
import orc
import skip_window
import voxel_types
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _mip(g, on=True, skip=1, uniform=1):
    _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP if on else vrc.PROJECTION_COMPOSITE)
    _opt(g, vrc.OPT_MIP_SKIP, skip)
    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)


def _check(s, r, fb, what):
    bad, worst, amb = mip_ref.check_frame(s, r, fb)
    print("%s: %d failing pixels (worst excess %.3g), %d ambiguous of %d hit" % (what, bad, worst, amb, int(r.hit().sum())))
    assert bad == 0, what


def _count_ok(r, n, what):
    """vrc_stats.samples with skipping off is |S|: mip_ref's count, where float64 can tell -- a grazed brick's sample and
    a last sample within the contract's window of a whole number of steps are taken or not by the last bit."""
    lo, hi = int(r.counts_lo.sum()), int(r.counts_hi.sum())
    print("%s: samples %d, mip_ref %d (certain %d .. %d with every doubtful sample)" % (what, n, int(r.counts.sum()), lo, hi))
    assert lo <= n <= hi, what
    if lo == hi:
        assert n == int(r.counts.sum())


@pytest.mark.parametrize("stepping", [1, 0])
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
@pytest.mark.parametrize("name", mip_scenes.COUNT)
def test_samples_with_skipping_off_equal_mip_ref(name, kernel, filter_mode, stepping):
    """Scenes in which float64 leaves no sample in doubt (test_mip_cpu.py asserts that of them): vrc_stats.samples is
    mip_ref's count, to the sample."""
    s, r = mip_scenes.get(name), mip_scenes.ref(name, filter_mode)
    assert (r.counts_lo == r.counts_hi).all()
    with GpuScene(s) as g:
        _mip(g, skip=0)
        fb, n, _ = g.render(kernel=kernel, filter_mode=filter_mode, stepping=stepping)
        _check(s, r, fb, "%s kernel %d filter %d stepping %d" % (name, kernel, filter_mode, stepping))
        print("%s: samples %d, mip_ref %d" % (name, n, int(r.counts.sum())))
        assert n == int(r.counts.sum())
        _mip(g, skip=0, uniform=0)
        assert g.render(kernel=kernel, filter_mode=filter_mode, stepping=stepping)[1] == n


@pytest.mark.parametrize("stepping", [1, 0])
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
@pytest.mark.parametrize("name", ["axis", "spin", "inside", "clip"])
def test_every_served_form_passes_the_rule(name, kernel, filter_mode, stepping):
    s, r = mip_scenes.get(name), mip_scenes.ref(name, filter_mode)
    with GpuScene(s) as g:
        _mip(g, skip=0)
        fb, n, stats = g.render(kernel=kernel, filter_mode=filter_mode, stepping=stepping)
        assert stats.kernel_variant == kernel
        assert b"vrc_k_raycast_mip" in g.L.vrc_last_kernel()
        _check(s, r, fb, "%s kernel %d filter %d stepping %d" % (name, kernel, filter_mode, stepping))
        _count_ok(r, n, name)
        # the second pin of the sample set: a composite render with an all-zero transfer function takes the same samples
        _mip(g, on=False)
        g.s.tf = np.zeros((256, 4), dtype=np.float32)
        _, n0, _ = g.render(kernel=kernel, filter_mode=filter_mode, stepping=stepping)
        assert n0 == n


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    """The maximum commutes with the affine image v = a + b q (b > 0) and the classification reads (v - r0) / (r1 - r0)
    alone: mip_ref's frame of the q scene is the frame the typed volume must give."""
    q, t, _ = mip_scenes.typed(image)
    r = mip_scenes.typed_ref(image, filter_mode)
    assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        _mip(g, skip=0)
        fb, n, _ = g.render(filter_mode=filter_mode)
        _check(q, r, fb, "%s filter %d" % (image, filter_mode))
        _count_ok(r, n, image)
        _mip(g, skip=1)
        fb1, n1, _ = g.render(filter_mode=filter_mode)
        assert np.array_equal(fb, fb1) and n1 <= n


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16", "spin", "axis"])
def test_skipping_and_uniform_bricks_change_no_pixel(name, filter_mode):
    """"skip" and "skip16" hold constant bricks next to noise (test_mip_cpu.py asserts it): lanes of one wave sit in a
    uniform slot, march and skip side by side."""
    s, r = mip_scenes.get(name), mip_scenes.ref(name, filter_mode)
    with GpuScene(s) as g:
        frames = {}
        for skip in (0, 1):
            for uniform in (0, 1):
                _mip(g, skip=skip, uniform=uniform)
                frames[skip, uniform] = g.render(kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode)[:2]
        fb, n = frames[0, 0]
        _check(s, r, fb, name)
        assert np.array_equal(frames[0, 1][0], fb) and frames[0, 1][1] == n, "uniform bricks: the same frame and count"
        for uniform in (0, 1):
            assert np.array_equal(frames[1, uniform][0], fb), "skipping: the same frame, bit for bit"
            assert frames[1, uniform][1] <= n
        print("%s filter %d: samples %d, with skipping %d" % (name, filter_mode, n, frames[1, 1][1]))
        _count_ok(r, n, name)
        if name in ("skip", "skip16"):
            assert frames[1, 0][1] < n and frames[1, 1][1] < n
        if name in ("skip", "skip16") and not filter_mode:
            # how many, not only fewer: the window tests/skip_window.py predicts from mip_ref and the words NumPy finds
            # in the uploaded bricks (tests/test_slot_words_cpu.py: it is narrow and lies below the count without skipping)
            w = skip_window.of(name, skip_window.MAX, skip_window.DDA)
            for uniform in (0, 1):
                skip_window.check(w, frames[1, uniform][1], "%s grid walk, uniform bricks %d" % (name, uniform))
            for uniform in (0, 1):  # ... and the loop in list order
                _mip(g, skip=1, uniform=uniform)
                fb1, n1, st = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
                assert st.kernel_variant == vrc.KERNEL_REFERENCE_ORDER and np.array_equal(fb1, fb)
                skip_window.check(skip_window.of(name, skip_window.MAX, skip_window.REFORDER), n1,
                                  "%s reference order, uniform bricks %d" % (name, uniform))


@pytest.mark.parametrize("kernel", [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA], ids=["reforder", "dda"])
def test_three_passes_equal_one(kernel):
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin")
    n = s.n_nodes
    with GpuScene(s) as g:
        _mip(g, skip=0)
        one, n1, _ = g.render(kernel=kernel)
        three, n3, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=[(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)])
        assert np.array_equal(one, three) and n1 == n3
        _mip(g, skip=1)
        skipped, _, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=[(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)])
        assert np.array_equal(one, skipped)
        _check(s, r, three, "three passes")


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_a_brick_without_overlap_takes_the_clamped_sampler(filter_mode):
    import scenes
    s = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    r = mip_ref.render(s, filter_mode=filter_mode)
    assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    with GpuScene(s) as g:
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA):
            _mip(g, skip=0)
            fb, n, _ = g.render(kernel=kernel, filter_mode=filter_mode)
            _check(s, r, fb, "nucleon kernel %d filter %d" % (kernel, filter_mode))
            _count_ok(r, n, "nucleon")
            _mip(g, skip=1)
            fb1, n1, _ = g.render(kernel=kernel, filter_mode=filter_mode)
            assert np.array_equal(fb, fb1) and n1 <= n


def test_a_non_grid_lod_cut():
    s = nongrid.overlapping_scene("hash_parents_some_children", viewport=(36, 28))
    s.tf = orc.linear_ramp_tf(0.8)
    r = mip_ref.render(s)
    assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    with GpuScene(s) as g:
        _mip(g, skip=0)
        fb, n, stats = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
        _check(s, r, fb, "non-grid cut")
        _count_ok(r, n, "non-grid cut")
        _mip(g, skip=1)
        fb1, n1, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER)
        assert np.array_equal(fb, fb1) and n1 <= n


def test_row_map_and_caller_owned_framebuffer():
    import torch
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin")
    with GpuScene(s) as g:
        _mip(g)
        full, _, _ = g.render()
        rows = np.array([3, 4, 5, 17, 18, 30, 35], dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        saved = g.s.H
        try:
            g.s.H = len(rows)  # the buffer GpuScene reads back
            band, _, _ = g.render()
        finally:
            g.s.H = saved
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        assert np.array_equal(band, full[rows])
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full)
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))
        _check(s, r, full, "full frame")


def test_refusals_name_the_option_and_leave_the_context_usable():
    s = mip_scenes.get("spin")
    with GpuScene(s) as g:
        _mip(g)
        good, _, _ = g.render()
        for kw, word in ((dict(kernel=vrc.KERNEL_LDS), "VRC_OPT_KERNEL"), (dict(kernel=vrc.KERNEL_PACKED, filter_mode=1), "VRC_OPT_KERNEL"),
                         (dict(variant=vrc.VARIANT_GLRAYCASTER), "VRC_OPT_VARIANT"),
                         (dict(ray_lod=(1.0, orc.world_space_per_pixel(s))), "vrc_set_ray_lod")):
            with pytest.raises(vrc.VrcError) as e:
                g.render(**kw)
            assert e.value.code == vrc.VRC_EINVAL and word in str(e.value), (kw, str(e.value))
        # the projection may not change inside a frame
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        vrc.check(g.L, g.L.vrc_set_ray_lod(g.ctx, 0, 0.0, 0.0))
        for o, v in ((vrc.OPT_KERNEL, vrc.KERNEL_AUTO), (vrc.OPT_VARIANT, 0), (vrc.OPT_FILTER, 0)):
            _opt(g, o, v)
        vrc.check(g.L, g.L.vrc_pre_render(g.ctx, view))
        vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        assert g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
        assert b"VRC_OPT_PROJECTION" in g.L.vrc_last_error()
        vrc.check(g.L, g.L.vrc_post_render(g.ctx, None))
        with pytest.raises(vrc.VrcError):
            _opt(g, vrc.OPT_PROJECTION, 2)
        _mip(g)
        again, _, _ = g.render()
        assert np.array_equal(good, again)


def test_composite_set_explicitly_is_the_frame_of_before():
    s = mip_scenes.get("spin")
    with GpuScene(s) as g:
        before, n0, _ = g.render()
        _mip(g)
        g.render()
        _mip(g, on=False)
        after, n1, _ = g.render()
        assert np.array_equal(before, after) and n0 == n1
