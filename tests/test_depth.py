"""The depth of a MIP frame (VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE, vrc_get_projection_depths) through the C ABI on the
GPU, held to the float64 reference of tests/depth_ref.py by its acceptance rule; tests/test_depth_cpu.py checks the rule,
the scenes and the host build on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import depth_ref
import mip_scenes
import nonfinite
import scenes
import voxel_types
from depth_ref import FOLD_MAX, FOLD_MIN
from gpu_run import GpuScene
from libre_amd import vrc
from ref64 import _vec

pytestmark = pytest.mark.gpu

FOLDS = {"max": FOLD_MAX, "min": FOLD_MIN}
FOLD_MEAN = 2
KERNELS = {"reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _mip(g, fold, depth=1, cue=0, skip=1, uniform=1):
    _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
    _opt(g, vrc.OPT_MIP_FOLD, fold)
    _opt(g, vrc.OPT_MIP_DEPTH, depth)
    _opt(g, vrc.OPT_MIP_DEPTH_CUE, cue)
    _opt(g, vrc.OPT_MIP_SKIP, skip)
    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)


def _values(g, h=None):
    h = g.s.H if h is None else h
    v = np.full((h, g.s.W), np.nan, dtype=np.float32)
    c = np.full((h, g.s.W), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    return v, c


def _depths(g, h=None):
    return vrc.projection_depths(g.L, g.ctx, g.s.W, g.s.H if h is None else h)


def _frame(g, **kw):
    """(frame, samples, values, counts, depths, xyz) of one depth-tracking frame"""
    fb, n, _ = g.render(**kw)
    return (fb, n) + _values(g) + _depths(g)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b) if isinstance(x, np.ndarray))


def _check_xyz(s, d, xyz, dirs):
    """host_xyz = origin + D x dir recomputed in float32, the product and the sum each rounded, bit for bit: from the
    read-back D and the float32 ray of the host build of vrc_setup_ray (strict float32, correctly rounded division and
    square root on both sides; a fused multiply-add or another order in the read-back kernel shows as a last bit).
    And, independently of the project's code, within 1e-5 of the float64 ray the reference casts through the pixel."""
    fin = np.isfinite(d)
    want = _vec(s.view.eyePosition, 3) + d[fin][:, None].astype(np.float64) * dirs[fin]
    assert fin.sum() > 100 and np.abs(xyz[fin] - want).max() <= 1e-5
    want32 = depth_ref.xyz32(d, depth_ref.rays32(s))
    differ = int((xyz[fin] != want32[fin]).sum())
    print("  host_xyz: %d of %d coordinates differ from the float32 recomputation" % (differ, 3 * int(fin.sum())))
    assert differ == 0


def _kernel_name(dda, fixed, mode, atlas="unsigned char", clamp=False):
    b = lambda x: "true" if x else "false"  # noqa: E731
    return ("vrc_k_raycast_mip<%s,%s,%s,%d,%s,false>" % (b(dda), b(clamp), b(fixed), mode, atlas)).encode()


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["axis", "spin", "inside", "clip"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_every_served_form_passes_the_rule(fold, name, kernel, filter_mode):
    what = "%s %s %s filter %d" % (fold, name, kernel, filter_mode)
    s, r = depth_ref.scene(name, filter_mode, FOLDS[fold]), depth_ref.ref(name, filter_mode, FOLDS[fold])
    tol = depth_ref.tolerance(s, filter_mode)
    # the instance a frame without depth launches: the name it had before there was a depth
    mode = (8 if filter_mode else 7) + 16 * FOLDS[fold]
    plain = _kernel_name(kernel == "dda", not filter_mode, mode)
    with GpuScene(s) as g:
        _mip(g, FOLDS[fold], skip=0)
        fb, n, v, c, d, xyz = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert g.L.vrc_last_kernel() == plain.replace(b",%d," % mode, b",%d," % (mode + 64))
        bad, worst = depth_ref.check(r, v, c, d, tol)
        print("%s: %d failing pixels of %d hit, worst depth error %.2g steps" % (what, bad, int(r.hit().sum()), worst))
        assert bad == 0, what
        assert np.isposinf(d[~r.hit()]).all()
        _check_xyz(s, d, xyz, r.dir)
        # depth off: the same frame and values, by the parent's instance
        _mip(g, FOLDS[fold], depth=0, skip=0)
        fb0, n0, _ = g.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert g.L.vrc_last_kernel() == plain
        v0, c0 = _values(g)
        assert np.array_equal(fb, fb0) and np.array_equal(v, v0) and np.array_equal(c, c0) and n == n0, what
        # the float stepping labels its samples by the same formula
        _mip(g, FOLDS[fold], skip=0)
        out = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=0)
        assert depth_ref.check(r, out[2], out[3], out[4], tol)[0] == 0, what + " stepping 0"


def _to_q(image):
    if image == "uint16":
        return lambda x: x
    im = voxel_types.IMAGES[image]
    return lambda x: (x - im.a) / im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_voxel_types(fold, image, filter_mode):
    """uint16, int16 and float pools: the pair commutes with the affine image v = a + b q (b > 0), so the reference of the
    q scene is that of the typed volume, whose values come back in its own units."""
    q, t, _ = mip_scenes.typed(image)
    exact = not filter_mode and image != "float"
    tol = 0.0 if exact else scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    r = depth_ref.render(q, fold=FOLDS[fold], filter_mode=filter_mode, tol=tol)
    assert depth_ref.multi_share(r) <= depth_ref.MULTI_CAP
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        out = {}
        for skip in (0, 1):
            _mip(g, FOLDS[fold], skip=skip)
            out[skip] = _frame(g, filter_mode=filter_mode)
        fb, n, v, c, d, xyz = out[0]
        bad, worst = depth_ref.check(r, _to_q(image)(v.astype(np.float64)), c, d, tol)
        print("%s %s filter %d: %d failing pixels, worst depth error %.2g steps" % (fold, image, filter_mode, bad, worst))
        assert bad == 0
        _check_xyz(q, d, xyz, r.dir)
        assert _same(out[0], out[1]) and out[1][1] <= n
        # depth off: the same frame and values, by the grid walk and by the reference-order loop
        for kernel in sorted(KERNELS):
            _mip(g, FOLDS[fold], skip=0)
            on = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
            assert _same(on, out[0]), kernel
            _mip(g, FOLDS[fold], depth=0, skip=0)
            fb0, n0, _ = g.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
            v0, c0 = _values(g)
            differ = int((v.view(np.uint32) != v0.view(np.uint32)).sum())
            print("  %s: %d values differ between depth on and off" % (kernel, differ))
            assert np.array_equal(fb, fb0) and differ == 0 and np.array_equal(c, c0) and n == n0, kernel


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_the_clamped_sampler_with_depth_on_and_off(fold, filter_mode):
    """A brick without overlap (the nucleon fixture) takes the clamped sampler: the same M bit for bit with depth tracking
    on and off, by both brick loops, and for point samples the rule.  (Trilinear samples of this smooth volume lie
    within the value tolerance of M over long stretches of a ray: 72 % to 85 % of the hit pixels have more than one
    candidate depth, above the cap, so the rule is not asked of them here; the hash scenes ask it of trilinear samples.)"""
    s = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    tol = depth_ref.tolerance(s, filter_mode)
    r = None
    if not filter_mode:
        r = depth_ref.render(s, fold=FOLDS[fold], filter_mode=filter_mode, tol=tol)
        assert depth_ref.multi_share(r) <= depth_ref.MULTI_CAP
    with GpuScene(s) as g:
        for kernel in sorted(KERNELS):
            _mip(g, FOLDS[fold])
            fb, n, v, c, d, xyz = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
            assert b"<%s,true,false," % (b"true" if kernel == "dda" else b"false") in g.L.vrc_last_kernel()
            assert (c > 0).sum() > 100 and np.isfinite(d[c > 0]).all() and np.isposinf(d[c == 0]).all()
            if r is not None:
                bad, worst = depth_ref.check(r, v, c, d, tol)
                print("nucleon %s %s: %d failing pixels, worst depth error %.2g steps" % (fold, kernel, bad, worst))
                assert bad == 0, kernel
            _mip(g, FOLDS[fold], depth=0)
            fb0, n0, _ = g.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
            v0, c0 = _values(g)
            assert np.array_equal(fb, fb0) and np.array_equal(v, v0) and np.array_equal(c, c0) and n == n0, kernel


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_nan_voxels_never_hold_the_depth(fold):
    case = nonfinite.case("allnan_brick")
    q, t = case.mq, case.mt
    tol = scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    r = depth_ref.render(q, fold=FOLDS[fold], tol=tol, nan_q=nonfinite.Q_NAN)
    v0, _, d0 = r.own()
    all_nan = r.certain & np.isinf(v0) & ~r.multi()
    assert all_nan.sum() > 50
    im = nonfinite.IMAGE
    with voxel_types.typed_gpu_scene(t) as g:
        out = {}
        for skip in (0, 1):
            _mip(g, FOLDS[fold], skip=skip)
            out[skip] = _frame(g)
        fb, n, v, c, d, _ = out[0]
        with np.errstate(invalid="ignore"):
            qv = (v.astype(np.float64) - im.a) / im.b
        assert depth_ref.check(r, qv, c, d, tol)[0] == 0
        assert np.isposinf(d[all_nan]).all() and (c[all_nan] == 1).all() and np.isinf(v[all_nan]).all()
        assert _same(out[0][:5], out[1][:5]) and out[1][1] <= n


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_skipping_and_uniform_bricks_change_no_bit(fold, name, filter_mode):
    s, r = depth_ref.scene(name, 0, FOLDS[fold]), depth_ref.ref(name, filter_mode, FOLDS[fold])
    with GpuScene(s) as g:
        out = {}
        for skip in (0, 1):
            for uniform in (0, 1):
                _mip(g, FOLDS[fold], skip=skip, uniform=uniform)
                out[skip, uniform] = _frame(g, kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode)
        fb, n, v, c, d, xyz = out[0, 0]
        assert depth_ref.check(r, v, c, d, depth_ref.tolerance(s, filter_mode))[0] == 0
        for key, o in out.items():
            assert _same(out[0, 0], o), key
        assert out[0, 1][1] == n, "uniform bricks: the same count"
        print("%s %s filter %d: samples %d, with skipping %d / %d" % (name, fold, filter_mode, n, out[1, 0][1], out[1, 1][1]))
        assert out[1, 0][1] < n and out[1, 1][1] < n


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["spin", "two blocks", "skip", "skip16"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_three_passes_equal_one(fold, name, kernel):
    """Any order of the passes, with skipping and uniform bricks on: on "two blocks" and "skip" / "skip16" a later pass
    brings nearer bricks that can only tie with the M held (tests/test_depth_cpu.py has the reasoning)."""
    s = depth_ref.two_blocks(fold == "min") if name == "two blocks" else depth_ref.scene(name, 0, FOLDS[fold])
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    with GpuScene(s) as g:
        for filter_mode in (0, 1):
            _mip(g, FOLDS[fold], skip=0, uniform=0)
            plain = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
            for uniform in (0, 1):
                _mip(g, FOLDS[fold], skip=1, uniform=uniform)
                one = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert _same(plain, one), (filter_mode, uniform)
                for order in (parts, parts[::-1], [parts[1], parts[2], parts[0]], [parts[2], parts[0], parts[1]]):
                    three = _frame(g, kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode, passes=order)
                    differ = int((one[4] != three[4]).sum())
                    assert _same(one, three), (filter_mode, uniform, order, "%d depths differ" % differ)
            if name != "two blocks":
                r = depth_ref.ref(name, filter_mode, FOLDS[fold])
                assert depth_ref.check(r, three[2], three[3], three[4], depth_ref.tolerance(s, filter_mode))[0] == 0


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_row_map_and_caller_owned_framebuffer(fold):
    s = depth_ref.scene("spin")
    with GpuScene(s) as g:
        _mip(g, FOLDS[fold])
        full = _frame(g)
        rows = np.array([3, 4, 5, 17, 18, 30, 35], dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        saved = g.s.H
        try:
            g.s.H = len(rows)  # the buffer GpuScene reads back
            band = _frame(g)
        finally:
            g.s.H = saved
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        for a, b in zip(full, band):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a[rows], b, equal_nan=True)
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full[0])
            assert _same(full[2:], _values(g) + _depths(g))
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))
        t, none = vrc.projection_depths(g.L, g.ctx, s.W, s.H, xyz=False)  # host_xyz may be NULL
        assert none is None and np.array_equal(t, full[4])


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_the_depth_cue(fold, filter_mode):
    """Strength 0 is the uncued frame bit for bit; a cued pixel is w times the uncued one, w recomputed in float32 from
    the read-back D and the ray's interval.  (To scenes.E0, the frame tolerance: the interval here is the reference's
    float64 one rounded to float32, not the kernel's own float32 chain.)"""
    s, r = depth_ref.scene("clip"), depth_ref.ref("clip", filter_mode, FOLDS[fold])
    interval = np.stack([r.tn_g, r.tf_g], axis=-1).astype(np.float32)
    with GpuScene(s) as g:
        _mip(g, FOLDS[fold], depth=0)
        plain, _, _ = g.render(filter_mode=filter_mode)
        _mip(g, FOLDS[fold], depth=1, cue=0)
        zero = _frame(g, filter_mode=filter_mode)
        assert np.array_equal(plain, zero[0])
        for depth in (0, 1):  # a cue above 0 tracks depth whatever VRC_OPT_MIP_DEPTH says
            _mip(g, FOLDS[fold], depth=depth, cue=600)
            cued = _frame(g, filter_mode=filter_mode)
            assert _same(cued[2:], zero[2:]), "the cue changes neither M nor D"
            hit = zero[3] > 0
            w = depth_ref.cue_weight(zero[4], interval, np.float32(600) / np.float32(1000.0))
            assert hit.sum() > 100 and w[hit].min() >= 0.4 - 1e-6 and w[hit].max() <= 1.0 and w[hit].min() < 0.9 * w[hit].max()
            assert np.abs(cued[0] - w[..., None] * zero[0])[hit].max() <= scenes.E0
            assert np.array_equal(cued[0][~hit], zero[0][~hit])


def test_refusals_name_the_option_and_leave_the_context_usable():
    s = depth_ref.scene("spin")
    with GpuScene(s) as g:
        t = np.zeros((s.H, s.W), dtype=np.float32)
        get = lambda: g.L.vrc_get_projection_depths(g.ctx, t.ctypes.data, None)  # noqa: E731
        # nothing to read before any depth frame, after a composite frame, after a MIP frame without depth, under the mean
        assert get() == vrc.VRC_EINVAL and b"vrc_get_projection_depths" in g.L.vrc_last_error()
        g.render()
        assert get() == vrc.VRC_EINVAL
        _mip(g, FOLD_MAX, depth=0)
        g.render()
        assert get() == vrc.VRC_EINVAL and b"VRC_OPT_MIP_DEPTH" in g.L.vrc_last_error()
        _mip(g, FOLD_MEAN, depth=1, cue=500)  # the mean reads neither option
        mean, _, _ = g.render()
        assert get() == vrc.VRC_EINVAL and b"VRC_MIP_FOLD_MEAN" in g.L.vrc_last_error()
        _mip(g, FOLD_MEAN, depth=0, cue=0)
        assert np.array_equal(mean, g.render()[0])
        _mip(g, FOLD_MIN)
        good = _frame(g)
        assert get() == vrc.VRC_OK and np.array_equal(t, good[4])
        g.render(passes=[])  # a new frame without a pass: nothing yet
        assert get() == vrc.VRC_EINVAL
        # bad option values
        for option, name, bad in ((vrc.OPT_MIP_DEPTH, "VRC_OPT_MIP_DEPTH", (2, -1)),
                                  (vrc.OPT_MIP_DEPTH_CUE, "VRC_OPT_MIP_DEPTH_CUE", (1001, -1))):
            for value in bad:
                with pytest.raises(vrc.VrcError) as e:
                    _opt(g, option, value)
                assert e.value.code == vrc.VRC_EINVAL and name in str(e.value)
        got = C.c_int64(-1)
        _opt(g, vrc.OPT_MIP_DEPTH_CUE, 1000)
        vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_MIP_DEPTH_CUE, C.byref(got)))
        assert got.value == 1000
        vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_MIP_DEPTH, C.byref(got)))
        assert got.value == 1
        _opt(g, vrc.OPT_MIP_DEPTH_CUE, 0)
        # neither option may change inside a frame
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        for option, name, other, back in ((vrc.OPT_MIP_DEPTH, b"VRC_OPT_MIP_DEPTH ", 0, 1),
                                          (vrc.OPT_MIP_DEPTH_CUE, b"VRC_OPT_MIP_DEPTH_CUE", 250, 0)):
            vrc.check(g.L, g.L.vrc_pre_render(g.ctx, view))
            vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            _opt(g, option, other)
            assert g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
            assert name in g.L.vrc_last_error()
            _opt(g, option, back)
            vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            vrc.check(g.L, g.L.vrc_post_render(g.ctx, None))
        # under the composite projection the options are not read
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        _opt(g, vrc.OPT_MIP_DEPTH_CUE, 700)
        composite, _, _ = g.render()
        _opt(g, vrc.OPT_MIP_DEPTH_CUE, 0)
        _opt(g, vrc.OPT_MIP_DEPTH, 0)
        assert np.array_equal(composite, g.render()[0])
        _mip(g, FOLD_MIN)
        assert _same(good, _frame(g))
