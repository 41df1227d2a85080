"""An isosurface frame (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO, vrc_set_isosurface, vrc_get_projection_gradients) through
the C ABI on the GPU, held to the float64 reference of tests/iso_ref.py by its acceptance rule; tests/test_iso_cpu.py
checks the rule, the scenes, the isovalues and the host build on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import depth_ref
import iso_ref
import mip_ref
import mip_scenes
import nonfinite
import scenes
import skip_window
import voxel_types
from gpu_run import GpuScene
from iso_ref import ISO
from libre_amd import vrc

pytestmark = pytest.mark.gpu

KERNELS = {"reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
AMBIENT = 0.25


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _iso(g, iso, ambient=AMBIENT, skip=1, uniform=1):
    vrc.set_isosurface(g.L, g.ctx, iso, ambient)  # (first: the projection is refused on a context without an isosurface)
    _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
    _opt(g, vrc.OPT_MIP_SKIP, skip)
    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)


def _readbacks(g, h=None):
    h = g.s.H if h is None else h
    v = np.full((h, g.s.W), np.nan, dtype=np.float32)
    c = np.full((h, g.s.W), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    d, _ = vrc.projection_depths(g.L, g.ctx, g.s.W, h, xyz=False)
    return v, c, d, vrc.projection_gradients(g.L, g.ctx, g.s.W, h)


def _frame(g, **kw):
    """(frame, samples, V, counts, D, G) of one isosurface frame"""
    fb, n, _ = g.render(**kw)
    return (fb, n) + _readbacks(g)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b) if isinstance(x, np.ndarray))


def _kernel_name(dda, fixed, mode, atlas="unsigned char", clamp=False):
    b = lambda x: "true" if x else "false"  # noqa: E731
    return ("vrc_k_raycast_mip<%s,%s,%s,%d,%s,false>" % (b(dda), b(clamp), b(fixed), mode, atlas)).encode()


def _check_shading(s, out, iso, ambient, frac_bits=8):
    """The frame is (c.rgb c.a s, c.a) with c the classification of the isovalue and s recomputed in float32 from the
    read-back G and the host build's float32 ray directions; missed pixels stay cleared."""
    fb, _, v, c, d, g = out
    hit = c == 1
    col = mip_ref.classify64(s, np.float64(iso), frac_bits).astype(np.float32)
    sh = iso_ref.shade32(g, depth_ref.rays32(s)[..., 5:8], ambient)
    want = np.empty_like(fb)
    want[..., :3] = col[:3][None, None, :] * sh[..., None]
    want[..., 3] = col[3]
    err = float(np.abs(fb - want)[hit].max())
    print("  shading: worst error %.3g over %d hit pixels (E0 = %.3g); s in [%.3f, %.3f]"
          % (err, int(hit.sum()), scenes.E0, float(sh[hit].min()), float(sh[hit].max())))
    assert hit.sum() >= 100 and err <= scenes.E0
    assert sh[hit].min() >= ambient - 1e-6 and sh[hit].max() <= 1.0 + 1e-6
    assert (fb[~hit] == 0).all()


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["axis", "spin", "inside", "clip"])
def test_every_served_form_passes_the_rule(name, kernel, filter_mode):
    what = "%s %s filter %d" % (name, kernel, filter_mode)
    s, r = iso_ref.scene(name, filter_mode), iso_ref.ref(name, filter_mode)
    tol = iso_ref.tolerance(s, filter_mode)
    mode = (8 if filter_mode else 7) + 16 * 3  # the first-crossing fold
    with GpuScene(s) as g:
        _iso(g, ISO[name], skip=0)
        out = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert g.L.vrc_last_kernel() == _kernel_name(kernel == "dda", not filter_mode, mode)
        bad, worst = iso_ref.check(r, out[2], out[3], out[4], out[5], tol)
        print("%s: %d failing pixels of %d hit, worst depth error %.2g steps" % (what, bad, int((out[3] == 1).sum()), worst))
        assert bad == 0, what
        _check_shading(s, out, ISO[name], AMBIENT)
        # the float stepping takes the same sample set and labels it by the same formula
        out0 = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=0)
        assert iso_ref.check(r, out0[2], out0[3], out0[4], out0[5], tol)[0] == 0, what + " stepping 0"
        # with skipping on: the same bits, fewer samples
        _iso(g, ISO[name], skip=1)
        on = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert _same(out, on) and on[1] < out[1], what


def _to_q(image):
    if image == "uint16":
        return (lambda x: x), 1.0
    im = voxel_types.IMAGES[image]
    return (lambda x: (x - im.a) / im.b), im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    """uint16, int16 (a negative isovalue) and float pools: the answer commutes with the affine image v = a + b q
    (b > 0): V and G come back in the volume's own units."""
    q, t, _ = mip_scenes.typed(image)
    tol = iso_ref.typed_tolerance(image, filter_mode)
    r = iso_ref.typed_ref(image, filter_mode)
    iso_q, iso_t = iso_ref.typed_iso(image)
    to_q, b = _to_q(image)
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        out = {}
        for skip in (0, 1):
            for kernel in sorted(KERNELS):
                _iso(g, iso_t, skip=skip)
                out[skip, kernel] = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        fb, n, v, c, d, grad = out[0, "dda"]
        bad, worst = iso_ref.check(r, to_q(v.astype(np.float64)), c, d, grad.astype(np.float64) / b, tol)
        print("%s filter %d: %d failing pixels of %d hit, worst depth error %.2g steps" % (image, filter_mode, bad, int((c == 1).sum()), worst))
        assert bad == 0
        for key, o in out.items():
            assert _same(out[0, "dda"], o), key
        assert out[1, "dda"][1] < n and out[1, "reforder"][1] < n


def test_nan_voxels_never_hit():
    case = nonfinite.case("allnan_brick")
    q, t = case.mq, case.mt
    tol = scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    r = iso_ref.nan_ref()
    im = nonfinite.IMAGE
    iso_t = float(np.float32(im.a + im.b * iso_ref.NAN_ISO_Q))
    # the rays that sample the NaN brick and nothing else up to the clip plane
    m = nonfinite.mref("allnan_brick")
    with voxel_types.typed_gpu_scene(t) as g:
        out = {}
        for skip in (0, 1):
            _iso(g, iso_t, skip=skip)
            out[skip] = _frame(g)
        fb, n, v, c, d, grad = out[0]
        with np.errstate(invalid="ignore"):
            qv = (v.astype(np.float64) - im.a) / im.b
        assert iso_ref.check(r, qv, c, d, grad.astype(np.float64) / im.b, tol)[0] == 0
        only_nan = m.certain & (m.m == nonfinite.Q_NAN) & r.miss() & ~r.hit()  # (the q scene's stand-in for NaN is its smallest value)
        assert only_nan.sum() > 50 and (c[only_nan] == 0).all() and np.isposinf(d[only_nan]).all()
        assert _same(out[0], out[1]) and out[1][1] <= n


def test_the_clamped_sampler():
    """A brick without overlap (the nucleon fixture) takes the clamped sampler, and the gradient's indices clamp at the
    slot's faces."""
    s, r = iso_ref.nucleon_scene(), iso_ref.nucleon_ref()
    with GpuScene(s) as g:
        out = {}
        for kernel in sorted(KERNELS):
            for skip in (0, 1):
                _iso(g, iso_ref.NUCLEON_ISO, skip=skip)
                out[kernel, skip] = o = _frame(g, kernel=KERNELS[kernel])
                assert b"<%s,true,false,55," % (b"true" if kernel == "dda" else b"false") in g.L.vrc_last_kernel()
                bad, worst = iso_ref.check(r, o[2], o[3], o[4], o[5])
                print("nucleon %s skip %d: %d failing pixels, worst depth error %.2g steps" % (kernel, skip, bad, worst))
                assert bad == 0, (kernel, skip)
        for key, o in out.items():
            assert _same(out["dda", 0], o), key
        for filter_mode in (0, 1):  # trilinear samples: the bitwise identities
            _iso(g, iso_ref.NUCLEON_ISO, skip=0)
            a = _frame(g, filter_mode=filter_mode)
            _iso(g, iso_ref.NUCLEON_ISO, skip=1)
            assert _same(a, _frame(g, filter_mode=filter_mode))


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_skipping_and_uniform_bricks_change_no_bit(name, filter_mode):
    s, r = iso_ref.scene(name), iso_ref.ref(name, filter_mode)
    with GpuScene(s) as g:
        out = {}
        for skip in (0, 1):
            for uniform in (0, 1):
                _iso(g, ISO[name], skip=skip, uniform=uniform)
                out[skip, uniform] = _frame(g, kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode)
        fb, n, v, c, d, grad = out[0, 0]
        assert iso_ref.check(r, v, c, d, grad, iso_ref.tolerance(s, filter_mode))[0] == 0
        for key, o in out.items():
            assert _same(out[0, 0], o), key
        print("%s filter %d: samples %d, with skipping %d / %d" % (name, filter_mode, n, out[1, 0][1], out[1, 1][1]))
        assert out[0, 1][1] == n and out[1, 1][1] == out[1, 0][1], "uniform bricks: the same count"
        assert out[1, 0][1] < n
        if not filter_mode:
            # how many, not only fewer (tests/skip_window.py: the window predicted from mip_ref, the largest voxel NumPy
            # finds in every uploaded brick and the header's rule), for the grid walk and for the loop in list order
            skip_window.check(skip_window.iso_of(name, skip_window.DDA), out[1, 0][1], "%s isosurface, grid walk" % name)
            for uniform in (0, 1):
                _iso(g, ISO[name], skip=1, uniform=uniform)
                o = _frame(g, kernel=vrc.KERNEL_REFERENCE_ORDER)
                assert iso_ref.check(r, o[2], o[3], o[4], o[5], iso_ref.tolerance(s, filter_mode))[0] == 0
                skip_window.check(skip_window.iso_of(name, skip_window.REFORDER), o[1],
                                  "%s isosurface, reference order, uniform bricks %d" % (name, uniform))
            _iso(g, ISO[name], skip=0, uniform=0)
        # without skipping the count is the MIP frame's without skipping
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        _opt(g, vrc.OPT_MIP_FOLD, 0)
        _opt(g, vrc.OPT_MIP_SKIP, 0)
        assert g.render(kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode)[1] == n


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["spin", "two blocks", "skip"])
def test_three_passes_equal_one(name, kernel):
    s = iso_ref.scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    with GpuScene(s) as g:
        for filter_mode in (0, 1):
            _iso(g, ISO[name], skip=0, uniform=0)
            plain = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
            for uniform in (0, 1):
                _iso(g, ISO[name], skip=1, uniform=uniform)
                one = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert _same(plain, one), (filter_mode, uniform)
                for order in (parts, parts[::-1], [parts[1], parts[2], parts[0]], [parts[2], parts[0], parts[1]]):
                    three = _frame(g, kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode, passes=order)
                    differ = int((one[4] != three[4]).sum())
                    assert _same(one, three), (filter_mode, uniform, order, "%d depths differ" % differ)


def test_row_map_and_caller_owned_framebuffer():
    s = iso_ref.scene("spin")
    with GpuScene(s) as g:
        _iso(g, ISO["spin"])
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
            assert _same(full[2:], _readbacks(g))
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


def test_ambient_one_is_the_constant_colour():
    s = iso_ref.scene("spin")
    with GpuScene(s) as g:
        _iso(g, ISO["spin"], ambient=1.0)
        fb, n, v, c, d, grad = _frame(g)
        hit = c == 1
        col = mip_ref.classify64(s, np.float64(ISO["spin"])).astype(np.float32)
        assert hit.sum() >= 100 and (fb[hit] == fb[hit][0]).all() and np.abs(fb[hit][0] - col).max() <= scenes.E0
        assert (fb[~hit] == 0).all()
        _iso(g, ISO["spin"], ambient=0.0)
        dark = _frame(g)
        assert _same((v, c, d, grad), dark[2:]), "the ambient share changes the frame alone"
        _check_shading(s, dark, ISO["spin"], 0.0)


def test_refusals_name_the_option_and_leave_the_context_usable():
    s = iso_ref.scene("spin")
    with GpuScene(s) as g:
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        grad = np.zeros((s.H, s.W, 3), dtype=np.float32)
        get = lambda: L.vrc_get_projection_gradients(g.ctx, grad.ctypes.data)  # noqa: E731
        composite, _, _ = g.render()
        assert get() == vrc.VRC_EINVAL and b"vrc_get_projection_gradients" in L.vrc_last_error()
        # before the first vrc_set_isosurface no render under the projection is served: already its selection is refused,
        # naming the function, and the context renders what it did
        assert L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO) == vrc.VRC_EINVAL
        assert b"vrc_set_isosurface" in L.vrc_last_error() and b"VRC_OPT_PROJECTION" in L.vrc_last_error()
        assert np.array_equal(composite, g.render()[0])
        # bad arguments name themselves and change nothing
        for iso, ambient, name in ((float("nan"), 0.5, b"iso_value"), (1.0, float("nan"), b"ambient"), (1.0, -0.01, b"ambient"),
                                   (1.0, 1.5, b"ambient")):
            assert L.vrc_set_isosurface(g.ctx, iso, ambient) == vrc.VRC_EINVAL and name in L.vrc_last_error()
        assert L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, 3) == vrc.VRC_EINVAL and b"VRC_OPT_PROJECTION" in L.vrc_last_error()
        _iso(g, ISO["spin"])
        good = _frame(g)
        assert get() == vrc.VRC_OK and np.array_equal(grad, good[5])
        # what a MIP frame is refused for
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            with pytest.raises(vrc.VrcError) as e:
                g.render(kernel=kernel)
            assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_KERNEL" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(variant=1)
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_VARIANT" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(ray_lod=(1.0, 0.01))
        assert e.value.code == vrc.VRC_EINVAL and "vrc_set_ray_lod" in str(e.value)
        assert _same(good, _frame(g))
        # neither value nor the projection may change inside a frame
        for change, name, back in ((lambda: vrc.set_isosurface(L, g.ctx, ISO["spin"] + 1.0, AMBIENT), b"vrc_set_isosurface",
                                    lambda: vrc.set_isosurface(L, g.ctx, ISO["spin"], AMBIENT)),
                                   (lambda: vrc.set_isosurface(L, g.ctx, ISO["spin"], 0.5), b"vrc_set_isosurface",
                                    lambda: vrc.set_isosurface(L, g.ctx, ISO["spin"], AMBIENT)),
                                   (lambda: _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), b"VRC_OPT_PROJECTION",
                                    lambda: _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO))):
            vrc.check(L, L.vrc_pre_render(g.ctx, view))
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            change()
            assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
            assert name in L.vrc_last_error()
            back()
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            vrc.check(L, L.vrc_post_render(g.ctx, None))
        g.render(passes=[])  # a new frame without a pass: nothing yet
        assert get() == vrc.VRC_EINVAL
        assert _same(good, _frame(g))
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        assert np.array_equal(composite, g.render()[0])
        assert get() == vrc.VRC_EINVAL


def test_nothing_else_changes():
    """With an isovalue set, a composite frame and MIP frames of every fold, with and without depth, are bit for bit those
    rendered before it was set, by the kernel instances of the same names."""
    s = iso_ref.scene("spin")

    def others(g):
        out = []
        for filter_mode in (0, 1):
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
            fb, n, _ = g.render(filter_mode=filter_mode)
            out.append((fb, n, g.L.vrc_last_kernel()))
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
            for fold in (0, 1, 2):
                for depth in (0, 1):
                    _opt(g, vrc.OPT_MIP_FOLD, fold)
                    _opt(g, vrc.OPT_MIP_DEPTH, depth)
                    fb, n, _ = g.render(filter_mode=filter_mode)
                    v = np.zeros((s.H, s.W), dtype=np.float32)
                    c = np.zeros((s.H, s.W), dtype=np.uint32)
                    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
                    out.append((fb, n, g.L.vrc_last_kernel(), v, c))
            _opt(g, vrc.OPT_MIP_FOLD, 0)
            _opt(g, vrc.OPT_MIP_DEPTH, 0)
        return out

    with GpuScene(s) as g:
        before = others(g)
        assert all(b",%d," % (m + 48) not in o[2] for o in before for m in (7, 8))
        _iso(g, ISO["spin"])
        _frame(g)
        after = others(g)
        assert len(before) == len(after)
        for a, b in zip(before, after):
            assert a[1] == b[1] and a[2] == b[2] and _same(a, b), a[2]
