"""A slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE, vrc_set_slice) through the C ABI on the GPU, held to the
float64 reference of tests/slice_ref.py by its acceptance rule; tests/test_slice_cpu.py checks the rule, the scenes, the
cap and the host build on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import mip_scenes
import nonfinite
import orc
import scenes
import slice_ref as sr
import voxel_types
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

KERNELS = {"reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
PROJECTION_SLICE = getattr(vrc, "PROJECTION_SLICE", 4)


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _get(g, option):
    v = C.c_int64()
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, option, C.byref(v)))
    return v.value


def _slice(g, plane, uniform=1):
    vrc.set_slice(g.L, g.ctx, plane)  # (first: the projection is refused on a context without a plane)
    _opt(g, vrc.OPT_PROJECTION, PROJECTION_SLICE)
    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)


def _readbacks(g, h=None):
    h = g.s.H if h is None else h
    v = np.full((h, g.s.W), np.nan, dtype=np.float32)
    c = np.full((h, g.s.W), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    d, xyz = vrc.projection_depths(g.L, g.ctx, g.s.W, h, xyz=True)
    return v, c, d, xyz


def _frame(g, **kw):
    """(frame, samples, V, counts, D, xyz) of one slice frame"""
    fb, n, _ = g.render(**kw)
    return (fb, n) + _readbacks(g)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b) if isinstance(x, np.ndarray))


def _kernel_name(dda, linear, atlas="unsigned char", big=False):
    b = lambda x: "true" if x else "false"  # noqa: E731
    return ("vrc_k_raycast_slice<%s,%s,%s,%s>" % (b(dda), b(linear), atlas, b(big))).encode()


def _check(r, out, what, to_q=None):
    fb, n, v, c, d, xyz = out
    vq = v.astype(np.float64) if to_q is None else to_q(v.astype(np.float64))
    bad = sr.check(r, vq, c, d, fb)
    print("%s: %d failing pixels; %d sampled of %d covered, %d with more than one candidate value" % (
        what, bad, int((c == 1).sum()), int(r.covered().sum()), int(r.multi().sum())))
    assert bad == 0, what
    assert n == int(c.sum()), "vrc_stats.samples: the pixels the pass sampled"
    # origin + D * dir of the pixel's ray lies on the plane
    hit = c == 1
    if hit.any():
        p = r.plane.astype(np.float64)
        off = np.abs(xyz[hit].astype(np.float64) @ p[:3] + p[3]) / np.sqrt(p[:3] @ p[:3])
        assert float(off.max()) <= 1e-5, what


# ---- 1. every served form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", sr.RULE_SCENES + ("behind", "outside", "face"))
def test_every_served_form_passes_the_rule(name, kernel, filter_mode):
    what = "%s %s filter %d" % (name, kernel, filter_mode)
    s, r = sr.scene(name), sr.ref(name, filter_mode)
    with GpuScene(s) as g:
        _slice(g, sr.plane(name))
        out = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert g.L.vrc_last_kernel() == _kernel_name(kernel == "dda", filter_mode)
        _check(r, out, what)
        if name in ("behind", "outside"):
            assert out[1] == 0 and not out[0].any() and not out[3].any() and np.isposinf(out[4]).all()
        if name == "face":  # every covered pixel matches one side or the other (the rule); none is unsampled
            assert (out[3][r.covered()] == 1).all()
        # samplesPerRay and the stepping are not read
        g.s.render.samplesPerRay, saved = 7, g.s.render.samplesPerRay
        try:
            assert _same(out, _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=0))
        finally:
            g.s.render.samplesPerRay = saved


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_a_cut_of_mixed_brick_sizes_in_list_order(filter_mode):
    s = sr.lod_scene()
    r = sr.render(s, sr.plane("oblique"), filter_mode)
    with GpuScene(s) as g:
        _slice(g, sr.plane("oblique"))
        out = _frame(g, kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode)
        assert g.L.vrc_last_kernel() == _kernel_name(False, filter_mode)
        _check(r, out, "lod cut filter %d" % filter_mode)


def test_edge_on():
    """A plane that contains the central ray, and one just beside it that the rays around the centre graze: no NaN or
    infinity in the frame; count 1 <=> D finite <=> pixel not cleared; V within the volume's own values."""
    s = sr.scene("edge-on")
    lo, hi = min(int(b.min()) for b in s.bricks.values()), max(int(b.max()) for b in s.bricks.values())
    sampled = 0
    with GpuScene(s) as g:
        for pl in (sr.plane("edge-on"), sr.plane_through((0.03, 0.0, 0.0), (1.0, 0.0, 0.0))):
            for kernel in sorted(KERNELS):
                for fm in (0, 1):
                    _slice(g, pl)
                    fb, n, v, c, d, _ = _frame(g, kernel=KERNELS[kernel], filter_mode=fm)
                    assert np.isfinite(fb).all()
                    assert np.array_equal(c == 1, np.isfinite(d)) and set(np.unique(c)) <= {0, 1}
                    assert not fb[c == 0].any() and n == int(c.sum())
                    assert ((v[c == 1] >= lo) & (v[c == 1] <= hi)).all()
                    sampled += n
    assert sampled > 0


# ---- 2., 3. voxel types, values that are not finite --------------------------------------------------------------------
def _to_q(image):
    if image == "uint16":
        return lambda x: x
    im = voxel_types.IMAGES[image]
    return lambda x: (x - im.a) / im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    """uint16, int16 and float pools: V comes back in the volume's own units, signed types un-shifted; the frame is the
    classification of (V - r0) / (r1 - r0), the q scene's."""
    q, t, _ = mip_scenes.typed(image)
    r = sr.typed_ref(image, filter_mode)
    atlas = {"uint16": "unsigned short", "int16": "unsigned short", "float": "float"}[image]
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        out = {}
        for kernel in sorted(KERNELS):
            _slice(g, sr.TYPED_PLANE)
            out[kernel] = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
            assert g.L.vrc_last_kernel() == _kernel_name(kernel == "dda", filter_mode, atlas)
            _check(r, out[kernel], "%s %s filter %d" % (image, kernel, filter_mode), _to_q(image))
        v = out["dda"][2][out["dda"][3] == 1]
        if image == "int16":
            assert v.min() < 0 < v.max()
        if image == "float":
            assert -1.0 <= v.min() < 0 < v.max() <= 1.0


def test_float_voxels_that_are_not_finite():
    """tests/nonfinite.py's contracts on its brick of NaNs, cut by an axial plane: a NaN voxel reads back as a NaN V with
    its count and depth and classifies as the first texel of the transfer function; with +infinity in its place the pixel
    is the last texel, with -infinity the first; a trilinear sample all of whose taps are NaN is NaN."""
    import copy
    case = nonfinite.case("allnan_brick")
    q, t = case.mq, case.mt
    im = nonfinite.IMAGE
    pl, r = sr.NAN_PLANE, sr.nan_ref()
    want = np.zeros((r.H, r.W), dtype=bool)
    for key, cs in r.cands.items():
        want[key] = bool(cs) and all(qv[0] == nonfinite.Q_NAN for qv in cs)  # (the q scene holds Q_NAN where t holds NaN)
    want &= r.sure
    inner = want.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(np.roll(want, dy, axis=0), dx, axis=1)
    assert want.sum() > 100 and inner.sum() > 50
    texel = lambda i: (t.tf[i] * np.array([t.tf[i][3]] * 3 + [1.0], dtype=np.float32)).astype(np.float32)  # noqa: E731
    assert texel(0).any() and not np.array_equal(texel(0), texel(255))
    for fill, is_it, colour in ((None, np.isnan, texel(0)), (np.inf, np.isposinf, texel(255)), (-np.inf, np.isneginf, texel(0))):
        u = t
        if fill is not None:
            u = copy.copy(t)
            u.bricks = {nid: np.where(np.isnan(b), np.float32(fill), b).astype(np.float32) for nid, b in t.bricks.items()}
        with voxel_types.typed_gpu_scene(u) as g:
            for kernel in sorted(KERNELS):
                _slice(g, pl)
                fb, n, v, c, d, _ = _frame(g, kernel=KERNELS[kernel])
                assert (c[want] == 1).all() and is_it(v[want]).all() and np.isfinite(d[want]).all(), (fill, kernel)
                assert np.abs(fb[want] - colour).max() <= scenes.E0, (fill, kernel)
                rest = np.isfinite(v)
                with np.errstate(invalid="ignore"):
                    vq = (v.astype(np.float64) - im.a) / im.b
                assert sr.check(r, np.where(rest, vq, nonfinite.Q_NAN), c, d) == 0, (fill, kernel)
                assert n == int(c.sum())
                if fill is None:
                    v1, c1 = _frame(g, kernel=KERNELS[kernel], filter_mode=1)[2:4]
                    assert (c1[inner] == 1).all() and np.isnan(v1[inner]).all(), kernel


# ---- 4. an atlas of more than 2^32 voxels --------------------------------------------------------------------------------
def test_an_atlas_of_more_than_2_pow_32_voxels():
    """bricks on both sides of the 4 Gi-voxel line: the BIG instances, whose slot base moves into the lane's pointer, give
    the small pool's frame and read-backs bit for bit"""
    s, pl = sr.scene("oblique"), sr.plane("oblique")
    small = {}
    with GpuScene(s) as g:
        for fm, kernel in ((0, "dda"), (1, "reforder")):
            _slice(g, pl)
            small[fm] = _frame(g, kernel=KERNELS[kernel], filter_mode=fm)
    L = vrc.load_library()
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    try:
        mb = [s.vi.maximumBlockSize[a] for a in range(3)]
        vrc.check(L, L.vrc_pool_create(ctx, 1, 0, 0, 1, vrc.u32x3(*mb), 6 * 1000 ** 3, C.byref(pool)))
        sb, ab, fs = C.c_size_t(), C.c_size_t(), C.c_uint32()
        ad, sl = vrc.u32x3(), vrc.u32x3()
        vrc.check(L, L.vrc_pool_info(pool, C.byref(sb), ad, C.byref(ab), sl, C.byref(fs)))
        atlas_dim = list(ad)
        assert atlas_dim[0] * atlas_dim[1] * atlas_dim[2] > 2 ** 32
        slot_dim = [atlas_dim[a] // sl[a] for a in range(3)]
        slots, high = {}, 0
        for nid in s.ids:
            brick = s.bricks[nid]
            slot = vrc.f32x3()
            vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(brick.shape[2], brick.shape[1], brick.shape[0]), slot))
            slots[nid] = (slot[0], slot[1], slot[2])
            idx = [int(round(slot[a] * sl[a])) for a in range(3)]
            high += ((idx[2] * sl[1] + idx[1]) * sl[0] + idx[0]) * slot_dim[0] * slot_dim[1] * slot_dim[2] >= 2 ** 32
        assert 0 < high < len(s.ids)
        nodes = (vrc.NodeData * s.n_nodes)()
        for k, nid in enumerate(s.sorted_ids):
            tp, ts = orc.f32x3(), orc.f32x3()
            orc.lib().orc_texture_object(C.byref(s.vi), C.byref(s.lod[nid]), orc.f32x3(*slots[nid]), orc.u32x3(*atlas_dim), tp, ts)
            for a in range(3):
                nodes[k].textureMin[a], nodes[k].textureSize[a] = tp[a], ts[a]
                nodes[k].aabbMin[a], nodes[k].aabbSize[a] = s.nodes[k].aabbMin[a], s.nodes[k].aabbSize[a]
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        vrc.check(L, L.vrc_update(ctx, s.tf.ctypes.data, None, 0))
        vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_COUNT_SAMPLES, 1))
        vrc.set_slice(L, ctx, pl)
        vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_PROJECTION, PROJECTION_SLICE))
        for fm, kernel in ((0, "dda"), (1, "reforder")):
            vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_FILTER, fm))
            vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_KERNEL, KERNELS[kernel]))
            vrc.check(L, L.vrc_pre_render(ctx, view))
            vrc.check(L, L.vrc_render(ctx, view, nodes, s.n_nodes, render, pool))
            fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
            vrc.check(L, L.vrc_post_render(ctx, fb.ctypes.data))
            assert L.vrc_last_kernel() == _kernel_name(kernel == "dda", fm, big=True)
            v = np.zeros((s.H, s.W), dtype=np.float32)
            c = np.zeros((s.H, s.W), dtype=np.uint32)
            vrc.check(L, L.vrc_get_projection_values(ctx, v.ctypes.data, c.ctypes.data))
            d, _ = vrc.projection_depths(L, ctx, s.W, s.H, xyz=False)
            assert _same((fb, v, c, d), (small[fm][0], small[fm][2], small[fm][3], small[fm][4])), (fm, kernel)
            assert int(c.sum()) > 100
    finally:
        if pool:
            L.vrc_pool_destroy(pool)
        L.vrc_ctx_destroy(ctx)


# ---- 5. the clamped sampler --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_a_brick_without_overlap(filter_mode):
    s, r = sr.nucleon_scene(), sr.nucleon_ref(filter_mode)
    with GpuScene(s) as g:
        for kernel in sorted(KERNELS):
            _slice(g, sr.NUCLEON_PLANE)
            _check(r, _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode), "nucleon %s filter %d" % (kernel, filter_mode))


# ---- 6. row map and caller-owned frame buffer -----------------------------------------------------------------------------
def test_row_map_and_caller_owned_framebuffer():
    s = sr.scene("oblique")
    with GpuScene(s) as g:
        _slice(g, sr.plane("oblique"))
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
        assert int(band[3].sum()) > 20
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full[0])
            assert _same(full[2:], _readbacks(g))
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


# ---- 7. two passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_two_passes_in_both_orders(kernel, filter_mode):
    s, pl, r = sr.scene("oblique"), sr.plane("oblique"), sr.ref("oblique", filter_mode)
    h = s.n_nodes // 2
    single = r.single_node()
    with GpuScene(s) as g:
        _slice(g, pl)
        one = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode)
        for passes in ([(0, h), (h, s.n_nodes)], [(h, s.n_nodes), (0, h)]):
            two = _frame(g, kernel=KERNELS[kernel], filter_mode=filter_mode, passes=passes)
            _check(r, two, "two passes %s filter %d" % (kernel, filter_mode))
            assert two[1] == one[1]
            for a, b in zip(one, two):
                if isinstance(a, np.ndarray):
                    assert np.array_equal(a[single], b[single])


# ---- 8. uniform bricks, the ray cache, the sample count ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["mem", "oblique"])
def test_uniform_bricks_the_ray_cache_and_the_count(name):
    s, r = sr.scene(name), sr.ref(name)
    with GpuScene(s) as g:
        for kernel in sorted(KERNELS):
            _slice(g, sr.plane(name), uniform=0)
            off = _frame(g, kernel=KERNELS[kernel])
            _check(r, off, "%s %s" % (name, kernel))
            _slice(g, sr.plane(name), uniform=1)
            on = _frame(g, kernel=KERNELS[kernel])
            assert _same(off, on) and off[1] == on[1] == int(on[3].sum()) > 100
            # a still view: the grid form stores its rays on the second render and loads them from the third on
            used = []
            for _ in range(3):
                again = _frame(g, kernel=KERNELS[kernel])
                used.append(_get(g, vrc.OPT_RAY_CACHE_USED))
                assert _same(on, again) and again[1] == on[1]
            assert used[-1] == (2 if kernel == "dda" else 0), used
            assert _get(g, vrc.OPT_WALK_CACHE_USED) == 0
            _opt(g, vrc.OPT_COUNT_SAMPLES, 0)
            fb, n, _ = g.render(kernel=KERNELS[kernel], count=False)
            assert np.array_equal(fb, on[0]) and _same(on[2:], _readbacks(g))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_option_and_leave_the_context_usable():
    s, pl = sr.scene("oblique"), sr.plane("oblique")
    with GpuScene(s) as g:
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        grad = np.zeros((s.H, s.W, 3), dtype=np.float32)
        composite, _, _ = g.render()
        # before the first vrc_set_slice the projection's selection is refused, naming the function
        assert L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, PROJECTION_SLICE) == vrc.VRC_EINVAL
        assert b"vrc_set_slice" in L.vrc_last_error() and b"VRC_OPT_PROJECTION" in L.vrc_last_error()
        assert L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, 3) == vrc.VRC_EINVAL and b"VRC_OPT_PROJECTION" in L.vrc_last_error()
        assert np.array_equal(composite, g.render()[0])
        # bad planes name the argument and change nothing
        f4 = lambda *p: (C.c_float * 4)(*p)  # noqa: E731
        assert L.vrc_set_slice(g.ctx, None) == vrc.VRC_EINVAL and b"plane" in L.vrc_last_error()
        assert L.vrc_set_option(g.ctx, vrc.OPT_PROJECTION, PROJECTION_SLICE) == vrc.VRC_EINVAL  # still no plane
        _slice(g, pl)
        good = _frame(g)
        for bad in (f4(float("nan"), 0, 1, 0), f4(0, float("inf"), 1, 0), f4(0, 0, 1, float("-inf")), f4(0, 0, 0, 0.5)):
            assert L.vrc_set_slice(g.ctx, bad) == vrc.VRC_EINVAL and b"plane" in L.vrc_last_error()
        assert _same(good, _frame(g)), "the plane set before stays"
        # the gradients belong to an isosurface frame
        assert L.vrc_get_projection_gradients(g.ctx, grad.ctypes.data) == vrc.VRC_EINVAL
        assert b"vrc_get_projection_gradients" in L.vrc_last_error()
        # what a MIP frame is refused for
        for kw, word in ((dict(kernel=vrc.KERNEL_LDS), "VRC_OPT_KERNEL"), (dict(kernel=vrc.KERNEL_PACKED, filter_mode=1), "VRC_OPT_KERNEL"),
                         (dict(variant=vrc.VARIANT_GLRAYCASTER), "VRC_OPT_VARIANT"),
                         (dict(ray_lod=(1.0, orc.world_space_per_pixel(s))), "vrc_set_ray_lod")):
            with pytest.raises(vrc.VrcError) as e:
                g.render(**kw)
            assert e.value.code == vrc.VRC_EINVAL and word in str(e.value) and "SLICE" in str(e.value), (kw, str(e.value))
        assert _same(good, _frame(g))
        # neither the plane nor the projection may change inside a frame
        moved = pl.copy()
        moved[3] += 0.05
        for change, name, back in ((lambda: vrc.set_slice(L, g.ctx, moved), b"vrc_set_slice", lambda: vrc.set_slice(L, g.ctx, pl)),
                                   (lambda: _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), b"VRC_OPT_PROJECTION",
                                    lambda: _opt(g, vrc.OPT_PROJECTION, PROJECTION_SLICE))):
            vrc.check(L, L.vrc_pre_render(g.ctx, view))
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            change()
            assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
            assert name in L.vrc_last_error()
            back()
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            vrc.check(L, L.vrc_post_render(g.ctx, None))
        g.render(passes=[])  # a new frame without a pass: nothing to read back yet
        v = np.zeros((s.H, s.W), dtype=np.float32)
        assert L.vrc_get_projection_values(g.ctx, v.ctypes.data, None) == vrc.VRC_EINVAL
        assert _same(good, _frame(g))
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        assert np.array_equal(composite, g.render()[0])


# ---- 10. nothing else changes ---------------------------------------------------------------------------------------------
def test_a_slice_frame_between_other_frames_changes_none_of_them():
    """Composite frames (six over a still view: compute, store, load and count, record, replay) and MIP frames before and
    after a slice frame on one context: frame by frame bit for bit those of a fresh context, by the kernel instances of
    the same names at the same step of the walk cache; the slice frame allocates no lists."""
    s = sr.scene("mem")

    def others(g):
        out = []
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        for _ in range(6):
            fb, n, _ = g.render(kernel=vrc.KERNEL_GRID_DDA)
            out.append((fb, n, g.L.vrc_last_kernel(), _get(g, vrc.OPT_WALK_CACHE_USED)))
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        for depth in (0, 1):
            _opt(g, vrc.OPT_MIP_DEPTH, depth)
            fb, n, _ = g.render()
            v = np.zeros((s.H, s.W), dtype=np.float32)
            c = np.zeros((s.H, s.W), dtype=np.uint32)
            vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
            out.append((fb, n, g.L.vrc_last_kernel(), v, c))
        _opt(g, vrc.OPT_MIP_DEPTH, 0)
        return out

    with GpuScene(s) as g:
        fresh = others(g)
    assert all(b"slice" not in o[2] for o in fresh)
    with GpuScene(s) as g:
        _slice(g, sr.plane("mem"))
        _frame(g, kernel=vrc.KERNEL_GRID_DDA)
        assert _get(g, vrc.OPT_WALK_CACHE_BYTES) == 0 and _get(g, vrc.OPT_WALK_CACHE_USED) == 0
        before = others(g)
        lists = _get(g, vrc.OPT_WALK_CACHE_BYTES)
        _slice(g, sr.plane("mem"))
        mid = _frame(g, kernel=vrc.KERNEL_GRID_DDA)
        assert b"vrc_k_raycast_slice" in g.L.vrc_last_kernel() and int(mid[3].sum()) > 100
        assert _get(g, vrc.OPT_WALK_CACHE_BYTES) == lists and _get(g, vrc.OPT_WALK_CACHE_USED) == 0
        after = others(g)
    # frame by frame: the same bits, the same count, the same kernel instance -- and, for the composite frames of the
    # still view, the same step of the walk cache (a slice frame is to the ray cache of the other projections what a MIP
    # frame is: it forgets, and the frames behind it compute, store and load as those of a fresh context do)
    assert fresh[5][3] == 4
    for a, b, c in zip(fresh, before, after):
        assert a[1] == b[1] == c[1] and a[2] == b[2] == c[2], (a[2], b[2], c[2])
        assert _same(a, b) and _same(a, c), a[2]
        if not isinstance(a[3], np.ndarray):
            assert a[3] == b[3] == c[3], (a[3], b[3], c[3])


# ---- 11. the GPU against the host build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["oblique", "clip", "axial"])
def test_the_gpu_frame_is_the_host_builds_on_pixels_with_one_candidate(name, kernel):
    """Frame, V, counts and D, bit for bit.  The host build here is the one that evaluates vrc_classify_mip as the device
    does (slice_ref.harness( fused ): VRC_LERP2 in the device's form, a compiler that contracts where VRC_FAST_FP lets
    it); its V, counts and D are also those of the plain host build of tests/test_slice_cpu.py."""
    s, r = sr.scene(name), sr.ref(name)
    one = r.sure & ~r.multi() & r.single_node()
    assert int(one.sum()) > 100
    form = sr.GRID if kernel == "dda" else 0
    host = sr.harness_render(s, form, sr.plane(name), fused=True)
    plain = sr.harness_render(s, form, sr.plane(name))
    for k in (2, 3, 4):
        assert np.array_equal(host[k], plain[k], equal_nan=True)
    with GpuScene(s) as g:
        _slice(g, sr.plane(name))
        fb, n, v, c, d, _ = _frame(g, kernel=KERNELS[kernel])
    for a, b in zip((v, c, d, fb), (host[2], host[3], host[4], host[0])):
        assert np.array_equal(a[one], b[one])
