"""A pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1) through the C ABI on the GPU: held to the float64
reference of tests/preint_ref.py by the frozen rule of tests/scenes.py, its table to preint_ref's own quadrature, and the
frame to the plain frame of the same context by the bitwise identities of the contract (include/vrc_hip.h, "A
pre-integrated composite frame").  tests/test_preint_cpu.py checks the rule, the scenes and the host build on the CPU.
Every test here fails on a library without the option: vrc_set_option refuses 32."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import mip_scenes
import orc
import preint_ref
import scenes
import voxel_types
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

KERNELS = {"auto": vrc.KERNEL_AUTO, "reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
NAME = b"vrc_k_raycast_preint<"


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _get(g, option):
    v = C.c_int64(-1)
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, option, C.byref(v)))
    return int(v.value)


def _frame(g, on, **kw):
    _opt(g, vrc.OPT_PREINTEGRATION, on)
    fb, n, _ = g.render(**kw)
    return fb, n, g.L.vrc_last_kernel()


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and a[1] == b[1]


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", preint_ref.NAMES)
def test_every_served_form_passes_the_rule(name, kernel, filter_mode):
    what = "%s %s filter %d" % (name, kernel, filter_mode)
    s, r = preint_ref.scene(name), preint_ref.ref(name, filter_mode)
    with GpuScene(s) as g:
        for stepping in (1, 0):
            fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=stepping)
            assert k.startswith(NAME) and (b",%d," % (15 if filter_mode else 14)) in k, k
            preint_ref.check(s, fb, r, "%s stepping %d" % (what, stepping))
            assert abs(n - r.samples) <= 1e-4 * r.samples + 8, (what, stepping, n, r.samples)
        off = _frame(g, 0, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert NAME not in off[2], off[2]


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    q, t, _ = mip_scenes.typed(image)
    r = preint_ref.typed_ref(image, filter_mode)
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        for kernel in ("dda", "reforder"):
            what = "%s %s filter %d" % (image, kernel, filter_mode)
            fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
            assert k.startswith(NAME) and (b"float" if image == "float" else b"unsigned short") in k, k
            preint_ref.check(q, fb, r, what)
            assert abs(n - r.samples) <= 1e-4 * r.samples + 8, (what, n, r.samples)


def test_the_clamped_sampler():
    """A brick without overlap (the nucleon fixture) takes the clamped sampler."""
    s = preint_ref.scene("nucleon")
    with GpuScene(s) as g:
        for filter_mode in (0, 1):
            r = preint_ref.ref("nucleon", filter_mode)
            for kernel in ("dda", "reforder"):
                fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert b"<%s,true,false,%d," % (b"true" if kernel == "dda" else b"false", 15 if filter_mode else 14) in k, k
                preint_ref.check(s, fb, r, "nucleon %s filter %d" % (kernel, filter_mode))


# ---- the table -----------------------------------------------------------------------------------------------------------
def _table(g):
    t, kind = vrc.preintegrated_table(g.L, g.ctx)
    return t, kind


def _check_table(g, s, kind, what, frac_bits=8):
    t, got_kind = _table(g)
    assert got_kind == kind, (what, got_kind)
    rd = s.render
    k = float(np.float32(np.float32(rd.maxSamplesPerRay) / np.float32(rd.samplesPerRay)))
    want = preint_ref.table(s.tf, float(rd.dataSourceRange[0]), float(rd.dataSourceRange[1]), k, kind, frac_bits=frac_bits)
    off = ~np.eye(256, dtype=bool)
    worst = float(np.abs(t.astype(np.float64) - want)[off].max())
    print("%s: worst |table - quadrature| off the diagonal %.3g" % (what, worst))
    assert worst <= 1e-6, what
    assert np.array_equal(t, t.transpose(1, 0, 2)), "%s: symmetric bit for bit" % what
    d = np.arange(256)
    if kind == preint_ref.TEXEL:
        assert float(np.abs(t[d, d].astype(np.float64) - want[d, d]).max()) <= 1e-6, what
    return t


def test_both_tables_against_the_reference_quadrature():
    s = copy.copy(preint_ref.scene("peak"))
    with GpuScene(s) as g:
        with pytest.raises(vrc.VrcError) as e:
            vrc.preintegrated_table(g.L, g.ctx)
        assert e.value.code == vrc.VRC_EINVAL
        _frame(g, 0)
        with pytest.raises(vrc.VrcError):
            vrc.preintegrated_table(g.L, g.ctx)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 0
        for frac_bits in (8, 0):
            _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA, frac_bits=frac_bits)
            t = _check_table(g, s, preint_ref.VALUE, "peak, value-indexed, frac bits %d" % frac_bits, frac_bits)
            # the diagonal: the classified table's entries, bit for bit -- what a volume of one value per brick shows
            lut = preint_ref.harness_lut(s.tf, 0.0, 255.0, np.float32(32.0) / np.float32(s.render.samplesPerRay), frac_bits)
            d = np.arange(256)
            assert float(np.abs(t[d, d].astype(np.float64) - lut).max()) <= 1e-6
        _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA, filter_mode=1)
        _check_table(g, s, preint_ref.TEXEL, "peak, texel-indexed")
    s = copy.copy(preint_ref.scene("spin"))
    with GpuScene(s) as g:
        _frame(g, 1)
        _check_table(g, s, preint_ref.VALUE, "spin, value-indexed")
        _frame(g, 1, filter_mode=1)
        _check_table(g, s, preint_ref.TEXEL, "spin, texel-indexed")


def test_the_value_indexed_diagonal_is_the_plain_frames_classified_table():
    """bit for bit: a one-brick volume of one value v shows lut[v] after one sample; here through the frames of `axis`
    (bricks of one value each), whose plain and pre-integrated frames are equal bit for bit, and entry by entry: every
    diagonal entry composited once from zero is the entry itself"""
    s = preint_ref.scene("axis")
    with GpuScene(s) as g:
        for frac_bits in (8, 0):
            for uniform in (1, 0):
                _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)
                for kernel in ("dda", "reforder"):
                    plain = _frame(g, 0, kernel=KERNELS[kernel], frac_bits=frac_bits)
                    pre = _frame(g, 1, kernel=KERNELS[kernel], frac_bits=frac_bits)
                    assert pre[2].startswith(NAME) and _same(plain, pre), (frac_bits, uniform, kernel)
                    assert plain[1] > 0 and float(plain[0][..., 3].max()) > 0.1


def test_the_table_is_rebuilt_when_its_inputs_change_and_only_then():
    s = copy.copy(preint_ref.scene("spin"))
    s.render = copy.copy(s.render)
    with GpuScene(s) as g:
        a = _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 1
        for _ in range(3):
            assert _same(a, _frame(g, 1))
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 1, "identical frames build nothing"
        _frame(g, 0)
        _frame(g, 1, kernel=vrc.KERNEL_REFERENCE_ORDER)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 1, "neither the plain frame between nor another kernel form"
        t0, _ = _table(g)
        # the kind
        _frame(g, 1, filter_mode=1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 2 and _table(g)[1] == preint_ref.TEXEL
        _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 3 and _table(g)[1] == preint_ref.VALUE
        assert np.array_equal(_table(g)[0], t0)
        # the transfer function
        saved = s.tf
        s.tf = preint_ref.peak_tf()
        _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 4
        _check_table(g, s, preint_ref.VALUE, "after vrc_update with another transfer function")
        s.tf = saved
        _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 5 and np.array_equal(_table(g)[0], t0)
        # samples per ray (k) and the range
        spr = s.render.samplesPerRay
        s.render.samplesPerRay = spr // 2
        _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 6
        _check_table(g, s, preint_ref.VALUE, "after a change of samplesPerRay")
        s.render.samplesPerRay = spr
        s.render.dataSourceRange[0], s.render.dataSourceRange[1] = 10.0, 200.0
        _frame(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 7
        _check_table(g, s, preint_ref.VALUE, "after a change of range")
        # read-only
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_PREINT_BUILDS, 0) == vrc.VRC_EINVAL
        assert b"VRC_OPT_PREINT_BUILDS" in g.L.vrc_last_error()


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spin", "peak", "clip"])
def test_uniform_bricks_change_no_bit(name):
    s = preint_ref.scene(name)
    with GpuScene(s) as g:
        for kernel in ("dda", "reforder"):
            out = {}
            for uniform in (0, 1):
                _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)
                out[uniform] = _frame(g, 1, kernel=KERNELS[kernel])
            assert _same(out[0], out[1]), kernel


@pytest.mark.parametrize("name", ["spin", "peak"])
def test_three_passes_equal_one(name):
    s = preint_ref.scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    with GpuScene(s) as g:
        asked = 0
        for filter_mode in (0, 1):
            kw = dict(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode)
            p1, p3 = _frame(g, 0, **kw), _frame(g, 0, passes=parts, **kw)
            if not _same(p1, p3):  # the precondition: the plain passes equal one pass
                continue
            l1, l3 = _frame(g, 1, **kw), _frame(g, 1, passes=parts, **kw)
            assert l1[2].startswith(NAME) and _same(l1, l3), filter_mode
            asked += 1
        assert asked >= 1


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_the_sample_count_is_the_plain_frames_where_no_ray_ends_early(filter_mode):
    for name in ("spin", "clip", "nucleon"):
        s = copy.copy(preint_ref.scene(name))
        tf = np.array(s.tf, dtype=np.float32).reshape(256, 4).copy()
        tf[:, 3] *= np.float32(0.02)
        s.tf = np.ascontiguousarray(tf)
        with GpuScene(s) as g:
            for kernel in ("dda", "reforder"):
                for stepping in (1, 0):
                    kw = dict(kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=stepping)
                    plain, pre = _frame(g, 0, **kw), _frame(g, 1, **kw)
                    assert float(plain[0][..., 3].max()) < 0.9 and float(pre[0][..., 3].max()) < 0.9
                    assert pre[2].startswith(NAME) and plain[1] == pre[1] > 0, (name, kernel, stepping)
                    assert not np.array_equal(plain[0], pre[0])


def test_an_atlas_of_more_than_2_pow_32_voxels():
    """(the pool of tests/test_gpu_parity.py::test_atlas_of_more_than_2_pow_32_voxels: bricks on both sides of the line;
    the BIG instances, whose slot base moves into the lane's pointer): the frame of the small pool, bit for bit"""
    from test_gpu_parity import _frames_in_a_large_pool
    s = scenes.get("hash64_spin")
    for flt, kernel in ((0, vrc.KERNEL_GRID_DDA), (1, vrc.KERNEL_REFERENCE_ORDER)):
        base = {vrc.OPT_FILTER: flt, vrc.OPT_KERNEL: kernel}
        with GpuScene(s) as g:
            small = _frame(g, 1, kernel=kernel, filter_mode=flt, stepping=0)  # (8-bit voxels of such an atlas step in float)
            plain_small = _frame(g, 0, kernel=kernel, filter_mode=flt, stepping=0)
        plain, pre = _frames_in_a_large_pool(vrc, s, 6 * 1000 ** 3, 2 ** 32,
                                             [({**base, vrc.OPT_PREINTEGRATION: 0}, None),
                                              ({**base, vrc.OPT_PREINTEGRATION: 1}, None)])
        assert pre[3].startswith("vrc_k_raycast_preint<") and pre[3].endswith(",true>"), pre[3]
        assert "preint" not in plain[3]
        assert np.array_equal(pre[0], small[0]) and pre[1] == small[1] > 0, "the frame of the small pool"
        assert np.array_equal(plain[0], plain_small[0])
        assert not np.array_equal(pre[0], plain[0])


def test_row_map_and_caller_owned_framebuffer():
    s = preint_ref.scene("spin")
    with GpuScene(s) as g:
        full = _frame(g, 1)
        rows = np.array([3, 4, 5, 17, 18, 30, 35], dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        saved = g.s.H
        try:
            g.s.H = len(rows)  # the buffer GpuScene reads back
            band = _frame(g, 1)
        finally:
            g.s.H = saved
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        assert band[2].startswith(NAME) and np.array_equal(full[0][rows], band[0])
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full[0])
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


# ---- what is refused, and what does not change -----------------------------------------------------------------------------
def test_refusals_name_the_option_and_leave_the_context_usable():
    s = preint_ref.scene("spin")
    with GpuScene(s) as g:
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        assert _get(g, vrc.OPT_PREINTEGRATION) == 0
        for bad in (2, -1):
            assert L.vrc_set_option(g.ctx, vrc.OPT_PREINTEGRATION, bad) == vrc.VRC_EINVAL
            assert b"VRC_OPT_PREINTEGRATION" in L.vrc_last_error()
        assert _get(g, vrc.OPT_PREINTEGRATION) == 0
        good = _frame(g, 1)
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            with pytest.raises(vrc.VrcError) as e:
                g.render(kernel=kernel, filter_mode=1)
            assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_KERNEL" in str(e.value) and "VRC_OPT_PREINTEGRATION" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(variant=1)
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_VARIANT" in str(e.value) and "VRC_OPT_PREINTEGRATION" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(ray_lod=(1.0, 0.01))
        assert e.value.code == vrc.VRC_EINVAL and "vrc_set_ray_lod" in str(e.value) and "VRC_OPT_PREINTEGRATION" in str(e.value)
        for option, value in ((vrc.OPT_SHADING, 1), (vrc.OPT_COMPOSITE_DEPTH, 500)):
            _opt(g, option, value)
            with pytest.raises(vrc.VrcError) as e:
                g.render()
            assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_PREINTEGRATION" in str(e.value)
            _opt(g, option, 0)
        assert _same(good, _frame(g, 1))
        # the option may not change inside a frame
        for first in (1, 0):
            _opt(g, vrc.OPT_PREINTEGRATION, first)
            vrc.check(L, L.vrc_pre_render(g.ctx, view))
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            _opt(g, vrc.OPT_PREINTEGRATION, 1 - first)
            assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
            assert b"VRC_OPT_PREINTEGRATION" in L.vrc_last_error()
            _opt(g, vrc.OPT_PREINTEGRATION, first)
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            vrc.check(L, L.vrc_post_render(g.ctx, None))
        assert _same(good, _frame(g, 1))


def test_depth_split_compaction_grey_table_are_the_plain_preintegrated_kernel():
    s = copy.copy(preint_ref.scene("inside"))
    with GpuScene(s) as g:
        want = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
        for option, value in ((vrc.OPT_DEPTH_SPLIT, 1), (vrc.OPT_ERT_COMPACTION, 4), (vrc.OPT_GREY_TABLE, 1)):
            _opt(g, option, value)
            got = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
            assert got[2] == want[2] and _same(got, want), option
            _opt(g, option, 0)


def test_nothing_else_changes():
    """With the option at 0 the composite frame is bit for bit that of a context that never set it, launched by the
    same kernel instances; MIP and isosurface frames are bit-identical with the option at 0 and 1."""
    s = preint_ref.scene("spin")

    def others(g, on):
        out = []
        for filter_mode in (0, 1):
            _opt(g, vrc.OPT_PREINTEGRATION, 0)
            for kernel in sorted(KERNELS):
                _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
                fb, n, _ = g.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
                out.append((fb, n, g.L.vrc_last_kernel()))
            _opt(g, vrc.OPT_PREINTEGRATION, on)  # MIP and isosurface frames ignore it
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
            fb, n, _ = g.render(filter_mode=filter_mode)
            out.append((fb, n, g.L.vrc_last_kernel()))
            vrc.set_isosurface(g.L, g.ctx, 150.0, 0.25)
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
            fb, n, _ = g.render(filter_mode=filter_mode)
            out.append((fb, n, g.L.vrc_last_kernel()))
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        return out

    with GpuScene(s) as never:
        never_set = []
        for filter_mode in (0, 1):
            for kernel in sorted(KERNELS):
                fb, n, _ = never.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
                never_set.append((fb, n, never.L.vrc_last_kernel()))
    with GpuScene(s) as g:
        before = others(g, 0)
        assert all(b"preint" not in o[2] for o in before)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 0, "no table is built, and none allocated, with the option at 0"
        composite = before[0:3] + before[5:8]
        for a, b in zip(never_set, composite):
            assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]), a[2]
        _frame(g, 1)
        _frame(g, 1, filter_mode=1)
        after = others(g, 1)
        assert _get(g, vrc.OPT_PREINT_BUILDS) == 2, "MIP and isosurface frames build no table"
        for a, b in zip(before, after):
            assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]), a[2]


def test_the_walk_cache_is_undisturbed():
    """Plain frames reach the replay; a pre-integrated frame reads 0 in VRC_OPT_WALK_CACHE_USED and allocates no lists; the
    plain frames after it are bit for bit the earlier ones, walked or replayed."""
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(100, 76), spin=(0.5, 0.35), spr=256)
    with GpuScene(s) as g:
        _opt(g, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS)
        modes, frames = [], []
        for _ in range(6):
            fb, n, _k = _frame(g, 0, kernel=vrc.KERNEL_GRID_DDA)
            modes.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            frames.append((fb, n))
        assert modes[-1] == 4 and b"vrc_k_raycast_replay<" in g.L.vrc_last_kernel(), modes
        held = _get(g, vrc.OPT_WALK_CACHE_BYTES)
        pre = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
        assert _get(g, vrc.OPT_WALK_CACHE_USED) == 0 and pre[2].startswith(NAME), pre[2]
        assert _get(g, vrc.OPT_WALK_CACHE_BYTES) == held, "a pre-integrated frame allocates no lists"
        assert _same(pre, frames[0]), "mem:// bricks hold one value each: the plain frame"
        seen = []
        for _ in range(5):
            fb, n, _k = _frame(g, 0, kernel=vrc.KERNEL_GRID_DDA)
            seen.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            assert np.array_equal(fb, frames[0][0]) and n == frames[0][1], seen
        assert seen[-1] == 4, seen  # idle after the pre-integrated frame, recorded again, never stale
