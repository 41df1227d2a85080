"""A shaded composite frame (VRC_OPT_SHADING = 1, VRC_OPT_SHADING_AMBIENT) through the C ABI on the GPU: held to the
float64 reference of tests/shade_ref.py by the frozen rule of tests/scenes.py, and to the unshaded frame of the same
context by the bitwise identities of the contract (include/vrc_hip.h, "A shaded composite frame").
tests/test_shade_cpu.py checks the rule, the scenes and the host build on the CPU.  Every test here fails on a library
without the option: vrc_set_option refuses 29."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import mip_scenes
import nonfinite
import orc
import scenes
import shade_ref
import voxel_types
from gpu_run import GpuScene
from libre_amd import vrc
from shade_ref import AMBIENT

pytestmark = pytest.mark.gpu

KERNELS = {"auto": vrc.KERNEL_AUTO, "reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
K1000 = int(round(AMBIENT * 1000))


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _get(g, option):
    v = C.c_int64(-1)
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, option, C.byref(v)))
    return int(v.value)


def _shading(g, on, k=K1000):
    _opt(g, vrc.OPT_SHADING_AMBIENT, k)
    _opt(g, vrc.OPT_SHADING, on)


def _frame(g, on, k=K1000, **kw):
    _shading(g, on, k)
    fb, n, _ = g.render(**kw)
    return fb, n, g.L.vrc_last_kernel()


def _identities(g, what, **kw):
    """identities 1 and 2 against the unshaded frame of the same context: alpha and the sample count; ambient 1000"""
    plain, lit, one = _frame(g, 0, **kw), _frame(g, 1, **kw), _frame(g, 1, 1000, **kw)
    assert b"vrc_k_raycast_shade<" not in plain[2] and b"vrc_k_raycast_shade<" in lit[2], (what, plain[2], lit[2])
    assert np.array_equal(plain[0][..., 3], lit[0][..., 3]), "%s: alpha" % what
    assert plain[1] == lit[1] == one[1] and plain[1] > 0, (what, plain[1], lit[1], one[1])
    assert np.array_equal(plain[0], one[0]), "%s: ambient 1000 is the unshaded frame" % what
    return plain, lit


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["axis", "spin", "inside", "clip", "nucleon"])
def test_every_served_form_passes_the_rule(name, kernel, filter_mode):
    what = "%s %s filter %d" % (name, kernel, filter_mode)
    s, r = shade_ref.scene(name), shade_ref.ref(name, filter_mode)
    with GpuScene(s) as g:
        fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
        assert k.startswith(b"vrc_k_raycast_shade<") and (b",%d," % (11 if filter_mode else 10)) in k, k
        shade_ref.check(s, fb, r, what)
        assert abs(n - r.samples) <= 1e-4 * r.samples + 8, (what, n, r.samples)
        fb0, _, _ = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=0)
        shade_ref.check(s, fb0, r, what + " stepping 0")
        if kernel != "auto" or not filter_mode:  # (AUTO's unshaded trilinear frame is the staged / packed form's)
            _identities(g, what, kernel=KERNELS[kernel], filter_mode=filter_mode)
            _identities(g, what + " stepping 0", kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=0)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    q, t, _ = mip_scenes.typed(image)
    r = shade_ref.typed_ref(image, filter_mode)
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        for kernel in ("dda", "reforder"):
            what = "%s %s filter %d" % (image, kernel, filter_mode)
            fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
            assert (b"float" if image == "float" else b"unsigned short") in k, k
            shade_ref.check(q, fb, r, what)
            _identities(g, what, kernel=KERNELS[kernel], filter_mode=filter_mode)


def test_the_clamped_sampler():
    """A brick without overlap (the nucleon fixture) takes the clamped sampler; the gradient's indices clamp at the slot's
    faces."""
    s = shade_ref.scene("nucleon")
    with GpuScene(s) as g:
        for filter_mode in (0, 1):
            r = shade_ref.ref("nucleon", filter_mode)
            for kernel in ("dda", "reforder"):
                what = "nucleon %s filter %d" % (kernel, filter_mode)
                fb, n, k = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert b"<%s,true,false,%d," % (b"true" if kernel == "dda" else b"false", 11 if filter_mode else 10) in k, k
                shade_ref.check(s, fb, r, what)
                _identities(g, what, kernel=KERNELS[kernel], filter_mode=filter_mode)


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3 * scenes.FUZZ_SCALE))
def test_identities_on_fuzzed_views_and_volumes(seed):
    rng = np.random.default_rng(7100 + seed)
    dtype = str(rng.choice(["u8", "u16"]))
    kw = dict(voxels=tuple(int(v) for v in rng.choice([32, 48, 64], 3)), block=int(rng.choice([16, 32])),
              viewport=(int(rng.integers(17, 60)), int(rng.integers(17, 60))), spr=int(rng.choice([64, 97, 128, 200])),
              volume="hash", spin=(float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.5, 1.5))),
              alpha=float(rng.choice([0.05, 0.3, 1.0])))
    if rng.random() < 0.3:
        kw["eye"] = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.1, 0.9)))
    s = orc.build_scene(dtype=dtype, **kw)
    with GpuScene(s) as g:
        for kernel in ("dda", "reforder"):
            for filter_mode in (0, 1):
                for stepping in (1, 0):
                    plain, lit = _identities(g, "seed %d %r %s filter %d stepping %d" % (seed, kw, kernel, filter_mode, stepping),
                                             kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=stepping)
                    assert not np.array_equal(plain[0], lit[0])


def test_identities_in_an_atlas_of_more_than_2_pow_32_voxels():
    """(the pool of tests/test_gpu_parity.py::test_atlas_of_more_than_2_pow_32_voxels: bricks on both sides of the line;
    the BIG instances, whose slot base moves into the lane's pointer)"""
    from test_gpu_parity import _frames_in_a_large_pool
    s = scenes.get("hash64_spin")
    for flt in (0, 1):
        for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
            base = {vrc.OPT_FILTER: flt, vrc.OPT_KERNEL: kernel}
            with GpuScene(s) as g:
                small = _frame(g, 1, kernel=kernel, filter_mode=flt, stepping=0)  # (8-bit voxels of such an atlas step in float)
            plain, lit, one = _frames_in_a_large_pool(
                vrc, s, 6 * 1000 ** 3, 2 ** 32,
                [({**base, vrc.OPT_SHADING: 0}, None),
                 ({**base, vrc.OPT_SHADING: 1, vrc.OPT_SHADING_AMBIENT: K1000}, None),
                 ({**base, vrc.OPT_SHADING: 1, vrc.OPT_SHADING_AMBIENT: 1000}, None)])
            assert lit[3].startswith("vrc_k_raycast_shade<") and lit[3].endswith(",true>"), lit[3]
            assert np.array_equal(plain[0][..., 3], lit[0][..., 3]) and plain[1] == lit[1] == one[1] > 0
            assert np.array_equal(plain[0], one[0])
            assert np.array_equal(lit[0], small[0]) and lit[1] == small[1], "the frame of the small pool"


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16", "axis"])
def test_uniform_bricks(name, filter_mode):
    s = shade_ref.scene(name)
    with GpuScene(s) as g:
        for kernel in ("dda", "reforder"):
            out = {}
            for uniform in (0, 1):
                _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)
                out[uniform] = _identities(g, "%s %s uniform %d" % (name, kernel, uniform), kernel=KERNELS[kernel],
                                           filter_mode=filter_mode)
            assert np.array_equal(out[0][1][0], out[1][1][0]) and out[0][1][1] == out[1][1][1]
            if name == "axis":  # mem://: every brick is one value: the unshaded frame, for any ambient
                for uniform in (0, 1):
                    _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)
                    assert np.array_equal(out[uniform][0][0], _frame(g, 1, 100, kernel=KERNELS[kernel], filter_mode=filter_mode)[0])
            else:
                shade_ref.check(s, out[1][1][0], shade_ref.ref(name, filter_mode), "%s %s filter %d" % (name, kernel, filter_mode))


@pytest.mark.parametrize("name", ["spin", "skip"])
def test_three_passes_equal_one(name):
    s = shade_ref.scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    with GpuScene(s) as g:
        asked = 0
        for filter_mode in (0, 1):
            kw = dict(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode)
            p1, p3 = _frame(g, 0, **kw), _frame(g, 0, passes=parts, **kw)
            assert np.array_equal(p1[0], p3[0]) and p1[1] == p3[1], "the precondition: the unshaded passes equal one pass"
            l1, l3 = _frame(g, 1, **kw), _frame(g, 1, passes=parts, **kw)
            assert np.array_equal(l1[0], l3[0]) and l1[1] == l3[1], filter_mode
            asked += 1
        assert asked == 2


def test_row_map_and_caller_owned_framebuffer():
    s = shade_ref.scene("spin")
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
        assert np.array_equal(full[0][rows], band[0])
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            g.render()
            assert np.array_equal(ext.cpu().numpy(), full[0])
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


def test_non_finite_float_voxels():
    """The all-NaN brick of tests/nonfinite.py: alpha is the unshaded frame's bit for bit, and rgb is finite wherever the
    unshaded frame's is."""
    t = nonfinite.case("allnan_brick").mt
    with voxel_types.typed_gpu_scene(t) as g:
        for filter_mode in (0, 1):
            for kernel in ("dda", "reforder"):
                plain = _frame(g, 0, kernel=KERNELS[kernel], filter_mode=filter_mode)
                lit = _frame(g, 1, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert np.array_equal(plain[0][..., 3], lit[0][..., 3], equal_nan=True) and plain[1] == lit[1]
                ok = np.isfinite(plain[0][..., :3]).all(axis=-1)
                assert ok.sum() > 100 and np.isfinite(lit[0][..., :3][ok]).all()


# ---- what is refused, and what does not change -----------------------------------------------------------------------------
def test_refusals_name_the_option_and_leave_the_context_usable():
    s = shade_ref.scene("spin")
    with GpuScene(s) as g:
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        assert _get(g, vrc.OPT_SHADING) == 0 and _get(g, vrc.OPT_SHADING_AMBIENT) == 250
        for option, bad, name in ((vrc.OPT_SHADING, 2, b"VRC_OPT_SHADING"), (vrc.OPT_SHADING, -1, b"VRC_OPT_SHADING"),
                                  (vrc.OPT_SHADING_AMBIENT, 1001, b"VRC_OPT_SHADING_AMBIENT"),
                                  (vrc.OPT_SHADING_AMBIENT, -1, b"VRC_OPT_SHADING_AMBIENT")):
            assert L.vrc_set_option(g.ctx, option, bad) == vrc.VRC_EINVAL and name in L.vrc_last_error()
        assert _get(g, vrc.OPT_SHADING) == 0 and _get(g, vrc.OPT_SHADING_AMBIENT) == 250
        good = _frame(g, 1)
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            with pytest.raises(vrc.VrcError) as e:
                g.render(kernel=kernel, filter_mode=1)
            assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_KERNEL" in str(e.value) and "VRC_OPT_SHADING" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(variant=1)
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_VARIANT" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(ray_lod=(1.0, 0.01))
        assert e.value.code == vrc.VRC_EINVAL and "vrc_set_ray_lod" in str(e.value)
        again = _frame(g, 1)
        assert np.array_equal(good[0], again[0]) and good[1] == again[1]
        # neither option may change inside a frame
        for change, name, back in ((lambda: _opt(g, vrc.OPT_SHADING, 0), b"VRC_OPT_SHADING", lambda: _opt(g, vrc.OPT_SHADING, 1)),
                                   (lambda: _opt(g, vrc.OPT_SHADING_AMBIENT, 500), b"VRC_OPT_SHADING_AMBIENT",
                                    lambda: _opt(g, vrc.OPT_SHADING_AMBIENT, K1000))):
            vrc.check(L, L.vrc_pre_render(g.ctx, view))
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            change()
            assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
            assert name in L.vrc_last_error()
            back()
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
            vrc.check(L, L.vrc_post_render(g.ctx, None))
        again = _frame(g, 1)
        assert np.array_equal(good[0], again[0])
        # MIP and isosurface frames do not read the option: the LDS refusal above is not theirs to give, and their frames
        # are those of a context that never set it
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        mip_lit = g.render()[0]
        _opt(g, vrc.OPT_SHADING, 0)
        assert np.array_equal(mip_lit, g.render()[0])


def test_depth_split_compaction_grey_table_are_the_plain_shaded_kernel():
    s = copy.copy(shade_ref.scene("inside"))
    with GpuScene(s) as g:
        want = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
        for option, value in ((vrc.OPT_DEPTH_SPLIT, 1), (vrc.OPT_ERT_COMPACTION, 4), (vrc.OPT_GREY_TABLE, 1)):
            _opt(g, option, value)
            got = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
            assert got[2] == want[2] and np.array_equal(got[0], want[0]) and got[1] == want[1], option
            _opt(g, option, 0)


def test_nothing_else_changes():
    """With the option at 0, composite, MIP and isosurface frames are launched by the kernel instances of the same names and
    are bit for bit what they were before a shaded frame was rendered on the context."""
    s = shade_ref.scene("spin")

    def others(g):
        out = []
        _shading(g, 0)
        for filter_mode in (0, 1):
            for kernel in sorted(KERNELS):
                _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
                fb, n, _ = g.render(kernel=KERNELS[kernel], filter_mode=filter_mode)
                out.append((fb, n, g.L.vrc_last_kernel()))
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
            fb, n, _ = g.render(filter_mode=filter_mode)
            out.append((fb, n, g.L.vrc_last_kernel()))
            vrc.set_isosurface(g.L, g.ctx, 150.0, 0.25)
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
            fb, n, _ = g.render(filter_mode=filter_mode)
            out.append((fb, n, g.L.vrc_last_kernel()))
            _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        return out

    with GpuScene(s) as g:
        before = others(g)
        names = [o[2] for o in before]
        assert all(b"shade" not in k for k in names)
        # the instances of today: the composite gather kernel for point samples (AUTO's trilinear frame is the tap-packed
        # mode 5 of the same kernel), the MIP kernel with the maximum (7 / 8) and the first-crossing fold (55 / 56)
        assert all(k.startswith(b"vrc_k_raycast<") for k in names[0:3] + names[5:8]), names
        assert b",0,unsigned char," in names[1] and b",1,unsigned char," in names[5 + 1] and b",5,unsigned int," in names[5], names
        assert names[3].startswith(b"vrc_k_raycast_mip<") and b",7," in names[3] and b",55," in names[4], names
        assert b",8," in names[5 + 3] and b",56," in names[5 + 4], names
        _frame(g, 1)
        _frame(g, 1, filter_mode=1)
        after = others(g)
        assert len(before) == len(after)
        for a, b in zip(before, after):
            assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]), a[2]


def test_the_walk_cache_is_undisturbed():
    """Unshaded frames reach the replay; a shaded frame reads 0 in VRC_OPT_WALK_CACHE_USED and allocates nothing; the
    unshaded frames after it are bit for bit the earlier ones, walked or replayed."""
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(100, 76), spin=(0.5, 0.35), spr=256)
    with GpuScene(s) as g:
        _opt(g, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS)
        _shading(g, 0)
        modes, frames = [], []
        for _ in range(6):
            fb, n, _st = g.render(kernel=vrc.KERNEL_GRID_DDA)
            modes.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            frames.append((fb, n))
        assert modes[-1] == 4 and b"vrc_k_raycast_replay<" in g.L.vrc_last_kernel(), modes
        assert all(np.array_equal(frames[0][0], f[0]) and frames[0][1] == f[1] for f in frames)
        held = _get(g, vrc.OPT_WALK_CACHE_BYTES)
        lit = _frame(g, 1, kernel=vrc.KERNEL_GRID_DDA)
        assert _get(g, vrc.OPT_WALK_CACHE_USED) == 0 and lit[2].startswith(b"vrc_k_raycast_shade<"), lit[2]
        assert _get(g, vrc.OPT_WALK_CACHE_BYTES) == held, "a shaded frame allocates no lists"
        assert lit[1] == frames[0][1] and np.array_equal(lit[0][..., 3], frames[0][0][..., 3])
        _shading(g, 0)
        seen = []
        for _ in range(5):
            fb, n, _st = g.render(kernel=vrc.KERNEL_GRID_DDA)
            seen.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            assert np.array_equal(fb, frames[0][0]) and n == frames[0][1], seen
        assert seen[-1] == 4, seen  # idle after the shaded frame, recorded again, never stale
