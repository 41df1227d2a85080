"""The depth of a composite frame (VRC_OPT_COMPOSITE_DEPTH) through the C ABI on the GPU: held to the float64 reference of
tests/cdepth_ref.py by its acceptance rule, and to the frame of the same context with the option at 0 by the bitwise
identities of the contract (include/vrc_hip.h, "The depth of a composite frame").  tests/test_cdepth_cpu.py checks the rule,
its caps and the host build on the CPU.  Every test here fails on a library without the option: vrc_set_option refuses 31."""
import ctypes as C
import types

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import cdepth_ref
import depth_ref
import mip_scenes
import orc
import scenes
import voxel_types
from cdepth_ref import tau_of
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

KERNELS = {"auto": vrc.KERNEL_AUTO, "reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
CDEPTH = b"vrc_k_raycast_cdepth<"


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _get(g, option):
    v = C.c_int64(-1)
    vrc.check(g.L, g.L.vrc_get_option(g.ctx, option, C.byref(v)))
    return int(v.value)


def _values(L, ctx, w, h):
    v = np.full((h, w), np.nan, dtype=np.float32)
    c = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(L, L.vrc_get_projection_values(ctx, v.ctypes.data, c.ctypes.data))
    return v, c


def _frame(g, k, h=None, **kw):
    """(frame, samples, kernel name, values, counts, depths, xyz) of one frame with the option at k; the read-backs only
    where k > 0"""
    _opt(g, vrc.OPT_COMPOSITE_DEPTH, k)
    fb, n, _ = g.render(**kw)
    name = g.L.vrc_last_kernel()
    if not k:
        return fb, n, name
    h = g.s.H if h is None else h
    return (fb, n, name) + _values(g.L, g.ctx, g.s.W, h) + vrc.projection_depths(g.L, g.ctx, g.s.W, h)


def _pair_identities(fb, k, c, d, what):
    """isfinite(D) <=> alpha >= tau, and count = isfinite(D)"""
    assert np.array_equal(np.isfinite(d), fb[..., 3] >= tau_of(k)), "%s: isfinite(D) <=> alpha >= tau %d" % (what, k)
    assert np.isposinf(d[~np.isfinite(d)]).all() and np.array_equal(c, np.isfinite(d).astype(np.uint32)), what


_RAYS = {}


def _rays32(s):
    """the float32 rays of the host build, computed once per scene and left unchanged"""
    if id(s) not in _RAYS:
        _RAYS[id(s)] = (s, depth_ref.rays32(s))  # (the scene is kept: its id stays its own)
    return _RAYS[id(s)][1]


def _xyz(s, d, xyz, what):
    """xyz = origin + D x dir, to the depth tests' tolerance, against the float32 rays of the host build"""
    fin = np.isfinite(d)
    want = depth_ref.xyz32(d, _rays32(s))
    if fin.any():
        assert np.abs(xyz[fin].astype(np.float64) - want[fin]).max() <= 1e-5, what


def _identities(g, what, taus=cdepth_ref.IDENTITY_TAUS, rays=None, **kw):
    """every identity against the option-0 frame of the same context; returns {k: frame tuple}"""
    plain = _frame(g, 0, **kw)
    assert CDEPTH not in plain[2], (what, plain[2])
    out = {}
    for k in taus:
        on = out[k] = _frame(g, k, **kw)
        assert on[2].startswith(CDEPTH), (what, on[2])
        assert np.array_equal(plain[0], on[0]) and plain[1] == on[1] and plain[1] > 0, "%s tau %d: frame and count" % (what, k)
        _pair_identities(on[0], k, on[4], on[5], what)
        _xyz(rays if rays is not None else g.s, on[5], on[6], what)
    _opt(g, vrc.OPT_COMPOSITE_DEPTH, 0)
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name,filter_mode,k", cdepth_ref.rule_cases(),
                         ids=["%s-%s-%d" % (n, "trilinear" if f else "nearest", k) for n, f, k in cdepth_ref.rule_cases()])
def test_every_served_form_passes_the_rule(name, filter_mode, k, kernel):
    s, r = cdepth_ref.scene(name), cdepth_ref.ref(name, filter_mode, k)
    tol = cdepth_ref.tolerance(s, filter_mode)
    with GpuScene(s) as g:
        for stepping in (1, 0):
            what = "%s %s filter %d tau %d stepping %d" % (name, kernel, filter_mode, k, stepping)
            fb, n, kn, v, c, d, xyz = _frame(g, k, kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=stepping)
            assert kn.startswith(CDEPTH) and (b",%d," % (13 if filter_mode else 12)) in kn, kn
            cdepth_ref.assert_rule(r, v, c, d, what, tol=tol)
            _pair_identities(fb, k, c, d, what)
            fin = np.isfinite(d)
            want = _vec3(s) + d[fin][:, None].astype(np.float64) * r.dir[fin]
            assert np.abs(xyz[fin] - want).max() <= 1e-5, what


def _vec3(s):
    return np.array([float(s.view.eyePosition[a]) for a in range(3)])


def _to_q(image):
    if image == "uint16":
        return lambda x: x
    im = voxel_types.IMAGES[image]
    return lambda x: (x - im.a) / im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_voxel_types(image, filter_mode):
    """uint16, int16 and float pools: the crossing does not move under the affine image v = a + b q (b > 0) of the volume
    with its range, so the reference of the q scene is the typed volume's, whose V comes back in its own units."""
    q, t, _ = mip_scenes.typed(image)
    exact = not filter_mode and image != "float"
    tol = 0.0 if exact else scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    with (GpuScene(t) if image == "uint16" else voxel_types.typed_gpu_scene(t)) as g:
        for kernel in ("dda", "reforder"):
            for k in cdepth_ref.RULE_TAUS:
                what = "%s %s filter %d tau %d" % (image, kernel, filter_mode, k)
                r = cdepth_ref.typed_ref(image, filter_mode, k)
                fb, n, kn, v, c, d, xyz = _frame(g, k, kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert kn.startswith(CDEPTH) and (b"float" if image == "float" else b"unsigned short") in kn, kn
                cdepth_ref.assert_rule(r, _to_q(image)(v.astype(np.float64)), c, d, what, tol=tol)
                if image == "int16":
                    assert v[c > 0].min() < 0.0, "V comes back un-shifted: the signed volume's own values"
            _identities(g, "%s %s filter %d" % (image, kernel, filter_mode), rays=q, kernel=KERNELS[kernel],
                        filter_mode=filter_mode)


def test_the_clamped_sampler():
    """A brick without overlap (the nucleon fixture) takes the clamped sampler: trilinear under the rule, point samples
    under the identities (the rule's windows are too wide there: tests/cdepth_ref.py)."""
    s = cdepth_ref.scene("nucleon")
    with GpuScene(s) as g:
        for kernel in ("dda", "reforder"):
            for k in cdepth_ref.RULE_TAUS:
                r = cdepth_ref.ref("nucleon", 1, k)
                fb, n, kn, v, c, d, xyz = _frame(g, k, kernel=KERNELS[kernel], filter_mode=1)
                assert b"<%s,true,false,13," % (b"true" if kernel == "dda" else b"false") in kn, kn
                cdepth_ref.assert_rule(r, v, c, d, "nucleon %s trilinear tau %d" % (kernel, k), tol=cdepth_ref.tolerance(s, 1))
            for filter_mode in (0, 1):
                out = _identities(g, "nucleon %s filter %d" % (kernel, filter_mode), kernel=KERNELS[kernel], filter_mode=filter_mode)
                assert b",true,false,%d," % (13 if filter_mode else 12) in out[500][2]


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", cdepth_ref.RULE_SCENES)
def test_identities_on_the_rule_scenes(name, filter_mode):
    with GpuScene(cdepth_ref.scene(name)) as g:
        for kernel in sorted(KERNELS):
            if kernel == "auto" and filter_mode:
                continue  # (AUTO's trilinear frame with the option at 0 is the staged / packed form's)
            for stepping in (1, 0):
                _identities(g, "%s %s filter %d stepping %d" % (name, kernel, filter_mode, stepping), kernel=KERNELS[kernel],
                            filter_mode=filter_mode, stepping=stepping)


@pytest.mark.parametrize("seed", range(3 * scenes.FUZZ_SCALE))
def test_identities_on_fuzzed_views_and_volumes(seed):
    rng = np.random.default_rng(7200 + seed)
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
                    _identities(g, "seed %d %r %s filter %d stepping %d" % (seed, kw, kernel, filter_mode, stepping),
                                kernel=KERNELS[kernel], filter_mode=filter_mode, stepping=stepping)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16", "axis"])
def test_uniform_bricks_change_no_bit(name, filter_mode):
    """(axis: a mem:// volume, every brick one value; skip / skip16: constant bricks among others)"""
    s = cdepth_ref.scene(name)
    with GpuScene(s) as g:
        for kernel in ("dda", "reforder"):
            out = {}
            for uniform in (0, 1):
                _opt(g, vrc.OPT_UNIFORM_BRICKS, uniform)
                out[uniform] = _identities(g, "%s %s uniform %d" % (name, kernel, uniform), kernel=KERNELS[kernel],
                                           filter_mode=filter_mode)
            for k in cdepth_ref.IDENTITY_TAUS:
                a, b = out[0][k], out[1][k]
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b) if isinstance(x, np.ndarray)) and a[1] == b[1], (kernel, k)


# ---- passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_passes(parts, filter_mode):
    """A node list in two and three passes by the reference-order loop: the rule against cdepth_ref rendered in the same
    passes, the equivalence after every pass, and no finite D changed by a later pass."""
    s, k = cdepth_ref.scene("spin"), 100
    n = s.n_nodes
    cuts = [(i * n // parts, (i + 1) * n // parts) for i in range(parts)]
    refs = cdepth_ref.render_passes(s, tau_of(k), cuts, filter_mode=filter_mode)
    tol = cdepth_ref.tolerance(s, filter_mode)
    with GpuScene(s) as g:
        L = g.L
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, k)
        g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=filter_mode)  # (sets every other option and the table)
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        vrc.check(L, L.vrc_pre_render(g.ctx, view))
        assert L.vrc_get_projection_depths(g.ctx, np.zeros((s.H, s.W), dtype=np.float32).ctypes.data, None) == vrc.VRC_EINVAL
        before = None
        for i, (a, b) in enumerate(cuts):
            sub = C.cast(C.byref(s.nodes, a * C.sizeof(vrc.NodeData)), C.POINTER(vrc.NodeData))
            vrc.check(L, L.vrc_render(g.ctx, view, sub, b - a, render, g.pool))
            assert L.vrc_last_kernel().startswith(CDEPTH)
            fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
            vrc.check(L, L.vrc_post_render(g.ctx, fb.ctypes.data))
            v, c = _values(L, g.ctx, s.W, s.H)
            d, xyz = vrc.projection_depths(L, g.ctx, s.W, s.H)
            what = "spin filter %d, pass %d of %d" % (filter_mode, i + 1, parts)
            _pair_identities(fb, k, c, d, what)
            cdepth_ref.assert_rule(refs[i], v, c, d, what, tol=tol)
            if before is not None:
                kept = np.isfinite(before[0])
                assert np.array_equal(before[0][kept], d[kept]) and np.array_equal(before[1][kept], v[kept]), what
            before = (d, v)
        assert np.isfinite(before[0]).sum() > 300


def test_row_map_and_caller_owned_framebuffer():
    s, k = cdepth_ref.scene("spin"), 500
    r = cdepth_ref.ref("spin", 0, k)
    with GpuScene(s) as g:
        full = _frame(g, k)
        cdepth_ref.assert_rule(r, full[3], full[4], full[5], "spin auto tau %d" % k)
        rows = np.array([3, 4, 5, 17, 18, 30, 35], dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        saved = g.s.H
        try:
            g.s.H = len(rows)  # the buffer GpuScene reads back
            band = _frame(g, k, h=len(rows))
        finally:
            g.s.H = saved
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        for a, b in zip(full, band):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a[rows], b, equal_nan=True), "a band's rows are the frame's"
        ext = torch.full((s.H, s.W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            mine = _frame(g, k)
            assert np.array_equal(ext.cpu().numpy(), full[0])
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(full[3:], mine[3:]))
            _pair_identities(ext.cpu().numpy(), k, mine[4], mine[5], "caller-owned frame buffer")
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


def test_identities_in_an_atlas_of_more_than_2_pow_32_voxels():
    """(the pool of tests/test_gpu_parity.py::test_atlas_of_more_than_2_pow_32_voxels: bricks on both sides of the line; the
    BIG instances, whose slot base moves into the lane's pointer.  The helper gives frames only, so the library handed
    to it reads the pair back where the frame is read back)"""
    from test_gpu_parity import _frames_in_a_large_pool
    s = scenes.get("hash64_spin")
    real = vrc.load_library()
    for flt in (0, 1):
        for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
            taps = []

            class Tap:
                def __getattr__(self, name):
                    return getattr(real, name)

                def vrc_post_render(self, ctx, fb):
                    rc = real.vrc_post_render(ctx, fb)
                    on = C.c_int64(0)
                    real.vrc_get_option(ctx, vrc.OPT_COMPOSITE_DEPTH, C.byref(on))
                    if rc == 0 and on.value:
                        taps.append(_values(real, ctx, s.W, s.H) + vrc.projection_depths(real, ctx, s.W, s.H))
                    return rc

            proxy = types.SimpleNamespace(**{n: getattr(vrc, n) for n in dir(vrc) if not n.startswith("__")})
            proxy.load_library = lambda: Tap()
            base = {vrc.OPT_FILTER: flt, vrc.OPT_KERNEL: kernel}
            with GpuScene(s) as g:
                small = _frame(g, 500, kernel=kernel, filter_mode=flt, stepping=0)  # (8-bit voxels of such an atlas step in float)
            cases = [({**base, vrc.OPT_COMPOSITE_DEPTH: k}, None) for k in (0,) + cdepth_ref.IDENTITY_TAUS]
            got = _frames_in_a_large_pool(proxy, s, 6 * 1000 ** 3, 2 ** 32, cases)
            plain = got[0]
            assert "cdepth" not in plain[3] and len(taps) == len(cdepth_ref.IDENTITY_TAUS)
            for k, on, (v, c, d, xyz) in zip(cdepth_ref.IDENTITY_TAUS, got[1:], taps):
                assert on[3].startswith("vrc_k_raycast_cdepth<") and on[3].endswith(",true>"), on[3]
                assert np.array_equal(plain[0], on[0]) and plain[1] == on[1] > 0
                _pair_identities(on[0], k, c, d, "large pool filter %d tau %d" % (flt, k))
                _xyz(s, d, xyz, "large pool")
                if k == 500:
                    assert np.array_equal(on[0], small[0]) and on[1] == small[1], "the frame of the small pool"
                    assert np.array_equal(v, small[3]) and np.array_equal(d, small[5]), "the pair of the small pool"


# ---- what is refused, and what does not change -----------------------------------------------------------------------------
def test_refusals_and_state():
    s = cdepth_ref.scene("spin")
    with GpuScene(s) as g:
        L = g.L
        view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
        render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
        nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
        t = np.zeros((s.H, s.W), dtype=np.float32)
        cnt = np.zeros((s.H, s.W), dtype=np.uint32)

        def refused():
            a = L.vrc_get_projection_depths(g.ctx, t.ctypes.data, None) == vrc.VRC_EINVAL
            msg = L.vrc_last_error()
            b = L.vrc_get_projection_values(g.ctx, t.ctypes.data, cnt.ctypes.data) == vrc.VRC_EINVAL
            return a and b and b"VRC_OPT_PROJECTION = MIP" in msg and b"VRC_OPT_PROJECTION = MIP" in L.vrc_last_error()

        assert _get(g, vrc.OPT_COMPOSITE_DEPTH) == 0
        for bad in (1000, -1):
            assert L.vrc_set_option(g.ctx, vrc.OPT_COMPOSITE_DEPTH, bad) == vrc.VRC_EINVAL
            assert b"VRC_OPT_COMPOSITE_DEPTH" in L.vrc_last_error()
        assert _get(g, vrc.OPT_COMPOSITE_DEPTH) == 0
        # with the option at 0 a composite frame refuses both read-backs, as before
        plain = _frame(g, 0)
        assert refused()
        good = _frame(g, 500)
        assert _get(g, vrc.OPT_COMPOSITE_DEPTH) == 500
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            with pytest.raises(vrc.VrcError) as e:
                g.render(kernel=kernel, filter_mode=1)
            assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_KERNEL" in str(e.value) and "VRC_OPT_COMPOSITE_DEPTH" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(variant=1)
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_VARIANT" in str(e.value) and "VRC_OPT_COMPOSITE_DEPTH" in str(e.value)
        with pytest.raises(vrc.VrcError) as e:
            g.render(ray_lod=(1.0, 0.01))
        assert e.value.code == vrc.VRC_EINVAL and "vrc_set_ray_lod" in str(e.value) and "VRC_OPT_COMPOSITE_DEPTH" in str(e.value)
        _opt(g, vrc.OPT_SHADING, 1)
        with pytest.raises(vrc.VrcError) as e:
            g.render()
        assert e.value.code == vrc.VRC_EINVAL and "VRC_OPT_SHADING" in str(e.value) and "VRC_OPT_COMPOSITE_DEPTH" in str(e.value)
        _opt(g, vrc.OPT_SHADING, 0)
        again = _frame(g, 500)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(good, again) if isinstance(a, np.ndarray)) and good[1] == again[1]
        # the option may not change inside a frame; the read-backs exist from the first pass to the next vrc_pre_render
        vrc.check(L, L.vrc_pre_render(g.ctx, view))
        assert refused(), "before the frame's first pass"
        vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
        vrc.check(L, L.vrc_get_projection_depths(g.ctx, t.ctypes.data, None))
        assert np.array_equal(t, good[5])
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, 100)
        assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
        assert b"VRC_OPT_COMPOSITE_DEPTH" in L.vrc_last_error()
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, 0)
        assert L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool) == vrc.VRC_EINVAL
        assert b"VRC_OPT_COMPOSITE_DEPTH" in L.vrc_last_error()
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, 500)
        vrc.check(L, L.vrc_post_render(g.ctx, None))
        vrc.check(L, L.vrc_get_projection_depths(g.ctx, t.ctypes.data, None))
        vrc.check(L, L.vrc_pre_render(g.ctx, view))
        assert refused(), "after the next vrc_pre_render"
        vrc.check(L, L.vrc_post_render(g.ctx, None))
        # MIP frames do not read the option
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        mip_on = g.render()[0]
        assert b"cdepth" not in L.vrc_last_kernel()
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, 0)
        assert np.array_equal(mip_on, g.render()[0])
        _opt(g, vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
        assert np.array_equal(_frame(g, 0)[0], plain[0])


def test_depth_split_compaction_grey_table_are_the_plain_depth_kernel():
    s = cdepth_ref.scene("inside")
    with GpuScene(s) as g:
        want = _frame(g, 500, kernel=vrc.KERNEL_GRID_DDA)
        for option, value in ((vrc.OPT_DEPTH_SPLIT, 1), (vrc.OPT_ERT_COMPACTION, 4), (vrc.OPT_GREY_TABLE, 1)):
            _opt(g, option, value)
            got = _frame(g, 500, kernel=vrc.KERNEL_GRID_DDA)
            assert got[2] == want[2] and got[1] == want[1], option
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got) if isinstance(a, np.ndarray)), option
            _opt(g, option, 0)


def test_the_walk_cache_is_undisturbed():
    """Plain frames reach the replay; a depth frame reads 0 in VRC_OPT_WALK_CACHE_USED and allocates nothing; the plain
    frames after it are bit for bit the earlier ones, and an unshaded still view replays again."""
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(100, 76), spin=(0.5, 0.35), spr=256)
    with GpuScene(s) as g:
        _opt(g, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS)
        modes, frames = [], []
        for _ in range(6):
            fb, n, _st = g.render(kernel=vrc.KERNEL_GRID_DDA)
            modes.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            frames.append((fb, n))
        assert modes[-1] == 4 and b"vrc_k_raycast_replay<" in g.L.vrc_last_kernel(), modes
        held = _get(g, vrc.OPT_WALK_CACHE_BYTES)
        on = _frame(g, 500, kernel=vrc.KERNEL_GRID_DDA)
        assert _get(g, vrc.OPT_WALK_CACHE_USED) == 0 and on[2].startswith(CDEPTH), on[2]
        assert _get(g, vrc.OPT_WALK_CACHE_BYTES) == held, "a depth frame allocates no lists"
        assert on[1] == frames[0][1] and np.array_equal(on[0], frames[0][0])
        _pair_identities(on[0], 500, on[4], on[5], "still view")
        _opt(g, vrc.OPT_COMPOSITE_DEPTH, 0)
        seen = []
        for _ in range(5):
            fb, n, _st = g.render(kernel=vrc.KERNEL_GRID_DDA)
            seen.append(_get(g, vrc.OPT_WALK_CACHE_USED))
            assert np.array_equal(fb, frames[0][0]) and n == frames[0][1], seen
        assert seen[-1] == 4, seen  # idle after the depth frame, recorded again, never stale
