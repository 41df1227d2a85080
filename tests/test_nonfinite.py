"""Float atlases with NaN and infinite voxels on the GPU through the C ABI: what include/vrc_hip.h promises of them --
the classification of a density that is not a number, the MIP maximum that drops NaN samples, the per-slot word the MIP
march skips bricks by, the upload's padding -- on the scenes of tests/nonfinite.py, which says why the uint16 scene with
its markers left as numbers is the reference.  Composite frames are held to tests/ref64.py by test_ref64_cpu.check, MIP
frames to tests/mip_ref.py by its check_frame; tests/test_nonfinite_cpu.py checks the scenes, the caps and the teeth of
these comparisons on the CPU."""
import ctypes as C

import numpy as np
import pytest

import mip_ref
import nonfinite as nf
import scenes
import voxel_types as vt
from libre_amd import vrc
from test_mip import _check, _count_ok, _mip, _opt
from test_ref64_cpu import check
from test_uniform_bricks import _reupload

pytestmark = pytest.mark.gpu

KERNELS = [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA]


# ---- composite ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.NAMES)
def test_composite_matches_ref64(name):
    c = nf.case(name)
    r = nf.ref(name)
    with vt.typed_gpu_scene(c.t) as g:
        for kernel in KERNELS + [vrc.KERNEL_AUTO]:
            for stepping in (1, 0):
                for grey in (1, 0):
                    _opt(g, vrc.OPT_GREY_TABLE, grey)
                    got, n, st = g.render(kernel=kernel, stepping=stepping)
                    assert b"float" in g.L.vrc_last_kernel()
                    assert np.isfinite(got).all()
                    check(c.q, got, n, r, name, "gpu kernel %d, stepping %d, grey %d" % (kernel, stepping, grey),
                          count=st.kernel_variant == vrc.KERNEL_GRID_DDA)
        _opt(g, vrc.OPT_GREY_TABLE, 1)
        if name in nf.TRILINEAR:
            r = nf.ref(name, 1)
            for kernel in KERNELS + [vrc.KERNEL_AUTO]:
                for stepping in (1, 0):
                    got, n, st = g.render(kernel=kernel, stepping=stepping, filter_mode=vrc.FILTER_TRILINEAR)
                    assert np.isfinite(got).all()
                    check(c.q, got, n, r, name + " trilinear", "gpu kernel %d, stepping %d" % (kernel, stepping),
                          count=st.kernel_variant == vrc.KERNEL_GRID_DDA)
    assert r.frame[..., 3].max() > 0.05


@pytest.mark.parametrize("name", nf.NAMES)
def test_nan_and_minus_infinity_render_as_the_range_minimum_bit_for_bit(name):
    """GPU against GPU, point samples: the float volume and the same volume with -1.0 (<= r0) in place of its NaN and
    -infinity voxels give the same frame and sample count -- composite and MIP."""
    c = nf.case(name)
    frames = []
    for t, mt in ((c.t, c.mt), (c.low, c.mlow)):  # mt: the same bricks under the transfer function of the MIP tests
        out = []
        with vt.typed_gpu_scene(t) as g:
            for kernel in KERNELS:
                for stepping in (1, 0):
                    g.s = t
                    _mip(g, on=False)
                    for grey in (1, 0):
                        _opt(g, vrc.OPT_GREY_TABLE, grey)
                        out.append(g.render(kernel=kernel, stepping=stepping)[:2])
                    g.s = mt
                    _mip(g, skip=0)
                    out.append(g.render(kernel=kernel, stepping=stepping)[:2])
        frames.append(out)
    for k, ((a, n_a), (b, n_b)) in enumerate(zip(*frames)):
        assert np.isfinite(a).all() and np.array_equal(a, b) and n_a == n_b, (name, k)
    assert frames[0][0][0][..., 3].max() > 0.05


# ---- MIP ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.NAMES)
def test_mip_matches_mip_ref_and_skipping_changes_no_pixel(name):
    c = nf.case(name)
    with vt.typed_gpu_scene(c.mt) as g:
        for f in (0, 1) if name in nf.TRILINEAR else (0,):
            r = nf.mref(name, f)
            for kernel in KERNELS:
                for stepping in (1, 0):
                    what = "%s mip kernel %d filter %d stepping %d" % (name, kernel, f, stepping)
                    _mip(g, skip=0)
                    fb, n, st = g.render(kernel=kernel, filter_mode=f, stepping=stepping)
                    assert st.kernel_variant == kernel and b"vrc_k_raycast_mip" in g.L.vrc_last_kernel()
                    assert np.isfinite(fb).all()
                    _check(c.mq, r, fb, what)
                    _count_ok(r, n, what)  # NaN voxels do not change S
                    _mip(g, skip=1)
                    fb1, n1, _ = g.render(kernel=kernel, filter_mode=f, stepping=stepping)
                    assert np.array_equal(fb, fb1) and n1 <= n, what
                    if name == "allnan_brick" and not f:
                        _all_nan_rays_show_the_first_texel(c, r, fb)


def _all_nan_rays_show_the_first_texel(c, r, fb):
    """A ray whose samples are all NaN has a sample set that is not empty and M = -infinity: the pixel is the
    classification of -infinity, the first texel premultiplied -- not the cleared value."""
    mask = nf.all_nan_rays(r)
    assert mask.sum() >= 50
    t0 = np.asarray(c.mq.tf, dtype=np.float64).reshape(256, 4)[0]
    want = np.array([t0[0] * t0[3], t0[1] * t0[3], t0[2] * t0[3], t0[3]])
    assert want[3] > 0.1
    assert not (fb[mask] == 0.0).all(axis=-1).any(), "left at the cleared value"
    assert (np.abs(fb[mask].astype(np.float64) - want).max(axis=-1) <= scenes.E0).all()


@pytest.mark.parametrize("kernel", KERNELS, ids=["reforder", "dda"])
def test_three_mip_passes_equal_one(kernel):
    """The running maximum between passes holds a float M that may be -infinity (a pass that met NaN voxels only)."""
    c = nf.case("speckle")
    passes = nf.passes3(c.mt)
    with vt.typed_gpu_scene(c.mt) as g:
        _mip(g, skip=0)
        one, n1, _ = g.render(kernel=kernel)
        three, n3, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=passes)
        assert np.array_equal(one, three) and n1 == n3
        _mip(g, skip=1)
        skipped, n3s, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, passes=passes)
        assert np.array_equal(one, skipped) and n3s <= n3
        _check(c.mq, nf.mref_passes("speckle"), three, "speckle in three passes")
        _check(c.mq, nf.mref("speckle"), three, "speckle in three passes against one")
    c = nf.case("allnan_brick")  # ... and here the first pass of many rays ends with M = -infinity
    with vt.typed_gpu_scene(c.mt) as g:
        _mip(g, skip=1)
        three, _, _ = g.render(kernel=kernel, passes=nf.passes3(c.mt))
        r3 = nf.mref_passes("allnan_brick")  # (its own reference: with a clip plane, where a pass ends a ray depends on its list)
        _check(c.mq, r3, three, "allnan_brick in three passes")
        _all_nan_rays_show_the_first_texel(c, r3, three)


# ---- the per-slot word --------------------------------------------------------------------------------------------------
def _on_off(g, L, what):
    """(frame, samples with skipping off, with skipping on), each held to mip_ref to the sample."""
    _mip(g, skip=0)
    fb, n, st = g.render(kernel=vrc.KERNEL_GRID_DDA)
    assert st.kernel_variant == vrc.KERNEL_GRID_DDA
    _check(L.twin, L.ref, fb, what)
    _mip(g, skip=1)
    fb1, n1, _ = g.render(kernel=vrc.KERNEL_GRID_DDA)
    print("%s: samples %d (mip_ref %d), with skipping %d (mip_ref: first bricks %d, front layer %d)" % (
        what, n, int(L.ref.counts.sum()), n1, L.first, int(L.ref_front.counts.sum())))
    assert np.array_equal(fb, fb1), what
    assert n == int(L.ref.counts.sum()), what
    return fb, n, n1


@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_every_ray_skips_every_brick_behind_the_front_layer(variant):
    """The word of a back brick comes from finite voxels below the front value mixed with NaNs of both signs.  A NaN
    that reached the atomicMax as its raw key, negative keys in the wrong order or a mishandled +infinity would let
    some ray march some back brick: the count with skipping on is nonfinite.Layers.first, to the sample."""
    L = nf.layers(variant)
    with vt.typed_gpu_scene(L.t) as g:
        _, _, n1 = _on_off(g, L, "layers %s" % variant)
        assert n1 == L.first


def test_the_word_follows_the_slot():
    """Release and upload again into the same slots, front and back contents swapped, and back -- once from host memory,
    once through vrc_pool_copy_to_slot_device: every frame and count is that of a fresh pool."""
    A, B = nf.layers("a"), nf.layers("swapped")
    with vt.typed_gpu_scene(B.t) as g:
        want_b = _on_off(g, B, "swapped, fresh")
    with vt.typed_gpu_scene(A.t) as g:
        want_a = _on_off(g, A, "a, fresh")
        assert want_a[2] == A.first and (want_a[0] != want_b[0]).any()
        for device in (False, True):
            _reupload(vrc, g, B.t, device)
            got = _on_off(g, B, "swapped over a, device %d" % device)
            assert np.array_equal(got[0], want_b[0]) and got[1:] == want_b[1:]
            _reupload(vrc, g, A.t, device)
            got = _on_off(g, A, "a over swapped, device %d" % device)
            assert np.array_equal(got[0], want_a[0]) and got[1:] == want_a[1:]


# ---- upload ---------------------------------------------------------------------------------------------------------------
def _special_floats(size, rng):
    """A float brick (z, y, x) with NaNs of both signs and a signalling payload, +-infinity, -0.0 and a denormal on its
    last plane along every axis and at its far corner."""
    brick = rng.standard_normal(size[::-1]).astype(np.float32)
    u = brick.view(np.uint32)
    special = np.concatenate([nf.NAN_BITS, [0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000400]]).astype(np.uint32)
    for sl in (np.s_[-1, :, :], np.s_[:, -1, :], np.s_[:, :, -1]):
        plane = u[sl]
        plane[...] = special[(np.arange(plane.size) % len(special)).reshape(plane.shape)]
    u[-1, -1, -1] = 0xFFA00001  # the far corner: a negative signalling NaN
    return brick


def _extremes(dt, size, rng):
    info = np.iinfo(dt)
    brick = rng.integers(info.min, info.max, size[::-1], dtype=dt, endpoint=True)
    edge = np.array([info.min, info.max, info.max - 1, info.min + 1, 0, info.max - 64, info.max - 65], dtype=dt)
    for sl in (np.s_[-1, :, :], np.s_[:, -1, :], np.s_[:, :, -1]):
        plane = brick[sl]
        plane[...] = edge[(np.arange(plane.size) % len(edge)).reshape(plane.shape)]
    brick[-1, -1, -1] = info.max
    return brick


@pytest.mark.parametrize("name", ["float", "int32", "uint32"])
def test_the_whole_slot_after_an_upload(name):
    """Bricks smaller than their slot go through the padding repack: the slot holds np.pad(brick, mode="edge"), bit for
    bit -- a NaN keeps its payload, -0.0 its sign, a denormal its value."""
    L = vrc.load_library()
    dt = np.dtype({"float": np.float32, "int32": np.int32, "uint32": np.uint32}[name])
    rng = np.random.default_rng(9)
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    try:
        vrc.check(L, L.vrc_pool_create_typed(ctx, vt.IMAGES[name].voxel_type, vrc.u32x3(24, 24, 24), 4 * 24 ** 3 * 4, C.byref(pool)))
        ad = vrc.u32x3()
        vrc.check(L, L.vrc_pool_info(pool, None, ad, None, vrc.u32x3(), None))
        for size in ((24, 24, 24), (18, 18, 18), (5, 18, 9)):
            brick = _special_floats(size, rng) if name == "float" else _extremes(dt, size, rng)
            slot = vrc.f32x3()
            vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(*size), slot))
            origin = [int(round(slot[a] * ad[a])) for a in range(3)]
            out = np.zeros((24, 24, 24), dtype=np.float32)
            vrc.check(L, L.vrc_pool_read_region(pool, vrc.u32x3(*origin), vrc.u32x3(24, 24, 24), out.ctypes.data))
            padded = np.pad(brick, [(0, 24 - size[2 - a]) for a in range(3)], mode="edge")
            want = padded if name == "float" else padded.astype(np.float32)  # round to nearest even, as NumPy converts
            assert want.dtype == np.float32 and want.shape == out.shape
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (name, size)
    finally:
        if pool:
            L.vrc_pool_destroy(pool)
        L.vrc_ctx_destroy(ctx)
