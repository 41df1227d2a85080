"""Signed, 32-bit and float voxels on the GPU through the C ABI (vrc_pool_create_typed, include/vrc_hip.h).

Frames are held to tests/ref64.py through affine images of uint16 / uint8 scenes (tests/voxel_types.py says why that
is exact) with test_ref64_cpu.check: scenes.assert_parity with ref64's own tie budget, no pixel left out, the grid
walk's sample count within 1e-4 n + 8 of ref64's.  The exact anchors are bit for bit."""
import ctypes as C

import numpy as np
import pytest

import nongrid
import orc
import ref64
import scenes
import voxel_types as vt
from test_ref64_cpu import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vrc():
    from libre_amd import vrc as v
    v.load_library()  # fails loudly when the HIP extension is missing
    return v


def _opt(vrc, g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


NP_TYPES = {"float": np.float32, "int32": np.int32, "uint32": np.uint32, "int16": np.int16, "int8": np.int8}


# ---- pool, upload, read back ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NP_TYPES))
def test_upload_and_read_region_round_trip(vrc, name):
    L = vrc.load_library()
    dt = np.dtype(NP_TYPES[name])
    voxel_type = vt.IMAGES[name].voxel_type
    rng = np.random.default_rng(7)
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    try:
        vrc.check(L, L.vrc_pool_create_typed(ctx, voxel_type, vrc.u32x3(18, 18, 18), 4 * 24 ** 3 * dt.itemsize, C.byref(pool)))
        got_type = C.c_int(-1)
        vrc.check(L, L.vrc_pool_voxel_type(pool, C.byref(got_type)))
        assert got_type.value == voxel_type
        sb = C.c_size_t()
        ad = vrc.u32x3()
        vrc.check(L, L.vrc_pool_info(pool, C.byref(sb), ad, None, vrc.u32x3(), None))
        assert sb.value == 24 ** 3 * dt.itemsize
        for size in ((18, 18, 18), (24, 24, 24), (5, 18, 9)):  # padded, whole-slot and ragged bricks
            if dt.kind == "f":
                brick = rng.standard_normal(size[::-1]).astype(np.float32)
                brick.flat[:4] = [np.inf, -np.inf, 0.0, -0.0]
            else:
                info = np.iinfo(dt)
                brick = rng.integers(info.min, info.max, size[::-1], dtype=dt, endpoint=True)
                brick.flat[:2] = [info.min, info.max]
            slot = vrc.f32x3()
            vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(*size), slot))
            origin = [int(round(slot[a] * ad[a])) for a in range(3)]
            out_dt = np.float32 if dt.itemsize == 4 else dt  # a 4-byte atlas holds float32
            out = np.zeros(size[::-1], dtype=out_dt)
            vrc.check(L, L.vrc_pool_read_region(pool, vrc.u32x3(*origin), vrc.u32x3(*size), out.ctypes.data))
            want = brick.astype(np.float32) if dt.itemsize == 4 else brick  # NumPy converts round-to-nearest-even
            assert (out.view(np.uint8) == want.view(np.uint8)).all(), (name, size)
            if size[0] < 24:  # the padding repeats the border voxel (clamp addressing baked in)
                edge = np.zeros((1, 1, 24 - size[0]), dtype=out_dt)
                vrc.check(L, L.vrc_pool_read_region(pool, vrc.u32x3(origin[0] + size[0], origin[1], origin[2]),
                                                    vrc.u32x3(24 - size[0], 1, 1), edge.ctypes.data))
                assert (edge.view(np.uint8).reshape(-1, out.itemsize) == want[0, 0, -1:].view(np.uint8)).all()
    finally:
        if pool:
            L.vrc_pool_destroy(pool)
        L.vrc_ctx_destroy(ctx)


# ---- every form that serves a type, against ref64 ------------------------------------------------------------------
def every_form(vrc, g, s, r_near, r_lin, what, staged):
    kernels = [vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA]
    names = {vrc.KERNEL_REFERENCE_ORDER: "reference order", vrc.KERNEL_GRID_DDA: "grid walk", vrc.KERNEL_LDS: "LDS",
             vrc.KERNEL_PACKED: "packed"}
    for uniform in ((1, 0) if staged else (1,)):
        _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, uniform)
        for kernel in kernels:
            for stepping in (1, 0):
                for grey in (1, 0):
                    _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                    got, n, st = g.render(kernel=kernel, stepping=stepping)
                    assert st.kernel_variant == kernel
                    check(s, got, n, r_near, what, "gpu %s, stepping %d, grey %d, uniform %d" % (names[kernel], stepping, grey, uniform),
                          count=kernel == vrc.KERNEL_GRID_DDA)
    _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
    _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, 1)
    got, n, st = g.render()  # AUTO: a grid-aligned list of one brick size goes to the grid walk
    assert st.kernel_variant == vrc.KERNEL_GRID_DDA
    check(s, got, n, r_near, what, "gpu AUTO")
    lin = list(kernels) + ([vrc.KERNEL_LDS, vrc.KERNEL_PACKED] if staged else [])
    if staged and s.atlas.dtype.itemsize == 1:
        got, n, st = g.render(kernel=vrc.KERNEL_LDS)
        assert st.kernel_variant == vrc.KERNEL_LDS
        check(s, got, n, r_near, what, "gpu LDS", count=False)
    for kernel in lin:
        for stepping in ((1, 0) if kernel in kernels else (1,)):
            got, n, st = g.render(kernel=kernel, filter_mode=vrc.FILTER_TRILINEAR, stepping=stepping)
            assert st.kernel_variant == kernel
            check(s, got, n, r_lin, what + " trilinear", "gpu %s, stepping %d" % (names[kernel], stepping),
                  count=kernel == vrc.KERNEL_GRID_DDA)
    got, n, st = g.render(filter_mode=vrc.FILTER_TRILINEAR)
    assert st.kernel_variant == (vrc.KERNEL_PACKED if staged else vrc.KERNEL_GRID_DDA)
    check(s, got, n, r_lin, what + " trilinear", "gpu AUTO", count=not staged)


@pytest.mark.parametrize("base", ["hash16", "smooth16", "hash32_clip"])
@pytest.mark.parametrize("image", sorted(vt.IMAGES))
def test_every_kernel_form_matches_ref64(vrc, base, image):
    im = vt.IMAGES[image]
    s, t, r = vt.ref(base, im)
    _, _, r_lin = vt.ref(base, im, filter_mode=1)
    with vt.typed_gpu_scene(t) as g:
        staged = image in ("int8", "int16") and min(s.vi.overlap[a] for a in range(3)) >= 1 and max(s.slot_dim) <= 248
        every_form(vrc, g, s, r, r_lin, "%s as %s" % (base, image), staged=staged)
        assert b"float" in g.L.vrc_last_kernel() or image in ("int8", "int16")


@pytest.mark.parametrize("image", sorted(vt.IMAGES))
def test_early_ray_termination_and_exact_tf_weight(vrc, image):
    im = vt.IMAGES[image]
    s, t, r = vt.ref("hash16_ert", im)
    with vt.typed_gpu_scene(t) as g:
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA):
            got, n, _ = g.render(kernel=kernel)
            check(s, got, n, r, "hash16_ert as %s" % image, "gpu kernel %d" % kernel, count=kernel == vrc.KERNEL_GRID_DDA)
    s, t, r = vt.ref("smooth16", im, frac_bits=0)
    with vt.typed_gpu_scene(t) as g:
        for stepping in (1, 0):
            got, n, _ = g.render(kernel=vrc.KERNEL_GRID_DDA, frac_bits=0, stepping=stepping)
            check(s, got, n, r, "smooth16 as %s exact weight" % image, "gpu grid walk, stepping %d" % stepping)


# ---- exact anchors ----------------------------------------------------------------------------------------------------
def _frames(vrc, g, linear_kernels):
    out = []
    for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_GRID_DDA):
        for stepping in (1, 0):
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                fb, n, _ = g.render(kernel=kernel, stepping=stepping)
                out.append((("point", kernel, stepping, grey), fb, n))
    _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
    for kernel in linear_kernels:
        fb, n, _ = g.render(kernel=kernel, filter_mode=vrc.FILTER_TRILINEAR)
        out.append((("trilinear", kernel), fb, n))
    return out


@pytest.mark.parametrize("image", ["int8", "int16"])
def test_signed_pool_equals_the_unsigned_pool_bit_for_bit(vrc, image):
    # an int8 pool with range (-128, 127) against the uint8 pool of v + 128 with (0, 255); int16 likewise
    from gpu_run import GpuScene
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    assert tuple(s.render.dataSourceRange) == ((0.0, 255.0) if image == "int8" else (0.0, 65535.0))
    lin = [vrc.KERNEL_GRID_DDA, vrc.KERNEL_LDS, vrc.KERNEL_PACKED]
    with vt.typed_gpu_scene(t) as g:
        signed = _frames(vrc, g, lin)
    with GpuScene(s) as g:  # vrc_pool_create
        unsigned = _frames(vrc, g, lin)
    for (k, a, n_a), (_, b, n_b) in zip(signed, unsigned):
        assert (a == b).all() and n_a == n_b, (image, k)
    assert signed[0][1][..., 3].max() > 0.05


@pytest.mark.parametrize("image", ["int32", "uint32"])
def test_32_bit_integer_pool_equals_the_float_pool_bit_for_bit(vrc, image):
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    f = vt.copy.copy(t)
    f.bricks = {nid: b.astype(np.float32) for nid, b in t.bricks.items()}
    f.atlas = t.atlas.astype(np.float32)
    f.voxel_type = vrc.VOXEL_FLOAT32
    with vt.typed_gpu_scene(t) as g:
        ints = _frames(vrc, g, [vrc.KERNEL_GRID_DDA])
    with vt.typed_gpu_scene(f) as g:
        floats = _frames(vrc, g, [vrc.KERNEL_GRID_DDA])
    for (k, a, n_a), (_, b, n_b) in zip(ints, floats):
        assert (a == b).all() and n_a == n_b, (image, k)


def test_typed_unsigned_pools_are_the_pools_of_vrc_pool_create(vrc):
    from gpu_run import GpuScene
    for dtype, voxel_type in (("u8", vrc.VOXEL_UINT8), ("u16", vrc.VOXEL_UINT16)):
        s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), volume="hash", spin=(0.5, 0.35), dtype=dtype)
        with GpuScene(s) as g:
            want, n_want, _ = g.render()
            info = g.info()
        with vt.typed_gpu_scene(s, voxel_type=voxel_type) as g:
            got, n_got, _ = g.render()
            assert g.info() == info
        assert (got == want).all() and n_got == n_want


# ---- passes, clip planes, lists that are no grid -----------------------------------------------------------------
@pytest.mark.parametrize("image", ["float", "int16"])
def test_two_passes_accumulate(vrc, image):
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    passes = [(0, s.n_nodes // 2), (s.n_nodes // 2, s.n_nodes)]
    r = ref64.render_passes(s, passes)
    with vt.typed_gpu_scene(t) as g:
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_AUTO):
            got, n, _ = g.render(kernel=kernel, passes=passes)
            check(s, got, n, r, "hash16 as %s in two passes" % image, "gpu kernel %d" % kernel, count=False)


@pytest.mark.parametrize("image", ["float", "uint32", "int8"])
def test_non_grid_brick_list(vrc, image):
    # parents and all their leaves: overlapping bricks, rendered in list order by every form
    im = vt.IMAGES[image]
    s = nongrid.overlapping_scene("hash_parents_all_leaves", dtype=im.base, data_range=im.q_range())
    t = vt.typed_scene(s, im)
    r = ref64.render(s)
    r_lin = ref64.render(s, filter_mode=1)
    with vt.typed_gpu_scene(t) as g:
        for kernel in (vrc.KERNEL_REFERENCE_ORDER, vrc.KERNEL_AUTO):
            for stepping in (1, 0):
                got, n, st = g.render(kernel=kernel, stepping=stepping)
                assert st.kernel_variant == vrc.KERNEL_REFERENCE_ORDER
                check(s, got, n, r, "non-grid list as %s" % image, "gpu kernel %d, stepping %d" % (kernel, stepping), count=False)
        got, n, _ = g.render(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=vrc.FILTER_TRILINEAR)
        check(s, got, n, r_lin, "non-grid list as %s trilinear" % image, "gpu reference order", count=False)


# ---- per-ray LOD --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1])
def test_per_ray_lod_on_a_float_hierarchy(vrc, filter_mode):
    # ref64 does not cover per-ray LOD: the float hierarchy is compared with the SAME hierarchy as its uint16 image,
    # both on the GPU, by scenes.assert_close_frames (a property check between two frames whose classification rounds
    # differently, not parity with a reference)
    from gpu_run import GpuScene
    im = vt.IMAGES["float"]
    vi = orc.mem_volume_info(64, 64, 64, 16)
    s = vt.q_scene("hash16", im, ids=orc.all_level_ids(vi, None), viewport=(48, 40))
    t = vt.typed_scene(s, im)
    lod = (1.5, orc.world_space_per_pixel(s))
    with GpuScene(s) as g:
        want, n_want, st = g.render(kernel=vrc.KERNEL_GRID_DDA, filter_mode=filter_mode, ray_lod=lod)
        assert st.kernel_variant == vrc.KERNEL_RAY_LOD
    with vt.typed_gpu_scene(t) as g:
        for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_AUTO):
            got, n_got, st = g.render(kernel=kernel, filter_mode=filter_mode, ray_lod=lod)
            assert st.kernel_variant == vrc.KERNEL_RAY_LOD and b"float" in g.L.vrc_last_kernel()
            scenes.assert_close_frames(got, want, "per-ray LOD, float against its uint16 image, filter %d" % filter_mode)
            assert abs(n_got - n_want) <= 1e-4 * n_want + 8
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            with pytest.raises(vrc.VrcError) as e:
                g.render(kernel=kernel, filter_mode=1, ray_lod=lod)
            assert e.value.code == vrc.VRC_EINVAL
    assert want[..., 3].max() > 0.05


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", ["float", "int32", "uint32"])
def test_staged_and_packed_forms_refuse_4_byte_pools(vrc, image):
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    with vt.typed_gpu_scene(t) as g:
        for kernel in (vrc.KERNEL_LDS, vrc.KERNEL_PACKED):
            for f in (0, 1):
                with pytest.raises(vrc.VrcError) as e:
                    g.render(kernel=kernel, filter_mode=f)
                assert e.value.code == vrc.VRC_EINVAL and "gathers" in str(e.value)
        g.render()  # the pool still renders


@pytest.mark.parametrize("name", sorted(NP_TYPES))
def test_histograms_are_unsupported(vrc, name):
    im = vt.IMAGES[name]
    s, t, _ = vt.ref("hash16", im)
    with vt.typed_gpu_scene(t) as g:
        L = g.L
        bins = np.zeros(256, dtype=np.uint64)
        slot = vrc.f32x3(*next(iter(g.slots.values())))
        rc = L.vrc_pool_histogram(g.pool, slot, vrc.u32x3(1, 1, 1), vrc.u32x3(16, 16, 16), 256, 1, bins.ctypes.data)
        assert rc == vrc.VRC_EUNSUPPORTED and b"not implemented" in L.vrc_last_error()
        overlap = vrc.u32x3(1, 1, 1)
        assert L.vrc_pool_enable_histograms(g.pool, 256, C.cast(overlap, C.c_void_p)) == vrc.VRC_EUNSUPPORTED
        scale = np.ones(1, dtype=np.uint64)
        sl = np.array(list(slot), dtype=np.float32)
        assert L.vrc_frame_histogram(g.ctx, g.pool, sl.ctypes.data, scale.ctypes.data, 1, 0) == vrc.VRC_EUNSUPPORTED
        assert L.vrc_pool_enable_histograms(g.pool, 0, None) == vrc.VRC_OK  # turning them off is no request


def test_unknown_voxel_type_and_the_pinned_refusals(vrc):
    L = vrc.load_library()
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    try:
        mb = vrc.u32x3(18, 18, 18)
        for bad in (-1, 7, 100):
            assert L.vrc_pool_create_typed(ctx, bad, mb, 1 << 20, C.byref(pool)) == vrc.VRC_EINVAL
            assert not pool and b"unknown voxel type" in L.vrc_last_error()
        assert L.vrc_pool_create_typed(ctx, vrc.VOXEL_FLOAT32, vrc.u32x3(0, 18, 18), 1 << 20, C.byref(pool)) == vrc.VRC_EINVAL
        for (nbytes, signed, is_float) in ((4, 0, 0), (4, 0, 1), (1, 1, 0), (2, 1, 0)):
            assert L.vrc_pool_create(ctx, nbytes, signed, is_float, 1, mb, 1 << 20, C.byref(pool)) == vrc.VRC_EUNSUPPORTED
            assert not pool and b"vrc_pool_create_typed" in L.vrc_last_error()
    finally:
        L.vrc_ctx_destroy(ctx)
