"""Signed, 32-bit and float voxels on the host build of the kernel code (no GPU needed): the march over the float atlas
(ATLAS_T = float: VRC_MODE_POINT, VRC_MODE_POINT_GREY, VRC_MODE_TRILINEAR; reference order and grid walk, both
steppings) and the offset-binary form of int8 / int16 against tests/ref64.py through affine images (tests/voxel_types.py
says why that is exact); the upload transforms against NumPy; the rule for voxels that are not numbers.

Every frame comparison is test_ref64_cpu.check: scenes.assert_parity with ref64's own tie budget, no pixel left out,
and for the grid walk the sample count within 1e-4 n + 8 of ref64's."""
import numpy as np
import pytest

import orc
import voxel_types as vt
from libre_amd import vrc
from test_ref64_cpu import check

POINT_FORMS = [0, vt.GRID, vt.FIXED, vt.GRID | vt.FIXED, vt.GREY | vt.FIXED, vt.GREY | vt.GRID | vt.FIXED]
LINEAR_FORMS = [vt.TRILINEAR, vt.TRILINEAR | vt.GRID]


def _name(form):
    return "host %s%s%s%s" % ("grid walk" if form & vt.GRID else "reference order", ", fixed-point" if form & vt.FIXED else "",
                              ", grey" if form & vt.GREY else "", ", trilinear" if form & vt.TRILINEAR else "")


@pytest.mark.parametrize("base", sorted(vt.BASES))
@pytest.mark.parametrize("image", sorted(vt.IMAGES))
def test_point_sampling_matches_ref64(base, image):
    im = vt.IMAGES[image]
    s, t, r = vt.ref(base, im)
    for form in POINT_FORMS:
        got, n = vt.harness_render(t, form)
        check(s, got, n, r, "%s as %s" % (base, image), _name(form), count=bool(form & vt.GRID))


@pytest.mark.parametrize("base", ["hash16", "smooth16", "hash32_clip"])
@pytest.mark.parametrize("image", sorted(vt.IMAGES))
def test_trilinear_matches_ref64(base, image):
    im = vt.IMAGES[image]
    s, t, r = vt.ref(base, im, filter_mode=1)
    for form in LINEAR_FORMS:
        got, n = vt.harness_render(t, form)
        check(s, got, n, r, "%s as %s trilinear" % (base, image), _name(form), count=bool(form & vt.GRID))


@pytest.mark.parametrize("image", ["float", "int32"])
def test_trilinear_of_float_bricks_goes_to_ref64_directly(image):
    # ref64's trilinear sampler takes bricks of any dtype: the typed scene itself, no image in between
    import ref64
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("smooth16", im, filter_mode=1)
    u = vt.copy.copy(t)
    u.bricks = {nid: b.astype(np.float32) for nid, b in t.bricks.items()}  # what the atlas holds
    r = ref64.render(u, filter_mode=1)
    for form in LINEAR_FORMS:
        got, n = vt.harness_render(t, form)
        check(u, got, n, r, "smooth16 as %s trilinear, ref64 on the float bricks" % image, _name(form),
              count=bool(form & vt.GRID))


@pytest.mark.parametrize("image", ["float", "uint32", "int16"])
def test_exact_tf_weight_matches_ref64(image):
    im = vt.IMAGES[image]
    s, t, r = vt.ref("smooth16", im, frac_bits=0)
    for form in (vt.GRID | vt.FIXED, vt.GRID):
        got, n = vt.harness_render(t, form, frac_bits=0)
        check(s, got, n, r, "smooth16 as %s exact weight" % image, _name(form))


def test_two_passes_accumulate():
    import nongrid
    import ref64
    im = vt.IMAGES["float"]
    s, t, _ = vt.ref("hash16", im)
    passes = [(0, s.n_nodes // 2), (s.n_nodes // 2, s.n_nodes)]
    r = ref64.render_passes(s, passes)
    for form in (vt.FIXED, 0):
        fb, total = None, 0
        for part in nongrid.passes_of(t, passes):
            part.voxel_type = t.voxel_type
            fb, n = vt.harness_render(part, form, fb=fb)
            total += n
        check(s, fb, total, r, "hash16 as float in two passes", _name(form), count=False)


# ---- signed voxels are the unsigned pool, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("image,unsigned", [("int8", vrc.VOXEL_UINT8), ("int16", vrc.VOXEL_UINT16)])
def test_signed_voxels_equal_their_unsigned_image_bit_for_bit(image, unsigned):
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    u = vt.copy.copy(s)  # the unsigned volume v + 128 / + 32768 with the type's range
    u.voxel_type = unsigned
    assert tuple(u.render.dataSourceRange) == ((0.0, 255.0) if image == "int8" else (0.0, 65535.0))
    for form in POINT_FORMS + LINEAR_FORMS:
        a, n_a = vt.harness_render(t, form)
        b, n_b = vt.harness_render(u, form)
        assert (a == b).all() and n_a == n_b, _name(form)
    if image == "int8":  # ... and per-sample classification of 8-bit voxels is the product harness's kernel 8
        b, n_b, _ = orc.harness_render(s, kernel=8)
        a, n_a = vt.harness_render(t, vt.GRID)
        assert (a == b).all() and n_a == n_b


@pytest.mark.parametrize("image", ["int32", "uint32"])
def test_32_bit_integers_equal_the_float_volume_of_the_same_values(image):
    im = vt.IMAGES[image]
    s, t, _ = vt.ref("hash16", im)
    f = vt.copy.copy(t)
    f.atlas = t.atlas.astype(np.float32)
    f.voxel_type = vrc.VOXEL_FLOAT32
    for form in (vt.GRID | vt.FIXED, vt.FIXED, vt.TRILINEAR | vt.GRID):
        a, n_a = vt.harness_render(t, form)
        b, n_b = vt.harness_render(f, form)
        assert (a == b).all() and n_a == n_b, _name(form)


# ---- the upload transforms ----------------------------------------------------------------------------------------------
def test_sign_flip_is_offset_binary():
    v8 = np.arange(-128, 128, dtype=np.int8)
    assert (vt.harness_xform(v8, vrc.VOXEL_INT8, np.uint8) == (v8.astype(np.int16) + 128).astype(np.uint8)).all()
    v16 = np.arange(-32768, 32768, dtype=np.int16)
    assert (vt.harness_xform(v16, vrc.VOXEL_INT16, np.uint16) == (v16.astype(np.int32) + 32768).astype(np.uint16)).all()
    # its own inverse (what vrc_pool_read_region applies)
    back = vt.harness_xform(vt.harness_xform(v16, vrc.VOXEL_INT16, np.uint16).view(np.int16), vrc.VOXEL_INT16, np.uint16)
    assert (back.view(np.int16) == v16).all()
    # the unsigned and the float type pass through
    u = np.arange(65536, dtype=np.uint16)
    assert (vt.harness_xform(u, vrc.VOXEL_UINT16, np.uint16) == u).all()
    f = np.array([0.0, -0.0, 1.5, np.inf, -np.inf, np.nan, 1e-40], dtype=np.float32)
    assert (vt.harness_xform(f, vrc.VOXEL_FLOAT32, np.float32).view(np.uint32) == f.view(np.uint32)).all()


def test_32_bit_integers_are_converted_round_to_nearest_even():
    rng = np.random.default_rng(32)
    edge = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6,
                     2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31, 2 ** 31 + 128, 2 ** 31 + 129, 2 ** 32 - 1,
                     2 ** 32 - 128, 2 ** 32 - 129], dtype=np.uint64)
    u = np.concatenate([edge, rng.integers(0, 2 ** 32, 20000, dtype=np.uint64)]).astype(np.uint32)
    assert (vt.harness_xform(u, vrc.VOXEL_UINT32, np.float32).view(np.uint32) == u.astype(np.float32).view(np.uint32)).all()
    i = u.view(np.int32)
    assert (vt.harness_xform(i, vrc.VOXEL_INT32, np.float32).view(np.uint32) == i.astype(np.float32).view(np.uint32)).all()
    # NumPy's conversion is the one meant: ties go to the even mantissa
    assert np.float32(np.uint32(2 ** 24 + 1)) == 2.0 ** 24 and np.float32(np.uint32(2 ** 24 + 3)) == 2.0 ** 24 + 4


# ---- voxels that are not numbers ------------------------------------------------------------------------------------------
def test_a_nan_density_classifies_as_the_first_texel():
    tf = orc.linear_ramp_tf(0.3).copy()
    tf[0] = [0.25, 0.5, 0.75, 0.125]  # a first texel one can recognise
    d = np.array([np.nan, -np.nan, -1e30, -np.inf, np.inf, 1e30], dtype=np.float32)
    e = vt.harness_classify(tf, d, -1.0, 1.0)
    assert np.isfinite(e).all()
    a0 = np.float32(0.125)
    first = np.array([0.25 * a0, 0.5 * a0, 0.75 * a0, a0], dtype=np.float32)
    for k in range(4):  # NaN, like anything below the range, takes texel 0 (alpha correction 1: alpha' = alpha)
        assert np.allclose(e[k], first, rtol=0, atol=1e-7), (k, e[k])
    assert (e[0] == e[2]).all() and (e[1] == e[2]).all()
    last = vt.harness_classify(tf, np.array([1.0], dtype=np.float32), -1.0, 1.0)[0]
    assert (e[4] == last).all() and (e[5] == last).all()


def test_a_nan_voxel_renders_as_the_range_minimum():
    # a float volume with NaN voxels gives the frame of the same volume with the range minimum in their place
    im = vt.IMAGES["float"]
    s, t, _ = vt.ref("hash16", im)
    hole = t.atlas.copy()
    mask = (s.atlas & 7) == 3
    assert 0.05 < mask.mean() < 0.3
    low = vt.copy.copy(t)
    low.atlas = np.where(mask, np.float32(-1.0), hole).astype(np.float32)
    nan = vt.copy.copy(t)
    nan.atlas = np.where(mask, np.float32(np.nan), hole).astype(np.float32)
    for form in (vt.GRID | vt.FIXED, 0):
        a, n_a = vt.harness_render(nan, form)
        b, n_b = vt.harness_render(low, form)
        assert np.isfinite(a).all() and (a == b).all() and n_a == n_b
