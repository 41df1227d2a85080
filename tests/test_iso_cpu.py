"""An isosurface frame (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO) on the CPU: the acceptance rule of tests/iso_ref.py (it
accepts the reference's own answer and rejects deliberate misreadings), the conditions that keep it honest for every
scene and isovalue the GPU tests use, and the host build of the per-ray code (tests/cpu_harness/iso_harness.cpp) held to
the rule, to a known answer and to the bitwise identities of the contract.  tests/test_iso.py takes the same scenes to a
GPU."""
import numpy as np
import pytest

import depth_ref
import iso_ref
import mip_scenes
import nonfinite
import scenes
from iso_ref import BOTH_CAP, FIXED, GRID, ISO, MULTI_CAP, SKIP, TRILINEAR, UNIFORM, ref, scene, tolerance

NAMES = ("axis", "spin", "inside", "clip", "skip", "skip16")
SPARSE = ("two blocks", "skip", "skip16")


def _forms(filter_mode):
    t = TRILINEAR if filter_mode else 0
    return {"walk": GRID | FIXED | t, "reforder": t, "walk float": GRID | t}


def _same(a, b, counts=False):
    """frame, V, counts, D and G bit for bit (the sample count too where asked)"""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b) if isinstance(x, np.ndarray)) and (
        not counts or a[1] == b[1])


def _caps(r, what, sparse=False):
    multi, both = r.shares()
    sure_hit, sure_miss = int((~r.miss()).sum()), int((r.miss() & ~r.hit()).sum())
    print("%s: %d pixels surely hit, %d surely miss; %.3f of the hit ones have more than one candidate depth, %.3f of all "
          "may hit or miss" % (what, sure_hit, sure_miss, multi, both))
    assert multi <= MULTI_CAP and both <= BOTH_CAP, what
    assert sure_hit >= 100, what
    if sparse:
        assert sure_miss >= 100, what


# ---- the conditions on every scene and isovalue the GPU tests use -----------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", NAMES)
def test_the_caps_hold_for_the_scenes(name, filter_mode):
    _caps(ref(name, filter_mode), "%s filter %d" % (name, filter_mode), name in SPARSE)


def test_the_caps_hold_for_two_blocks():
    """(point samples: a trilinear sample inside a block of 200s is 200 up to rounding, which is the isovalue -- every
    such pixel may hit or miss; the GPU tests ask only bitwise identities of that frame)"""
    _caps(ref("two blocks", 0), "two blocks", True)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_caps_hold_for_the_voxel_types(image, filter_mode):
    _caps(iso_ref.typed_ref(image, filter_mode), "%s filter %d" % (image, filter_mode))
    assert iso_ref.typed_iso(image)[1] < 0 or image != "int16", "a negative isovalue for the signed type"


def test_the_caps_hold_for_the_nan_brick_and_the_nucleon():
    _caps(iso_ref.nan_ref(), "allnan_brick")
    _caps(iso_ref.nucleon_ref(), "nucleon")


# ---- the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spin", "two blocks"])
def test_the_rule_accepts_its_own_answer_and_rejects_misreadings(name):
    """The reference's own answer passes; a depth taken at the last crossing, at the segment's start, one sample late or
    in a later brick does not, nor a gradient with a component negated or taken at the neighbouring voxel."""
    r = ref(name, 0)
    assert iso_ref.check(r, *r.own()) == (0, 0.0)
    for m in iso_ref.MUTATIONS:
        bad = iso_ref.check(r, *r.own(m))[0]
        print("%s, %s: %d of %d pixels rejected" % (name, m, bad, int((~r.miss()).sum())))
        assert bad > 0, m
    # a hit reported as a miss, and a miss as a hit
    v, c, d, g = r.own()
    y, x = [int(a[0]) for a in np.nonzero(c)]
    c2, d2, g2 = c.copy(), d.copy(), g.copy()
    c2[y, x], d2[y, x], g2[y, x] = 0, np.inf, 0.0
    assert iso_ref.check(r, v, c2, d2, g2)[0] == 1
    y, x = [int(a[0]) for a in np.nonzero(r.miss() & ~r.hit())]
    c2, d2 = c.copy(), d.copy()
    c2[y, x], d2[y, x] = 1, 1.0
    assert iso_ref.check(r, v, c2, d2, g)[0] == 1


# ---- the host build ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", NAMES)
def test_the_host_build_passes_the_rule(name, filter_mode):
    s, r = scene(name, filter_mode), ref(name, filter_mode)
    tol = tolerance(s, filter_mode)
    for what, form in _forms(filter_mode).items():
        out = iso_ref.harness_render(s, form, ISO[name])
        bad, worst = iso_ref.check(r, out[2], out[3], out[4], out[5], tol)
        print("%s filter %d %s: %d failing pixels, worst depth error %.2g steps" % (name, filter_mode, what, bad, worst))
        assert bad == 0, what
        assert np.isposinf(out[4][out[3] == 0]).all() and (out[5][out[3] == 0] == 0).all()


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16", "two blocks", "spin"])
def test_skipping_and_uniform_bricks_change_no_bit(name, filter_mode):
    s = scene(name, filter_mode)
    t = TRILINEAR if filter_mode else 0
    for loop in (GRID | FIXED, 0):
        out = {(k, u): iso_ref.harness_render(s, loop | t | (SKIP if k else 0) | (UNIFORM if u else 0), ISO[name])
               for k in (0, 1) for u in (0, 1)}
        for key, o in out.items():
            assert _same(out[0, 0], o), (loop, key)
        n = out[0, 0][1]
        print("%s filter %d loop %d: samples %d, with skipping %d / %d" % (name, filter_mode, loop, n, out[1, 0][1], out[1, 1][1]))
        assert out[0, 1][1] == n and out[1, 1][1] == out[1, 0][1], "uniform bricks: the same count"
        assert out[1, 0][1] < n
        # without skipping the count is the MIP frame's
        assert n == mip_scenes.harness_render(s, loop | t)[1]


@pytest.mark.parametrize("name", ["spin", "two blocks", "skip"])
def test_three_passes_in_four_orders_equal_one(name):
    s = scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    for filter_mode in (0, 1):
        t = TRILINEAR if filter_mode else 0
        plain = iso_ref.harness_render(s, t, ISO[name])
        for extra in (0, SKIP | UNIFORM):
            one = iso_ref.harness_render(s, t | extra, ISO[name])
            assert _same(plain, one)
            walk = iso_ref.harness_render(s, GRID | t | extra, ISO[name])
            assert _same(plain, walk), "the grid walk and the reference-order loop"
            for order in (parts, parts[::-1], [parts[1], parts[2], parts[0]], [parts[2], parts[0], parts[1]]):
                three = iso_ref.harness_render(s, t | extra, ISO[name], passes=order)
                assert _same(one, three), (filter_mode, extra, order)


def test_the_known_answer_on_two_blocks():
    """V = 200, D = the near block's first sample, G = the exact integer difference across the block's face times the
    brick's voxels per world unit: along z the voxel above the block's top layer is 0 and the one below is 200."""
    s, r = scene("two blocks"), ref("two blocks", 0)
    for form in (GRID | FIXED | SKIP | UNIFORM, 0):
        fb, n, v, c, d, g = iso_ref.harness_render(s, form, 200.0, ambient=1.0)
        hit = c == 1
        assert hit.sum() >= 100 and (v[hit] == depth_ref.BLOCK_VALUE).all()
        # the unit cube holds 64 voxels a side: the near block's top face lies at z = (54 - 32) / 64 of the world
        rays = iso_ref.harness_render.rays.astype(np.float64)
        top = (float(depth_ref.NEAR_FAR_Z[0] + 4) / 64.0) * float(s.view.aabbMax[2] - s.view.aabbMin[2]) + float(s.view.aabbMin[2])
        t_face = (top - rays[..., 4]) / rays[..., 7]
        step = 1.0 / float(s.render.samplesPerRay)
        inner = hit & np.roll(hit, 1, 0) & np.roll(hit, -1, 0) & np.roll(hit, 1, 1) & np.roll(hit, -1, 1)
        assert inner.sum() >= 50
        assert (d[inner] >= t_face[inner] - 1e-5).all() and (d[inner] < t_face[inner] + step + 1e-5).all()
        nd = s.nodes[0]
        vpw = np.float32(16.0) / np.float32(nd.aabbSize[2])
        want = np.float32(0 - depth_ref.BLOCK_VALUE) * vpw
        assert (g[inner][:, 2] == want).all() and (g[inner][:, :2] == 0).all()
        # ambient = 1: the constant colour
        colour = fb[hit]
        assert (colour == colour[0]).all() and colour[0][3] > 0 and (fb[~hit] == 0).all()
        assert iso_ref.check(r, v, c, d, g)[0] == 0


def test_the_thresholds():
    """The integer threshold is the ceiling, clamped; the float one is the smallest float whose report reaches iso."""
    import ctypes as C
    h = iso_ref.harness()
    h.iso_harness_int_threshold.restype = C.c_uint32
    h.iso_harness_float_threshold.restype = C.c_float
    it = lambda iso, shift, top: h.iso_harness_int_threshold(C.c_float(iso), C.c_float(shift), C.c_uint32(top))  # noqa: E731
    assert it(10.0, 0.0, 255) == 10 and it(10.25, 0.0, 255) == 11 and it(-3.0, 0.0, 255) == 0 and it(255.5, 0.0, 255) == 256
    assert it(-0.5, 128.0, 255) == 128 and it(-100.25, 32768.0, 65535) == 32668 and it(np.inf, 0.0, 255) == 256
    ft = lambda iso, shift: np.float32(h.iso_harness_float_threshold(C.c_float(iso), C.c_float(shift)))  # noqa: E731
    assert ft(0.3, 0.0) == np.float32(0.3)
    for iso, shift in ((-100.3, 32768.0), (0.001, 32768.0), (-32767.99, 32768.0), (12.5, 128.0), (-127.7, 128.0)):
        t = ft(iso, shift)
        rep = lambda d: np.float32(np.float64(d) - np.float64(shift))  # noqa: E731
        assert rep(t) >= np.float32(iso) and rep(np.nextafter(t, np.float32(-np.inf))) < np.float32(iso), (iso, shift)


def test_nan_voxels_never_hit_on_the_host():
    case = nonfinite.case("allnan_brick")
    r = iso_ref.nan_ref()
    tol = scenes.E0 * (float(case.mq.render.dataSourceRange[1]) - float(case.mq.render.dataSourceRange[0]))
    assert iso_ref.check(r, *r.own(), tol=tol)[0] == 0
