"""The references of the minimum and mean folds (tests/fold_ref.py) checked on the CPU -- their own definitions, and the
conditions that keep their acceptance rules honest for every scene tests/test_fold.py takes to a GPU -- and the host build
of the folds' per-ray code (tests/cpu_harness/fold_harness.cpp) held to them."""
import copy

import numpy as np
import pytest

import fold_ref
import mip_ref
import mip_scenes
import scenes
from fold_ref import FOLD_MAX, FOLD_MEAN, FOLD_MIN

MIN_SCENES = ["axis", "spin", "inside", "clip", "skip", "skip16"]  # what tests/test_fold.py renders with the minimum
GRID, FIXED, TRILINEAR, SKIP, UNIFORM = mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.TRILINEAR, mip_scenes.SKIP, mip_scenes.UNIFORM
FORMS = [0, GRID, FIXED, GRID | FIXED, TRILINEAR, GRID | TRILINEAR]  # list and grid walk, float and fixed stepping, both filters


def _own_min_frame(s, r):
    f = mip_ref.classify64(s, np.where(r.certain, r.m, 0.0))
    f[~r.certain] = 0.0
    return f


def _own_mean_frame(s, r):
    v, c = fold_ref.own_mean(r)
    f = mip_ref.classify64(s, v.astype(np.float64))
    f[c == 0] = 0.0
    return f, v, c


# ---- conditions on the references alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("name", MIN_SCENES)
def test_ambiguous_minip_pixels_are_capped(name, filter_mode):
    """MIP's cap: pixels with more than one acceptable outcome are at most 5 % of the hit pixels."""
    r = fold_ref.min_ref(name, filter_mode)
    hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
    print("%s filter %d: %d hit pixels, %d ambiguous (%.1f %%)" % (name, filter_mode, hit, amb, 100.0 * amb / hit))
    assert hit > 100
    assert amb <= 0.05 * hit


@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_ambiguous_minip_pixels_of_the_typed_scenes_are_capped(image, filter_mode):
    q, _, _ = mip_scenes.typed(image)
    r = fold_ref.min_render(q, filter_mode=filter_mode)
    hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
    print("%s filter %d: %d hit pixels, %d ambiguous" % (image, filter_mode, hit, amb))
    assert hit > 100 and amb <= 0.05 * hit


@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("name", fold_ref.MEAN_SCENES)
def test_settled_mean_pixels_are_most(name, filter_mode):
    """A settled pixel pins the mean to one number: at least 75 % of the hit pixels, or the rule says too little."""
    r = fold_ref.mean_ref(name, filter_mode)
    hit, settled = int(r.hit().sum()), int(r.settled.sum())
    print("%s filter %d: %d hit pixels, %d settled (%.1f %%)" % (name, filter_mode, hit, settled, 100.0 * settled / hit))
    assert hit > 100
    assert settled >= 0.75 * hit


def test_the_face_matched_volume_is_noise_with_equal_planes_at_brick_faces():
    vol = fold_ref.face_matched_noise(48)
    for i in (16, 32):
        assert (vol[i - 1] == vol[i]).all() and (vol[:, i - 1] == vol[:, i]).all() and (vol[:, :, i - 1] == vol[:, :, i]).all()
    assert len(np.unique(vol)) == 256 and abs(float(vol.mean()) - 127.5) < 1.0


def test_the_minimum_is_the_brute_force_minimum_of_the_sure_samples():
    """min_render against the definition, where no sample is in doubt: the certain maximum of the complement scene is
    top - the certain minimum, and it never exceeds the certain maximum of the scene itself."""
    r, rmax = fold_ref.min_ref("count96"), mip_scenes.ref("count96")
    assert (r.certain == rmax.certain).all() and (r.counts == rmax.counts).all()
    assert (r.m[r.certain] <= rmax.m[r.certain]).all() and (r.m[r.certain] < rmax.m[r.certain]).mean() > 0.9


def test_mean_counts_are_mip_refs():
    for name in ("spin", "clip", "count96"):
        s = fold_ref.mean_scene(name)
        r, q = fold_ref.mean_ref(name), mip_ref.render(s)
        assert (r.count_lo == q.counts_lo).all() and (r.count_hi == q.counts_hi).all(), name
        # the mean lies between the extremes of the same samples
        sure = r.settled & q.certain
        assert (r.hi[sure] <= q.m[sure]).all()


def test_passes_meet_in_the_running_state():
    s = fold_ref.mean_scene("spin")
    n = s.n_nodes
    passes = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    r, q = fold_ref.mean_ref("spin"), fold_ref.mean_render_passes(s, passes)
    assert (q.n == r.n).all() and (q.count_hi == r.count_hi).all()
    assert np.array_equal(q.lo, r.lo, equal_nan=True) and np.array_equal(q.hi, r.hi, equal_nan=True)
    t = mip_scenes.get("spin")
    a, b = fold_ref.min_ref("spin"), fold_ref.min_render(t, passes=passes)
    assert (a.m == b.m).all() and (a.certain == b.certain).all()


# ---- the rules have teeth -----------------------------------------------------------------------------------------------
def test_the_minimum_rule_accepts_its_own_frame_and_has_teeth():
    s, r = mip_scenes.get("spin"), fold_ref.min_ref("spin")
    assert fold_ref.check_min_frame(s, r, _own_min_frame(s, r))[0] == 0
    # a MAX frame of the same scene
    rmax = mip_scenes.ref("spin")
    fmax = mip_ref.classify64(s, np.where(rmax.certain, rmax.m, 0.0))
    fmax[~rmax.certain] = 0.0
    assert fold_ref.check_min_frame(s, r, fmax)[0] > 0.5 * r.hit().sum()
    for mutation in fold_ref.MUTATIONS:
        q = fold_ref.min_render(s, _mutate=mutation)
        bad = fold_ref.check_min_frame(s, r, _own_min_frame(s, q))[0]
        print(mutation, bad)
        assert bad > 0, mutation
    # a pixel without samples must stay cleared
    f = _own_min_frame(s, r)
    y, x = [int(v[0]) for v in np.nonzero(~r.hit())]
    f[y, x] = 1e-3
    assert fold_ref.check_min_frame(s, r, f)[0] == 1


def test_the_mean_rule_accepts_its_own_frame_and_has_teeth():
    s, r = fold_ref.mean_scene("spin"), fold_ref.mean_ref("spin")
    frame, v, c = _own_mean_frame(s, r)
    assert fold_ref.check_mean_values(s, r, v, c, exact=True)[0] == 0
    assert fold_ref.check_frame_against_values(s, frame, v, c)[0] == 0
    # a MAX frame of the same scene, with the values and counts a MAX read-back holds
    rmax = mip_ref.render(s)
    vmax, cmax = np.where(rmax.certain, rmax.m, 0.0).astype(np.float32), rmax.certain.astype(np.uint32)
    assert fold_ref.check_mean_values(s, r, vmax, cmax, exact=True)[0] > 0.5 * r.hit().sum()
    fmax = mip_ref.classify64(s, vmax.astype(np.float64))
    assert fold_ref.check_frame_against_values(s, fmax, v, c)[0] > 0.5 * r.hit().sum()
    for mutation in fold_ref.MUTATIONS:
        q = fold_ref.mean_render(s, _mutate=mutation)
        _, vq, cq = _own_mean_frame(s, q)
        bad = fold_ref.check_mean_values(s, r, vq, cq, exact=True)[0]
        print(mutation, bad)
        assert bad > 0.5 * r.hit().sum(), mutation
    # one sample too many in one pixel, one ulp-and-a-bit off in another, a stale value under a cleared pixel
    y, x = [int(a[0]) for a in np.nonzero(r.settled)]
    c2 = c.copy()
    c2[y, x] += 1
    assert fold_ref.check_mean_values(s, r, v, c2, exact=True)[0] == 1
    v2 = v.copy()
    v2[y, x] = np.nextafter(np.nextafter(v2[y, x], np.float32(np.inf)), np.float32(np.inf))
    assert fold_ref.check_mean_values(s, r, v2, c, exact=True)[0] == 1
    f2 = frame.copy()
    y0, x0 = [int(a[0]) for a in np.nonzero(c == 0)]
    f2[y0, x0] = 1e-3
    assert fold_ref.check_frame_against_values(s, f2, v, c)[0] == 1


def test_a_value_tolerance_of_e0_times_the_range_is_one_frame_tolerance():
    """Where the transfer function's alpha has slope alpha_max / range, a value off by E0 x range moves the pixel by at
    most E0: the read-back tolerance of float and trilinear means asks no less of a value than the frame rule does of
    its classification."""
    s = fold_ref.mean_scene("spin")
    r0, r1 = float(s.render.dataSourceRange[0]), float(s.render.dataSourceRange[1])
    v = np.linspace(r0, r1 - 1.0, 97)
    d = np.abs(mip_ref.classify64(s, v + scenes.E0 * (r1 - r0)) - mip_ref.classify64(s, v)).max()
    assert d <= scenes.E0 * 1.7, d  # (premultiplied colour of a ramp: slope up to 2 alpha_max^2 = 1.28)


# ---- the host build of the folds' per-ray code --------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["axis", "spin", "inside", "clip"])
def test_host_build_minimum_passes_the_rule(name, form):
    s = mip_scenes.get(name)
    fm = 1 if form & TRILINEAR else 0
    r = fold_ref.min_ref(name, fm)
    fb, n, v, c = fold_ref.harness_render(s, form, FOLD_MIN)
    bad, worst, amb = fold_ref.check_min_frame(s, r, fb)
    print("%s form %d: %d failing (worst excess %.3g), %d ambiguous" % (name, form, bad, worst, amb))
    assert bad == 0
    assert fold_ref.check_candidates(r, v, c, tol=scenes.E0 * 255.0 if fm else 0.0) == 0
    assert fold_ref.check_frame_against_values(s, fb, v, c)[0] == 0
    # |S| is the maximum's
    assert n == mip_scenes.harness_render(s, form)[1]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", fold_ref.MEAN_SCENES)
def test_host_build_mean_passes_the_rule(name, form):
    s = fold_ref.mean_scene(name)
    fm = 1 if form & TRILINEAR else 0
    r = fold_ref.mean_ref(name, fm)
    fb, n, v, c = fold_ref.harness_render(s, form, FOLD_MEAN)
    bad, worst, settled = fold_ref.check_mean_values(s, r, v, c, exact=not fm)
    print("%s form %d: %d failing values (worst excess %.3g), %d settled of %d hit" % (
        name, form, bad, worst, settled, int(r.hit().sum())))
    assert bad == 0
    bad, worst = fold_ref.check_frame_against_values(s, fb, v, c)
    assert bad == 0, worst
    assert n == int(c.sum()) == mip_scenes.harness_render(s, form)[1]
    if name in mip_scenes.COUNT:
        assert (r.count_lo == r.count_hi).all() and n == int(r.count_lo.sum())


@pytest.mark.parametrize("form", [FIXED, 0, TRILINEAR])
def test_host_build_three_passes_equal_one(form):
    k = mip_scenes.get("spin").n_nodes
    passes = [(0, k // 3), (k // 3, 2 * k // 3), (2 * k // 3, k)]
    s = mip_scenes.get("spin")
    one, three = fold_ref.harness_render(s, form, FOLD_MIN), fold_ref.harness_render(s, form, FOLD_MIN, passes=passes)
    assert np.array_equal(one[0], three[0]) and one[1] == three[1]
    assert np.array_equal(one[2], three[2]) and np.array_equal(one[3], three[3])
    s = fold_ref.mean_scene("spin")
    one, three = fold_ref.harness_render(s, form, FOLD_MEAN), fold_ref.harness_render(s, form, FOLD_MEAN, passes=passes)
    assert one[1] == three[1] and np.array_equal(one[3], three[3])  # counts: exact
    if form & TRILINEAR:
        # a float64 sum in another order: the read-back rule's tolerance, both ways
        assert np.abs(one[2].astype(np.float64) - three[2]).max() <= scenes.E0 * 255.0
    else:
        assert np.array_equal(one[2], three[2]) and np.array_equal(one[0], three[0])  # integer sums: exact


@pytest.mark.parametrize("form", [GRID | FIXED, TRILINEAR, 0])
@pytest.mark.parametrize("name", ["skip", "skip16", "spin"])
def test_host_build_skipping_and_uniform_bricks_change_no_minimum(name, form):
    """The complement of mip_scenes.skip_volume: a dark brick nearest the eye, constant bricks above and below the noise."""
    s = fold_ref.complemented_scene(name)
    plain = fold_ref.harness_render(s, form, FOLD_MIN)
    r = fold_ref.min_render(s, filter_mode=1 if form & TRILINEAR else 0)
    assert fold_ref.check_min_frame(s, r, plain[0])[0] == 0
    for extra in (UNIFORM, SKIP, SKIP | UNIFORM):
        other = fold_ref.harness_render(s, form | extra, FOLD_MIN)
        assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[2], other[2]) and np.array_equal(plain[3], other[3])
        if extra == UNIFORM:
            assert other[1] == plain[1]
        else:
            assert other[1] <= plain[1]
            if name in ("skip", "skip16"):
                assert other[1] < plain[1]


@pytest.mark.parametrize("form", [GRID | FIXED, 0])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_host_build_uniform_bricks_change_no_integer_mean(name, form):
    s = mip_scenes.get(name)
    assert mip_scenes.uniform_and_mixed(s)[0] >= 2
    plain = fold_ref.harness_render(s, form, FOLD_MEAN)
    for extra in (UNIFORM, SKIP | UNIFORM):
        other = fold_ref.harness_render(s, form | extra, FOLD_MEAN)
        assert np.array_equal(plain[0], other[0]) and plain[1] == other[1]
        assert np.array_equal(plain[2], other[2]) and np.array_equal(plain[3], other[3])


@pytest.mark.parametrize("form", [TRILINEAR, TRILINEAR | GRID])
def test_host_build_trilinear_min_skipping_with_large_positive_neighbours(form):
    """The mirror of test_mip_cpu.py's large negative neighbours: a float atlas whose few dark voxels sit among neighbours
    of 1e6 to 2.6e8.  An interpolation's rounding error scales with its larger term, not with the slot's minimum, and the
    skipped frame must still be the marched one."""
    s = mip_scenes.get("spin")
    t = copy.copy(s)
    v = s.atlas.astype(np.float32)
    t.atlas = np.ascontiguousarray(np.where(v < 105.0, v, np.float32(1e6) * (v + np.float32(1.0))).astype(np.float32))
    assert (t.atlas < 255).sum() > 100 and (t.atlas > 1e6).sum() > 0.5 * t.atlas.size
    plain = fold_ref.harness_render(t, form, FOLD_MIN)
    skipped = fold_ref.harness_render(t, form | SKIP, FOLD_MIN)
    assert (plain[0][..., 3] > 0).sum() > 100
    assert np.array_equal(plain[0], skipped[0]) and np.array_equal(plain[2], skipped[2]) and skipped[1] < plain[1]


def test_host_build_fold_max_is_the_mip_harness():
    s = mip_scenes.get("spin")
    for form in (GRID | FIXED, TRILINEAR):
        fb, n, v, c = fold_ref.harness_render(s, form, FOLD_MAX)
        fb0, n0 = mip_scenes.harness_render(s, form)
        assert np.array_equal(fb, fb0) and n == n0
        r = mip_scenes.ref("spin", 1 if form & TRILINEAR else 0)
        assert fold_ref.check_candidates(r, v, c, tol=scenes.E0 * 255.0 if form & TRILINEAR else 0.0) == 0


def test_host_build_float_voxels():
    q, t, _ = mip_scenes.typed("float")
    for fm, form in ((0, GRID | FIXED), (1, GRID | TRILINEAR)):
        r = fold_ref.min_render(q, filter_mode=fm)
        for scene in (q, t):
            fb, n, v, c = fold_ref.harness_render(scene, form, FOLD_MIN)
            assert fold_ref.check_min_frame(q, r, fb)[0] == 0
            fb1, n1, v1, c1 = fold_ref.harness_render(scene, form | SKIP | UNIFORM, FOLD_MIN)
            assert np.array_equal(fb, fb1) and np.array_equal(v, v1) and n1 <= n


def test_the_frame_only_mean_rule_of_the_plugin_scene_has_teeth():
    """tests/test_fold_host.py has no read-back: its mean frame is held to the classification of the reference interval."""
    s = mip_scenes.host_mem_scene()
    r = fold_ref.mean_render(s)
    assert r.settled.sum() >= 0.75 * r.hit().sum()
    frame, _, _ = _own_mean_frame(s, r)
    assert fold_ref.check_mean_frame(s, r, frame, exact=True)[0] == 0
    rmax = mip_ref.render(s)
    fmax = mip_ref.classify64(s, np.where(rmax.certain, rmax.m, 0.0))
    fmax[~rmax.certain] = 0.0
    assert fold_ref.check_mean_frame(s, r, fmax, exact=True)[0] > 0.5 * r.hit().sum()
    for mutation in fold_ref.MUTATIONS:
        q = fold_ref.mean_render(s, _mutate=mutation)
        assert fold_ref.check_mean_frame(s, r, _own_mean_frame(s, q)[0], exact=True)[0] > 0, mutation
    rmin = fold_ref.min_render(s)
    assert rmin.ambiguous().sum() <= 0.05 * rmin.hit().sum()


@pytest.mark.parametrize("which", ["bands", "passes"])
def test_the_other_plugin_scenes_keep_the_conditions(which):
    """tests/test_fold_host.py's row-band and multi-pass scenes: the minimum's ambiguity cap and the mean's settled share."""
    import orc
    s = orc.build_scene(**(fold_ref.BANDS_MEM if which == "bands" else fold_ref.PASSES_MEM))
    rmin, rmean = fold_ref.min_render(s), fold_ref.mean_render(s)
    hit = int(rmean.hit().sum())
    print("%s: %d hit, %d ambiguous (minimum), %d settled (mean)" % (which, hit, int(rmin.ambiguous().sum()), int(rmean.settled.sum())))
    assert hit > 100 and rmin.ambiguous().sum() <= 0.05 * hit and rmean.settled.sum() >= 0.75 * hit
    if which != "bands":
        return
    # a reference cut to row bands is the reference of those rows
    rows = np.array([8, 9, 40, 41, 42])
    for r in (rmin, rmean):
        cut = fold_ref.band_rows(r, rows)
        frame = (_own_min_frame(s, r) if r is rmin else _own_mean_frame(s, r)[0])[rows]
        check = fold_ref.check_min_frame(s, cut, frame) if r is rmin else fold_ref.check_mean_frame(s, cut, frame, exact=True)
        assert check[0] == 0
        assert (fold_ref.check_min_frame(s, cut, frame[::-1]) if r is rmin else fold_ref.check_mean_frame(s, cut, frame[::-1], exact=True))[0] > 0
