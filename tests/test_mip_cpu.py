"""The maximum-intensity reference (tests/mip_ref.py) checked on the CPU: its own definition, and the conditions that keep
its acceptance rule honest for every scene tests/test_mip.py takes to a GPU."""
import numpy as np
import pytest

import mip_ref
import mip_scenes
import orc
import ref64
import scenes


def _own_frame(s, r):
    f = mip_ref.classify64(s, np.where(r.certain, r.m, 0.0))
    f[~r.certain] = 0.0
    return f


@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(mip_scenes.SCENES))
def test_ambiguous_pixels_are_capped(name, filter_mode):
    """Pixels with more than one acceptable outcome: at most 5 % of the hit pixels, or the rule says too little."""
    r = mip_scenes.ref(name, filter_mode)
    hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
    print("%s filter %d: %d hit pixels, %d ambiguous" % (name, filter_mode, hit, amb))
    assert hit > 100
    assert amb <= 0.05 * hit


@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_ambiguous_pixels_of_the_typed_scenes_are_capped(image, filter_mode):
    r = mip_scenes.typed_ref(image, filter_mode)
    hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
    print("%s filter %d: %d hit pixels, %d ambiguous" % (image, filter_mode, hit, amb))
    assert hit > 100 and amb <= 0.05 * hit


@pytest.mark.parametrize("filter_mode", [0, 1])
@pytest.mark.parametrize("which", ["mem", "nucleon", "nucleon_default_view", "non_grid"])
def test_ambiguous_pixels_of_the_remaining_gpu_scenes_are_capped(which, filter_mode):
    """The scenes tests/test_mip_host.py renders through the plugin, and the nucleon and non-grid scenes of
    tests/test_mip.py."""
    if which == "mem":
        s = mip_scenes.host_mem_scene()
    elif which == "nucleon":
        s = mip_scenes.host_nucleon_scene()
    elif which == "nucleon_default_view":
        s = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    else:
        import nongrid
        s = nongrid.overlapping_scene("hash_parents_some_children", viewport=(36, 28))
    r = mip_ref.render(s, filter_mode=filter_mode)
    hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
    print("%s filter %d: %d hit pixels, %d ambiguous" % (which, filter_mode, hit, amb))
    assert hit > 100 and amb <= 0.05 * hit


@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_the_skipping_scene_has_constant_bricks_next_to_noise(name):
    """Constant WITH the overlap, or the upload does not call the slot uniform."""
    s = mip_scenes.get(name)
    assert [s.vi.overlap[a] for a in range(3)] == [mip_scenes.OVERLAP] * 3
    uniform, mixed = mip_scenes.uniform_and_mixed(s)
    values = {int(b.flat[0]) for b in s.bricks.values() if (b == b.flat[0]).all()}
    print("%s: %d uniform bricks (%d values), %d mixed" % (name, uniform, len(values), mixed))
    assert uniform >= 2 and len(values) >= 2 and mixed >= 1
    # a constant brick that a ray reaches behind noise, and whose value beats the noise: it is taken, not skipped
    r = mip_scenes.ref(name)
    top = max(values)
    assert (r.m[r.certain] == top).sum() > 8


@pytest.mark.parametrize("name", mip_scenes.COUNT)
def test_the_count_scenes_leave_no_sample_in_doubt(name):
    r = mip_scenes.ref(name)
    assert (r.counts_lo == r.counts_hi).all() and (r.counts == r.counts_lo).all() and r.counts.sum() > 10000


def _counts_ok(r, each, n, what):
    """The sample count against mip_ref: pixel by pixel, equal wherever float64 leaves no sample in doubt, inside the
    interval its doubtful samples span elsewhere."""
    sure = r.counts_lo == r.counts_hi
    print("%s: samples %d, mip_ref %d; %d of %d pixels without a doubtful sample" % (
        what, n, int(r.counts.sum()), int(sure.sum()), sure.size))
    assert sure.mean() > 0.8  # (of mip_ref alone; the axis view, which looks along brick faces, has the fewest: 85 %)
    assert (each[sure] == r.counts[sure]).all(), what
    assert ((r.counts_lo <= each) & (each <= r.counts_hi)).all(), what
    assert n == int(each.sum())


@pytest.mark.parametrize("tf", [orc.linear_ramp_tf(0.8), mip_scenes.colour_ramp_tf()], ids=["ramp", "colour"])
def test_a_flipped_lerp_weight_stays_below_half_e0(tf):
    """The pixel is ONE classification: a flip of the 1.8 fixed-point weight moves it by (largest texel-to-texel step of
    the premultiplied colour) / 256."""
    tf = np.asarray(tf, dtype=np.float64).reshape(256, 4)
    pm = tf.copy()
    pm[:, :3] *= tf[:, 3:4]
    step = np.abs(np.diff(pm, axis=0)).max()
    assert step / 256.0 < scenes.E0 / 2.0, step


def test_sample_set_is_the_transparent_composite():
    """|S| per pixel = the samples ref64 composites with an all-transparent transfer function (brute force, 8-bit)."""
    s = mip_scenes.get("spin")
    s.tf = np.zeros((256, 4), dtype=np.float32)
    assert (ref64.render(s).counts == mip_scenes.ref("spin").counts).all()
    s = mip_scenes.get("clip")
    s.tf = np.zeros((256, 4), dtype=np.float32)
    assert (ref64.render(s).counts == mip_scenes.ref("clip").counts).all()


def test_the_rule_accepts_its_own_frame_and_has_teeth():
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin")
    assert mip_ref.check_frame(s, r, _own_frame(s, r))[0] == 0
    # a composite-mode frame of the same scene
    assert mip_ref.check_frame(s, r, ref64.render(s).frame)[0] > 0.5 * r.hit().sum()
    for mutation in mip_ref.MUTATIONS:
        q = mip_ref.render(s, _mutate=mutation)
        bad = mip_ref.check_frame(s, r, _own_frame(s, q))[0]
        print(mutation, bad)
        assert bad > 0, mutation


def test_passes_meet_in_the_running_maximum():
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin")
    n = s.n_nodes
    q = mip_ref.render_passes(s, [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)])
    assert (q.m == r.m).all() and (q.certain == r.certain).all() and (q.counts == r.counts).all()


def test_a_pixel_without_samples_must_stay_cleared():
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin")
    f = _own_frame(s, r)
    y, x = [int(v[0]) for v in np.nonzero(~r.hit())]
    f[y, x] = 1e-3
    assert mip_ref.check_frame(s, r, f)[0] == 1


# ---- the host build of the MIP per-ray code of vrc_core.h (tests/cpu_harness/mip_harness.cpp) ---------------------------
@pytest.mark.parametrize("form", [0, mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.GRID | mip_scenes.FIXED,
                                  mip_scenes.TRILINEAR, mip_scenes.GRID | mip_scenes.TRILINEAR])
@pytest.mark.parametrize("name", sorted(mip_scenes.SCENES))
def test_host_build_passes_the_rule(name, form):
    s = mip_scenes.get(name)
    r = mip_scenes.ref(name, 1 if form & mip_scenes.TRILINEAR else 0)
    each = np.zeros((s.H, s.W), dtype=np.int64)
    fb, n = mip_scenes.harness_render(s, form, per_pixel=each)
    bad, worst, amb = mip_ref.check_frame(s, r, fb)
    print("%s form %d: %d failing (worst excess %.3g), %d ambiguous" % (name, form, bad, worst, amb))
    assert bad == 0
    _counts_ok(r, each, n, name)
    if name in mip_scenes.COUNT:
        assert n == int(r.counts.sum())


@pytest.mark.parametrize("form", [mip_scenes.GRID | mip_scenes.FIXED, mip_scenes.TRILINEAR, 0])
@pytest.mark.parametrize("name", ["skip", "skip16", "spin", "axis"])
def test_host_build_skipping_and_uniform_bricks_change_no_pixel(name, form):
    s = mip_scenes.get(name)
    plain, n = mip_scenes.harness_render(s, form)
    uniform, nu = mip_scenes.harness_render(s, form | mip_scenes.UNIFORM)
    assert np.array_equal(plain, uniform) and n == nu
    for extra in (mip_scenes.SKIP, mip_scenes.SKIP | mip_scenes.UNIFORM):
        skipped, ns = mip_scenes.harness_render(s, form | extra)
        assert np.array_equal(plain, skipped)
        assert ns <= n
        if name in ("skip", "skip16"):
            assert ns < n
    k = s.n_nodes
    passes = [(0, k // 3), (k // 3, 2 * k // 3), (2 * k // 3, k)]
    three, n3 = mip_scenes.harness_render(s, (form & ~mip_scenes.GRID) | mip_scenes.SKIP, passes=passes)
    assert np.array_equal(plain, three)
    three, n3 = mip_scenes.harness_render(s, form & ~mip_scenes.GRID, passes=passes)
    assert np.array_equal(plain, three) and n3 == n


def test_host_build_16_bit_and_float_voxels():
    q, t, _ = mip_scenes.typed("float")
    for fm, form in ((0, mip_scenes.GRID | mip_scenes.FIXED), (1, mip_scenes.GRID | mip_scenes.TRILINEAR)):
        r = mip_scenes.typed_ref("float", fm)
        for scene in (q, t):
            each = np.zeros((q.H, q.W), dtype=np.int64)
            fb, n = mip_scenes.harness_render(scene, form, per_pixel=each)
            assert mip_ref.check_frame(q, r, fb)[0] == 0
            _counts_ok(r, each, n, "hash16")
            fb1, n1 = mip_scenes.harness_render(scene, form | mip_scenes.SKIP | mip_scenes.UNIFORM)
            assert np.array_equal(fb, fb1) and n1 <= n


@pytest.mark.parametrize("form", [0, mip_scenes.GRID, mip_scenes.TRILINEAR | mip_scenes.GRID])
def test_host_build_clamped_sampler_and_non_grid_cut(form):
    import nongrid
    s = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    r = mip_ref.render(s, filter_mode=1 if form & mip_scenes.TRILINEAR else 0)
    assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    each = np.zeros((s.H, s.W), dtype=np.int64)
    fb, n = mip_scenes.harness_render(s, form, per_pixel=each)
    assert mip_ref.check_frame(s, r, fb)[0] == 0
    _counts_ok(r, each, n, "nucleon")
    fb1, n1 = mip_scenes.harness_render(s, form | mip_scenes.SKIP | mip_scenes.UNIFORM)
    assert np.array_equal(fb, fb1) and n1 <= n
    if form == 0:
        s = nongrid.overlapping_scene("hash_parents_some_children", viewport=(36, 28))
        s.tf = orc.linear_ramp_tf(0.8)
        r = mip_ref.render(s)
        assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
        each = np.zeros((s.H, s.W), dtype=np.int64)
        fb, n = mip_scenes.harness_render(s, mip_scenes.FIXED, per_pixel=each)
        assert mip_ref.check_frame(s, r, fb)[0] == 0
        _counts_ok(r, each, n, "non-grid cut")
        fb1, n1 = mip_scenes.harness_render(s, mip_scenes.FIXED | mip_scenes.SKIP)
        assert np.array_equal(fb, fb1) and n1 <= n


@pytest.mark.parametrize("form", [mip_scenes.TRILINEAR, mip_scenes.TRILINEAR | mip_scenes.GRID])
def test_host_build_trilinear_skipping_with_large_negative_neighbours(form):
    """A float atlas whose few bright voxels sit among neighbours of -1e6 to -2.6e8: an interpolation's rounding error
    scales with its larger term, not with the slot's maximum, and the skipped frame must still be the marched one."""
    import copy
    s = mip_scenes.get("spin")
    t = copy.copy(s)
    v = s.atlas.astype(np.float32)
    t.atlas = np.ascontiguousarray(np.where(v > 150.0, v, np.float32(-1e6) * (v + np.float32(1.0))).astype(np.float32))
    assert (t.atlas > 0).sum() > 100 and (t.atlas < -1e6).sum() > 0.9 * t.atlas.size
    plain, n = mip_scenes.harness_render(t, form)
    skipped, ns = mip_scenes.harness_render(t, form | mip_scenes.SKIP)
    assert (plain[..., 3] > 0).sum() > 100
    assert np.array_equal(plain, skipped) and ns < n
