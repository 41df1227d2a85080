"""A shaded composite frame (VRC_OPT_SHADING = 1) on the CPU: the float64 restatement of tests/shade_ref.py under the
frozen rule of tests/scenes.py (it accepts its own frame and rejects deliberate misreadings of the shading), the honesty
of every scene and filter the GPU tests use (the host build of the per-ray code, tests/cpu_harness/shade_harness.cpp, is
inside the rule WITH its frame-level caps), the bitwise identities of the contract on the host build, a known answer, and
the stand-alone program that runs every sampler under the address and undefined-behaviour sanitizers.
tests/test_shade.py takes the same scenes to a GPU."""
import os
import subprocess

import numpy as np
import pytest

import mip_scenes
import orc
import scenes
import shade_ref
from shade_ref import AMBIENT, FIXED, GRID, TRILINEAR, UNIFORM, harness_render

SCENES = shade_ref.NAMES + ("nucleon",)


def _forms(filter_mode):
    t = TRILINEAR if filter_mode else 0
    return {"walk fixed": GRID | FIXED | t, "walk float": GRID | t, "reference order": FIXED | t}


def _same(a, b):
    return np.array_equal(a.frame, b.frame, equal_nan=True) and a.samples == b.samples and np.array_equal(a.each, b.each)


# ---- the rule has teeth -------------------------------------------------------------------------------------------------
def _rejected(s, r, filter_mode, mutate, what):
    bad = shade_ref.render(s, filter_mode=filter_mode, mutate=mutate)
    orc._LAST_SCENE = s
    try:
        scenes.assert_parity(bad.frame, r.frame, what, budget=r.budget)
    except AssertionError as e:
        print("%s: rejected (%s)" % (what, str(e)[:150]))
        return True
    return False


@pytest.mark.parametrize("name,filter_mode", [("nucleon", 0), ("nucleon", 1), ("spin", 0)])
def test_the_rule_accepts_its_own_frame_and_rejects_misreadings(name, filter_mode):
    s, r = shade_ref.scene(name), shade_ref.ref(name, filter_mode)
    shade_ref.check(s, r.frame, r, "%s filter %d: shade_ref's own frame" % (name, filter_mode))
    for m in ("no_shading", "ambient_ignored", "one_sided", "axes_swapped", "neighbour_x"):
        assert _rejected(s, r, filter_mode, m, "%s filter %d, %s" % (name, filter_mode, m)), m
    if filter_mode:
        assert _rejected(s, r, 1, "trilinear_floor_half", "%s trilinear, the gradient at floor(c - 0.5)" % name)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_the_rule_rejects_a_gradient_not_scaled_by_voxels_per_world(filter_mode):
    """(on a node whose voxels per world unit differ between the axes; on an isotropic one the scale cancels in s)"""
    s = shade_ref.scene("aniso")
    r = shade_ref.ref("aniso", filter_mode)
    shade_ref.check(s, r.frame, r, "aniso filter %d: shade_ref's own frame" % filter_mode)
    assert _rejected(s, r, filter_mode, "unscaled", "aniso filter %d, unscaled" % filter_mode)


def test_the_reference_keeps_alpha_and_count_of_ref64():
    """(the issue's observation: shading leaves the float64 alpha and the sample counts of tests/ref64.py bit for bit)"""
    import ref64
    for name, filter_mode in (("spin", 0), ("nucleon", 0), ("nucleon", 1)):
        s, r = shade_ref.scene(name), shade_ref.ref(name, filter_mode)
        plain = ref64.render(s, filter_mode=filter_mode)
        assert np.array_equal(plain.frame[..., 3], r.frame[..., 3]) and plain.samples == r.samples
        assert np.array_equal(plain.counts, r.counts)
        one = shade_ref.render(s, filter_mode=filter_mode, ambient=1.0)
        assert np.array_equal(one.frame, plain.frame)
        print("%s filter %d: mean rgb %.3g -> %.3g, mean budget %.3g -> %.3g" % (
            name, filter_mode, plain.frame[..., :3].mean(), r.frame[..., :3].mean(), plain.budget.mean(), r.budget.mean()))


# ---- honesty of the scenes: the host build, float32, every served form, WITH the caps ----------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_passes_the_rule_with_its_caps(name, filter_mode):
    s, r = shade_ref.scene(name), shade_ref.ref(name, filter_mode)
    for what, form in _forms(filter_mode).items():
        out = harness_render(s, form)
        shade_ref.check(s, out.frame, r, "%s filter %d %s" % (name, filter_mode, what))
        assert abs(out.samples - r.samples) <= 1e-4 * r.samples + 8, (what, out.samples, r.samples)


def _typed_host_scene(image):
    """what the host build renders of a typed image: uint16 as it is; int16 as the pool stores it (offset binary: the
    q scene itself); float as floats"""
    q, t, _ = mip_scenes.typed(image)
    return t if image == "float" else q


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_host_build_passes_the_rule_on_the_voxel_types(image, filter_mode):
    s, r = _typed_host_scene(image), shade_ref.typed_ref(image, filter_mode)
    for what, form in _forms(filter_mode).items():
        out = harness_render(s, form)
        shade_ref.check(mip_scenes.typed(image)[0], out.frame, r, "%s filter %d %s" % (image, filter_mode, what))


# ---- the identities of the contract, bit for bit, on the host build ----------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", SCENES)
def test_alpha_count_and_ambient_one(name, filter_mode):
    s = shade_ref.scene(name)
    for what, form in _forms(filter_mode).items():
        plain = harness_render(s, form, shading=0)
        lit = harness_render(s, form)
        assert np.array_equal(plain.frame[..., 3], lit.frame[..., 3]), what
        assert plain.samples == lit.samples and np.array_equal(plain.each, lit.each), what
        assert _same(plain, harness_render(s, form, ambient=1.0)), what
        if name not in ("axis",):
            assert not np.array_equal(plain.frame, lit.frame), "%s: the shading changes the colours" % what
        assert (lit.frame[..., :3] <= plain.frame[..., :3] + 1e-6).all(), "s <= 1"


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["axis", "skip", "skip16"])
def test_uniform_bricks(name, filter_mode):
    """mem:// bricks are constant with their overlap: the frame is the unshaded frame for any ambient, with the uniform
    shortcut and with the gradients gathered; on `skip` the shortcut changes no bit of the shaded frame"""
    s = shade_ref.scene(name)
    t = TRILINEAR if filter_mode else 0
    for loop in (GRID | FIXED, FIXED):
        lit = {u: harness_render(s, loop | t | (UNIFORM if u else 0), ambient=0.1) for u in (0, 1)}
        assert _same(lit[0], lit[1]), (loop, "uniform bricks on and off")
        if name == "axis":
            assert _same(lit[0], harness_render(s, loop | t, shading=0)), loop
        if name == "skip" and not filter_mode:
            assert lit[1].gathered.sum() < lit[0].gathered.sum(), "the uniform march gathers nothing"


def _transparent_below(s, level):
    t = np.array(s.tf, dtype=np.float32).reshape(256, 4).copy()
    t[:level, 3] = 0.0
    return np.ascontiguousarray(t)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "skip", "skip16", "nucleon"])
def test_the_gradient_skip_changes_no_bit(name, filter_mode):
    """A transfer function with a transparent range: rays with skipped samples and rays without, the same frame."""
    s = shade_ref.scene(name)
    saved = s.tf
    try:
        s.tf = _transparent_below(s, 100 if name != "nucleon" else 40)
        for what, form in _forms(filter_mode).items():
            on, off = harness_render(s, form, skip=1), harness_render(s, form, skip=0)
            assert _same(on, off), what
            # (the counts are of samples TAKEN: those of a group behind the early exit are taken and not composited)
            assert off.skipped.sum() == 0 and (off.gathered >= off.each).all()
            assert np.array_equal(on.gathered + on.skipped, off.gathered) and (on.gathered <= off.gathered).all()
            with_skip = int(((on.skipped > 0) & (on.each > 0)).sum())
            without = int(((on.skipped == 0) & (on.each > 0)).sum())
            print("%s filter %d %s: %d rays with a skipped sample, %d without" % (name, filter_mode, what, with_skip, without))
            if name == "spin":
                assert with_skip >= 100 and without >= 100
    finally:
        s.tf = saved


@pytest.mark.parametrize("name", ["spin", "skip"])
def test_three_passes_equal_one(name):
    s = shade_ref.scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    for filter_mode in (0, 1):
        t = TRILINEAR if filter_mode else 0
        for form in (FIXED | t, t):
            plain1, plain3 = harness_render(s, form, shading=0), harness_render(s, form, shading=0, passes=parts)
            if not _same(plain1, plain3):  # the precondition
                print("%s filter %d form %d: the unshaded passes differ from one pass; nothing to ask" % (name, filter_mode, form))
                continue
            assert _same(harness_render(s, form), harness_render(s, form, passes=parts)), (filter_mode, form)


# ---- a known answer -----------------------------------------------------------------------------------------------------
def test_the_known_answer_on_a_ramp():
    """One brick holds v = x: G = (k, 0, 0) on every interior sample, so s = ambient + (1 - ambient) |dir.x|: the frame's
    rgb over the unshaded rgb is that, on the pixels whose rays stay a voxel away from the brick's border."""
    s = scenes.nucleon_scene(viewport=(44, 36), spin=(0.6, 0.25))
    nid = s.ids[0]
    ramp = np.broadcast_to((40 + 4 * np.arange(41, dtype=np.uint8))[None, None, :], (41, 41, 41))
    s.bricks[nid] = np.ascontiguousarray(ramp)
    s.atlas[:] = 0
    s.atlas[:41, :41, :41] = ramp
    s.atlas[41:, :, :] = s.atlas[40:41, :, :]
    s.atlas[:, 41:, :] = s.atlas[:, 40:41, :]
    s.atlas[:, :, 41:] = s.atlas[:, :, 40:41]
    for filter_mode in (0, 1):
        for what, form in _forms(filter_mode).items():
            plain, lit = harness_render(s, form, shading=0), harness_render(s, form, ambient=AMBIENT)
            rays = lit.rays.astype(np.float64)
            want = AMBIENT + (1.0 - AMBIENT) * np.abs(rays[..., 0])
            # the pixels well inside the silhouette: those whose neighbours, three pixels deep, all hit too -- their rays
            # stay more than a voxel away from the brick's side faces.  (At the faces a ray enters and leaves through the
            # clamped difference is halved, which points the same way: s is the same there)
            hit = plain.frame[..., 3] > 0
            inner = hit.copy()
            for k in range(1, 4):
                for ax in (0, 1):
                    inner &= np.roll(hit, k, ax) & np.roll(hit, -k, ax)
            inner[:3], inner[-3:], inner[:, :3], inner[:, -3:] = False, False, False, False
            assert inner.sum() >= 50 and (plain.frame[..., 0][inner] > 1e-3).all()
            ratio = lit.frame[..., 0].astype(np.float64) / np.where(inner, plain.frame[..., 0], 1.0)
            worst = float(np.abs(ratio - want)[inner].max())
            print("ramp filter %d %s: %d pixels, s in [%.3f, %.3f], worst |ratio - s| %.2g"
                  % (filter_mode, what, int(inner.sum()), want[inner].min(), want[inner].max(), worst))
            assert worst <= 1e-5, what


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------
def test_every_sampler_as_a_stand_alone_program_under_the_sanitizers():
    """2 x 2 x 2 bricks of 8^3 with overlaps 0 and 1, atlases of exactly the slots' elements, rays along faces, edges
    and diagonals, every sampler and voxel type, every gradient gathered: no gather leaves the atlas."""
    exe = shade_ref.build(os.path.join(shade_ref.HERE, "cpu_harness", "shade_san"),
                          ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSHADE_HARNESS_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    rays, samples, gradients, skipped = [int(words[0][i]) for i in (1, 3, 5, 7)]
    assert rays > 5000 and samples > 100000 and gradients == samples and skipped == 0
