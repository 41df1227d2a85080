"""The depth of a composite frame (VRC_OPT_COMPOSITE_DEPTH) on the CPU: the float64 restatement of tests/cdepth_ref.py and
its acceptance rule (it accepts its own read-back and rejects deliberate misreadings), the caps on the rule's windows for
every case the GPU tests use, the host build of the per-ray code (tests/cpu_harness/cdepth_harness.cpp) under the rule, the
bitwise identities of the contract on the host build, a known answer, and the stand-alone program that runs every sampler
under the address and undefined-behaviour sanitizers.  tests/test_cdepth.py takes the same scenes to a GPU."""
import os
import subprocess

import numpy as np
import pytest

import cdepth_ref
import mip_scenes
import orc
import scenes
from cdepth_ref import FIXED, GRID, TRILINEAR, UNIFORM, harness_render, tau_of

CASES = cdepth_ref.rule_cases()
IDS = ["%s-%s-%d" % (n, "trilinear" if f else "nearest", k) for n, f, k in CASES]


def _forms(filter_mode):
    t = TRILINEAR if filter_mode else 0
    return {"walk fixed": GRID | FIXED | t, "walk float": GRID | t, "reference order": FIXED | t}


def _same_frame(a, b):
    return np.array_equal(a.frame, b.frame, equal_nan=True) and a.samples == b.samples and np.array_equal(a.each, b.each)


def _same_pair(a, b):
    return (np.array_equal(a.depths, b.depths) and np.array_equal(a.bits, b.bits) and np.array_equal(a.counts, b.counts))


def _equivalence(frame, depths, k, what):
    """isfinite(D) <=> alpha >= tau, on every pixel"""
    assert np.array_equal(np.isfinite(depths), frame[..., 3] >= tau_of(k)), what


def _halves(s):
    return [(0, s.n_nodes // 2), (s.n_nodes // 2, s.n_nodes)]


# ---- the rule has teeth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,filter_mode,k", [("spin", 0, 500), ("spin", 1, 100), ("nucleon", 1, 500), ("clip", 0, 100)])
def test_the_rule_accepts_its_own_read_back_and_rejects_misreadings(name, filter_mode, k):
    r = cdepth_ref.ref(name, filter_mode, k)
    tol = cdepth_ref.tolerance(cdepth_ref.scene(name), filter_mode)
    cdepth_ref.assert_rule(r, *r.own(), "%s filter %d tau %d: cdepth_ref's own read-back" % (name, filter_mode, k), tol=tol)
    assert r.own_hit.sum() >= 300
    for m in ("off_by_one", "before_composite", "segment_start", "first_opaque"):
        bad, _ = cdepth_ref.check(r, *r.own(mutate=m), tol=tol)
        print("%s filter %d tau %d, %s: %d pixels rejected" % (name, filter_mode, k, m, bad))
        assert bad >= 50, m


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_the_rule_rejects_a_depth_overwritten_by_a_later_pass(filter_mode):
    s = cdepth_ref.scene("spin")
    one, two = cdepth_ref.render_passes(s, tau_of(100), _halves(s), filter_mode=filter_mode)
    tol = cdepth_ref.tolerance(s, filter_mode)
    cdepth_ref.assert_rule(two, *two.own(), "spin in two passes, filter %d" % filter_mode, tol=tol)
    again = int((one.own_hit & np.isfinite(two.last_t)).sum())
    bad, _ = cdepth_ref.check(two, *two.own(mutate="later_pass", earlier=one), tol=tol)
    print("filter %d: %d pixels crossed in the first pass and are sampled in the second; %d rejected" % (filter_mode, again, bad))
    assert again >= 50 and bad >= 50


# ---- the caps: conditions on the reference alone, for every (scene, filter, tau) the GPU tests hold to the rule ---------------
@pytest.mark.parametrize("name,filter_mode,k", CASES, ids=IDS)
def test_the_windows_stay_inside_their_caps(name, filter_mode, k):
    r = cdepth_ref.ref(name, filter_mode, k)
    share, longest = r.multi_share(), r.longest()
    print("%s filter %d tau %d: %d crossing pixels, %.1f %% with more than one candidate, longest window %d samples"
          % (name, filter_mode, k, int(r.opened.sum()), 100.0 * share, longest))
    assert r.opened.sum() >= 300
    assert share <= cdepth_ref.MAX_MULTI and longest <= cdepth_ref.MAX_WINDOW


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_windows_of_the_typed_scenes_stay_inside_their_caps(image, filter_mode):
    for k in cdepth_ref.RULE_TAUS:
        r = cdepth_ref.typed_ref(image, filter_mode, k)
        print("%s filter %d tau %d: %d crossing pixels, %.1f %% with more than one candidate, longest window %d"
              % (image, filter_mode, k, int(r.opened.sum()), 100.0 * r.multi_share(), r.longest()))
        assert r.opened.sum() >= 100
        assert r.multi_share() <= cdepth_ref.MAX_MULTI and r.longest() <= cdepth_ref.MAX_WINDOW


# ---- the host build, float32, every served form, under the rule ------------------------------------------------------------
@pytest.mark.parametrize("name,filter_mode,k", CASES, ids=IDS)
def test_the_host_build_passes_the_rule(name, filter_mode, k):
    s, r = cdepth_ref.scene(name), cdepth_ref.ref(name, filter_mode, k)
    for what, form in _forms(filter_mode).items():
        out = harness_render(s, form, k)
        cdepth_ref.assert_rule(r, out.values, out.counts, out.depths, "%s filter %d tau %d %s" % (name, filter_mode, k, what),
                               tol=cdepth_ref.tolerance(s, filter_mode))


def _typed_host_scene(image):
    """what the host build renders of a typed image: uint16 as it is; int16 as the pool stores it (offset binary: the
    q scene itself); float as floats"""
    q, t, _ = mip_scenes.typed(image)
    return t if image == "float" else q


def _typed_to_q(image):
    """the host build's V of the float image back in q's units (the integer images are rendered as q itself)"""
    import voxel_types
    if image != "float":
        return lambda x: x
    im = voxel_types.IMAGES[image]
    return lambda x: (x - im.a) / im.b


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_host_build_passes_the_rule_on_the_voxel_types(image, filter_mode):
    s, q = _typed_host_scene(image), mip_scenes.typed(image)[0]
    exact = not filter_mode and image != "float"
    tol = 0.0 if exact else scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    for k in cdepth_ref.RULE_TAUS:
        r = cdepth_ref.typed_ref(image, filter_mode, k)
        for what, form in _forms(filter_mode).items():
            out = harness_render(s, form, k)
            cdepth_ref.assert_rule(r, _typed_to_q(image)(out.values.astype(np.float64)), out.counts, out.depths,
                                   "%s filter %d tau %d %s" % (image, filter_mode, k, what), tol=tol)


# ---- the identities of the contract, bit for bit, on the host build ----------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", cdepth_ref.RULE_SCENES + ("nucleon", "skip", "skip16"))
def test_the_frame_is_untouched_and_the_depth_is_finite_where_alpha_crossed(name, filter_mode):
    s = cdepth_ref.scene(name)
    for what, form in _forms(filter_mode).items():
        plain = harness_render(s, form, 0)
        crossed = []
        for k in cdepth_ref.IDENTITY_TAUS:
            out = harness_render(s, form, k)
            assert _same_frame(plain, out), (what, k)
            _equivalence(out.frame, out.depths, k, (what, k))
            assert np.array_equal(out.counts, np.isfinite(out.depths).astype(np.uint32)), (what, k)
            crossed.append(int(out.counts.sum()))
        assert crossed == sorted(crossed, reverse=True) and crossed[0] > 0, (what, crossed)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16"])
def test_uniform_bricks_change_no_bit(name, filter_mode):
    s = cdepth_ref.scene(name)
    t = TRILINEAR if filter_mode else 0
    for loop in (GRID | FIXED, FIXED, GRID):
        for k in cdepth_ref.IDENTITY_TAUS:
            off, on = harness_render(s, loop | t, k), harness_render(s, loop | t | UNIFORM, k)
            assert _same_frame(off, on) and _same_pair(off, on), (loop, k)
            assert on.counts.sum() > 0 or k == 999


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "skip"])
def test_two_passes(name, filter_mode):
    """after each pass: the equivalence; the first pass's finite D is not touched by the second; and the whole frame, if
    the plain passes add up to the plain frame, has the pair of one pass"""
    s = cdepth_ref.scene(name)
    t = TRILINEAR if filter_mode else 0
    for form in (FIXED | t, GRID | FIXED | t, UNIFORM | FIXED | t):
        for k in (100, 500):
            two = harness_render(s, form, k, passes=_halves(s))
            (f1, d1), (f2, d2) = two.after
            _equivalence(f1, d1, k, (form, k, "first pass"))
            _equivalence(f2, d2, k, (form, k, "second pass"))
            kept = np.isfinite(d1)
            assert kept.sum() > 50 and np.array_equal(d1[kept], d2[kept]), (form, k)
            if name == "spin":
                assert (np.isfinite(d2) & ~kept).sum() > 0, "the second pass crosses somewhere too"
            assert _same_frame(two, harness_render(s, form, 0, passes=_halves(s))), (form, k)


# ---- a known answer -----------------------------------------------------------------------------------------------------
def test_the_known_answer_on_a_constant_volume():
    """The centre ray runs down the z axis through two bricks that hold one value: every sample adds the same alpha' a, so
    the alpha after i samples is the chain A <- A + a (1 - A), computed here by hand; the first i with A >= tau is the
    crossing, brick 0 takes the first n0 = ceil(depth of a brick / step) samples, and D = tNear_b + j_b x step with the
    bricks' tNear from the eye's distance to their faces.  Thresholds the chain passes within 1e-5 are left out."""
    value = 200
    vol = np.full((32, 16, 16), value, dtype=np.uint8)
    s = orc.build_scene(voxels=(16, 16, 32), block=16, viewport=(8, 8), spr=64, volume=vol, alpha=0.8)
    assert s.n_nodes == 2
    y, x = s.H // 2, s.W // 2
    step = 1.0 / float(s.render.samplesPerRay)
    eye_z = float(s.view.eyePosition[2])
    near = [eye_z - (float(s.nodes[b].aabbMin[2]) + float(s.nodes[b].aabbSize[2])) for b in range(2)]
    assert near[0] < near[1], "front to back"
    n0 = int(np.ceil(float(s.nodes[0].aabbSize[2]) / step - 1e-9))
    total = n0 + int(np.ceil(float(s.nodes[1].aabbSize[2]) / step - 1e-9))
    a = cdepth_ref.table_alpha(s, value)
    chain, acc = [], 0.0
    for _ in range(total):
        acc += a * (1.0 - acc)
        chain.append(acc)
    checked = 0
    for k in (50, 100, 300, 500, 700, 900, 990):
        tau = float(tau_of(k))
        j = next((i for i, v in enumerate(chain) if v >= tau), None)
        if any(abs(v - tau) <= 1e-5 for v in chain):
            continue
        want = np.inf if j is None else (near[0] + j * step if j < n0 else near[1] + (j - n0) * step)
        for uniform in (0, UNIFORM):
            for what, form in _forms(0).items():
                out = harness_render(s, form | uniform, k)
                d = float(out.depths[y, x])
                if j is None:
                    assert np.isposinf(d) and out.counts[y, x] == 0, (k, what)
                else:
                    assert out.counts[y, x] == 1 and out.values[y, x] == value, (k, what)
                    assert abs(d - want) <= 0.25 * step, (k, what, uniform, j, d, want)
        checked += 1
        print("tau %d: crossing at sample %s of %d (brick 0 takes %d), D %.6f" % (k, j, total, n0, want))
    assert checked >= 4


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------
def test_every_sampler_as_a_stand_alone_program_under_the_sanitizers():
    """2 x 2 x 2 bricks of 8^3 with overlaps 0 and 1, atlases of exactly the slots' elements, rays along faces, edges
    and diagonals, every sampler and voxel type: no gather leaves the atlas, and every ray's state agrees with its alpha."""
    exe = cdepth_ref.build(os.path.join(cdepth_ref.HERE, "cpu_harness", "cdepth_san"),
                           ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DCDEPTH_HARNESS_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    rays, samples, crossings = [int(words[0][i]) for i in (1, 3, 5)]
    assert rays > 5000 and samples > 100000 and crossings > 1000
