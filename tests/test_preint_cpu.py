"""A pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1) on the CPU: the float64 restatement of
tests/preint_ref.py under the frozen rule of tests/scenes.py (it accepts its own frame and rejects deliberate misreadings
of the contract), the honesty of every scene and filter the GPU tests use (the host build of the per-ray code,
tests/cpu_harness/preint_harness.cpp, is inside the rule WITH its frame-level caps), the host build of the table builder
against preint_ref's own quadrature, the grouped march against a one-sample-at-a-time loop, the bitwise identities of the
contract, and the stand-alone program that runs every sampler under the address and undefined-behaviour sanitizers.
tests/test_preint.py takes the same scenes to a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mip_scenes
import orc
import preint_ref
import scenes
from preint_ref import FIXED, GRID, TEXEL, TRILINEAR, UNIFORM, VALUE, harness_render

SCENES = preint_ref.NAMES


def _forms(filter_mode):
    t = TRILINEAR if filter_mode else 0
    return {"walk fixed": GRID | FIXED | t, "walk float": GRID | t, "reference order": FIXED | t}


def _same(a, b):
    return np.array_equal(a.frame, b.frame, equal_nan=True) and a.samples == b.samples and np.array_equal(a.each, b.each)


# ---- the rule has teeth -------------------------------------------------------------------------------------------------
def _rejected(s, r, filter_mode, mutate, what):
    bad = preint_ref.render(s, filter_mode=filter_mode, mutate=mutate)
    orc._LAST_SCENE = s
    try:
        scenes.assert_parity(bad.frame, r.frame, what, budget=r.budget)
    except AssertionError as e:
        print("%s: rejected (%s)" % (what, str(e)[:150]))
        return True
    return False


#: the scenes on which a misreading can show: `peak` is the case the feature exists for; `spin` and `clip` have several
#: bricks per ray, a colour ramp (spin) and 96 / 128 samples per ray against 32 (k = 1/3, 1/4); every scene has k != 1
TEETH = [
    ("peak", 0, ("no_preintegration", "front_only", "mean_of_classifications", "alpha_mean", "carried_across_visits",
                 "colour_unweighted", "correction_ignored")),
    ("peak", 1, ("no_preintegration", "front_only", "mean_of_classifications", "alpha_mean", "carried_across_visits",
                 "colour_unweighted", "correction_ignored")),
    ("spin", 0, ("no_preintegration", "carried_across_visits", "front_only", "mean_of_classifications", "colour_unweighted",
                 "correction_ignored")),
    ("clip", 1, ("no_preintegration", "carried_across_visits", "front_only", "correction_ignored")),
    ("nucleon", 0, ("no_preintegration", "front_only", "correction_ignored")),
]


@pytest.mark.parametrize("name,filter_mode,mutations", TEETH, ids=["%s-%d" % (t[0], t[1]) for t in TEETH])
def test_the_rule_accepts_its_own_frame_and_rejects_misreadings(name, filter_mode, mutations):
    s, r = preint_ref.scene(name), preint_ref.ref(name, filter_mode)
    preint_ref.check(s, r.frame, r, "%s filter %d: preint_ref's own frame" % (name, filter_mode))
    for m in mutations:
        assert _rejected(s, r, filter_mode, m, "%s filter %d, %s" % (name, filter_mode, m)), m


def test_peak_is_the_case_the_feature_exists_for():
    """consecutive samples straddle the spike: the plain frame misses most of what the pre-integrated frame shows"""
    import ref64
    s = preint_ref.scene("peak")
    plain, pre = ref64.render(s), preint_ref.ref("peak", 0)
    hit = pre.frame[..., 3] > 1e-3
    assert hit.sum() >= 200
    # every ray through the ball crosses the shell of the spike's values twice: the pre-integrated opacity is even ...
    a = pre.frame[..., 3][hit]
    rough = np.abs(plain.frame[..., 3] - pre.frame[..., 3])[hit]
    print("peak: %d rays, pre-integrated alpha %.3f +- %.3f, plain differs by mean %.3f max %.3f"
          % (hit.sum(), a.mean(), a.std(), rough.mean(), rough.max()))
    assert rough.mean() > 0.05 and rough.max() > 0.3   # ... and the plain frame's rings are not


# ---- honesty of the scenes: the host build, float32, every served form, WITH the caps -------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_passes_the_rule_with_its_caps(name, filter_mode):
    s, r = preint_ref.scene(name), preint_ref.ref(name, filter_mode)
    for what, form in _forms(filter_mode).items():
        out = harness_render(s, form)
        preint_ref.check(s, out.frame, r, "%s filter %d %s" % (name, filter_mode, what))
        assert abs(out.samples - r.samples) <= 1e-4 * r.samples + 8, (what, out.samples, r.samples)


def _typed_host_scene(image):
    """what the host build renders of a typed image: uint16 as it is; int16 as the pool stores it (offset binary: the
    q scene itself); float as floats"""
    q, t, _ = mip_scenes.typed(image)
    return t if image == "float" else q


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_host_build_passes_the_rule_on_the_voxel_types(image, filter_mode):
    s, r = _typed_host_scene(image), preint_ref.typed_ref(image, filter_mode)
    for what, form in _forms(filter_mode).items():
        out = harness_render(s, form)
        preint_ref.check(mip_scenes.typed(image)[0], out.frame, r, "%s filter %d %s" % (image, filter_mode, what))


# ---- the table ------------------------------------------------------------------------------------------------------------
def _ramp_tf():
    return mip_scenes.colour_ramp_tf()


def _crossing_tf():
    """alpha climbs through 255/256 in the middle of texel intervals, stays above and comes back"""
    tf = mip_scenes.colour_ramp_tf().copy()
    tf[:, 3] = 0.1
    tf[60:64, 3] = (0.5, 0.99, 1.0, 0.999)
    tf[64:70, 3] = 1.0
    tf[70:73, 3] = (0.9985, 0.4, 0.0)
    tf[200, 3] = 1.0   # a one-texel spike to full opacity
    return np.ascontiguousarray(tf.astype(np.float32))


TABLE_CASES = {
    "ramp": (_ramp_tf, 0.0, 255.0, 32.0 / 96.0),
    "peak": (preint_ref.peak_tf, 0.0, 255.0, 32.0 / 24.0),
    "crossing": (_crossing_tf, 0.0, 255.0, 1.0),
    "crossing, a range inside the values": (_crossing_tf, 20.5, 200.25, 0.25),
}


@pytest.mark.parametrize("kind", [VALUE, TEXEL], ids=["value", "texel"])
@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_the_host_builder_against_the_reference_quadrature(case, kind):
    make, r0, r1, k = TABLE_CASES[case]
    tf = make()
    k32 = float(np.float32(k))
    got = preint_ref.harness_table(tf, r0, r1, k32, kind).astype(np.float64)
    want = preint_ref.table(tf, r0, r1, k32, kind)
    off = ~np.eye(256, dtype=bool)
    worst = float(np.abs(got - want)[off].max())
    print("%s kind %d: worst |builder - quadrature| off the diagonal %.3g; largest entry %.3f" % (case, kind, worst, want.max()))
    assert worst <= 1e-6
    # symmetric bit for bit
    assert np.array_equal(got, got.transpose(1, 0, 2))
    if kind == TEXEL:  # the diagonal: the plain classification at the texel, exact weights
        d = np.arange(256)
        assert float(np.abs(got[d, d] - want[d, d]).max()) <= 1e-6


@pytest.mark.parametrize("frac_bits", [8, 0])
def test_the_value_indexed_diagonal_is_the_classified_table(frac_bits):
    for case in ("ramp", "crossing, a range inside the values"):
        make, r0, r1, k = TABLE_CASES[case]
        tf = make()
        got = preint_ref.harness_table(tf, r0, r1, np.float32(k), VALUE, frac_bits=frac_bits)
        lut = preint_ref.harness_lut(tf, r0, r1, np.float32(k), frac_bits=frac_bits)
        d = np.arange(256)
        assert np.array_equal(got[d, d].view(np.uint32), lut.view(np.uint32)), case
    # (the two quantisations differ somewhere: the test can tell them apart)
    make, r0, r1, k = TABLE_CASES["crossing, a range inside the values"]
    assert not np.array_equal(preint_ref.harness_lut(make(), r0, r1, np.float32(k), frac_bits=8),
                              preint_ref.harness_lut(make(), r0, r1, np.float32(k), frac_bits=0))


@pytest.mark.parametrize("kind", [VALUE, TEXEL], ids=["value", "texel"])
def test_a_constant_transfer_function_gives_the_plain_entry_everywhere(kind):
    tf = np.tile(np.array([0.3, 0.6, 0.9, 0.4], dtype=np.float32), (256, 1))
    k = float(np.float32(32.0 / 96.0))
    got = preint_ref.harness_table(tf, 0.0, 255.0, k, kind).astype(np.float64)
    alpha = 1.0 - (1.0 - float(np.float32(0.4))) ** k
    plain = np.array([float(np.float32(0.3)) * alpha, float(np.float32(0.6)) * alpha, float(np.float32(0.9)) * alpha, alpha])
    assert float(np.abs(got - plain).max()) <= 1e-6


def test_the_known_answer_of_a_step_onto_a_spike():
    """alpha 0 at texel m and a1 <= 255/256 at texel m + 1: over [m, m + 1], taubar = 1 + (1 - a1) ln(1 - a1) / a1"""
    m = 77
    for a1 in (0.25, 0.9, 255.0 / 256.0):
        tf = np.zeros((256, 4), dtype=np.float32)
        tf[:, :3] = 0.5
        tf[m + 1, 3] = a1
        a1 = float(tf[m + 1, 3])
        for k in (1.0, 0.25):
            got = preint_ref.harness_table(tf, 0.0, 255.0, k, TEXEL).astype(np.float64)
            taubar = 1.0 + (1.0 - a1) * np.log(1.0 - a1) / a1
            want = 1.0 - np.exp(-k * taubar)
            print("a1 %.4f k %.2f: alpha %.9f, known %.9f" % (a1, k, got[m, m + 1, 3], want))
            assert abs(got[m, m + 1, 3] - want) <= 1e-6 and abs(got[m + 1, m, 3] - want) <= 1e-6
            assert np.abs(got[m, m + 1, :3] - 0.5 * want).max() <= 1e-6
            assert (got[:m, :m] == 0.0).all()   # int tau = 0: E = 0


# ---- the march, bit for bit against a one-sample-at-a-time loop over the same table ------------------------------------------
def _groups():
    p, t = C.c_int(0), C.c_int(0)
    preint_ref.harness().preint_harness_groups(C.byref(p), C.byref(t))
    return p.value, t.value


@pytest.mark.parametrize("voxel_bytes,linear", [(1, 0), (2, 0), (1, 1), (2, 1)],
                         ids=["u8 point", "u16 point", "u8 trilinear", "u16 trilinear"])
def test_the_grouped_march_is_the_sample_by_sample_loop(voxel_bytes, linear):
    """segments of 1 ... 3 G + 2 samples; transfer functions from nearly transparent (no ray leaves early) to nearly
    opaque with k = 2 (a ray leaves at its visit's first sample)"""
    group = _groups()[0 if (voxel_bytes == 1 and not linear) else 1]
    exits = np.zeros(64, dtype=np.uint32)
    H = preint_ref.harness()
    H.preint_harness_march.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_void_p]
    sweep = [(0.01, 1.0)] + [(0.1 + 0.03 * j, 1.0) for j in range(50)] + [(1.6 + 0.2 * j, 1.0) for j in range(24)] + [
        (20.0, 1.0), (1.3, 2.0), (4.0, 2.0), (20.0, 2.0)]
    for alpha, k in sweep:
        rc = H.preint_harness_march(voxel_bytes, linear, alpha, k, 3 * group + 2, exits.ctypes.data)
        assert rc == 0, "alpha %.2f k %.1f: the marches differ on a segment of %d samples" % (alpha, k, rc)
    at = set(int(i) for i in np.nonzero(exits)[0])
    print("group %d; rays left early at samples %s" % (group, sorted(at)))
    assert 1 in at, "a ray that leaves at the first sample of its visit"
    assert group in at and group + 1 in at, "the last sample of a group and the first of the next"
    assert any(1 < i < group for i in at), "a sample in the middle of a group"
    assert any(i > 2 * group for i in at), "a sample of the tail"


# ---- the identities of the contract, bit for bit, on the host build --------------------------------------------------------
@pytest.mark.parametrize("loop", [GRID | FIXED, GRID, FIXED], ids=["walk fixed", "walk float", "reference order"])
def test_bricks_of_one_value_give_the_plain_frame(loop):
    """mem:// bricks are constant with their overlap (8-bit, point samples): every step is E(v, v), a copy of the
    classified table's entry -- the plain frame and count, with the uniform march and without it"""
    s = preint_ref.scene("axis")
    for frac_bits in (8, 0):
        plain = harness_render(s, loop, preint=0, frac_bits=frac_bits)
        assert plain.samples > 0 and float(plain.frame[..., 3].max()) > 0.1
        for u in (0, UNIFORM):
            assert _same(plain, harness_render(s, loop | u, frac_bits=frac_bits)), (frac_bits, u)


@pytest.mark.parametrize("name", ["spin", "peak", "clip"])
def test_uniform_bricks_change_no_bit(name):
    s = preint_ref.scene(name)
    for loop in (GRID | FIXED, FIXED):
        assert _same(harness_render(s, loop), harness_render(s, loop | UNIFORM)), loop


@pytest.mark.parametrize("name", ["spin", "peak"])
def test_three_passes_equal_one(name):
    s = preint_ref.scene(name)
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    asked = 0
    for filter_mode in (0, 1):
        t = TRILINEAR if filter_mode else 0
        for form in (FIXED | t, t):
            plain1, plain3 = harness_render(s, form, preint=0), harness_render(s, form, preint=0, passes=parts)
            if not _same(plain1, plain3):  # the precondition
                print("%s filter %d form %d: the plain passes differ from one pass; nothing to ask" % (name, filter_mode, form))
                continue
            asked += 1
            assert _same(harness_render(s, form), harness_render(s, form, passes=parts)), (filter_mode, form)
    assert asked >= 1


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "clip", "nucleon"])
def test_the_sample_count_is_the_plain_frames_where_no_ray_ends_early(name, filter_mode):
    """a transfer function whose largest classified opacity keeps every ray below 0.999: the samples are the plain
    frame's, one for one"""
    s = preint_ref.scene(name)
    saved = s.tf
    try:
        tf = np.array(saved, dtype=np.float32).reshape(256, 4).copy()
        tf[:, 3] *= np.float32(0.02)
        s.tf = np.ascontiguousarray(tf)
        for what, form in _forms(filter_mode).items():
            plain, pre = harness_render(s, form, preint=0), harness_render(s, form)
            assert float(plain.frame[..., 3].max()) < 0.9 and float(pre.frame[..., 3].max()) < 0.9
            assert plain.samples == pre.samples and np.array_equal(plain.each, pre.each), what
            assert not np.array_equal(plain.frame, pre.frame), what
    finally:
        s.tf = saved


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------
def test_every_sampler_as_a_stand_alone_program_under_the_sanitizers():
    """2 x 2 x 2 bricks of 8^3 with overlaps 0 and 1, atlases of exactly the slots' elements, tables of exactly 256 x 256
    entries, rays along faces, edges and diagonals, every sampler and voxel type: no gather leaves the atlas, no read the
    table."""
    exe = preint_ref.build(os.path.join(preint_ref.HERE, "cpu_harness", "preint_san"),
                           ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DPREINT_HARNESS_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    words = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rays ")]
    assert len(words) == 1
    rays, samples, marches = int(words[0][1]), int(words[0][3]), int(words[0][7])
    assert rays > 5000 and samples > 100000 and marches == 0
