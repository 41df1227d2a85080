"""The depth of a MIP frame (VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE) on the CPU: the acceptance rule of
tests/depth_ref.py (it accepts the reference's own frame and rejects deliberate misreadings), the condition that keeps it
honest on every scene used (at most half of the hit pixels have more than one candidate depth), and the host build of the
depth-tracking per-ray code (tests/cpu_harness/depth_harness.cpp) held to the rule, to a known answer and to the bitwise
identities of the contract.  tests/test_depth.py takes the same scenes to a GPU."""
import itertools

import numpy as np
import pytest

import depth_ref
import mip_scenes
import nonfinite
import scenes
from depth_ref import FOLD_MAX, FOLD_MIN
from mip_scenes import FIXED, GRID, SKIP, TRILINEAR, UNIFORM
from ref64 import _slab, _vec

FOLDS = {"max": FOLD_MAX, "min": FOLD_MIN}
NAMES = ("axis", "spin", "inside", "clip", "skip", "skip16")
from depth_ref import BLOCK_VALUE, BLOCK_XY, MULTI_CAP, NEAR_FAR_Z, ref, scene, tolerance, two_blocks  # noqa: E402


def _forms(filter_mode):
    t = TRILINEAR if filter_mode else 0
    return {"walk": GRID | FIXED | SKIP | UNIFORM | t, "reforder": t, "reforder skip": SKIP | UNIFORM | t}


# ---- the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_the_rule_accepts_its_own_frame_and_rejects_misreadings(fold):
    """The reference's own pair of every pixel passes; a depth taken at the last of the tied samples, at the segment's
    start, one sample late, or in a later brick with an equal M does not."""
    cases = {"spin": ref("spin", 0, FOLDS[fold]),
             "two blocks": depth_ref.render(two_blocks(fold == "min"), fold=FOLDS[fold])}
    for name, r in cases.items():
        assert depth_ref.check(r, *r.own()) == (0, 0.0), name
        for m in depth_ref.MUTATIONS:
            bad = depth_ref.check(r, *r.own(m))[0]
            print("%s %s, %s: %d of %d pixels rejected" % (name, fold, m, bad, int(r.certain.sum())))
            if name == "two blocks" and m == "segment_start":
                continue  # (along the axis the blocks' rays may well start a segment on the block)
            assert bad > 0, (name, m)
    # the later brick: every ray through both blocks
    r = cases["two blocks"]
    both = _through_both(two_blocks(fold == "min"), r)
    _, _, d = r.own("later_brick")
    _, _, d0 = r.own()
    assert both.sum() >= 1 and (d[both] > d0[both] + 0.5).all()


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_the_host_build_passes_the_rule(fold, name, filter_mode):
    s, r = scene(name, filter_mode, FOLDS[fold]), ref(name, filter_mode, FOLDS[fold])
    share = depth_ref.multi_share(r)
    print("%s %s filter %d: %d hit pixels, %.3f of them with more than one candidate depth" % (name, fold, filter_mode, int(r.hit().sum()), share))
    assert share <= MULTI_CAP
    assert int(r.hit().sum()) > 100
    tol = tolerance(s, filter_mode)
    first = None
    for what, form in _forms(filter_mode).items():
        fb, n, v, c, d, xyz = depth_ref.harness_render(s, form, FOLDS[fold])
        bad, worst = depth_ref.check(r, v, c, d, tol)
        print("  %s: %d failing pixels, worst depth error %.2g steps" % (what, bad, worst))
        assert bad == 0, what
        assert np.isposinf(d[~r.hit()]).all(), "an empty S reads +infinity"
        # the frame is the classification of M with or without the depth: bit for bit
        fb0, n0, v0, c0, _, _ = depth_ref.harness_render(s, form, FOLDS[fold], depth=0)
        assert np.array_equal(fb, fb0) and np.array_equal(v, v0) and np.array_equal(c, c0) and n0 <= n, what
        # every form: the same pairs (the depth labels the sample's index, whatever the stepping)
        if first is None:
            first = (fb, v, c, d)
        assert all(np.array_equal(a, b) for a, b in zip(first, (fb, v, c, d))), what
        # origin + D x dir, where D is finite
        fin = np.isfinite(d)
        o = _vec(s.view.eyePosition, 3)
        want = o + d[fin][:, None].astype(np.float64) * r.dir[fin]
        assert np.abs(xyz[fin] - want).max() <= 1e-5
        # ... and bit for bit origin + D x dir recomputed in float32 from the ray and the read-back D
        assert np.array_equal(xyz[fin], depth_ref.xyz32(d, depth_ref.harness_render.interval)[fin])


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_nan_voxels_never_hold_the_depth(fold):
    """tests/nonfinite.py's float volume with one brick all NaN: a NaN sample equals no M, and a ray that takes nothing
    else has M = -/+infinity and D = +infinity with a count of 1."""
    case = nonfinite.case("allnan_brick")
    q, t = case.mq, case.mt
    tol = scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
    r = depth_ref.render(q, fold=FOLDS[fold], tol=tol, nan_q=nonfinite.Q_NAN)
    assert depth_ref.multi_share(r) <= MULTI_CAP
    v0, c0, d0 = r.own()
    all_nan = r.certain & np.isinf(v0) & ~r.multi()
    assert all_nan.sum() > 50 and np.isposinf(d0[all_nan]).all()
    im = nonfinite.IMAGE
    out = {}
    for what, form in _forms(0).items():
        fb, n, v, c, d, _ = depth_ref.harness_render(t, form, FOLDS[fold])
        with np.errstate(invalid="ignore"):
            qv = (v.astype(np.float64) - im.a) / im.b
        bad, worst = depth_ref.check(r, qv, c, d, tol)
        print("%s %s: %d failing pixels, %d all-NaN rays" % (fold, what, bad, int(all_nan.sum())))
        assert bad == 0, what
        assert np.isposinf(d[all_nan]).all() and (c[all_nan] == 1).all()
        assert np.isinf(v[all_nan]).all() and ((v[all_nan] > 0) == (fold == "min")).all()
        out[what] = (fb, v, c, d)
    for what in out:
        assert all(np.array_equal(a, b) for a, b in zip(out["walk"], out[what])), what


# ---- the known answer ---------------------------------------------------------------------------------------------------
def _block_box(s, z0, shrink=0.0):
    lo, hi = _vec(s.view.aabbMin, 3), _vec(s.view.aabbMax, 3)
    v0 = np.array([BLOCK_XY + shrink, BLOCK_XY + shrink, z0 + shrink]) / 64.0
    v1 = np.array([BLOCK_XY + 4.0 - shrink, BLOCK_XY + 4.0 - shrink, z0 + 4.0 - shrink]) / 64.0
    return lo + v0 * (hi - lo), lo + v1 * (hi - lo)


def _through_both(s, r):
    """pixels whose rays run through the interior columns of both blocks (half a voxel inside their sides)"""
    d = r.dir.reshape(-1, 3)
    ok = np.ones(d.shape[0], dtype=bool)
    for z0 in NEAR_FAR_Z:
        b0, b1 = _block_box(s, z0)
        tn, tf = _slab(r.origin, d, b0, b1)
        for t in (tn, tf):  # inside the shrunk cross-section where it enters and where it leaves the block
            p = r.origin + d * t[:, None]
            s0, s1 = _block_box(s, z0, 0.5)
            ok &= (tf > tn) & (p[:, 0] > s0[0]) & (p[:, 0] < s1[0]) & (p[:, 1] > s0[1]) & (p[:, 1] < s1[1])
    return ok.reshape(r.H, r.W)


@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_two_blocks_on_one_ray_report_the_nearer(fold):
    s = two_blocks(fold == "min")
    r = depth_ref.render(s, fold=FOLDS[fold])
    both = _through_both(s, r)
    assert both.sum() >= 1
    d64 = r.dir.reshape(-1, 3)
    entry = {}
    for z0 in NEAR_FAR_Z:
        tn, _ = _slab(r.origin, d64, *_block_box(s, z0))
        entry[z0] = tn.reshape(r.H, r.W)[both]
    near, far = np.minimum(entry[50], entry[10]), np.maximum(entry[50], entry[10])
    assert (far - near > 0.5).all()
    want = BLOCK_VALUE if fold == "max" else 255 - BLOCK_VALUE
    for what, form in _forms(0).items():
        fb, n, v, c, d, _ = depth_ref.harness_render(s, form, FOLDS[fold])
        assert (v[both] == want).all() and (c[both] == 1).all(), what
        # the first sample inside the nearer block: within one step behind its face
        assert (d[both] >= near - 0.25 * r.step).all() and (d[both] <= near + 1.25 * r.step).all(), (what, d[both], near)
        assert depth_ref.check(r, v, c, d)[0] == 0, what


# ---- identities on the host build ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["skip", "skip16", "two blocks"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_skipping_and_uniform_bricks_change_no_bit(fold, name, filter_mode):
    s = two_blocks(fold == "min") if name == "two blocks" else scene(name, 0, FOLDS[fold])
    t = TRILINEAR if filter_mode else 0
    out = {}
    for walk in (0, GRID | FIXED):
        for skip in (0, SKIP):
            for uniform in (0, UNIFORM):
                out[walk, skip, uniform] = depth_ref.harness_render(s, walk | skip | uniform | t, FOLDS[fold])
    fb, n, v, c, d, xyz = out[0, 0, 0]
    for key, (fb1, n1, v1, c1, d1, xyz1) in out.items():
        assert np.array_equal(fb, fb1) and np.array_equal(v, v1) and np.array_equal(c, c1), key
        assert np.array_equal(d, d1) and np.array_equal(xyz, xyz1, equal_nan=True), key
        assert n1 <= n, key
    assert out[0, 0, UNIFORM][1] == n, "uniform bricks: the same count"
    print("%s %s filter %d: samples %d, with skipping %d" % (name, fold, filter_mode, n, out[0, SKIP, UNIFORM][1]))
    # (trilinear samples of a constant brick equal its value only up to rounding: under the margin the constant bricks
    # of "two blocks" can still tie with the M they gave, and the minimum's 255 -- unlike the maximum's 0, whose margin
    # is 0 -- skips none of them)
    if not (name == "two blocks" and filter_mode and fold == "min"):
        assert out[0, SKIP, UNIFORM][1] < n, "something was skipped"


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "two blocks", "skip", "skip16"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_three_passes_equal_one_in_any_order(fold, name, filter_mode):
    """The passes meet in the running (M, D), whatever their order -- also where a later pass brings a NEARER brick that
    can only tie with the M held: "two blocks" (the far block's pass first: the near block ties, its constant
    neighbours tie with the background) and "skip" / "skip16" (constant bricks beside noise).  There a brick that is
    skipped because it cannot beat M, or a uniform slot that does not take D over, leaves a depth too far."""
    s = two_blocks(fold == "min") if name == "two blocks" else scene(name, 0, FOLDS[fold])
    n = s.n_nodes
    parts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    t = TRILINEAR if filter_mode else 0
    plain = depth_ref.harness_render(s, t, FOLDS[fold])
    for form in (SKIP | t, SKIP | UNIFORM | t, GRID | FIXED | SKIP | UNIFORM | t):
        one = depth_ref.harness_render(s, form, FOLDS[fold])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, one) if isinstance(a, np.ndarray)), form
        if form & GRID:
            continue  # (a pass of the grid walk needs the whole grid)
        for order in itertools.permutations(parts):
            three = depth_ref.harness_render(s, form, FOLDS[fold], passes=list(order))
            for k, (a, b) in enumerate(zip(one, three)):
                if isinstance(a, np.ndarray):
                    assert np.array_equal(a, b, equal_nan=True), (form, order, k, int((a != b).sum()))


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", ["spin", "clip", "inside"])
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_the_cue_is_w_times_the_uncued_pixel(fold, name, filter_mode):
    s = scene(name)
    form = GRID | FIXED | SKIP | UNIFORM | (TRILINEAR if filter_mode else 0)
    plain = depth_ref.harness_render(s, form, FOLDS[fold], depth=0)
    zero = depth_ref.harness_render(s, form, FOLDS[fold], depth=1, cue=0)
    assert np.array_equal(plain[0], zero[0]), "strength 0 is the uncued frame"
    d = zero[4]
    interval = depth_ref.harness_render.interval.copy()
    for cue in (1000, 350):
        cued = depth_ref.harness_render(s, form, FOLDS[fold], depth=1, cue=cue)
        assert np.array_equal(cued[4], d) and np.array_equal(cued[2], zero[2]), "the cue changes neither M nor D"
        w = depth_ref.cue_weight(d, interval, np.float32(cue) / np.float32(1000.0))
        hit = zero[3] > 0
        assert hit.sum() > 100 and (w[hit] >= 0).all() and (w[hit] <= 1).all() and w[hit].min() < 0.9 * w[hit].max()
        want = (w[..., None] * zero[0]).astype(np.float32)
        assert np.array_equal(cued[0][hit], want[hit]), cue
        assert np.array_equal(cued[0][~hit], zero[0][~hit])
