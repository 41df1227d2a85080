"""Float volumes with NaN and infinite voxels (tests/nonfinite.py) on the CPU: the scenes are what they claim, the MIP
references keep the caps that keep mip_ref's rule honest, the host build of the kernel code (vrc_core.h) renders every
scene as include/vrc_hip.h says -- held to tests/ref64.py by test_ref64_cpu.check and to tests/mip_ref.py by its
check_frame, the same rules and numbers as everywhere -- and the comparisons notice the three plausible wrong readings
of the contract.  tests/test_nonfinite.py takes the same scenes to the GPU."""
import copy

import numpy as np
import pytest

import mip_ref
import mip_scenes as ms
import nonfinite as nf
import ref64
import scenes
import voxel_types as vt
from test_ref64_cpu import check
from test_voxel_types_cpu import LINEAR_FORMS, POINT_FORMS, _name

MIP_POINT_FORMS = [0, ms.GRID, ms.FIXED, ms.GRID | ms.FIXED]
MIP_LINEAR_FORMS = [ms.TRILINEAR, ms.TRILINEAR | ms.GRID]


def _is_nan(a):
    return a != a


# ---- the scenes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.NAMES)
def test_the_scene_is_what_it_claims(name):
    c = nf.case(name)
    assert tuple(c.q.render.dataSourceRange) == (float(nf.Q_R0), float(nf.Q_R1))
    assert [c.q.vi.overlap[a] for a in range(3)] == [4, 4, 4] and c.q.slot_dim == [24, 24, 24]
    assert c.q.W <= 48 and c.q.H <= 48
    # the markers occur where they were placed and nowhere else; nothing below Q_NAN
    for mark in (nf.Q_NAN, nf.Q_NINF, nf.Q_PINF):
        placed = c.placed.get(mark, np.zeros(c.vol.shape, dtype=bool))
        assert ((c.vol == mark) == placed).all(), mark
    assert c.vol.min() >= nf.Q_NAN and c.placed[nf.Q_NAN].sum() > 0
    # the float scene: NaN / -inf / +inf exactly at the markers, the image of q elsewhere (typed_scene's asserts hold
    # it exact in float32), brick by brick -- so the overlap borders agree -- and in the atlas
    for q, t, low in [(c.q.bricks[nid], c.t.bricks[nid], c.low.bricks[nid]) for nid in c.q.ids] + [(c.q.atlas, c.t.atlas, c.low.atlas)]:
        assert t.dtype == np.float32 and (_is_nan(t) == (q == nf.Q_NAN)).all()
        assert ((t == -np.inf) == (q == nf.Q_NINF)).all() and ((t == np.inf) == (q == nf.Q_PINF)).all()
        plain = ~np.isin(q, [nf.Q_NAN, nf.Q_NINF, nf.Q_PINF])
        assert (t[plain] == nf.IMAGE.apply(q)[plain]).all()
        assert (low[plain] == t[plain]).all() and (low[(q == nf.Q_NAN) | (q == nf.Q_NINF)] == -1.0).all()
        assert ((low == np.inf) == (q == nf.Q_PINF)).all() and np.isfinite(low[q != nf.Q_PINF]).all()
    # NaNs of both signs, quiet and signalling
    bits = np.concatenate([b.view(np.uint32)[_is_nan(b)] for b in c.t.bricks.values()])
    assert set(np.unique(bits)) == set(int(b) for b in nf.NAN_BITS)
    assert (bits >> 31).min() == 0 and (bits >> 31).max() == 1 and ((bits & 0x00400000) == 0).any()
    if name in nf.TRILINEAR:  # the shell: every voxel within Chebyshev distance 2 of a NaN voxel is <= r0 in q, varied
        near = nf.dilate(c.placed[nf.Q_NAN], 2)
        assert (c.vol[near] <= nf.Q_R0).all()
        shell = c.vol[near & ~c.placed[nf.Q_NAN]]
        assert len(np.unique(shell)) > 100
        assert not np.isin(c.vol, [nf.Q_NINF, nf.Q_PINF]).any()
    print("%s: %d NaN, %d -inf, %d +inf of %d voxels" % (name, (c.vol == nf.Q_NAN).sum(), (c.vol == nf.Q_NINF).sum(),
                                                          (c.vol == nf.Q_PINF).sum(), c.vol.size))


def test_what_the_scenes_are_for():
    c = nf.case("speckle")
    assert 0.05 < c.placed[nf.Q_NAN].mean() < 0.2 and c.placed[nf.Q_PINF].sum() >= 8 and c.placed[nf.Q_NINF].sum() >= 8
    c = nf.case("cores")
    x, y, z = [np.nonzero(c.placed[nf.Q_NAN].any(axis=ax))[0] for ax in ((0, 1), (0, 2), (1, 2))]
    for face in (16, 32):  # NaNs on both sides of brick faces, along every axis: they lie in overlap borders
        for along in (x, y, z):
            assert face - 1 in along and face in along
    assert c.placed[nf.Q_NAN][0, 0, 0] and c.placed[nf.Q_NAN][63, 63, 63]
    c = nf.case("allnan_brick")
    nid = [n for n in c.q.ids if c.q.lod[n].voxelBoxMin[:] == [16 * b for b in nf.ALLNAN]]
    assert len(nid) == 1 and _is_nan(c.t.bricks[nid[0]]).all(), "the slot holds nothing but NaN"
    assert sum(1 for b in c.t.bricks.values() if _is_nan(b).all()) == 1
    r = nf.mref("allnan_brick")
    assert nf.all_nan_rays(r).sum() >= 50, "rays that sample nothing but NaN"
    c = nf.case("ragged")
    assert c.vol.shape == (56, 40, 48)
    inner = np.zeros(c.vol.shape, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert not c.placed[nf.Q_NAN][inner].any() and all(c.placed[nf.Q_NAN][sl].any() for sl in (
        np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]))


@pytest.mark.parametrize("name", nf.NAMES)
def test_ambiguous_pixels_of_the_mip_references_are_capped(name):
    for f in (0, 1) if name in nf.TRILINEAR else (0,):
        r = nf.mref(name, f)
        hit, amb = int(r.hit().sum()), int(r.ambiguous().sum())
        print("%s filter %d: %d hit pixels, %d ambiguous" % (name, f, hit, amb))
        assert hit > 100 and amb <= 0.05 * hit
    if name in ("speckle", "allnan_brick"):
        r = nf.mref_passes(name)
        assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
        assert name == "speckle" or nf.all_nan_rays(r).sum() >= 50


@pytest.mark.parametrize("variant", sorted(nf.LAYERS))
def test_the_layers_leave_no_sample_in_doubt(variant):
    L = nf.layers(variant)
    for r in (L.ref, L.ref_front):
        assert (r.counts_lo == r.counts_hi).all() and (r.counts == r.counts_lo).all()
        assert int(r.ambiguous().sum()) <= 0.05 * int(r.hit().sum())
    # every ray that meets the volume meets the front layer first, and there is something behind it to skip
    assert ((L.ref.counts > 0) == (L.ref_front.counts > 0)).all() and L.ref_front.counts.sum() > 5000
    assert L.ref.counts.sum() > 2 * L.ref_front.counts.sum()
    assert 0.8 * L.ref_front.counts.sum() < L.first <= L.ref_front.counts.sum()
    assert _is_nan(L.t.atlas).mean() > 0.05 and np.isfinite(L.twin.atlas).all()
    bits = L.t.atlas.view(np.uint32)[_is_nan(L.t.atlas)]
    assert (bits >> 31).min() == 0 and (bits >> 31).max() == 1
    if variant != "swapped":
        front, _, (b0, b1), _ = nf.LAYERS[variant]
        fz = nf.FRONT_Z - 4
        assert (L.vol[fz:] == front).all() and b1 < front
        back = L.vol[:fz][~L.nan[:fz]]
        assert back.min() >= np.float32(b0) and back.max() <= np.float32(b1)
        # bricks: the front layer's are constant with their overlap; no back brick holds a value above the front's
        for nid, b in L.t.bricks.items():
            if L.t.lod[nid].voxelBoxMin[2] >= nf.FRONT_Z:
                assert (b == front).all()
            else:
                assert np.nanmax(b) <= front and _is_nan(b).any()


# ---- the host build of the kernel code ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.NAMES)
def test_host_build_composite_matches_ref64(name):
    c = nf.case(name)
    r = nf.ref(name)
    for form in POINT_FORMS:
        got, n = vt.harness_render(c.t, form)
        assert np.isfinite(got).all()
        check(c.q, got, n, r, name, _name(form), count=bool(form & vt.GRID))
        if form in (0, vt.GRID | vt.FIXED):  # the exact anchor: NaN and -inf render as a density <= r0 does
            low, n_low = vt.harness_render(c.low, form)
            assert np.array_equal(got, low) and n == n_low
    if name in nf.TRILINEAR:
        r = nf.ref(name, 1)
        for form in LINEAR_FORMS:
            got, n = vt.harness_render(c.t, form)
            assert np.isfinite(got).all()
            check(c.q, got, n, r, name + " trilinear", _name(form), count=bool(form & vt.GRID))


def _mip_ok(s, r, fb, n, what):
    bad, worst, amb = mip_ref.check_frame(s, r, fb)
    print("%s: %d failing pixels (worst excess %.3g), %d ambiguous of %d hit; samples %d, mip_ref %d .. %d" % (
        what, bad, worst, amb, int(r.hit().sum()), n, int(r.counts_lo.sum()), int(r.counts_hi.sum())))
    assert np.isfinite(fb).all() and bad == 0, what
    assert int(r.counts_lo.sum()) <= n <= int(r.counts_hi.sum()), what


@pytest.mark.parametrize("name", nf.NAMES)
def test_host_build_mip_matches_mip_ref(name):
    c = nf.case(name)
    for f, forms in ((0, MIP_POINT_FORMS), (1, MIP_LINEAR_FORMS if name in nf.TRILINEAR else [])):
        for form in forms:
            r = nf.mref(name, f)
            fb, n = ms.harness_render(c.mt, form)
            _mip_ok(c.mq, r, fb, n, "%s host mip form %d" % (name, form))
            fb1, n1 = ms.harness_render(c.mt, form | ms.SKIP)
            assert np.array_equal(fb, fb1) and n1 <= n
            if not f:  # NaN samples drop out, -inf cannot win: the frame and |S| of the low twin
                low, n_low = ms.harness_render(c.mlow, form)
                assert np.array_equal(fb, low) and n == n_low
    if name == "allnan_brick":
        fb, _ = ms.harness_render(c.mt, ms.GRID | ms.FIXED)
        _all_nan_rays_show_the_first_texel(c, nf.mref(name), fb)
    if name in ("speckle", "allnan_brick"):  # the running maximum between passes may be -infinity
        fb, n = ms.harness_render(c.mt, ms.FIXED, passes=nf.passes3(c.mt))
        _mip_ok(c.mq, nf.mref_passes(name), fb, n, "%s host mip in three passes" % name)


def _all_nan_rays_show_the_first_texel(c, r, fb):
    """A ray of NaN samples only has a sample set that is not empty: M = -infinity, the pixel is the first texel of the
    transfer function, premultiplied -- not the cleared value."""
    mask = nf.all_nan_rays(r)
    assert mask.sum() >= 50
    t0 = np.asarray(c.mq.tf, dtype=np.float64).reshape(256, 4)[0]
    want = np.array([t0[0] * t0[3], t0[1] * t0[3], t0[2] * t0[3], t0[3]])
    assert want[3] > 0.1, "the first texel must not look like the cleared value"
    assert (np.abs(fb[mask].astype(np.float64) - want).max(axis=-1) <= scenes.E0).all()
    assert (np.abs(mip_ref.classify64(c.mq, np.array(-1e30)) - want) < 1e-12).all()  # what anything <= r0 classifies as


@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_host_build_skips_every_back_brick_of_the_layers(variant):
    L = nf.layers(variant)
    assert tuple(L.twin.render.dataSourceRange) == (-1.0, 1.0) and (L.twin.atlas[L.t.atlas != L.t.atlas] == -1.0).all()
    for form in (ms.GRID, ms.GRID | ms.FIXED, 0):
        fb, n = ms.harness_render(L.t, form)
        _mip_ok(L.twin, L.ref, fb, n, "layers %s form %d" % (variant, form))
        assert n == int(L.ref.counts.sum())
        fb1, n1 = ms.harness_render(L.t, form | ms.SKIP)
        assert np.array_equal(fb, fb1)
        assert n1 == L.first, "to the sample: every ray's first brick and no other"
    S = nf.layers("swapped")  # what the GPU test swaps "a" with: noise in front, rays of NaN samples only at its rim
    fb, n = ms.harness_render(S.t, ms.GRID)
    _mip_ok(S.twin, S.ref, fb, n, "layers swapped")
    assert np.array_equal(ms.harness_render(S.t, ms.GRID | ms.SKIP)[0], fb)


# ---- teeth: the three plausible wrong readings, applied to the EXPECTED side ---------------------------------------------
def _with_nan_as(c, s, q_value):
    u = copy.copy(s)
    u.bricks = {nid: np.where(b == nf.Q_NAN, np.uint16(q_value), b) for nid, b in c.q.bricks.items()}
    return u


def test_a_nan_classified_as_the_last_texel_is_noticed():
    c = nf.case("speckle")
    got, n = vt.harness_render(c.t, vt.GRID | vt.FIXED)
    check(c.q, got, n, nf.ref("speckle"), "speckle", "control")
    wrong = ref64.render(_with_nan_as(c, c.q, 65533))  # >= r1: texel 255
    with pytest.raises(AssertionError):
        check(c.q, got, n, wrong, "speckle", "NaN as the last texel", count=False)


def test_a_nan_that_beats_every_number_in_the_maximum_is_noticed():
    c = nf.case("speckle")
    fb, _ = ms.harness_render(c.mt, ms.GRID | ms.FIXED)
    assert mip_ref.check_frame(c.mq, nf.mref("speckle"), fb)[0] == 0
    wrong = mip_ref.render(_with_nan_as(c, c.mq, 65533))
    bad = mip_ref.check_frame(c.mq, wrong, fb)[0]
    print("NaN as the largest value: %d failing pixels" % bad)
    assert bad > 0.5 * wrong.hit().sum()


def test_an_all_nan_ray_left_at_the_cleared_value_is_noticed():
    c = nf.case("allnan_brick")
    r = nf.mref("allnan_brick")
    fb, _ = ms.harness_render(c.mt, ms.GRID | ms.FIXED)
    assert mip_ref.check_frame(c.mq, r, fb)[0] == 0
    mask = nf.all_nan_rays(r)
    wrong = copy.copy(r)  # the sample set of those rays called empty
    wrong.certain, wrong.maybe, wrong.m = r.certain & ~mask, r.maybe & ~mask, np.where(mask, -np.inf, r.m)
    wrong.extra = {k: v for k, v in r.extra.items() if not mask[k]}
    bad = mip_ref.check_frame(c.mq, wrong, fb)[0]
    print("all-NaN rays expected cleared: %d failing pixels of %d such rays" % (bad, mask.sum()))
    assert bad == mask.sum()
