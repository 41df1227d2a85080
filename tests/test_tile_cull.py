"""The tile culling of the five reference-order kernels (vrc_k_raycast, _mip, _shade, _cdepth, _preint) on the GPU, held
to the unculled loop of the same kernel bit for bit, in each of the block's four regimes (libre_amd/csrc/vrc_core.h, "tile
culling"; tests/test_tile_cull_cpu.py does the same on the host build and checks the scenes' regimes there).

  comparator A: the scene's own list (the culled regime) against the same list with never-hit entries added at its end until
      it is one entry too long for 16-bit indices (the plain loop) -- frame, sample count and every read-back equal; and
      against the list padded to the longest culled length with its entries spread out (indices up to the last one).
  comparator B: the list in passes short enough for the plain loop, where a projection's passes equal one pass.

Every threshold comes from the host build (tests/cull.py: limits()).

Two memory-safe mutated builds of the library were run against this module once when it was written:
  `(uint8_t)i` in place of `(uint16_t)i` at the candidate store, in all five kernels: 59 of the 85 tests red (every
      comparison whose list has an entry past index 255: the spread lists, the 4096-brick scenes);
  margin 0 in all five kernels: none red, and none can be -- tests/test_tile_cull_cpu.py, mutation (a), says why no frame
      depends on the margin; the host tests that see it are the per-ray statement under supersampling and the masks."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import cdepth_ref
import cull
import iso_ref
import mip_ref
import mip_scenes
import nongrid
import preint_ref
import shade_ref
import voxel_types
from gpu_run import GpuScene
from libre_amd import vrc
from test_ref64_cpu import case as ref64_case, check as ref64_check, ref as ref64_ref

pytestmark = pytest.mark.gpu

FOLD_MAX, FOLD_MIN, FOLD_MEAN, FOLD_FIRST = 0, 1, 2, 3
ISO_VALUE, AMBIENT, TAU = 150.0, 0.25, 500


def _opt(g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def _values(g, h):
    v = np.full((h, g.s.W), np.nan, dtype=np.float32)
    c = np.full((h, g.s.W), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(g.L, g.L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    return v, c


def _depths(g, h):
    return vrc.projection_depths(g.L, g.ctx, g.s.W, h)


def _gradients(g, h):
    return (vrc.projection_gradients(g.L, g.ctx, g.s.W, h),)


class Form:
    """One entry of the matrix: the options that select it, the kernel it must launch and the read-backs it serves."""

    def __init__(self, name, launches, modes, options=(), iso=False, readbacks=(), scene="u8", passes=False, **render):
        self.name, self.launches, self.modes, self.options, self.iso = name, launches, modes, options, iso
        self.readbacks, self.scene, self.passes = readbacks, scene, passes
        self.render = dict(render, kernel=render.get("kernel", vrc.KERNEL_REFERENCE_ORDER))

    def setup(self, g):
        if self.iso:
            vrc.set_isosurface(g.L, g.ctx, ISO_VALUE, AMBIENT)
        for option, value in self.options:
            _opt(g, option, value)

    def frame(self, g, passes=None):
        """(frame, samples, read-backs ...) with the instance asserted: the <false, ...> (reference-order) one of the kernel"""
        fb, n, _ = g.render(passes=passes, **self.render)
        k = g.L.vrc_last_kernel()
        assert k.startswith(self.launches + b"<false,"), (self.name, k)
        assert self.modes is None or any((b",%d," % m) in k for m in self.modes), (self.name, k)
        out = (fb, n)
        for rb in self.readbacks:
            out += rb(g, fb.shape[0])
        return out


def _forms():
    P, MIP, ISO = vrc.OPT_PROJECTION, vrc.PROJECTION_MIP, vrc.PROJECTION_ISO
    out = [Form("composite-u8-grey", b"vrc_k_raycast", (3,), [(vrc.OPT_GREY_TABLE, 1)]),
           Form("composite-u8", b"vrc_k_raycast", (0,), [(vrc.OPT_GREY_TABLE, 0)]),
           Form("composite-u16", b"vrc_k_raycast", (2, 4), scene="u16"),
           Form("composite-trilinear", b"vrc_k_raycast", (1,), filter_mode=1),
           # (VRC_KERNEL_PACKED walks the grid where the list is one: the reference-order instance takes a list that is none)
           Form("composite-packed", b"vrc_k_raycast", (5, 6), scene="overlap", kernel=vrc.KERNEL_PACKED, filter_mode=1),
           Form("composite-gl-spp1", b"vrc_k_raycast", None, scene="gl1", variant=1),
           Form("composite-gl-spp2", b"vrc_k_raycast", None, scene="gl2", variant=1),
           Form("composite-gl-spp3", b"vrc_k_raycast", None, scene="gl3", variant=1),
           Form("composite-float", b"vrc_k_raycast", None, scene="float")]
    for f, flt in ((0, "nearest"), (1, "trilinear")):
        base = 8 if f else 7
        for fold, name in ((FOLD_MAX, "max"), (FOLD_MIN, "min"), (FOLD_MEAN, "mean")):
            o = [(P, MIP), (vrc.OPT_MIP_FOLD, fold), (vrc.OPT_MIP_SKIP, 0)]
            out.append(Form("mip-%s-%s" % (name, flt), b"vrc_k_raycast_mip", (base + 16 * fold,), o, readbacks=(_values,),
                            passes=True, filter_mode=f))
            if fold != FOLD_MEAN:
                out.append(Form("mip-%s-depth-%s" % (name, flt), b"vrc_k_raycast_mip", (base + 16 * fold + 64,),
                                o + [(vrc.OPT_MIP_DEPTH, 1)], readbacks=(_values, _depths), passes=True, filter_mode=f))
        out.append(Form("iso-%s" % flt, b"vrc_k_raycast_mip", (base + 16 * FOLD_FIRST,), [(P, ISO), (vrc.OPT_MIP_SKIP, 0)], iso=True,
                        readbacks=(_values, _depths, _gradients), passes=True, filter_mode=f))
        out.append(Form("shade-%s" % flt, b"vrc_k_raycast_shade", (11 if f else 10,),
                        [(vrc.OPT_SHADING_AMBIENT, int(round(AMBIENT * 1000))), (vrc.OPT_SHADING, 1)], passes=True, filter_mode=f))
        out.append(Form("cdepth-%s" % flt, b"vrc_k_raycast_cdepth", (13 if f else 12,), [(vrc.OPT_COMPOSITE_DEPTH, TAU)],
                        readbacks=(_values, _depths), filter_mode=f))
        out.append(Form("preint-%s" % flt, b"vrc_k_raycast_preint", (15 if f else 14,), [(vrc.OPT_PREINTEGRATION, 1)], passes=True,
                        filter_mode=f))
    return out


FORMS = {f.name: f for f in _forms()}
#: one form per copy of the block and filter, for the scenes of 4096 bricks
PER_KERNEL = ["composite-u8", "composite-trilinear", "mip-max-depth-nearest", "iso-trilinear", "shade-nearest", "shade-trilinear",
              "cdepth-nearest", "cdepth-trilinear", "preint-nearest", "preint-trilinear"]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b)) and len(a) == len(b)


def _differ(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not (np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y)]


# ---- scenes and their padded lists, once per module ------------------------------------------------------------------------
_CACHE = {}


def _scene(name, kind):
    """The scene of that name for a form's kind of pool: 8- or 16-bit voxels, the glRaycaster variant at 1 to 3 samples per
    pixel, or -- one scene each, with its own view -- the float image of tests/voxel_types.py and an overlapping list of
    tests/nongrid.py."""
    key = (name, kind)
    if key not in _CACHE:
        if kind == "float":
            s = mip_scenes.typed("float")[1]
        elif kind == "overlap":
            s = nongrid.overlapping_scene("hash_parents_all_leaves")
        else:
            s = cull.scene(name, "u16" if kind == "u16" else "u8")
        if kind.startswith("gl"):
            s = copy.copy(s)
            s.render = type(s.render)(s.render.samplesPerRay, int(kind[2:]), s.render.maxSamplesPerRay, 0,
                                      (C.c_float * 2)(*[float(v) for v in s.render.dataSourceRange]))
        _CACHE[key] = s
    return _CACHE[key]


def _padded(s, total, where):
    key = (id(s), total, where)
    if key not in _CACHE:
        _CACHE[key] = (s, cull.padded(s, total, where))  # (the scene is kept: its id stays its own)
    return _CACHE[key][1]


def _gpu(s):
    return voxel_types.typed_gpu_scene(s) if hasattr(s, "voxel_type") else GpuScene(s)


def _with_list(g, t):
    """the context's scene with another node list (same pool, same view)"""
    g.s = t
    return g


def _regimes(s, **kw):
    return cull.tile_masks(s, **kw)[2]


def _comparator_a(form, g, s, what, variant=0, interleaved=True):
    """The list's own frame -- culled in every tile the masks say -- against the padded lists'."""
    lim = cull.limits()
    own = form.frame(_with_list(g, s))
    assert own[1] > 0 and own[0][..., 3].max() > 0.0, "%s: an empty frame shows nothing" % what
    long_list = _padded(s, lim.upper + 1, "end")
    assert (_regimes(long_list, variant=variant) == cull.LONG).all()
    plain = form.frame(_with_list(g, long_list))
    assert _same(own, plain), "%s: culled list against the plain loop of the padded list: outputs %s differ" % (what, _differ(own, plain))
    if interleaved:
        spread = _padded(s, lim.upper, "interleaved")
        assert np.array_equal(_regimes(spread, variant=variant), _regimes(s, variant=variant)) and spread.real[-1] == lim.upper - 1
        far = form.frame(_with_list(g, spread))
        assert _same(own, far), "%s: the list spread over %d entries: outputs %s differ" % (what, lim.upper, _differ(own, far))
    _with_list(g, s)
    return own


# ---- comparator A over the matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FORMS))
def test_culled_list_equals_the_plain_loop_of_the_padded_list(name):
    form = FORMS[name]
    variant = form.render.get("variant", 0)
    for scene_name in ("hash64", "hash64_clip", "hash64_inside"):
        s = _scene(scene_name, form.scene)
        assert s.n_nodes > cull.limits().lower and (_regimes(s, variant=variant) == cull.CULLED).all()
        with _gpu(s) as g:
            form.setup(g)
            _comparator_a(form, g, s, "%s %s" % (name, scene_name), variant)
        if form.scene in ("float", "overlap"):
            break  # (one scene of its own)


@pytest.mark.parametrize("name", PER_KERNEL)
def test_the_regimes_around_the_waves_array(name):
    """4096 bricks behind one tile, all of which survive the culling: the first `candidates` entries fill the wave's array to
    its last entry, one more overflows it; and a frame of 3 x 2 tiles of which the masks put some on either side."""
    form, lim = FORMS[name], cull.limits()
    dense = _scene("dense8", "u8")
    kept, _, _ = cull.tile_masks(dense)
    assert kept.all() and dense.n_nodes > lim.candidates + 1
    with _gpu(dense) as g:
        form.setup(g)
        for n, regime in ((lim.candidates, cull.CULLED), (lim.candidates + 1, cull.OVERFLOW)):
            key = ("first", n)
            if key not in _CACHE:
                _CACHE[key] = cull.first(dense, n)
            t = _CACHE[key]
            assert _regimes(t).tolist() == [regime]
            _comparator_a(form, g, t, "%s first %d of dense8" % (name, n))
    wide = _scene("dense8_wide", "u8")
    _, counts, regimes = cull.tile_masks(wide)
    assert set(regimes.tolist()) == {cull.CULLED, cull.OVERFLOW} and ((counts > lim.candidates) == (regimes == cull.OVERFLOW)).all()
    with _gpu(wide) as g:
        form.setup(g)
        _comparator_a(form, g, wide, "%s dense8_wide" % name, interleaved=False)


@pytest.mark.parametrize("name", PER_KERNEL)
def test_the_lower_boundary(name):
    """The first `lower` entries run the plain loop, one more is culled: each against its padded list, and (comparator B, no
    clip planes) the culled list of lower + 1 entries against the passes of `lower` entries and of one."""
    form, lim = FORMS[name], cull.limits()
    s = _scene("hash64", "u8")
    with _gpu(s) as g:
        form.setup(g)
        for n, regime in ((lim.lower, cull.SHORT), (lim.lower + 1, cull.CULLED)):
            t = cull.first(s, n)
            assert (_regimes(t) == regime).all()
            own = _comparator_a(form, g, t, "%s first %d" % (name, n), interleaved=regime == cull.CULLED)
        if form.passes:
            two = form.frame(_with_list(g, t), passes=[(0, lim.lower), (lim.lower, lim.lower + 1)])
            assert np.array_equal(own[0], two[0]), "%s: %d entries against passes of %d and 1" % (name, lim.lower + 1, lim.lower)


# ---- comparator B ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, f in FORMS.items() if f.passes))
def test_culled_list_equals_passes_too_short_to_cull(name):
    """Where a projection's passes equal one pass (tests/test_mip.py, test_fold.py, test_iso.py, test_depth.py; test_shade.py
    and test_preint.py under their precondition, kept here): the list in passes of at most `lower` entries -- no pass is
    culled -- gives the culled frame bit for bit.  Scenes without clip planes (tests/nongrid.py: oracle_passes)."""
    form = FORMS[name]
    for scene_name in ("hash64", "hash64_inside"):
        s = _scene(scene_name, form.scene)
        assert len(s.planes) == 0
        parts = cull.passes_of(s)
        assert max(b - a for a, b in parts) <= cull.limits().lower and len(parts) > 1
        with _gpu(s) as g:
            if form.launches in (b"vrc_k_raycast_shade", b"vrc_k_raycast_preint"):
                kw = dict(kernel=vrc.KERNEL_REFERENCE_ORDER, filter_mode=form.render.get("filter_mode", 0))
                p1, pn = g.render(**kw), g.render(passes=parts, **kw)
                assert np.array_equal(p1[0], pn[0]) and p1[1] == pn[1], "the precondition: the plain frame's passes equal one pass"
            form.setup(g)
            one = form.frame(g)
            many = form.frame(g, passes=parts)
            assert one[0][..., 3].max() > 0.0
            assert np.array_equal(one[0], many[0]), "%s %s: %d pixels differ" % (name, scene_name, int((one[0] != many[0]).any(axis=-1).sum()))


# ---- a tile whose rows lie far apart -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PER_KERNEL)
def test_row_map_band_equals_the_full_frames_rows(name):
    form = FORMS[name]
    s = _scene("hash64", "u8")
    rows = np.array(cull.ROW_MAP, dtype=np.uint32)
    assert (cull.tile_masks(s, row_map=cull.ROW_MAP)[2] == cull.CULLED).all()
    with _gpu(s) as g:
        form.setup(g)
        full = form.frame(g)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        band_scene = copy.copy(s)
        band_scene.H = len(rows)  # the buffer GpuScene reads back
        try:
            band = form.frame(_with_list(g, band_scene))
            # and the band's own padded list: the plain loop under the same row map
            long_list = copy.copy(_padded(s, cull.limits().upper + 1, "end"))
            long_list.H = len(rows)
            plain = form.frame(_with_list(g, long_list))
        finally:
            _with_list(g, s)
            vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
        for k, (a, b) in enumerate(zip(full[2:], band[2:])):
            assert np.array_equal(a[rows], b, equal_nan=True), "%s: read-back %d" % (name, k)
        assert np.array_equal(full[0][rows], band[0]), name
        assert _same(band, plain), "%s: the band against its padded list: outputs %s differ" % (name, _differ(band, plain))


# ---- equal, and right: one scene per kernel against its float64 reference -----------------------------------------------------
def _a_on(form, s):
    with _gpu(s) as g:
        form.setup(g)
        return _comparator_a(form, g, s, form.name + " on the reference's scene")


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_composite_culled_frame_against_ref64(filter_mode):
    s = ref64_case("hash64_spin")[0]
    own = _a_on(FORMS["composite-trilinear" if filter_mode else "composite-u8"], s)
    ref64_check(s, own[0], own[1], ref64_ref("hash64_spin", filter_mode=filter_mode), "hash64_spin", "gpu reference order, culled",
                count=False)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_mip_culled_frame_against_mip_ref(filter_mode):
    s, r = mip_scenes.get("spin"), mip_scenes.ref("spin", filter_mode)
    own = _a_on(FORMS["mip-max-%s" % ("trilinear" if filter_mode else "nearest")], s)
    bad, worst, _ = mip_ref.check_frame(s, r, own[0])
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_iso_culled_frame_against_iso_ref(filter_mode):
    assert iso_ref.ISO["spin"] == ISO_VALUE
    s, r = iso_ref.scene("spin", filter_mode), iso_ref.ref("spin", filter_mode)
    own = _a_on(FORMS["iso-%s" % ("trilinear" if filter_mode else "nearest")], s)
    bad, worst = iso_ref.check(r, own[2], own[3], own[4], own[6], iso_ref.tolerance(s, filter_mode))
    assert bad == 0 and (own[3] == 1).sum() > 100, (bad, worst)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_shade_culled_frame_against_shade_ref(filter_mode):
    assert shade_ref.AMBIENT == AMBIENT
    s, r = shade_ref.scene("spin"), shade_ref.ref("spin", filter_mode)
    own = _a_on(FORMS["shade-%s" % ("trilinear" if filter_mode else "nearest")], s)
    shade_ref.check(s, own[0], r, "shade, culled, filter %d" % filter_mode)


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_cdepth_culled_frame_against_cdepth_ref(filter_mode):
    s, r = cdepth_ref.scene("spin"), cdepth_ref.ref("spin", filter_mode, TAU)
    own = _a_on(FORMS["cdepth-%s" % ("trilinear" if filter_mode else "nearest")], s)
    cdepth_ref.assert_rule(r, own[2], own[3], own[4], "cdepth, culled, filter %d" % filter_mode, tol=cdepth_ref.tolerance(s, filter_mode))


@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_preint_culled_frame_against_preint_ref(filter_mode):
    s, r = preint_ref.scene("spin"), preint_ref.ref("spin", filter_mode)
    own = _a_on(FORMS["preint-%s" % ("trilinear" if filter_mode else "nearest")], s)
    preint_ref.check(s, own[0], r, "preint, culled, filter %d" % filter_mode)
