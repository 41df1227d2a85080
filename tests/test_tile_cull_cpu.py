"""The tile culling of the reference-order kernels (libre_amd/csrc/vrc_core.h, "tile culling") on the CPU: the product's
vrc_make_tile_pyramid and vrc_pyramid_may_hit under the wave's culling loop as tests/cpu_harness/cull_harness.cpp restates
it, built by g++ without contraction and by clang with -mfma.

  - conservative, exactly: per tile, the bricks the pyramid keeps include every brick some ray of the tile marches or
    stops at, by the kernel's own float32 per-ray test (no tolerance) and by the float64 statement of tests/cull.py;
  - culled equals unculled: the frame and the sample count of vrc_pixel_reference_order over the candidates are those of
    candidates = nullptr, bit for bit, in every mode the harness builds, for one pass and for two;
  - the four regimes of the rule, each by construction, at their boundaries;
  - a stand-alone program under the address and undefined-behaviour sanitizers.

No GPU.  tests/test_tile_cull.py carries the same comparison to the five kernels.

Mutations tried on scratch copies when the module was written (the tests that turned red; the module had 405 then, (b)
was run again with the test added for it):
  (a) margin 0 instead of one pixel: the "keeps every brick" cases gl_spp2 and gl_spp3, and the four-regimes test (the one
      tile no longer keeps the whole list).  No frame changes, and none can: every ray but the jittered sub-rays of the
      glRaycaster variant lies inside or on the margin-less pyramid, a brick such a ray meets touches the plane and is
      kept by the rounding allowance, and a brick that only a jittered sub-ray meets is discarded by the supersampled
      pixel anyway (its sub-ray 0 is the centre ray).  The margin is a rounding reserve on top of the allowance.
  (b) s < +1e-5f * mag: test_a_box_that_touches_a_side_plane_is_kept only -- behind a pixel of margin no ray reaches a
      brick that merely touches a side plane, so no scene sees the allowance; that test was added for it.
  (c) no winding flip: 283 tests, every family.
  (d) r1 from the tile's first row: 270 tests, every family.
  (e) candidates in descending order: 130 tests, every frame comparison (the kept sets do not change)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cull
import nongrid
import orc
from test_cpu_harness import _fuzz_scene

FLAVOURS = ["", "fma"]
HAVE_CLANG = os.path.exists("/opt/rocm/lib/llvm/bin/clang++")
CSRC = os.path.join(orc.ROOT, "libre_amd", "csrc")


def _flavours():
    return [f for f in FLAVOURS if f == "" or HAVE_CLANG]


class Case:
    def __init__(self, s, row_map=None, variant=0, tiles=None, expect_stop=False, expect_hits=True):
        self.s, self.row_map, self.variant, self.tiles, self.expect_stop = s, row_map, variant, tiles, expect_stop
        self.expect_hits = expect_hits  # (from far away the volume can fall between the rays of every pixel)

    def kw(self):
        return dict(row_map=self.row_map, variant=self.variant, tiles=self.tiles)


# ---- the cases -------------------------------------------------------------------------------------------------------------
N_VIEWS = 166
SPINS = [(0.0, 0.0), (0.5, 0.35), (-0.7, 0.25), (1.2, -0.3), (2.3, -0.4), (3.0, 1.2), (-2.1, -1.0), (0.2, 0.9), (1.5, 0.2),
         (-1.1, 0.4), (2.6, 0.9), (-3.0, -0.1)]


def _view(i):
    """The seeded views: eyes from 0.05 to 400 units from the centre (below 0.5: inside the unit volume), twelve spins,
    viewports from 9x9 to 70x70, bricks of 8, 16 and 32 voxels, both variants."""
    rng = np.random.default_rng(9000 + i)
    dist = float(np.exp(rng.uniform(np.log(0.05), np.log(400.0))))
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    if abs(direction[1]) > 0.95:  # (lookAt's up vector is +y)
        direction = np.array([0.6, 0.0, 0.8])
    s = orc.build_scene(voxels=(64, 64, 64), block=int(rng.choice([8, 16, 32])), spin=SPINS[i % len(SPINS)],
                        viewport=(int(rng.integers(9, 71)), int(rng.integers(9, 71))),
                        eye=tuple(float(v) for v in dist * direction), spr=64)
    return Case(s, variant=int(i % 2), expect_hits=dist < 10.0)


HASH = dict(voxels=(64, 64, 64), block=16, volume="hash", spin=(0.5, 0.35), spr=96, alpha=0.3)


def _gl(spp):
    s = orc.build_scene(viewport=(44, 36), **HASH)
    s.render = orc.RenderData(s.render.samplesPerRay, spp, 32, 0, (orc.C.c_float * 2)(0.0, 255.0))
    return Case(s, variant=1)


def _mixed():
    vi = orc.mem_volume_info(64, 64, 64, 16)
    coarse = orc.pack(1, 0, 0, 0)
    ids = [coarse] + [i for i in orc.leaf_ids(vi) if orc.lib().orc_nodeid_parent(i) != coarse]
    return Case(orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), spin=(0.4, 0.3), ids=ids, volume="hash"))


def _sample_of_tiles():
    s = orc.build_scene(viewport=(1024, 1024), **HASH)
    tx, ty = cull.tiles_of(s)
    tiles = np.sort(np.random.default_rng(77).choice(tx * ty, size=256, replace=False))
    return Case(s, tiles=tiles)


NAMED = {
    "vp17x15": lambda: Case(orc.build_scene(viewport=(17, 15), **HASH)),
    "vp60x52": lambda: Case(orc.build_scene(viewport=(60, 52), **HASH)),
    "vp1024_256tiles": _sample_of_tiles,
    "eye40": lambda: Case(orc.build_scene(viewport=(44, 36), eye=(0.0, 0.0, 40.0), **HASH), expect_hits=False),
    "eye400": lambda: Case(orc.build_scene(viewport=(44, 36), eye=(0.0, 0.0, 400.0), **HASH), expect_hits=False),
    "eye4000": lambda: Case(orc.build_scene(viewport=(44, 36), eye=(0.0, 0.0, 4000.0), **HASH), expect_hits=False),
    "eye_in_brick": lambda: Case(orc.build_scene(viewport=(44, 36), eye=(0.1, 0.05, 0.2), **HASH)),
    "eye_on_brick_corner": lambda: Case(orc.build_scene(viewport=(44, 36), eye=(0.25, 0.25, 0.25), **HASH)),
    "sortfirst_centre": lambda: Case(orc.build_scene(viewport=(48, 48), tile=(12, 24, 24, 12, 48, 48), **HASH)),
    "sortfirst_offcentre": lambda: Case(orc.build_scene(viewport=(1024, 768), tile=(520, 400, 56, 40, 1024, 768), **HASH)),
    "clip1": lambda: Case(orc.build_scene(viewport=(44, 36), planes=[[0.6, 0.0, 0.8, 0.3]], **HASH)),
    "clip2_break": lambda: Case(orc.build_scene(viewport=(44, 36), planes=cull.CLIP_PLANES, **HASH), expect_stop=True),
    "clip3": lambda: Case(orc.build_scene(viewport=(44, 36), planes=cull.CLIP_PLANES + [[0.0, 1.0, 0.0, 0.3]], **HASH)),
    "flat128x32x64_b8": lambda: Case(orc.build_scene(voxels=(128, 32, 64), block=8, viewport=(44, 36), volume="hash",
                                                     spin=(0.5, 0.35), spr=96, alpha=0.3)),
    "mixed_levels": _mixed,
    "overlapping": lambda: Case(nongrid.overlapping_scene("hash_parents_some_children")),
    "row_map": lambda: Case(cull.scene("hash64"), row_map=cull.ROW_MAP),
    "row_bands": lambda: Case(orc.build_scene(viewport=(56, 72), **HASH),
                              row_map=[r for (y0, h) in cull.BANDS for r in range(y0, y0 + h)]),
    "gl_spp1": lambda: _gl(1),
    "gl_spp2": lambda: _gl(2),
    "gl_spp3": lambda: _gl(3),
}
CASES = ["view%03d" % i for i in range(N_VIEWS)] + sorted(NAMED) + ["ragged_uvf"]


@functools.lru_cache(maxsize=4)
def _build_case(name):
    if name.startswith("view"):
        return _view(int(name[4:]))
    if name == "ragged_uvf":  # the host library reads the UVF file
        import __graft_entry__ as g
        g.build_host()
        from libre_amd import driver
        driver.load_library()
        return Case(nongrid.uvf_scene(driver, "uvf_leaves"))
    return NAMED[name]()


def _case(name):
    return _build_case(name)


def _family(name):
    return "views" if name.startswith("view") else name


#: (tile, brick) pairs checked / kept / needed per case family, printed by the last test of the module
TALLY = {}


# ---- conservative, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_pyramid_keeps_every_brick_a_ray_of_the_tile_needs(name):
    c = _case(name)
    s = c.s
    want64 = cull.needed64(s, **c.kw())
    for flavour in _flavours():
        kept, counts, _ = cull.tile_masks(s, flavour=flavour, **c.kw())
        need = cull.needed(s, flavour=flavour, **c.kw())
        # the kernel's own float32 per-ray test: no tolerance
        dropped = np.argwhere((need != 0) & ~kept)
        assert dropped.size == 0, "%s %r: (tile, brick) dropped although a ray marches or stops at it: %s" % (name, flavour, dropped[:8])
        dropped = np.argwhere((want64 != 0) & ~kept)
        assert dropped.size == 0, "%s %r: (tile, brick) dropped against the float64 statement: %s" % (name, flavour, dropped[:8])
        # not vacuous: some tile keeps fewer bricks than the list has; and both statements of "needed" find bricks
        assert counts.min() < s.n_nodes, (name, counts)
        assert not c.expect_hits or ((need != 0).any() and (want64 != 0).any()), name
        if c.expect_stop:
            assert (need & cull.STOP).any() and (want64 & cull.STOP).any(), "the reference's break fires in this case"
        t = TALLY.setdefault((_family(name), flavour), [0, 0, 0])
        t[0] += kept.size
        t[1] += int(kept.sum())
        t[2] += int((need != 0).sum())
    print("%s: %d pairs, kept %d, needed %d, kept/needed %.2f" % (name, kept.size, kept.sum(), (need != 0).sum(),
                                                                 kept.sum() / max(1, (need != 0).sum())))


@pytest.mark.parametrize("name", ["hash64", "hash64_inside"])
def test_a_box_that_touches_a_side_plane_is_kept(name):
    """The rounding allowance of vrc_pyramid_may_hit, by itself.  A box whose furthest-inside vertex lies ON a side plane of
    the pyramid is met by the rays in that plane: it must be kept although float32 puts the vertex a few ulps to either
    side.  The same box a hundredth of its distance further out is culled, and further in it is kept -- which pins the
    planes' orientation (the winding flip) too.  The planes are restated in float64 from the four corner directions."""
    s = cull.scene(name)
    eye = np.array([float(s.view.eyePosition[a]) for a in range(3)])
    size = np.array([0.25, 0.125, 0.0625])
    checked = 0
    for corners in ((7.0, 7.0, 16.0, 16.0), (-1.0, -1.0, 8.0, 8.0), (23.0, 15.0, 32.0, 24.0), (39.0, 31.0, 44.0, 36.0)):
        x0, y0, x1, y1 = corners
        d = [cull.direction64(s, x, y) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
        centre = sum(d) / 4.0
        for k in range(4):
            a, b = d[k], d[(k + 1) & 3]
            n = np.cross(a, b)
            if n @ centre < 0.0:
                n = -n
            for t in (0.4, 1.0, 2.5):
                for w in (0.2, 0.5, 0.8):
                    p = eye + t * (w * a + (1.0 - w) * b) / np.linalg.norm(centre)   # on the plane, between its two edges
                    out = -n / np.linalg.norm(n) * 0.01 * np.linalg.norm(p - eye)
                    boxes = []
                    for shift in (0.0, 1.0, -1.0):   # touching, outside, inside
                        v = p + shift * out            # the vertex furthest inside: max of n . v over the box
                        boxes.append(np.concatenate([v - np.where(n > 0.0, size, 0.0), size]))
                    for flavour in _flavours():
                        keeps = cull.pyramid_keeps(s, corners, boxes, flavour=flavour)
                        assert keeps.tolist() == [True, False, True], (name, corners, k, t, w, flavour, keeps)
                    checked += 1
    assert checked == 4 * 4 * 9


def test_padding_entries_are_never_hit():
    """tests/cull.py: padded() -- no ray of any tile marches or stops at an added entry, and no tile keeps one; the scene's
    own entries keep their masks."""
    lim = cull.limits()
    for s in (cull.scene("hash64"), cull.scene("hash64_clip"), cull.scene("hash64_inside"), cull.scene("dense8_wide")):
        base_kept, _, base_regimes = cull.tile_masks(s)
        for total, where in ((lim.upper + 1, "end"), (lim.upper, "interleaved")):
            p = cull.padded(s, total, where)
            pad = np.ones(p.n_nodes, dtype=bool)
            pad[p.real] = False
            assert pad.sum() == total - s.n_nodes and p.real.max() == (s.n_nodes - 1 if where == "end" else total - 1)
            for flavour in _flavours():
                assert not cull.needed(p, flavour=flavour)[:, pad].any()
                kept, _, regimes = cull.tile_masks(p, flavour=flavour)
                assert not kept[:, pad].any()
                assert (regimes == cull.LONG).all() if total > lim.upper else np.array_equal(regimes, base_regimes)
            assert np.array_equal(cull.tile_masks(p)[0][:, p.real], base_kept)


# ---- culled equals unculled on the host --------------------------------------------------------------------------------------
def _assert_culled_equals_plain(s, what, modes, flavour="", **kw):
    for mode in modes:
        a, na, regimes = cull.render(s, mode, True, flavour=flavour, **kw)
        b, nb, _ = cull.render(s, mode, False, flavour=flavour, **kw)
        assert np.array_equal(a, b) and na == nb, "%s %s %r: culled %d samples, plain %d, %d pixels differ" % (
            what, mode, flavour, na, nb, int((a != b).any(axis=-1).sum()))
    return regimes


@pytest.mark.parametrize("name", CASES)
def test_culled_frame_equals_the_plain_loops_frame(name):
    c = _case(name)
    modes = ["table"] if c.s.atlas.dtype.itemsize == 1 else ["point"]
    for flavour in _flavours():
        regimes = _assert_culled_equals_plain(c.s, name, modes, flavour, **c.kw())
    if c.s.n_nodes > cull.limits().lower:
        assert (regimes == cull.CULLED).all(), (name, regimes)


@pytest.mark.parametrize("dtype", ["u8", "u16"])
@pytest.mark.parametrize("name", ["hash64", "hash64_clip", "hash64_inside"])
def test_culled_equals_plain_in_every_mode_the_harness_builds(name, dtype):
    s = cull.scene(name, dtype)
    modes = [m for m in cull.MODES if not (dtype == "u16" and m == "table")]
    for flavour in _flavours():
        _assert_culled_equals_plain(s, "%s %s" % (name, dtype), modes, flavour)
    # a frame that is something: the modes differ from each other
    frames = {m: cull.render(s, m)[0] for m in modes}
    assert frames["point"][..., 3].max() > 0.05
    assert not np.array_equal(frames["point"], frames["trilinear"]) and not np.array_equal(frames["point"], frames["shade"])


@pytest.mark.parametrize("seed", range(16))
def test_culled_equals_plain_on_fuzzed_views(seed):
    rng = np.random.default_rng(1000 + seed)
    kw = _fuzz_scene(rng)
    s = orc.build_scene(**kw)
    for flavour in _flavours():
        _assert_culled_equals_plain(s, "seed %d %r" % (seed, kw), ["table", "trilinear", "shade"], flavour)
    ov, _ = nongrid.fuzz_scene(np.random.default_rng(2000 + seed))
    _assert_culled_equals_plain(ov, "overlapping, seed %d" % seed, ["table"])


@pytest.mark.parametrize("name", ["hash64", "hash64_clip"])
def test_a_frame_of_two_passes(name):
    """Each pass culls its own list; the second accumulates onto the first's pixels."""
    s = cull.scene(name)
    half = s.n_nodes // 2
    assert half > cull.limits().lower
    for mode in ("table", "trilinear", "shade"):
        frames = []
        for culled in (True, False):
            fb, n = None, 0
            for t in nongrid.passes_of(s, [(0, half), (half, s.n_nodes)]):
                fb, k, regimes = cull.render(t, mode, culled, fb=fb)
                assert (regimes == cull.CULLED).all()
                n += k
            frames.append((fb, n))
        assert np.array_equal(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1], (name, mode)
        if name == "hash64":  # (with clip planes every pass starts the reference's loop anew: tests/nongrid.py)
            one, n_one, _ = cull.render(s, mode, True)
            assert np.array_equal(one, frames[0][0]) and n_one == frames[0][1], (name, mode)


# ---- the four regimes, by construction ---------------------------------------------------------------------------------------
def test_the_thresholds_are_the_kernels():
    """cull_limits() against the sources: the condition around the block, the two comparisons with the candidates' array
    and the margins stand in the shared block of vrc_kernel_frame.h, which the kernels of vrc_kernels_mip.h,
    vrc_kernels_shade.hip and vrc_kernels_cdepth.hip each call once, carrying none of them themselves -- and once each in
    vrc_kernels.hip, whose code object is held to the last byte and did not stay so with the call, and in
    vrc_kernels_preint.hip, whose 8-bit point-sampled instance ran 6-7 % slower over the shared pieces; nowhere else.
    The tile is the wave's, and the candidates' array is the macro of vrc_core.h."""
    lim = cull.limits()
    block, own = "vrc_kernel_frame.h", ("vrc_kernels.hip", "vrc_kernels_preint.hip")
    callers = ("vrc_kernels_mip.h", "vrc_kernels_shade.hip", "vrc_kernels_cdepth.hip")
    pieces = (r"f\.nodeCount > (\d+)u && f\.nodeCount <= (\d+)u", r"at < VRC_TILE_CANDIDATES", r"nCand <= VRC_TILE_CANDIDATES",
              r"- 1\.0f, r0 - 1\.0f", r"r1 \+ 1\.0f")
    sources = sorted(n for n in os.listdir(CSRC) if n.endswith((".h", ".hip")))
    assert block in sources and all(k in sources for k in own + callers)
    for f in sources:
        text = open(os.path.join(CSRC, f)).read()
        counts = [len(re.findall(p, text)) for p in pieces]
        assert counts == ([1] * len(pieces) if f == block or f in own else [0] * len(pieces)), (f, counts)
        calls = len(re.findall(r"vrc_frame_cull_tile< DDA >\(", text))
        assert calls == (1 if f in callers else 0), (f, calls)
        if f in callers:
            assert '#include "%s"' % block in text, f
        if f == block or f in own:
            m = re.findall(pieces[0], text)
            assert (int(m[0][0]), int(m[0][1])) == (lim.lower, lim.upper), (f, m)
    assert len(re.findall(r"vrc_frame_cull_tile\(", open(os.path.join(CSRC, block)).read())) == 1, "one definition"
    core = open(os.path.join(CSRC, "vrc_core.h")).read()
    assert int(re.search(r"#define VRC_TILE_CANDIDATES (\d+)u", core).group(1)) == lim.candidates
    internal = open(os.path.join(CSRC, "vrc_internal.h")).read()
    assert int(re.search(r"#define VRC_TILE_W (\d+)u", internal).group(1)) == lim.tile_w and lim.tile_w * lim.tile_h == 64
    assert lim.upper < 2 ** 16, "the candidates are 16-bit indices"


def test_the_four_regimes_at_their_boundaries():
    lim = cull.limits()
    s = cull.scene("dense8")
    assert s.W == lim.tile_w and s.H == lim.tile_h
    kept, counts, _ = cull.tile_masks(s)
    assert kept.shape == (1, s.n_nodes) and kept.all() and s.n_nodes > lim.candidates + 1, "the one tile keeps the whole list"
    lists = [(cull.first(s, lim.lower), cull.SHORT), (cull.first(s, lim.lower + 1), cull.CULLED),
             (cull.first(s, lim.candidates), cull.CULLED), (cull.first(s, lim.candidates + 1), cull.OVERFLOW),
             (cull.padded(s, lim.upper), cull.OVERFLOW), (cull.padded(s, lim.upper + 1), cull.LONG),
             (cull.padded(cull.first(s, lim.candidates), lim.upper, "interleaved"), cull.CULLED),
             (cull.padded(cull.first(s, lim.candidates), lim.upper + 1, "interleaved"), cull.LONG)]
    for t, regime in lists:
        for flavour in _flavours():
            a, na, regimes = cull.render(t, "table", True, flavour=flavour)
            b, nb, _ = cull.render(t, "table", False, flavour=flavour)
            assert regimes.tolist() == [regime], (t.n_nodes, regimes, regime)
            assert np.array_equal(a, b) and na == nb and na > 0, (t.n_nodes, regime)
    # the culled list of the wave's array filled to the last entry is the frame of the same bricks unpadded
    full, n_full, _ = cull.render(cull.first(s, lim.candidates), "table", True)
    far, n_far, _ = cull.render(lists[6][0], "table", True)
    assert np.array_equal(full, far) and n_full == n_far
    # a frame of several tiles on both sides of the array's size
    w = cull.scene("dense8_wide")
    _, counts, regimes = cull.tile_masks(w)
    assert set(regimes.tolist()) == {cull.CULLED, cull.OVERFLOW} and ((counts > lim.candidates) == (regimes == cull.OVERFLOW)).all()
    _assert_culled_equals_plain(w, "dense8_wide", ["table"])


# ---- the stand-alone sanitizer program ---------------------------------------------------------------------------------------
def _dump(path, s, row_map=None):
    """The scene as the flat file tests/host_san/cull_selftest.cpp reads: a header of uint32 words, then the arrays."""
    rows = np.asarray(row_map if row_map is not None else [], dtype=np.uint32)
    head = np.array([0x4C4C5543, s.atlas.dtype.itemsize] + list(s.atlas_dim) + list(s.slot_dim) +
                    [s.W, len(rows) if len(rows) else s.H, len(s.planes), s.n_nodes, len(rows), orc.C.sizeof(orc.ViewData),
                     orc.C.sizeof(orc.NodeData), orc.C.sizeof(orc.RenderData)], dtype=np.uint32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(bytes(s.view))
        f.write(bytes(s.render))
        f.write(np.ascontiguousarray(s.planes, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(s.tf, dtype=np.float32).tobytes())
        f.write(rows.tobytes())
        f.write(bytes(s.nodes)[:s.n_nodes * orc.C.sizeof(orc.NodeData)])
        f.write(np.ascontiguousarray(s.atlas).tobytes())


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/host_san/cull_selftest.cpp: the culling loop and both loops of the lanes with the wave's array allocated to
    its exact size, on the lists that fill it to the last entry and overflow it by one, and on a row-map frame."""
    lim = cull.limits()
    s = cull.scene("dense8")
    files = []
    for name, t, rows in (("fill", cull.first(s, lim.candidates), None), ("overflow", cull.first(s, lim.candidates + 1), None),
                          ("rows", cull.scene("hash64"), cull.ROW_MAP)):
        files.append(str(tmp_path / (name + ".bin")))
        _dump(files[-1], t, rows)
    exe = str(tmp_path / "cull_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           os.path.join(orc.ROOT, "tests", "host_san", "cull_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "DONE" in out.stdout, text
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text
    assert "fill.bin: regime %d" % cull.CULLED in text and "overflow.bin: regime %d" % cull.OVERFLOW in text, text
    assert text.count("equal 1") == 3, text


def test_tally():
    """(prints what the module checked: run with -s)"""
    for (family, flavour), (pairs, kept, need) in sorted(TALLY.items()):
        print("%-20s %-4s %9d pairs  kept %8d  needed %8d  kept/needed %.2f" % (family, flavour or "g++", pairs, kept, need, kept / max(1, need)))
