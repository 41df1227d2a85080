"""The free body of the lean march on the GPU (VRC_OPT_LEAN_FREE_MARCH, VRC_OPT_LEAN_FREE_MARCH_USED; include/vrc_hip.h).

At 1 (the default) an uncounted replayed lean frame marches a uniform visit without the early-exit test where the visit
cannot reach the exit threshold (vrc_core.h: vrc_lean_free_visit, vrc_march_uniform_free); at 0 every lane takes the
tested march, as it always did.  Nothing of the result may change: on one view, from one set of lists, the frames of
option 0, 1 and 0 again are equal bit for bit (numpy.array_equal); the read-back says 1 exactly on the frames that were
allowed the body; and changing the option keeps the lists (VRC_OPT_WALK_CACHE_USED stays 4).  No tolerance appears.  The
option-0 frames are what tests/test_walk_cache.py, tests/test_walk_lean.py and tests/test_walk_uniform_only.py hold to
the walked frame.

The scene is mem:// 128^3 in bricks of 32 at 128 x 128 with 512 samples per ray: four slabs of bricks.  Three transfer
functions: a ramp of alpha 0.05, under which no visit fails the pre-test; alpha 1.0, under which most do and rays end
early; and one in between, found by bisection so that the most opaque ray ends between 0.99 and the exit threshold: such
a ray's last visit fails the pre-test (w_0 + n e.w >= w_n > 0.99), its first ones and its neighbours' pass, and no ray
ends early -- both bodies in one wave.  The first-visit table is left at its default except where a test says otherwise,
so the later visits are the ones marched; with it at 0 the first visit, from zero, is marched by the free body too."""
import copy

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import orc
from test_walk_cache import _get, _gpu, _opt, always, mode, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

VIEWPORT = (128, 128)
VIEWS = [(0.0, 0.0), (0.5, 0.35)]
_built = {}


def scene(volume="mem", spin=(0.0, 0.0)):
    key = (volume, spin)
    if key not in _built:
        _built[key] = orc.build_scene(voxels=(128, 128, 128), block=32, viewport=VIEWPORT, volume=volume, spin=spin, spr=512)
    return copy.copy(_built[key])


def used(vrc, g):
    return _get(vrc, g, vrc.OPT_LEAN_FREE_MARCH_USED)


def until_replayed(vrc, g, what, **kw):
    """Uncounted frames until the view is replayed; the read-back is 0 on every frame that is not."""
    for _ in range(8):
        g.render(count=False, **kw)
        if mode(vrc, g) == 4:
            return
        assert used(vrc, g) == 0, what
    raise AssertionError("%s: never replayed" % what)


def zero_one_zero(vrc, g, what, uniform, **kw):
    """Option 0, 1 and 0 on g's view, uncounted: one set of lists, three equal frames.  Returns the frame."""
    assert _get(vrc, g, vrc.OPT_LEAN_FREE_MARCH) == 1  # the default: the frames on the way to the replay run under it
    until_replayed(vrc, g, what, **kw)
    got = []
    for value in (0, 1, 0):
        _opt(vrc, g, vrc.OPT_LEAN_FREE_MARCH, value)
        fb, _, _ = g.render(count=False, **kw)
        assert mode(vrc, g) == 4, "%s: option %d started the lists over" % (what, value)
        assert used(vrc, g) == value, (what, value)
        assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1 and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform, what
        assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_replay<false,"), what
        got.append(fb)
    _opt(vrc, g, vrc.OPT_LEAN_FREE_MARCH, 1)
    for value, fb in zip((1, 0), got[1:]):
        assert np.array_equal(fb, got[0]), "%s: option %d, %d pixels differ" % (what, value, int((fb != got[0]).any(axis=-1).sum()))
    return got[0]


def alpha_between(vrc, g):
    """The ramp's alpha under which the frame's most opaque ray ends in (0.99, 0.999): bisection on rendered frames (the
    final opacity rises with the ramp's alpha).  Found with the option at 0, so that nothing under test chooses it."""
    _opt(vrc, g, vrc.OPT_LEAN_FREE_MARCH, 0)
    lo, hi = 0.05, 1.0
    try:
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            g.s.tf = table(mid, False)
            top = float(g.render(count=False)[0][..., 3].max())
            if 0.99 < top < 0.999:
                return mid
            lo, hi = (mid, hi) if top <= 0.99 else (lo, mid)
    finally:
        _opt(vrc, g, vrc.OPT_LEAN_FREE_MARCH, 1)
    raise AssertionError("no ramp ends the most opaque ray between 0.99 and the threshold")


@pytest.mark.parametrize("spin", VIEWS)
def test_three_transfer_functions_and_a_coloured_one(vrc, spin):
    with _gpu(scene(spin=spin)) as g:
        between = alpha_between(vrc, g)
        for alpha, coloured in ((0.05, False), (1.0, False), (between, False), (between, True), (1.0, True)):
            g.s.tf = table(alpha, coloured)
            what = "mem spin %r alpha %g coloured %d" % (spin, alpha, coloured)
            fb = zero_one_zero(vrc, g, what, 1)
            assert g.L.vrc_last_kernel().endswith(b",uniform,lean>"), what
            assert (b"<false,3," in g.L.vrc_last_kernel()) == (not coloured), what  # the grey form and the four-float one
            top = fb[..., 3].max()
            if alpha == 0.05:
                assert 0.05 < top < 0.99, "no visit of this frame fails the pre-test"
            elif alpha == 1.0:
                assert top > 0.999, "rays end early"
            else:
                seen = fb[..., 3][fb[..., 3] > 0]
                assert 0.99 < top < 0.999 and seen.min() < 0.9, "both bodies, and no ray ends early"


def test_the_first_visit_marched_from_zero(vrc):
    # without the table every visit is marched, the first one from a start alpha of exactly zero
    s = scene(spin=VIEWS[1])
    with _gpu(s) as g:
        _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, 0)
        with_table = None
        for alpha in (0.05, 1.0):
            g.s.tf = table(alpha, False)
            fb = zero_one_zero(vrc, g, "no table, alpha %g" % alpha, 1)
            assert _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE_USED) == 0
            _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, 1)
            for _ in range(3):  # (the second frame of a transfer function builds the table)
                with_table, _, _ = g.render(count=False)
            assert _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE_USED) == 1 and used(vrc, g) == 1
            assert np.array_equal(with_table, fb)
            _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, 0)


def test_a_second_pass_into_the_buffer_starts_above_zero(vrc):
    # the same node list twice in one frame: the second pass composites onto the first (clearFirst = 0), so its visits
    # start from the alpha the first pass left -- the pre-test reads it, and the pass is allowed the body like any other
    s = scene(spin=VIEWS[1])
    with _gpu(s) as g:
        twice = [(0, s.n_nodes), (0, s.n_nodes)]
        for alpha in (0.05, alpha_between(vrc, g)):
            g.s.tf = table(alpha, False)
            once = zero_one_zero(vrc, g, "one pass, alpha %g" % alpha, 1)
            both = zero_one_zero(vrc, g, "two passes, alpha %g" % alpha, 1, passes=twice)
            assert not np.array_equal(once, both) and (both[..., 3] >= once[..., 3]).all()


def test_a_counted_frame_keeps_the_tested_march(vrc):
    s = scene(spin=VIEWS[1])
    with _gpu(s) as g:
        g.s.tf = table(alpha_between(vrc, g), False)
        plain = zero_one_zero(vrc, g, "uncounted", 1)
        counted = {}
        for value in (0, 1, 0):
            _opt(vrc, g, vrc.OPT_LEAN_FREE_MARCH, value)
            fb, n, _ = g.render(count=True)
            assert mode(vrc, g) == 4 and used(vrc, g) == 0, value
            assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_replay<true,"), value
            assert n > 0 and np.array_equal(fb, plain), value
            counted.setdefault(value, n)
            assert counted[value] == n
        assert counted[1] == counted[0]


def test_bricks_that_gather(vrc):
    s = scene("hash", spin=(0.5, 0.35))
    with _gpu(s) as g:
        always(vrc, g)
        for alpha, coloured in ((0.05, False), (1.0, True)):
            g.s.tf = table(alpha, coloured)
            what = "hash alpha %g coloured %d" % (alpha, coloured)
            fb = zero_one_zero(vrc, g, what, 0)
            assert g.L.vrc_last_kernel().endswith(b",lean>") and b"uniform" not in g.L.vrc_last_kernel(), what
            assert fb[..., 3].max() > 0.05, what


def test_row_bands(vrc):
    s = scene(spin=VIEWS[1])
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(2, 13)) + list(range(17, 27)) + list(range(60, 101)), dtype=np.uint32)
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g:
        whole = zero_one_zero(vrc, g, "whole frame", 1)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        g.s = copy.copy(banded)
        part = zero_one_zero(vrc, g, "row bands", 1)
        assert np.array_equal(part, whole[rows])


def test_the_option_and_its_read_back(vrc):
    with _gpu(scene()) as g:
        assert _get(vrc, g, vrc.OPT_LEAN_FREE_MARCH) == 1 and used(vrc, g) == 0
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_LEAN_FREE_MARCH, 2) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_LEAN_FREE_MARCH, -1) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_LEAN_FREE_MARCH_USED, 1) == vrc.VRC_EINVAL
        assert _get(vrc, g, vrc.OPT_LEAN_FREE_MARCH) == 1
        # a view that is never replayed is never allowed the body
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        for _ in range(3):
            g.render(count=False)
            assert mode(vrc, g) == 0 and used(vrc, g) == 0
