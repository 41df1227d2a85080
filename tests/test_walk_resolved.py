"""The resolved visit words of the uniform-only replay on the GPU (VRC_OPT_WALK_RESOLVED, VRC_OPT_WALK_RESOLVED_USED;
include/vrc_hip.h).

At 1 (the default) an uncounted frame replayed by the uniform-only instance reads one word per visit, resolved once from
the lists and the bricks' uniformity words (vrc_core.h: vrc_walk_resolved_word); at 0 it reads the list word and the
uniformity word of every visit as it always did.  Nothing of the result may change: on one view, from one set of lists,
the frames of option 0, 1 and 0 again are equal bit for bit (numpy.array_equal); the read-back says 1 exactly on the
frames that were handed the words; and changing the option keeps the lists (VRC_OPT_WALK_CACHE_USED stays 4).  No
tolerance appears.  The option-0 frames are what tests/test_walk_cache.py, tests/test_walk_lean.py and
tests/test_walk_uniform_only.py hold to the walked frame.

The scene is that of tests/test_first_visit_table.py -- mem:// 128^3 in bricks of 32 with 512 samples per ray -- at
128 x 128 and at 100 x 76, whose last tiles in x and y are partial."""
import copy

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import orc
from test_walk_cache import _get, _gpu, _opt, always, mode, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

VIEWPORT = (128, 128)
PARTIAL = (100, 76)
TURNED = (0.5236, 0.3491)
_built = {}


def scene(volume="mem", viewport=VIEWPORT, spin=(0.0, 0.0)):
    key = (volume, viewport, spin)
    if key not in _built:
        _built[key] = orc.build_scene(voxels=(128, 128, 128), block=32, viewport=viewport, volume=volume, spin=spin, spr=512)
    return copy.copy(_built[key])


def used(vrc, g):
    return _get(vrc, g, vrc.OPT_WALK_RESOLVED_USED)


def until_replayed(vrc, g, what, **kw):
    """Uncounted frames until the view is replayed; the read-back is 0 on every frame that is not."""
    for _ in range(8):
        g.render(count=False, **kw)
        if mode(vrc, g) == 4:
            return
        assert used(vrc, g) == 0, what
    raise AssertionError("%s: never replayed" % what)


def zero_one_zero(vrc, g, what, uniform=1, handed=1, **kw):
    """Option 0, 1 and 0 on g's view, uncounted: one set of lists, three equal frames.  Returns the frame."""
    assert _get(vrc, g, vrc.OPT_WALK_RESOLVED) == 1  # the default: the frames on the way to the replay run under it
    until_replayed(vrc, g, what, **kw)
    assert used(vrc, g) == handed, what  # the first frame that is handed the instance builds the words and reads them
    got = []
    for value in (0, 1, 0):
        _opt(vrc, g, vrc.OPT_WALK_RESOLVED, value)
        fb, _, _ = g.render(count=False, **kw)
        assert mode(vrc, g) == 4, "%s: option %d started the lists over" % (what, value)
        assert used(vrc, g) == value * handed, (what, value)
        assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1 and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform, what
        name = g.L.vrc_last_kernel()
        assert name.startswith(b"vrc_k_raycast_replay<false,") and name.endswith(b",uniform,lean>") == (uniform == 1), (what, name)
        got.append(fb)
    _opt(vrc, g, vrc.OPT_WALK_RESOLVED, 1)
    for value, fb in zip((1, 0), got[1:]):
        assert np.array_equal(fb, got[0]), "%s: option %d, %d pixels differ" % (what, value, int((fb != got[0]).any(axis=-1).sum()))
    return got[0]


@pytest.mark.parametrize("viewport", [VIEWPORT, PARTIAL])
@pytest.mark.parametrize("spin", [(0.0, 0.0), TURNED])
def test_two_views_under_three_transfer_functions(vrc, spin, viewport):
    with _gpu(scene(viewport=viewport, spin=spin)) as g:
        for alpha, coloured in ((0.05, False), (1.0, False), (0.3, True)):
            g.s.tf = table(alpha, coloured)
            what = "mem %r spin %r alpha %g coloured %d" % (viewport, spin, alpha, coloured)
            fb = zero_one_zero(vrc, g, what)
            assert (b"<false,3," in g.L.vrc_last_kernel()) == (not coloured), what  # the grey form and the four-float one
            assert fb[..., 3].max() > 0.05 and (fb[..., 3] == 0.0).any(), what  # rays that hit and rays that miss
            if alpha == 1.0:
                assert fb[..., 3].max() > 0.999, "rays end early"


def test_a_counted_frame_reads_the_lists(vrc):
    s = scene(spin=TURNED)
    s.tf = table(0.3, False)
    with _gpu(s) as g:
        plain = zero_one_zero(vrc, g, "uncounted")
        counted = {}
        for value in (0, 1):
            _opt(vrc, g, vrc.OPT_WALK_RESOLVED, value)
            fb, n, _ = g.render(count=True)
            assert mode(vrc, g) == 4 and used(vrc, g) == 0, value
            assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_replay<true,"), value
            counted[value] = (fb, n)
        assert counted[1][1] == counted[0][1] > 0
        assert np.array_equal(counted[1][0], counted[0][0]) and np.array_equal(counted[1][0], plain)
        # and the words are still there for the uncounted frame behind it
        fb, _, _ = g.render(count=False)
        assert mode(vrc, g) == 4 and used(vrc, g) == 1 and np.array_equal(fb, plain)


def test_two_passes(vrc):
    # the same node list twice in one frame: the second pass composites onto the first (clearFirst = 0, the four-float
    # form) and reads the same words
    s = scene(viewport=PARTIAL, spin=TURNED)
    s.tf = table(0.05, False)
    with _gpu(s) as g:
        twice = [(0, s.n_nodes), (0, s.n_nodes)]
        once = zero_one_zero(vrc, g, "one pass")
        both = zero_one_zero(vrc, g, "two passes", passes=twice)
        assert not np.array_equal(once, both) and (both[..., 3] >= once[..., 3]).all()


def test_row_bands(vrc):
    s = scene(spin=TURNED)
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(2, 13)) + list(range(17, 27)) + list(range(60, 101)), dtype=np.uint32)
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g:
        whole = zero_one_zero(vrc, g, "whole frame")
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        g.s = copy.copy(banded)
        part = zero_one_zero(vrc, g, "row bands")
        assert np.array_equal(part, whole[rows])


def test_a_view_that_gathers_is_not_handed_the_words(vrc):
    s = scene("hash", viewport=PARTIAL, spin=(0.5, 0.35))
    s.tf = table(0.05, False)
    with _gpu(s) as g:
        always(vrc, g)
        fb = zero_one_zero(vrc, g, "hash", uniform=0, handed=0)
        assert fb[..., 3].max() > 0.05


def test_a_budget_too_small_for_the_words_keeps_the_lists(vrc):
    s = scene(viewport=PARTIAL, spin=TURNED)
    s.tf = table(0.3, False)
    with _gpu(s) as g:
        want = zero_one_zero(vrc, g, "default budget")
        lists = _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES)
        plane = 13 * 10 * 64 * 4  # bytes of one plane: whole tiles
        visits = (lists // plane - 1) // 4
        assert lists == (1 + 4 * visits) * plane and visits >= 2, lists
        # the lists fit, the words beside them do not by one byte (a new budget starts the lists over)
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, lists + visits * plane - 1)
        fb = zero_one_zero(vrc, g, "lists and no words", handed=0)
        assert np.array_equal(fb, want)
        # and with that byte they do
        _opt(vrc, g, vrc.OPT_WALK_CACHE_BUDGET, lists + visits * plane)
        fb = zero_one_zero(vrc, g, "lists and words")
        assert np.array_equal(fb, want)


# the upload case of tests/test_walk_uniform_only.py: an upload turns a uniform brick into a mixed one while the lists
# and the words are valid.  The frames after it are the walked ones and read no words; with the brick put back the view
# is replayed by the uniform-only instance again -- at 1 by itself, at VRC_WALK_CACHE_ALWAYS once the lists start over
# (until then they stay, and the frame reads them) -- from words built anew
@pytest.mark.parametrize("option", [1, 2])
def test_an_upload_drops_the_words_and_the_next_uniform_replay_builds_them_again(vrc, option):
    s = scene(viewport=PARTIAL, spin=TURNED)
    s.tf = table(0.3, False)
    nid = s.sorted_ids[len(s.sorted_ids) // 2]
    kept = np.ascontiguousarray(s.bricks[nid])
    noise = np.random.default_rng(7).integers(30, 230, size=kept.shape, dtype=np.uint8)
    assert noise.dtype == kept.dtype and noise.min() != noise.max() and kept.min() == kept.max()
    size = vrc.u32x3(noise.shape[2], noise.shape[1], noise.shape[0])

    def upload(brick):
        for x in (g, ref):
            slot = vrc.f32x3()
            vrc.check(x.L, x.L.vrc_pool_release_slot(x.pool, vrc.f32x3(*x.slots[nid])))
            vrc.check(x.L, x.L.vrc_pool_copy_to_slot(x.pool, brick.ctypes.data, size, slot))
            assert (slot[0], slot[1], slot[2]) == x.slots[nid]

    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_CACHE, option)
        before = zero_one_zero(vrc, g, "before the upload")
        walked, _, _ = ref.render(count=False)
        assert mode(vrc, ref) == 0 and used(vrc, ref) == 0 and np.array_equal(before, walked)
        upload(noise)
        walked, _, _ = ref.render(count=False)
        assert not np.array_equal(before, walked)
        for i in range(6):
            fb, _, _ = g.render(count=False)
            assert used(vrc, g) == 0 and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == 0, i
            assert np.array_equal(fb, walked), "frame %d after the upload (mode %d)" % (i, mode(vrc, g))
        upload(kept)
        walked, _, _ = ref.render(count=False)
        assert np.array_equal(before, walked)
        if option == 2:  # the lists have outlived both uploads, what their count pass said of the bricks has not
            fb, _, _ = g.render(count=False)
            assert mode(vrc, g) == 4 and used(vrc, g) == 0 and np.array_equal(fb, walked)
            _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
            _opt(vrc, g, vrc.OPT_WALK_CACHE, option)
        again = zero_one_zero(vrc, g, "the brick put back")
        assert np.array_equal(again, before)


def test_the_option_and_its_read_back(vrc):
    with _gpu(scene()) as g:
        assert _get(vrc, g, vrc.OPT_WALK_RESOLVED) == 1 and used(vrc, g) == 0
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_RESOLVED, 2) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_RESOLVED, -1) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_RESOLVED_USED, 1) == vrc.VRC_EINVAL
        assert _get(vrc, g, vrc.OPT_WALK_RESOLVED) == 1
        # a view that is never replayed is never handed the words
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        for _ in range(3):
            g.render(count=False)
            assert mode(vrc, g) == 0 and used(vrc, g) == 0
