"""The first-visit table of the lean replay on the GPU (VRC_OPT_FIRST_VISIT_TABLE, VRC_OPT_FIRST_VISIT_TABLE_USED;
include/vrc_hip.h).

At 1 (the default) an uncounted replayed lean frame that starts from cleared pixels takes the result of a ray's first
visit, where that is a uniform brick of fewer than 256 steps, from a table built from the classified table
(vrc_core.h: vrc_first_visit_row); at 0 it marches that visit as it always did.  Nothing of the result may change: on
one view, from one set of lists, the frames of option 0, 1 and 0 again are equal bit for bit (numpy.array_equal); the
read-back says 1 exactly on the frames that were handed the table; and changing the option keeps the lists
(VRC_OPT_WALK_CACHE_USED stays 4).  No tolerance appears.  The option-0 frames are what tests/test_walk_cache.py,
tests/test_walk_lean.py and tests/test_walk_uniform_only.py hold to the walked frame.

The scene is mem:// 128^3 in bricks of 32 at 128 x 128 with 512 samples per ray: four slabs of bricks, first visits of 0
to about 150 steps.  In bricks of 64 every whole first visit takes 256 steps or more and is marched with the table
handed over."""
import copy

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import orc
from test_walk_cache import _get, _gpu, _opt, always, mode, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

VIEWPORT = (128, 128)
TURNED = (0.5236, 0.3491)
_built = {}


def scene(volume="mem", block=32, spin=(0.0, 0.0)):
    key = (volume, block, spin)
    if key not in _built:
        _built[key] = orc.build_scene(voxels=(128, 128, 128), block=block, viewport=VIEWPORT, volume=volume, spin=spin, spr=512)
    return copy.copy(_built[key])


def used(vrc, g):
    return _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE_USED)


def until_replayed(vrc, g, what, **kw):
    """Uncounted frames until the view is replayed; the read-back is 0 on every frame that is not."""
    for _ in range(8):
        g.render(count=False, **kw)
        if mode(vrc, g) == 4:
            return
        assert used(vrc, g) == 0, what
    raise AssertionError("%s: never replayed" % what)


def zero_one_zero(vrc, g, what, uniform, handed=1, **kw):
    """Option 0, 1 and 0 on g's view, uncounted: one set of lists, three equal frames.  Returns the frame."""
    assert _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE) == 1  # the default: the frames on the way to the replay run under it
    until_replayed(vrc, g, what, **kw)
    got = []
    for value in (0, 1, 0):
        _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, value)
        fb, _, _ = g.render(count=False, **kw)
        assert mode(vrc, g) == 4, "%s: option %d started the lists over" % (what, value)
        assert used(vrc, g) == value * handed, (what, value)
        assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1 and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform, what
        assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_replay<false,"), what
        got.append(fb)
    _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, 1)
    for value, fb in zip((1, 0), got[1:]):
        assert np.array_equal(fb, got[0]), "%s: option %d, %d pixels differ" % (what, value, int((fb != got[0]).any(axis=-1).sum()))
    return got[0]


@pytest.mark.parametrize("spin", [(0.0, 0.0), TURNED])
def test_the_uniform_only_replay_under_three_transfer_functions(vrc, spin):
    with _gpu(scene(spin=spin)) as g:
        for alpha, coloured in ((0.05, False), (1.0, False), (0.3, True)):
            g.s.tf = table(alpha, coloured)
            what = "mem spin %r alpha %g coloured %d" % (spin, alpha, coloured)
            fb = zero_one_zero(vrc, g, what, 1)
            assert g.L.vrc_last_kernel().endswith(b",uniform,lean>"), what
            assert (b"<false,3," in g.L.vrc_last_kernel()) == (not coloured), what  # the grey form and the four-float one
            assert fb[..., 3].max() > 0.05, what
            if alpha == 1.0:
                assert fb[..., 3].max() > 0.999, "rays end early, inside their first brick"


def test_first_visits_longer_than_the_rows_are_marched(vrc):
    s = scene(block=64)
    s.tf = table(0.05, False)
    with _gpu(s) as g:
        fb = zero_one_zero(vrc, g, "mem in bricks of 64", 1)
        assert fb[..., 3].max() > 0.05


def test_a_second_pass_into_the_buffer_does_not_read_the_table(vrc):
    # the same node list twice in one frame: the second pass composites onto the first (clearFirst = 0), so it is not
    # handed the table -- the read-back, which is the last pass's, says 0 under either option
    s = scene(spin=TURNED)
    s.tf = table(0.05, False)
    with _gpu(s) as g:
        twice = [(0, s.n_nodes), (0, s.n_nodes)]
        once = zero_one_zero(vrc, g, "one pass", 1)
        both = zero_one_zero(vrc, g, "two passes", 1, handed=0, passes=twice)
        assert not np.array_equal(once, both) and (both[..., 3] >= once[..., 3]).all()


def test_a_counted_frame_marches_every_visit(vrc):
    s = scene(spin=TURNED)
    s.tf = table(0.3, False)
    with _gpu(s) as g:
        plain = zero_one_zero(vrc, g, "uncounted", 1)
        counted = {}
        for value in (0, 1):
            _opt(vrc, g, vrc.OPT_FIRST_VISIT_TABLE, value)
            fb, n, _ = g.render(count=True)
            assert mode(vrc, g) == 4 and used(vrc, g) == 0, value
            assert g.L.vrc_last_kernel().startswith(b"vrc_k_raycast_replay<true,"), value
            counted[value] = (fb, n)
        assert counted[1][1] == counted[0][1] > 0
        assert np.array_equal(counted[1][0], counted[0][0]) and np.array_equal(counted[1][0], plain)


def test_first_visits_that_gather(vrc):
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
    s = scene(spin=TURNED)
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


def test_an_edit_a_frame_builds_nothing_and_the_second_frame_of_a_table_does(vrc):
    s = scene(spin=TURNED)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_FIRST_VISIT_TABLE, 0)
        g.s.tf = ref.s.tf = table(0.05, False)
        until_replayed(vrc, g, "the edited view")
        until_replayed(vrc, ref, "the reference")

        def frame(alpha, coloured, want):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            fb, _, _ = g.render(count=False)
            assert mode(vrc, g) == 4 and used(vrc, g) == want, (alpha, coloured, want)
            wfb, _, _ = ref.render(count=False)
            assert mode(vrc, ref) == 4 and used(vrc, ref) == 0
            assert np.array_equal(fb, wfb), (alpha, coloured, want)

        for alpha, coloured in ((0.1, False), (0.2, False), (0.6, True), (0.4, False)):  # a new transfer function every frame
            frame(alpha, coloured, 0)
        frame(0.5, False, 0)  # the first frame of this one: still marched
        frame(0.5, False, 1)  # the second: built and used
        frame(0.5, False, 1)


def test_the_option_and_its_read_back(vrc):
    with _gpu(scene()) as g:
        assert _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE) == 1 and used(vrc, g) == 0
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_FIRST_VISIT_TABLE, 2) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_FIRST_VISIT_TABLE, -1) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_FIRST_VISIT_TABLE_USED, 1) == vrc.VRC_EINVAL
        assert _get(vrc, g, vrc.OPT_FIRST_VISIT_TABLE) == 1
        # a view that is never replayed is never handed the table
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        for _ in range(3):
            g.render(count=False)
            assert mode(vrc, g) == 0 and used(vrc, g) == 0
