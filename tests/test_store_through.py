"""Write-through pixel stores of the replayed frame on the GPU (VRC_OPT_STORE_THROUGH, VRC_OPT_STORE_THROUGH_USED;
include/vrc_hip.h).

At 1 (the default) a replayed frame stores its pixels with 16-byte write-through stores through a buffer resource
(vrc_core.h: vrc_store_pixel); at 0 with the plain stores it always had.  Nothing of the result may change: on one view,
from one set of lists, the frames of option 0, 1 and 0 again are equal bit for bit (numpy.array_equal), and so are their
sample counts; the read-back says 1 exactly on the replayed frames of option 1; and changing the option keeps the lists
(VRC_OPT_WALK_CACHE_USED stays 4).  No tolerance appears.  The option-0 frames are what tests/test_walk_cache.py,
tests/test_walk_lean.py and tests/test_walk_uniform_only.py hold to the walked frame.

The C ABI has no switch for the form of the lists: the host takes the lean form where the step allows it.  The lean and
the other form are therefore reached as tests/test_walk_lean.py reaches them, with 256 and 300 samples per ray, and each
case asserts which one it got (VRC_OPT_WALK_LEAN_USED)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import orc
from test_walk_cache import _get, _gpu, _opt, always, mode, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

VOXELS, BLOCK = (64, 64, 64), 16
VIEWPORT = (40, 24)  # 5 x 3 whole tiles of 8 x 8
ODD = (43, 29)  # 6 x 4 tiles: neither side a multiple of 8, so the edge tiles have lanes outside the frame, and the
#                 frame's last byte is not the last byte of a tile row
TURNED = (0.5236, 0.3491)
_built = {}


def scene(volume, spin=(0.0, 0.0), viewport=ODD, spr=0, **kw):
    key = (volume, spin, viewport, spr, repr(sorted(kw.items())))
    if key not in _built:
        _built[key] = orc.build_scene(voxels=VOXELS, block=BLOCK, viewport=viewport, volume=volume, spin=spin, spr=spr, **kw)
    return copy.copy(_built[key])


def through(vrc, g):
    return _get(vrc, g, vrc.OPT_STORE_THROUGH_USED)


def until_replayed(vrc, g, what, **kw):
    """Frames until the view is replayed; the read-back is 0 on every frame that is not."""
    for _ in range(8):
        g.render(**kw)
        if mode(vrc, g) == 4:
            return
        assert through(vrc, g) == 0, what
    raise AssertionError("%s: never replayed" % what)


def zero_one_zero(vrc, g, what, lean, uniform, **kw):
    """Option 0, 1 and 0 on g's view: one set of lists, three equal frames.  Returns the frame."""
    assert _get(vrc, g, vrc.OPT_STORE_THROUGH) == 1  # the default: the frames on the way to the replay run under it
    until_replayed(vrc, g, what, **kw)
    got = []
    for value in (0, 1, 0):
        _opt(vrc, g, vrc.OPT_STORE_THROUGH, value)
        fb, n, _ = g.render(**kw)
        assert mode(vrc, g) == 4, "%s: option %d started the lists over" % (what, value)
        assert through(vrc, g) == value, (what, value)
        assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == lean and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform, what
        assert b"vrc_k_raycast_replay<" in g.L.vrc_last_kernel(), what
        got.append((fb, n))
    _opt(vrc, g, vrc.OPT_STORE_THROUGH, 1)
    for value, (fb, n) in zip((1, 0), got[1:]):
        assert np.array_equal(fb, got[0][0]), "%s: option %d, %d pixels differ" % (
            what, value, int((fb != got[0][0]).any(axis=-1).sum()))
        assert n == got[0][1] and (n > 0) == kw.get("count", True), (what, value, n, got[0][1])
    return got[0]


@pytest.mark.parametrize("viewport", [VIEWPORT, ODD])
@pytest.mark.parametrize("spin", [(0.0, 0.0), TURNED])
def test_the_uniform_only_lean_replay(vrc, spin, viewport):
    s = scene("mem", spin, viewport)
    with _gpu(s) as g:
        for alpha, coloured in ((0.05, False), (1.0, True)):
            g.s.tf = table(alpha, coloured)
            what = "mem %r spin %r alpha %g coloured %d" % (viewport, spin, alpha, coloured)
            fb, _ = zero_one_zero(vrc, g, what, 1, 1)
            assert g.L.vrc_last_kernel().endswith(b",uniform,lean>"), what
            assert fb[..., 3].max() > 0.05, what
            zero_one_zero(vrc, g, what + " uncounted", 1, 1, count=False)


@pytest.mark.parametrize("spr,lean", [(256, 1), (300, 0)])
def test_lists_with_gather_visits_lean_and_not(vrc, spr, lean):
    s = scene("hash", (0.5, 0.35), ODD, spr)
    with _gpu(s) as g:
        always(vrc, g)
        for alpha, coloured in ((0.05, False), (1.0, True)):
            g.s.tf = table(alpha, coloured)
            what = "hash spr %d alpha %g coloured %d" % (spr, alpha, coloured)
            fb, _ = zero_one_zero(vrc, g, what, lean, 0)
            assert g.L.vrc_last_kernel().endswith(b",lean>") == (lean == 1), what
            assert fb[..., 3].max() > 0.05, what
            zero_one_zero(vrc, g, what + " uncounted", lean, 0, count=False)


@pytest.mark.parametrize("volume,spr,lean,uniform", [("mem", 0, 1, 1), ("hash", 256, 1, 0), ("hash", 300, 0, 0)])
def test_rays_without_a_visit_are_cleared_over_a_sentinel(vrc, volume, spr, lean, uniform):
    # seen from the default eye the volume does not fill the viewport: the rays at the rim miss it (count == 0), and the
    # frame's clear is folded into the march, so those pixels are written by the replay's clear store and by nothing else
    s = scene(volume, TURNED, ODD, spr)
    s.tf = table(0.3, False)
    with _gpu(s) as g:
        if volume == "hash":
            always(vrc, g)
        ext = torch.empty((s.H, s.W, 4), dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            until_replayed(vrc, g, volume)
            frames = {}
            for value in (0, 1):
                _opt(vrc, g, vrc.OPT_STORE_THROUGH, value)
                ext.fill_(-77.0)
                torch.cuda.synchronize()
                fb, n, _ = g.render()
                assert mode(vrc, g) == 4 and through(vrc, g) == value
                assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == lean and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform
                frames[value] = (ext.cpu().numpy(), n)
                assert np.array_equal(frames[value][0], fb)
            missed = frames[0][0][..., 3] == 0.0
            assert 0 < missed.sum() < missed.size, "rays that miss and rays that hit"
            assert (frames[1][0][missed] == 0.0).all() and (frames[0][0][missed] == 0.0).all()  # all four floats, exactly
            assert not (frames[1][0] == -77.0).any(), "a pixel of the sentinel is left"
            assert np.array_equal(frames[1][0], frames[0][0]) and frames[1][1] == frames[0][1]
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


@pytest.mark.parametrize("volume,spr,lean,uniform", [("mem", 0, 1, 1), ("hash", 300, 0, 0)])
def test_two_passes_into_one_buffer(vrc, volume, spr, lean, uniform):
    # the same node list twice in one frame: the second pass composites onto the first (clearFirst = 0: it loads the
    # pixel, plainly, and stores it through), and since every vrc_render repeats the one before, both passes are replayed
    s = scene(volume, TURNED, ODD, spr)
    s.tf = table(0.05, False)
    with _gpu(s) as g:
        if volume == "hash":
            always(vrc, g)
        twice = [(0, s.n_nodes), (0, s.n_nodes)]
        once, _ = zero_one_zero(vrc, g, volume + " one pass", lean, uniform)
        both, _ = zero_one_zero(vrc, g, volume + " two passes", lean, uniform, passes=twice)
        assert not np.array_equal(once, both) and (both[..., 3] >= once[..., 3]).all()


def test_row_bands(vrc):
    s = scene("mem", TURNED, ODD)
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(2, 13)) + list(range(17, 27)), dtype=np.uint32)  # 21 rows: a partial tile row
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g:
        whole, _ = zero_one_zero(vrc, g, "whole frame", 1, 1)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        g.s = copy.copy(banded)
        part, _ = zero_one_zero(vrc, g, "row bands", 1, 1)
        assert np.array_equal(part, whole[rows])
        zero_one_zero(vrc, g, "row bands uncounted", 1, 1, count=False)


@pytest.mark.parametrize("volume,spr,lean,uniform", [("mem", 0, 1, 1), ("hash", 256, 1, 0)])
def test_a_consumer_right_behind_the_frame_on_the_same_stream(vrc, volume, spr, lean, uniform):
    # vrc_post_render's copy to the host (every frame of this file is read that way) and, here, torch kernels queued on
    # the context's stream behind a frame that nothing has waited for: a copy and a reduction of the pixel buffer
    s = scene(volume, TURNED, ODD, spr)
    s.tf = table(0.3, False)
    stream = torch.cuda.Stream(device="cuda:0")
    view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
    render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
    nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))
    with _gpu(s) as g:
        vrc.check(g.L, g.L.vrc_ctx_set_stream(g.ctx, C.c_void_p(stream.cuda_stream)))
        if volume == "hash":
            always(vrc, g)
        ext = torch.zeros((s.H, s.W, 4), dtype=torch.float32, device="cuda:0")
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), s.W, s.H))
        try:
            until_replayed(vrc, g, volume)
            seen = {}
            for value in (0, 1, 0):
                _opt(vrc, g, vrc.OPT_STORE_THROUGH, value)
                fb, n, _ = g.render()  # the read-back of vrc_post_render( ctx, host )
                with torch.cuda.stream(stream):
                    ext.fill_(5.0)
                vrc.check(g.L, g.L.vrc_pre_render(g.ctx, view))
                vrc.check(g.L, g.L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
                with torch.cuda.stream(stream):
                    copy_ = ext.clone()
                    total = ext.sum(dtype=torch.float64)
                    alpha = ext[..., 3].max()
                stream.synchronize()
                assert mode(vrc, g) == 4 and through(vrc, g) == value
                assert _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == lean and _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED) == uniform
                assert np.array_equal(copy_.cpu().numpy(), fb), "option %d: the copy behind the frame" % value
                seen.setdefault("fb", fb)
                seen.setdefault("n", n)
                seen.setdefault("total", total.item())
                seen.setdefault("alpha", alpha.item())
                assert np.array_equal(fb, seen["fb"]) and n == seen["n"], value
                assert total.item() == seen["total"] and alpha.item() == seen["alpha"], value
            assert seen["alpha"] == float(seen["fb"][..., 3].max()) > 0.05
            assert abs(seen["total"] - float(np.sum(seen["fb"], dtype=np.float64))) <= 1e-9 * abs(seen["total"])  # (float64 sums
            #                                                        of about 5000 floats in two orders: 1e-16 each, relative)
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))


def test_the_option_and_its_read_back(vrc):
    s = scene("mem", (0.0, 0.0), VIEWPORT)
    with _gpu(s) as g:
        assert _get(vrc, g, vrc.OPT_STORE_THROUGH) == 1 and through(vrc, g) == 0
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_STORE_THROUGH, 2) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_STORE_THROUGH, -1) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_STORE_THROUGH_USED, 1) == vrc.VRC_EINVAL
        assert _get(vrc, g, vrc.OPT_STORE_THROUGH) == 1
        # a view that is never replayed never stores through
        _opt(vrc, g, vrc.OPT_WALK_CACHE, 0)
        for _ in range(3):
            g.render()
            assert mode(vrc, g) == 0 and through(vrc, g) == 0
