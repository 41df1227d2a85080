"""A pixel buffer that grows inside a frame, through the C ABI on the GPU.

The per-pixel state of a MIP, isosurface or composite-depth frame (running value, depth, sum and count, gradient) lives
in buffers of the context that grow with the pixel buffer in use.  A later pass of a frame whose pixel buffer grew
(vrc_set_framebuffer between two passes) gets new buffers filled with "nothing known as far as this buffer knows" --
all bits set for the value, +infinity for the depth, zero for sum, count and gradient; each buffer its own fill.  So
the pass into the larger, zeroed buffer must leave exactly what a fresh context leaves that renders this pass alone:
the frame and every read-back, bit for bit.  Smallest shape at which the buffers really grow over more than one tile:
16 x 16 pixels (2 x 2 tiles) to 24 x 24 (3 x 3), 32^3 voxels in 16^3 bricks, on contexts that have seen no larger buffer."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library under test loads its HIP runtime: both then share one

import orc
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

ISO, TAU = 118.0, 300
KINDS = {  # options, and which read-backs the frame has beside values and counts
    "mip-max-depth": ([(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), (vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MAX), (vrc.OPT_MIP_DEPTH, 1)], "d"),
    "min": ([(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), (vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MIN)], ""),
    "mean": ([(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP), (vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MEAN)], ""),
    "iso": ([(vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)], "dg"),
    "composite-depth": ([(vrc.OPT_COMPOSITE_DEPTH, TAU)], "d"),
}
_SCENES = []


def _scenes():
    if not _SCENES:
        small = orc.build_scene(voxels=(32, 32, 32), block=16, viewport=(16, 16), spr=0, alpha=0.6, volume="hash",
                                spin=(0.5, 0.35))
        _SCENES.extend([small, orc.with_viewport(small, 24, 24)])
    return _SCENES


def _begin(g, kind):
    L, s = g.L, g.s
    if kind == "iso":
        vrc.set_isosurface(L, g.ctx, ISO, 0.25)
    for option, value in KINDS[kind][0]:
        vrc.check(L, L.vrc_set_option(g.ctx, option, value))
    vrc.check(L, L.vrc_update(g.ctx, s.tf.ctypes.data, None, 0))


def _view(s):
    return C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))


def _pass(g, s):
    vrc.check(g.L, g.L.vrc_render(g.ctx, _view(s), C.cast(s.nodes, C.POINTER(vrc.NodeData)), s.n_nodes,
                                  C.cast(C.byref(s.render), C.POINTER(vrc.RenderData)), g.pool))


def _readbacks(g, kind, w, h):
    L = g.L
    v = np.full((h, w), np.nan, dtype=np.float32)
    c = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
    vrc.check(L, L.vrc_get_projection_values(g.ctx, v.ctypes.data, c.ctypes.data))
    out = {"values": v, "counts": c}
    if "d" in KINDS[kind][1]:
        out["depths"], out["xyz"] = vrc.projection_depths(L, g.ctx, w, h)
    if "g" in KINDS[kind][1]:
        out["gradients"] = vrc.projection_gradients(L, g.ctx, w, h)
    return out


def _grown(kind, lib=None):
    """pass A at 16 x 16 into the context's own buffer, then pass B of the same frame into a zeroed 24 x 24 one"""
    small, large = _scenes()
    with GpuScene(small, lib=lib) as g:  # lib: a developer A/B build
        _begin(g, kind)
        vrc.check(g.L, g.L.vrc_pre_render(g.ctx, _view(small)))
        _pass(g, small)
        ext = torch.zeros((large.H, large.W, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, C.c_void_p(ext.data_ptr()), large.W, large.H))
        try:
            _pass(g, large)
            vrc.check(g.L, g.L.vrc_synchronize(g.ctx))
            out = _readbacks(g, kind, large.W, large.H)
            out["frame"] = ext.cpu().numpy()
        finally:
            vrc.check(g.L, g.L.vrc_set_framebuffer(g.ctx, None, 0, 0))
    return out


def _fresh(kind, lib=None):
    """vrc_pre_render and pass B alone at 24 x 24"""
    small, large = _scenes()
    with GpuScene(small, lib=lib) as g:  # lib: a developer A/B build
        _begin(g, kind)
        vrc.check(g.L, g.L.vrc_pre_render(g.ctx, _view(large)))
        _pass(g, large)
        out = _readbacks(g, kind, large.W, large.H)
        fb = np.zeros((large.H, large.W, 4), dtype=np.float32)
        vrc.check(g.L, g.L.vrc_post_render(g.ctx, fb.ctypes.data))
        out["frame"] = fb
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_later_pass_into_a_grown_buffer_is_the_pass_alone(kind):
    grown, fresh = _grown(kind), _fresh(kind)
    assert sorted(grown) == sorted(fresh)
    for name in sorted(fresh):
        a, b = grown[name], fresh[name]
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32))
        print("  %s %s: %d of %d words differ" % (kind, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
        assert same, "%s: %s after growth differs from the pass alone" % (kind, name)
    # the case has substance: pixels that the volume covers and pixels that it does not, and a state that is not all empty
    assert 0 < int((fresh["frame"][..., 3] > 0).sum()) < fresh["frame"][..., 3].size
    if "depths" in fresh:
        assert np.isfinite(fresh["depths"]).any() and np.isposinf(fresh["depths"]).any()
    if "gradients" in fresh:
        assert (fresh["gradients"] != 0).any()
    assert (fresh["counts"] > 0).any()
