"""The uniform march counted in integers, on the GPU: with VRC_OPT_UNIFORM_BRICKS on, a wave whose bricks are uniform and
whose step is a power of two marches them on the sample count (vrc_core.h: vrc_march_uniform_counted), any other step on
the float chain; either way the frame and the sample count equal the general march's (option off), bit for bit.
tests/test_uniform_intsteps_cpu.py shows on the host build which form a step takes and holds the counting identity;
the off frames are what tests/test_gpu_parity.py holds to the oracle.  No tolerance appears here."""
import pytest

import orc
from test_uniform_bricks import _gpu, _opt, on_off, vrc  # noqa: F401  (vrc: the module's fixture)
from test_uniform_bricks_cpu import assert_split, mixed_scene, mixed_volume

pytestmark = pytest.mark.gpu

SPR = [64, 256, 1024, 100, 300, 1000]  # 1 / spr is the step: the first three are counted, the others are not


def forms(vrc, s, what):
    """Grey and four-float tables, grid walk and reference order, counted and not."""
    with _gpu(s) as g:
        for grey in (1, 0):
            _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
            for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
                fb, _ = on_off(vrc, g, "%s grey %d kernel %d" % (what, grey, kernel), kernel=kernel)
        _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
        on_off(vrc, g, what + " uncounted", count=False)
    return fb


@pytest.mark.parametrize("alpha", [0.05, 1.0])
@pytest.mark.parametrize("spr", SPR)
def test_all_uniform(vrc, spr, alpha):
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(64, 64), spin=(0.5, 0.35), alpha=alpha, spr=spr)
    assert s.render.samplesPerRay == spr
    fb = forms(vrc, s, "mem spr %d alpha %g" % (spr, alpha))
    assert fb[..., 3].max() > 0.05
    if alpha == 1.0:
        assert fb[..., 3].max() > 0.999  # early ray termination fires inside uniform bricks


@pytest.mark.parametrize("alpha", [0.05, 1.0])
@pytest.mark.parametrize("spr", SPR)
def test_mixed_volume(vrc, spr, alpha):
    s = mixed_scene(viewport=(64, 64), alpha=alpha, spr=spr)
    assert_split(s)
    forms(vrc, s, "mixed spr %d alpha %g" % (spr, alpha))


@pytest.mark.parametrize("spr", [0, 256, 300])
@pytest.mark.parametrize("alpha", [0.05, 1.0])
def test_tiles_inside_bricks_and_across_their_faces(vrc, spr, alpha):
    # 4^3 bricks of 32^3 voxels under 256^2 pixels: a brick covers several 8x8 tiles, so one frame holds waves whose
    # 64 rays are all in one brick (the same node, slot word and sample count in every lane) and waves that straddle
    # a brick face or corner (lanes in different bricks, with different counts, some of them with none)
    for spin in ((0.0, 0.0), (0.5, 0.35)):
        s = orc.build_scene(voxels=(128, 128, 128), block=32, viewport=(256, 256), spin=spin, alpha=alpha, spr=spr)
        with _gpu(s) as g:
            for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
                fb, _ = on_off(vrc, g, "128^3 spin %r spr %d kernel %d" % (spin, spr, kernel), kernel=kernel)
            assert fb[..., 3].max() > 0.05


@pytest.mark.parametrize("spr", [256, 300])
@pytest.mark.parametrize("volume", ["mem", "mixed"])
def test_per_ray_lod(vrc, volume, spr):
    vi = orc.mem_volume_info(64, 64, 64, 16)
    kw = dict(voxels=(64, 64, 64), block=16, viewport=(64, 48), spin=(1.2, 0.3), ids=orc.all_level_ids(vi, None), spr=spr)
    if volume == "mixed":
        kw["volume"] = mixed_volume()
    s = orc.build_scene(**kw)
    with _gpu(s) as g:
        for sse in (0.5, 1.5):
            lod = (sse, orc.world_space_per_pixel(s))
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                on_off(vrc, g, "%s ray lod sse %g grey %d spr %d" % (volume, sse, grey, spr), kernel=vrc.KERNEL_GRID_DDA,
                       ray_lod=lod)
