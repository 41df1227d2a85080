"""Uniform bricks on the host build of the per-ray code (no GPU needed): vrc_march_brick with the per-slot uniformity
words (vrc_frame::slotInfo, vrc_dev_node::slotInfoIndex from vrc_build_tables) composites the general march's frame and
sample count bit for bit, and does so without reading the voxels of a uniform brick (tests/cpu_harness/
uniform_harness.cpp overwrites them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "uniform_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libuniform_harness.so")

_H = None


def harness():
    global _H
    if _H is None:
        deps = [SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (OUT, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, OUT)
        _H = C.CDLL(OUT)
        _H.uniform_harness_render.restype = C.c_int
    return _H


GRID, FIXED, GREY, RAYLOD = 1, 2, 4, 8


def render(s, form, use_info, fb=None, ray_lod=None):
    clear_first = fb is None
    if fb is None:
        fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    samples, uniform = C.c_uint64(0), C.c_uint32(0)
    rc = harness().uniform_harness_render(
        C.c_void_p(s.atlas.ctypes.data), orc.u32x3(*s.atlas_dim), orc.u32x3(*s.slot_dim), C.c_void_p(fb.ctypes.data),
        C.c_uint32(s.W), C.c_uint32(s.H), C.c_void_p(s.planes.ctypes.data if len(s.planes) else None),
        C.c_uint32(len(s.planes)), C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(s.n_nodes), s.nodes,
        C.byref(s.render), C.c_int(form | (RAYLOD if ray_lod else 0)), C.c_int(use_info), C.c_int(1 if clear_first else 0),
        C.c_float(ray_lod[0] if ray_lod else 0.0), C.c_float(ray_lod[1] if ray_lod else 0.0), C.byref(samples),
        C.byref(uniform))
    assert rc == 0, "uniform_harness_render: %d" % rc
    return fb, int(samples.value), int(uniform.value)


def mixed_volume():
    vol = orc.hash_volume(64, 64, 64)
    vol[:, :, 28:] = 90
    vol[40:, :, 28:] = 0
    return vol


def mixed_scene(**kw):
    kw.setdefault("spin", (1.2, 0.3))
    kw.setdefault("viewport", (40, 40))
    return orc.build_scene(voxels=(64, 64, 64), block=16, volume=mixed_volume(), **kw)


def assert_split(s):
    """At least a quarter of the bricks uniform (overlap included), at least a quarter not."""
    uni = sum(1 for b in s.bricks.values() if (b == b.flat[0]).all())
    assert 4 * uni >= len(s.bricks) and 4 * (len(s.bricks) - uni) >= len(s.bricks), (uni, len(s.bricks))
    return uni


FORMS = [0, GRID, FIXED, GRID | FIXED, GREY | FIXED, GREY | GRID | FIXED]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alpha", [0.05, 1.0])
def test_constant_bricks_equal_the_general_march(form, alpha):
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), spin=(0.5, 0.35), alpha=alpha)
    want, n_want, _ = render(s, form, 0)
    got, n_got, uniform = render(s, form, 1)
    assert uniform == s.n_nodes
    assert (got == want).all() and n_got == n_want
    assert want[..., 3].max() > 0.05
    if alpha == 1.0:
        assert want[..., 3].max() > 0.999  # early ray termination fires inside uniform bricks
    # ... and the uniform march does not look at the voxels: the same frame from an atlas that holds other values
    blind, n_blind, _ = render(s, form, 2)
    assert (blind == want).all() and n_blind == n_want


@pytest.mark.parametrize("form", FORMS)
def test_mixed_volume_equals_the_general_march(form):
    s = mixed_scene()
    uni = assert_split(s)
    want, n_want, _ = render(s, form, 0)
    got, n_got, uniform = render(s, form, 1)
    assert uniform >= uni
    assert (got == want).all() and n_got == n_want
    blind, n_blind, _ = render(s, form, 2)
    assert (blind == want).all() and n_blind == n_want


def test_the_general_march_of_this_harness_is_the_product_harness():
    # the reference frame of the tests above is the frame tests/test_cpu_harness.py holds against the oracle
    s = mixed_scene()
    a, n_a, _ = render(s, GRID, 0)
    b, n_b, _ = orc.harness_render(s, kernel=2)
    assert (a == b).all() and n_a == n_b
    a, n_a, _ = render(s, GRID | FIXED, 0)
    b, n_b, _ = orc.harness_render(s, kernel=4)
    assert (a == b).all() and n_a == n_b


def test_clip_planes_and_second_pass():
    s = mixed_scene(planes=[[0.6, 0.0, 0.8, 0.2]], alpha=1.0)
    for form in (GRID | FIXED, FIXED):
        want, n_want, _ = render(s, form, 0)
        got, n_got, _ = render(s, form, 1)
        assert (got == want).all() and n_got == n_want
        # a second pass into the frame: pixels already past the early-exit threshold stay as they are
        assert (want[..., 3] > 0.999).any()
        want2, n_want2, _ = render(s, form, 0, fb=want.copy())
        got2, n_got2, _ = render(s, form, 1, fb=got.copy())
        assert (got2 == want2).all() and n_got2 == n_want2


def test_one_voxel_is_enough():
    base = np.full((64, 64, 64), 90, dtype=np.uint8)
    odd = base.copy()
    odd[24, 24, 24] = 255  # interior of one brick, on the rays through the middle of the frame
    edge = base.copy()
    edge[24, 24, 33] = 255  # interior of a brick, and in the overlap of its neighbour along x
    # (a viewport fine enough that every voxel column of the volume has a ray through it, a transfer function thin
    # enough that the rays get there)
    kw = dict(voxels=(64, 64, 64), block=16, viewport=(128, 128), spin=(0.0, 0.0), alpha=0.05)
    plain, _, uniform = render(orc.build_scene(volume=base, **kw), GRID | FIXED, 1)
    assert uniform == 64
    for vol in (odd, edge):
        s = orc.build_scene(volume=vol, **kw)
        off, n_off, _ = render(s, GRID | FIXED, 0)
        on, n_on, uniform = render(s, GRID | FIXED, 1)
        assert uniform < 64
        assert (on == off).all() and n_on == n_off
    s = orc.build_scene(volume=odd, **kw)
    assert (render(s, GRID | FIXED, 1)[0] != plain).any()  # the voxel is seen


@pytest.mark.parametrize("sse", [0.5, 1.5, 1e3])
def test_per_ray_lod(sse):
    vi = orc.mem_volume_info(64, 64, 64, 16)
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 32), volume=mixed_volume(), spin=(1.2, 0.3),
                        ids=orc.all_level_ids(vi, None))
    lod = (sse, orc.world_space_per_pixel(s))
    for form in (0, FIXED, GREY | FIXED):
        want, n_want, _ = render(s, form, 0, ray_lod=lod)
        got, n_got, uniform = render(s, form, 1, ray_lod=lod)
        assert uniform > 0
        assert (got == want).all() and n_got == n_want
        blind, n_blind, _ = render(s, form, 2, ray_lod=lod)
        assert (blind == want).all() and n_blind == n_want


@pytest.mark.parametrize("seed", range(12))
def test_random_views_of_the_mixed_volume(seed):
    rng = np.random.default_rng(31000 + seed)
    kw = dict(viewport=(int(rng.integers(9, 40)), int(rng.integers(9, 40))),
              spin=(float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.5, 1.5))),
              alpha=float(rng.choice([0.05, 0.3, 1.0])))
    if rng.random() < 0.3:  # eye inside or near the volume
        kw["eye"] = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.1, 0.9)))
    if rng.random() < 0.3:
        kw["spr"] = int(rng.choice([97, 300, 700]))
    s = mixed_scene(**kw)
    for form in (GRID, GRID | FIXED, FIXED, GREY | GRID | FIXED):
        want, n_want, _ = render(s, form, 0)
        got, n_got, _ = render(s, form, 2)
        assert (got == want).all() and n_got == n_want, (seed, form, kw)
