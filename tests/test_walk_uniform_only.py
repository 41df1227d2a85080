"""The uniform-only instances of the replay on the GPU (VRC_OPT_WALK_UNIFORM_ONLY, VRC_OPT_WALK_UNIFORM_ONLY_USED;
include/vrc_hip.h).

A view that replays lean lists and none of whose visits gathers -- by the count pass of those lists, while the pool has
taken no upload since -- is marched by vrc_k_raycast_replay<...,uniform,lean>, which holds no gather march.  Nothing of
the result may change: every frame here, on the way to the replay and in it, and every sample count equals bit for bit
the frame of a context with VRC_OPT_WALK_CACHE = 0 (what tests/test_ray_cache.py and tests/test_gpu_parity.py hold to the
oracle).  No tolerance appears.  Every frame also asserts what the read-back says -- 1 exactly on the replayed frames of
such a view, 0 everywhere else -- and that the kernel's name agrees with it.

Scenes: 256^3 voxels in 64 bricks of 64^3 (visits of about 64 to 80 steps at the automatic step: whole groups of 32 and
remainders) and 128^3 voxels in one brick (four groups and more), viewports of 96 x 80 and 70 x 52 pixels (partial tiles
on the second), the default camera and one turned by 30 and 20 degrees.  The views the form must not take, or must
leave, use the shapes of tests/test_walk_cache.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import orc
from test_uniform_bricks_cpu import assert_split
from test_walk_cache import FRESH, VIEWPORT, VOXELS, _get, _gpu, _opt, always, frame, scene, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

TURNED = (0.5235988, 0.3490659)  # 30 and 20 degrees
SCENES = {"64 bricks": dict(voxels=(256, 256, 256), block=64), "one brick": dict(voxels=(128, 128, 128), block=128)}
_built = {}


def uniform_scene(name, viewport, spin):
    key = (name, viewport, spin)
    if key not in _built:
        _built[key] = orc.build_scene(viewport=viewport, volume="mem", spin=spin, **SCENES[name])
    return copy.copy(_built[key])


def used(vrc, g):
    return _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY_USED)


def steady(vrc, g, ref, what, expect=FRESH, uniform=1, **kw):
    """Frames of g reading the modes of `expect` (None: whatever it reads), each equal -- pixels and sample count -- to
    the frame of ref (walk cache off); the read-back is `uniform` on the replayed frames and 0 on the others, and the
    kernel's name says the uniform-only form exactly where the read-back is 1."""
    want, m, _ = frame(vrc, ref, **kw)
    assert m == 0 and used(vrc, ref) == 0, what
    for i, e in enumerate(expect):
        (fb, n), m, _ = frame(vrc, g, **kw)
        assert e is None or m == e, "%s: frame %d read mode %d, expected %r" % (what, i, m, expect)
        name = g.L.vrc_last_kernel()
        u = used(vrc, g)
        if e is not None or uniform == 0:
            assert u == (uniform if m == 4 else 0), (what, i, m, u)
        assert (b"vrc_k_raycast_replay<" in name and b",uniform" in name) == (u == 1), (what, m, u, name)
        assert u == 0 or _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1, what  # (a lean form)
        assert np.array_equal(fb, want[0]), "%s frame %d (mode %d): %d pixels differ" % (
            what, i, m, int((fb != want[0]).any(axis=-1).sum()))
        assert n == want[1] and (n > 0) == kw.get("count", True), (what, i, n, want[1])
    return want


@pytest.mark.parametrize("spin", [(0.0, 0.0), TURNED])
@pytest.mark.parametrize("viewport", [(96, 80), (70, 52)])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_uniform_volume_is_replayed_by_the_uniform_only_instance(vrc, name, viewport, spin):
    s = uniform_scene(name, viewport, spin)
    assert s.n_nodes == (64 if name == "64 bricks" else 1)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)  # (g keeps the defaults: walk cache 1, uniform-only 1)
        assert _get(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY) == 1
        expect = FRESH
        # alpha 1.0 crosses the threshold inside a visit's first group, 0.3 and 0.05 further on: in later groups and in
        # remainders (enumerated sample by sample on the host build: tests/test_walk_lean_cpu.py)
        for alpha, coloured in ((0.05, False), (1.0, True), (1.0, False), (0.3, False), (0.05, True)):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            what = "%s %r spin %r alpha %g coloured %d" % (name, viewport, spin, alpha, coloured)
            fb, _ = steady(vrc, g, ref, what, expect=expect)
            assert (b"<true,%d," % (0 if coloured else 3)) in g.L.vrc_last_kernel(), what
            assert fb[..., 3].max() > 0.05 and (fb[..., 3] == 0.0).any(), what  # rays that hit and rays that miss
            if alpha == 1.0 and name == "64 bricks":  # (the one brick holds one value, whose entry stays below it)
                assert fb[..., 3].max() > 0.999, what  # early ray termination
            steady(vrc, g, ref, what + " uncounted", expect=(4,), count=False)
            assert (b"<false,%d," % (0 if coloured else 3)) in g.L.vrc_last_kernel(), what
            expect = (4,)  # the transfer function changes nothing of the lists


def test_row_bands(vrc):
    s = uniform_scene("64 bricks", (96, 80), TURNED)
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        whole = steady(vrc, g, ref, "whole frame")
        for x in (g, ref):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows.ctypes.data, len(rows)))
            x.s = copy.copy(banded)
        part = steady(vrc, g, ref, "row bands")
        assert np.array_equal(part[0], whole[0][rows])
        steady(vrc, g, ref, "row bands uncounted", expect=(4,), count=False)


def test_option_zero_keeps_the_lean_instance_and_the_lists(vrc):
    s = uniform_scene("64 bricks", (70, 52), TURNED)
    s.tf = table(0.3, False)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY, 0)
        steady(vrc, g, ref, "option 0", uniform=0)
        assert g.L.vrc_last_kernel().endswith(b",24,lean>") and _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1
        _opt(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY, 1)  # the same lists, the other instance: nothing starts over
        steady(vrc, g, ref, "option 1", expect=(4, 4))
        assert g.L.vrc_last_kernel().endswith(b",24,uniform,lean>")
        _opt(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY, 0)
        steady(vrc, g, ref, "option 0 again", expect=(4, 4), uniform=0)
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_UNIFORM_ONLY, 2) == vrc.VRC_EINVAL
        assert g.L.vrc_set_option(g.ctx, vrc.OPT_WALK_UNIFORM_ONLY_USED, 1) == vrc.VRC_EINVAL


def one_noise_brick_volume():
    """One brick of noise in the middle of a constant volume (its overlap makes the neighbours' slots mixed too)."""
    vol = np.full(VOXELS[::-1], 90, dtype=np.uint8)
    vol[32:48, 32:48, 32:48] = orc.hash_volume(*VOXELS)[32:48, 32:48, 32:48]
    return vol


@pytest.mark.parametrize("volume", ["one noise brick", "mixed", "hash"])
def test_a_view_with_a_visit_that_gathers_keeps_the_lean_instance(vrc, volume):
    if volume == "one noise brick":
        s = orc.build_scene(voxels=VOXELS, block=16, viewport=VIEWPORT, volume=one_noise_brick_volume(), spin=(0.5, 0.35),
                            spr=256)
        uni = sum(1 for b in s.bricks.values() if (b == b.flat[0]).all())
        assert 0 < len(s.bricks) - uni <= 27, (uni, len(s.bricks))
    else:
        s = scene(volume)
        if volume == "mixed":
            assert_split(s)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        if volume != "one noise brick":  # (at 1 a view most of whose visits gather is not replayed at all)
            always(vrc, g)
        for alpha, coloured in ((0.05, False), (1.0, True)):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            steady(vrc, g, ref, "%s alpha %g" % (volume, alpha), expect=FRESH if not coloured else (4, 4), uniform=0)
            assert g.L.vrc_last_kernel().endswith(b",24,lean>") and _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1


# an upload turns a uniform brick into a mixed one while the lists are valid (the upload case of tests/test_walk_cache.py
# and tests/test_walk_lean.py): at 1 the view is counted again, at VRC_WALK_CACHE_ALWAYS the lists stay -- and in both
# the frames after the upload are the walked ones and the uniform-only form has been left
@pytest.mark.parametrize("option", [1, 2])
def test_an_upload_that_makes_a_uniform_brick_mixed_leaves_the_form(vrc, option):
    s = scene("mem")
    s.tf = table(0.3, False)
    nid = s.sorted_ids[len(s.sorted_ids) // 2]
    noise = np.random.default_rng(7).integers(30, 230, size=s.bricks[nid].shape, dtype=np.uint8)
    assert noise.shape == s.bricks[nid].shape and noise.dtype == s.bricks[nid].dtype and noise.min() != noise.max()
    size = vrc.u32x3(noise.shape[2], noise.shape[1], noise.shape[0])
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        _opt(vrc, g, vrc.OPT_WALK_CACHE, option)
        before = steady(vrc, g, ref, "before the upload")
        assert used(vrc, g) == 1
        for x in (g, ref):
            slot = vrc.f32x3()
            vrc.check(x.L, x.L.vrc_pool_release_slot(x.pool, vrc.f32x3(*x.slots[nid])))
            vrc.check(x.L, x.L.vrc_pool_copy_to_slot(x.pool, noise.ctypes.data, size, slot))
            assert (slot[0], slot[1], slot[2]) == x.slots[nid]
        after = steady(vrc, g, ref, "after the upload", expect=(None,) * 5 if option == 1 else (4,) * 3, uniform=0)
        assert not np.array_equal(before[0], after[0])
        assert frame(vrc, g)[1] == 4 and used(vrc, g) == 0 and _get(vrc, g, vrc.OPT_WALK_LEAN_USED) == 1
        assert g.L.vrc_last_kernel().endswith(b",24,lean>")


def test_the_judged_instance_runs_eight_workgroups_per_cu(vrc):
    # The grey form in groups of 14 is what bench.py's frame takes (more than 6144 tiles: smaller launches take the
    # group of 24).  Its uniform-only instance needs 20 registers and 4 KiB of LDS and says amdgpu_waves_per_eu( 8, 8 ):
    # the runtime's own occupancy calculator must agree -- eight workgroups of four waves per compute unit, eight waves
    # per SIMD -- where the lean instance it replaces has six (profiles/r15_uniform_only.txt)
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(704, 640), volume="mem", spin=(0.5, 0.35))
    with _gpu(s) as g:
        for _ in FRESH:
            g.render(count=False)
        assert used(vrc, g) == 1
        assert g.L.vrc_last_kernel() == b"vrc_k_raycast_replay<false,3,unsigned char,14,uniform,lean>", g.L.vrc_last_kernel()
        wgs, threads = C.c_int(), C.c_int()
        vrc.check(g.L, g.L.vrc_last_kernel_occupancy(C.byref(wgs), C.byref(threads)))
        assert (wgs.value, threads.value) == (8, 256), (wgs.value, threads.value)
        _opt(vrc, g, vrc.OPT_WALK_UNIFORM_ONLY, 0)
        g.render(count=False)
        assert g.L.vrc_last_kernel() == b"vrc_k_raycast_replay<false,3,unsigned char,14,lean>", g.L.vrc_last_kernel()
        vrc.check(g.L, g.L.vrc_last_kernel_occupancy(C.byref(wgs), C.byref(threads)))
        assert (wgs.value, threads.value) == (6, 256), (wgs.value, threads.value)
