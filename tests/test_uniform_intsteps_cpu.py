"""The uniform march counted in integers, on the host build of the per-ray code (no GPU needed).

A uniform brick segment whose step is a power of two (and whose length is below 2^24 steps) is marched on its sample
count n = ceil(travel / stepSize) instead of on the float chain `travel -= stepSize` (vrc_core.h:
vrc_exact_step_count, vrc_march_uniform_counted).  Held here, bit for bit in frame and sample count:
the general march == the uniform float chain == the counted form; that a step which is not a power of two keeps the
float chain; and the counting identity itself against the loop it replaces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import test_uniform_bricks_cpu as ub

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "intsteps_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libintsteps_harness.so")

GRID, FIXED, GREY, RAYLOD = ub.GRID, ub.FIXED, ub.GREY, ub.RAYLOD
GENERAL, CHAIN, COUNTED = "general", "chain", "counted"

_H = None


def harness():
    global _H
    if _H is None:
        deps = [SRC, ub.SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (OUT, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, OUT)
        _H = C.CDLL(OUT)
        _H.uniform_harness_render.restype = C.c_int
        _H.intsteps_segment.restype = C.c_int
    return _H


def render(s, form, which, ray_lod=None):
    """(frame, samples, segments on the float chain, segments counted) of one of the three marches."""
    H = harness()
    H.intsteps_set_form(C.c_int(1 if which == CHAIN else 0))
    taken = (C.c_uint64 * 2)()
    H.intsteps_taken(taken)  # reset
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    samples, uniform = C.c_uint64(0), C.c_uint32(0)
    rc = H.uniform_harness_render(
        C.c_void_p(s.atlas.ctypes.data), orc.u32x3(*s.atlas_dim), orc.u32x3(*s.slot_dim), C.c_void_p(fb.ctypes.data),
        C.c_uint32(s.W), C.c_uint32(s.H), C.c_void_p(s.planes.ctypes.data if len(s.planes) else None),
        C.c_uint32(len(s.planes)), C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(s.n_nodes), s.nodes,
        C.byref(s.render), C.c_int(form | (RAYLOD if ray_lod else 0)), C.c_int(0 if which == GENERAL else 2), C.c_int(1),
        C.c_float(ray_lod[0] if ray_lod else 0.0), C.c_float(ray_lod[1] if ray_lod else 0.0), C.byref(samples),
        C.byref(uniform))
    H.intsteps_set_form(C.c_int(0))
    assert rc == 0, "uniform_harness_render: %d" % rc
    H.intsteps_taken(taken)
    return fb, int(samples.value), int(taken[0]), int(taken[1])


def three_ways(s, form, power_of_two, ray_lod=None, some_uniform=True):
    want, n_want, chain0, counted0 = render(s, form, GENERAL, ray_lod)
    assert chain0 == 0 and counted0 == 0  # no uniformity words: no uniform segments
    a, n_a, chain_a, counted_a = render(s, form, CHAIN, ray_lod)
    assert counted_a == 0 and (chain_a > 0 or not some_uniform)
    b, n_b, chain_b, counted_b = render(s, form, COUNTED, ray_lod)
    assert chain_b + counted_b == chain_a  # the same segments, whichever way they are marched
    if power_of_two:
        assert chain_b == 0 and counted_b == chain_a, "a power-of-two step is counted"
    else:
        assert counted_b == 0, "a step that is not a power of two keeps the float chain"
    assert (a == want).all() and n_a == n_want
    assert (b == want).all() and n_b == n_want
    return want


FORMS = [0, GRID, FIXED, GRID | FIXED, GREY | FIXED, GREY | GRID | FIXED]
SPR = [(64, True), (256, True), (1024, True), (100, False), (300, False), (1000, False)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alpha", [0.05, 1.0])
@pytest.mark.parametrize("spr,pow2", SPR)
def test_constant_bricks_three_ways(form, alpha, spr, pow2):
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(24, 24), spin=(0.5, 0.35), alpha=alpha, spr=spr)
    assert s.render.samplesPerRay == spr
    want = three_ways(s, form, pow2)
    assert want[..., 3].max() > 0.05
    if alpha == 1.0:
        assert want[..., 3].max() > 0.999  # early ray termination fires inside uniform bricks


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alpha", [0.05, 1.0])
@pytest.mark.parametrize("spr,pow2", SPR)
def test_mixed_volume_three_ways(form, alpha, spr, pow2):
    s = ub.mixed_scene(viewport=(24, 24), alpha=alpha, spr=spr)
    ub.assert_split(s)
    three_ways(s, form, pow2)


@pytest.mark.parametrize("spr,pow2", [(256, True), (300, False)])
@pytest.mark.parametrize("sse", [0.5, 1.5])
def test_per_ray_lod_three_ways(spr, pow2, sse):
    vi = orc.mem_volume_info(64, 64, 64, 16)
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 32), volume=ub.mixed_volume(), spin=(1.2, 0.3),
                        ids=orc.all_level_ids(vi, None), spr=spr)
    lod = (sse, orc.world_space_per_pixel(s))
    for form in (0, FIXED, GREY | FIXED):
        # a coarser brick's step is stepSize * 2^level: counted as well.  (At 1.5 pixels per voxel the rays of this view
        # stay in coarse bricks that mix values: nothing uniform to march, and the frames agree all the same.)
        three_ways(s, form, pow2, ray_lod=lod, some_uniform=sse < 1.0)


def travel_values(step, rng):
    """Lengths around every kind of edge: multiples of the step and their float neighbours, below one step, tiny, random,
    and the 2^24-step limit from both sides."""
    f32 = np.float32
    ks = np.concatenate([np.arange(1, 40), rng.integers(40, 5000, 300), [2 ** 12, 2 ** 16 - 1, 2 ** 16, 2 ** 20 + 1]])
    exact = (ks.astype(np.float64) * float(step)).astype(f32)
    vals = [exact, np.nextafter(exact, f32(0)), np.nextafter(exact, f32(np.inf)),
            (rng.uniform(0.0, 1.0, 400) * float(step)).astype(f32),
            (rng.uniform(0.0, 600.0, 3000) * float(step)).astype(f32),
            np.array([np.finfo(f32).tiny, 1e-30, float(step) * 2.0 ** -30], dtype=f32)]
    v = np.concatenate(vals).astype(f32)
    v = v[v > 0]
    small = np.ones(len(v), dtype=np.uint32)  # run the loop for all of these
    edge = f32(float(step) * 2.0 ** 24)
    edges = np.array([np.nextafter(edge, f32(0)), np.nextafter(np.nextafter(edge, f32(0)), f32(0)), edge,
                      np.nextafter(edge, f32(np.inf)), edge * f32(2), edge * f32(1000)], dtype=f32)
    run = np.array([1, 1, 0, 0, 0, 0], dtype=np.uint32)  # 2^24 trips each: only below the limit
    return np.concatenate([v, edges]), np.concatenate([small, run]), len(v)


def count(travel, step, trips):
    H = harness()
    travel = np.ascontiguousarray(travel, dtype=np.float32)
    trips = np.ascontiguousarray(trips, dtype=np.uint32).copy()
    exact = np.zeros(len(travel), dtype=np.uint8)
    n = np.zeros(len(travel), dtype=np.uint32)
    H.intsteps_count(C.c_void_p(travel.ctypes.data), C.c_uint32(len(travel)), C.c_float(step),
                     C.c_void_p(exact.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(trips.ctypes.data))
    return exact.astype(bool), n, trips


@pytest.mark.parametrize("spr", [64, 256, 1024, 2048])
@pytest.mark.parametrize("level", [0, 3])
def test_the_count_is_the_trip_count_of_the_float_chain(spr, level):
    step = np.float32(np.float32(1.0) / np.float32(spr)) * np.float32(1 << level)
    rng = np.random.default_rng(7000 + spr + level)
    travel, run, n_small = travel_values(step, rng)
    assert len(travel) > 4000
    exact, n, trips = count(travel, step, run)
    assert exact[:n_small].all()  # every one of these is shorter than 2^24 steps
    assert exact[n_small:].tolist() == [True, True, False, False, False, False]  # travel < 2^24 * stepSize, strictly
    ran = run != 0
    assert (n[ran] == trips[ran]).all(), (travel[ran][n[ran] != trips[ran]][:5], step)
    assert trips[n_small] == 2 ** 24 - 1 and trips[n_small + 1] == 2 ** 24 - 2  # the floats next below 2^24 steps
    assert n[:n_small].min() == 1  # lengths below one step: one sample


@pytest.mark.parametrize("spr", [100, 300, 1000])
def test_other_steps_are_not_counted(spr):
    step = np.float32(np.float32(1.0) / np.float32(spr))
    travel = (np.random.default_rng(spr).uniform(0.0, 3.0, 500)).astype(np.float32) + np.float32(1e-6)
    exact, _, _ = count(travel, step, np.zeros(len(travel), dtype=np.uint32))
    assert not exact.any()


def test_steps_outside_the_normal_range_are_not_counted():
    f32 = np.float32
    travel = np.array([1.0], dtype=f32)
    for step in (f32(2.0) ** 127, f32(2.0) ** -127, f32(2.0) ** -149, f32(np.inf), f32(-0.5), f32(0.0)):
        exact, _, _ = count(travel, step, np.zeros(1, dtype=np.uint32))
        assert not exact.any(), step
    exact, n, trips = count(np.array([3.0 * 2.0 ** 126], dtype=f32), f32(2.0) ** 126, np.ones(1, dtype=np.uint32))
    assert exact.all() and n[0] == 3 and trips[0] == 3
    exact, n, trips = count(np.array([2.5 * 2.0 ** -126], dtype=f32), f32(2.0) ** -126, np.ones(1, dtype=np.uint32))
    assert exact.all() and n[0] == 3 and trips[0] == 3


@pytest.mark.parametrize("alpha_entry", [0.003, 0.05, 0.4, 0.97, 1.0])
def test_one_segment_both_forms_at_every_length(alpha_entry):
    """Every length from 1 to 150 samples (every split into whole groups, halves, quarters ... and the chain's groups of
    14 with tails of 4), from a colour that makes the early exit cross at every place in a group."""
    H = harness()
    step = np.float32(1.0 / 1024.0)
    out = (C.c_float * 2)()
    cnt = C.c_uint32(0)
    crossed = 0
    for n in range(1, 151):
        for frac in (1.0, 0.37):
            travel = np.float32((n - 1 + frac) * float(step))
            for start in (0.0, 0.5, 0.99, 0.9985):
                rc = H.intsteps_segment(C.c_float(travel), C.c_float(step), C.c_float(0.3 * alpha_entry),
                                        C.c_float(alpha_entry), C.c_float(0.2 * start), C.c_float(start), out,
                                        C.byref(cnt))
                assert rc == 0, (n, frac, start)
                assert cnt.value <= n
                crossed += 1 if cnt.value < n else 0
                if out[1] <= 0.999:
                    assert cnt.value == n
    assert crossed > 0
