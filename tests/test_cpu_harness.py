"""CPU-side checks of the HIP kernel's per-ray code (libre_amd/csrc/vrc_core.h +
vrc_tables.h compiled by g++ in tests/cpu_harness) against the oracle.  No GPU needed; the
same headers are what hipcc compiles into the gfx950 kernel."""
import numpy as np
import pytest

import nongrid
import orc
import scenes


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_reference_order_matches_oracle(name):
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4)
    got, n_got, _ = orc.harness_render(s, kernel=1)
    scenes.assert_parity(got, want, name)
    scenes.assert_no_tie_bias(got, want, orc.oracle_render(s, threads=4, entry_bias=orc.ENTRY_BIAS)[0], name)
    # same bricks, same per-brick loop: the sample count is identical -- except where a
    # boundary sample reads the neighbouring voxel and a ray crosses the early-exit threshold
    # one sample sooner or later (only the high-opacity noise scene)
    if name == "hash64_ert":
        assert abs(n_got - n_want) <= 1e-4 * n_want
    else:
        assert n_got == n_want


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_grid_dda_matches_oracle(name):
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4)
    got, n_got, grid_ok = orc.harness_render(s, kernel=2)
    assert grid_ok
    scenes.assert_parity(got, want, name)
    scenes.assert_no_tie_bias(got, want, orc.oracle_render(s, threads=4, entry_bias=orc.ENTRY_BIAS)[0], name)
    # the walk hands the cells around tied edges / corners to the reference's slab test: the same samples, one
    # for one (the high-opacity noise scene: a ray may cross the early-exit threshold a sample sooner or later)
    if name == "hash64_ert":
        assert abs(n_got - n_want) <= 1e-4 * n_want
    else:
        assert n_got == n_want


def test_reference_order_is_bit_exact_on_constant_bricks():
    # with constant bricks voxel flips cannot matter and there is no FMA on the host build:
    # the restructured arithmetic (hoisted 1/dir, classified table) is bit-identical
    s = scenes.get("mem64_spin")
    want, _ = orc.oracle_render(s, threads=4)
    got, _, _ = orc.harness_render(s, kernel=1)
    assert (got == want).all()


def test_exact_tf_weights_option():
    s = scenes.get("hash64_spin")
    want, _ = orc.oracle_render(s, threads=4, frac_bits=0)
    got, _, _ = orc.harness_render(s, kernel=2, frac_bits=0)
    scenes.assert_parity(got, want)


def test_nucleon_single_brick_overlap0():
    s = scenes.nucleon_scene()
    want, n_want = orc.oracle_render(s, threads=4)
    assert want[..., 3].max() > 0.05
    for k in (1, 2):
        got, n_got, _ = orc.harness_render(s, kernel=k)
        scenes.assert_parity(got, want, "nucleon k%d" % k)
        assert n_got == n_want


def test_multipass_accumulates():
    # CudaRaycastPipeline.cpp:149-185: passes of front-to-back node ranges accumulate through
    # the persistent pixel buffer (Renderer.cu:151-157, 229)
    s = scenes.get("hash64_spin")
    want, _ = orc.oracle_render(s, threads=4)
    half = s.n_nodes // 2
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    full_nodes, n = s.nodes, s.n_nodes
    try:
        s.nodes = (orc.NodeData * half)(*full_nodes[:half])
        s.n_nodes = half
        fb, _, _ = orc.harness_render(s, kernel=2, fb=fb)
        s.nodes = (orc.NodeData * (n - half))(*full_nodes[half:])
        s.n_nodes = n - half
        fb, _, _ = orc.harness_render(s, kernel=2, fb=fb)
    finally:
        s.nodes, s.n_nodes = full_nodes, n
    scenes.assert_parity(fb, want, "multipass")


def test_partial_node_set_uses_grid_with_holes():
    # async mode renders whatever is resident: drop a third of the bricks
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), volume="hash", spin=(0.5, 0.35))
    keep = [nid for i, nid in enumerate(s.ids) if i % 3 != 0]
    s2 = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), volume="hash",
                         spin=(0.5, 0.35), ids=keep)
    want, n_want = orc.oracle_render(s2, threads=4)
    got, n_got, grid_ok = orc.harness_render(s2, kernel=2)
    assert grid_ok
    scenes.assert_parity(got, want, "holes")


def test_mixed_lod_node_set():
    # a coarse brick next to fine bricks (the LOD cut mixes levels): the grid is built at the
    # finest cell size and a coarse node covers 2x2x2 cells
    vi = orc.mem_volume_info(64, 64, 64, 16)
    assert vi.depth == 3
    coarse = orc.pack(1, 0, 0, 0)
    fine = [i for i in orc.leaf_ids(vi) if orc.lib().orc_nodeid_parent(i) != coarse]
    ids = [coarse] + fine
    s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), spin=(0.4, 0.3), ids=ids)
    want, _ = orc.oracle_render(s, threads=4)
    ref, _, _ = orc.harness_render(s, kernel=1)
    scenes.assert_parity(ref, want, "mixed ref-order")
    got, _, grid_ok = orc.harness_render(s, kernel=2)
    assert grid_ok
    # bricks of different sizes: the reference composites them in the host's centre-distance order, which is
    # not a visibility order for every ray; the grid walk takes them along the ray.
    # Where the two orders differ, two samples swap places: a second-order effect (weight^2)
    scenes.assert_parity(got, want, "mixed dda", e0=2e-4)


def test_sort_first_tile_equals_crop():
    # a tile rendered with the pixel offset + full-frame matrices equals the crop
    # of the full frame, bit for bit (same ray arithmetic)
    s = scenes.get("hash64_spin")
    full, _, _ = orc.harness_render(s, kernel=2)
    x0, y0, w, h = 8, 16, 24, 32
    W, H = s.W, s.H
    try:
        s.W, s.H = w, h
        tile, _, _ = orc.harness_render(s, kernel=2, pixel_off=(x0, y0))
    finally:
        s.W, s.H = W, H
    # the viewport in ViewData stays the full frame; only the buffer is the tile
    assert (tile == full[y0:y0 + h, x0:x0 + w]).all()


def test_sort_first_tile_with_subfrustum_matches_oracle():
    # the Equalizer way (livre/eq/Channel.cpp:151-157): origin-0 viewport + off-axis frustum
    kw = dict(scenes.SCENES["hash64_spin"])
    kw["viewport"] = (48, 48)
    full = orc.build_scene(**kw)
    want_full, _ = orc.oracle_render(full, threads=4)
    t = orc.build_scene(tile=(12, 24, 24, 12, 48, 48), **kw)
    want, _ = orc.oracle_render(t, threads=4)
    got, _, _ = orc.harness_render(t, kernel=2)
    scenes.assert_parity(got, want, "tile")
    # and the sub-frustum tile is the crop of the full frame up to float rounding of the matrices
    scenes.assert_close_frames(want, want_full[24:36, 12:36], "tile vs crop")


def test_sanitized_build_runs_clean():
    # ASan + UBSan on the host build of the per-ray code (the GPU pool cannot run sanitizers)
    s = scenes.get("hash_clip")
    import subprocess, sys, os, textwrap
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import orc, scenes
        s = scenes.get("hash_clip")
        a, n, _ = orc.harness_render(s, kernel=2, sanitize=True)
        b, m, _ = orc.harness_render(s, kernel=1, sanitize=True)
        for k in (4, 6, 8, 9, 10, 12):  # fixed-point stepping, trilinear, per-sample classification, tap-packed atlas
            orc.harness_render(s, kernel=k, sanitize=True)
        orc.harness_render(s, kernel=2, sanitize=True, variant=1)  # glRaycaster rules
        s = scenes.nucleon_scene(viewport=(24, 24))
        for k in (2, 5, 6):  # clamped sampler, point and trilinear
            orc.harness_render(s, kernel=k, sanitize=True)
        s16 = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(24, 24), volume="hash",
                              spin=(0.5, 0.35), dtype="u16")
        for k in (5, 6, 7, 8):  # 16-bit voxels
            orc.harness_render(s16, kernel=k, sanitize=True)
        print("OK", n, m)
    """ % os.path.dirname(os.path.abspath(__file__)))
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("name", ["hash64_ert", "hash64_spin", "hash_clip", "mem64_ert"])
def test_gpu_like_fma_contraction_keeps_parity(name):
    # the gfx950 build contracts a*b+c in the sample loop (voxel index, compositing) but not
    # in ray / brick-segment set-up (VRC_STRICT_FP); emulate that on the host with clang -mfma
    import os
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no clang")
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4)
    got, n_got, _ = orc.harness_render(s, kernel=2, sanitize="fma")
    scenes.assert_parity(got, want, name)
    assert abs(n_got - n_want) <= 2e-4 * n_want + 8


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_fixed_point_stepping_matches_oracle(name):
    # VRC_OPT_STEPPING = 1 (the default on the GPU): 8.24 voxel-space increments inside a brick
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4)
    for kernel in (3, 4):  # reference order / grid DDA with fixed-point stepping
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want, "%s k%d" % (name, kernel))
        assert abs(n_got - n_want) <= 2e-4 * n_want + 8
    # same sample count as the float chain: the stepping changes positions, never the count
    _, n_float, _ = orc.harness_render(s, kernel=2)
    assert n_got == n_float
    # the march in slices of the ray (VRC_OPT_ERT_COMPACTION's launches): every brick in exactly one slice, in the
    # order of the walk -- the same frame and count, bit for bit
    for parts in (2, 5):
        sliced, n_sliced, _ = orc.harness_render(s, kernel=4, parts=parts)
        assert (sliced == got).all() and n_sliced == n_got, "%s in %d slices" % (name, parts)


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_trilinear_extension_matches_oracle(name):
    # VRC_OPT_FILTER = 1: the reference integrator with a trilinear fetch and per-sample
    # classification (extension; the oracle's fetch_trilinear is the definition)
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4, filter_mode=1)
    for kernel in (5, 6):  # reference order / grid DDA
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want, "%s k%d" % (name, kernel))
        assert abs(n_got - n_want) <= 2e-4 * n_want + 8


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_tap_packed_trilinear_matches_oracle(name):
    # the trilinear filter through the tap-packed atlas (VRC_KERNEL_PACKED; vrc_core.h: vrc_march_segment_packed):
    # 16-bit texels holding a voxel and its z neighbour, two 4-byte reads per sample -- against the oracle's fetch_trilinear, for
    # both brick enumerations and with the (grey, alpha) colours of a grey transfer function
    s = scenes.get(name)
    if min(s.vi.overlap[a] for a in range(3)) < 1 or s.atlas.dtype.itemsize != 1:
        pytest.skip("the packed atlas takes its +1 neighbours from the overlap")
    want, n_want = orc.oracle_render(s, threads=4, filter_mode=1)
    frames = {}
    for kernel in (9, 10):  # reference order / grid DDA
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want, "%s k%d" % (name, kernel))
        assert abs(n_got - n_want) <= 2e-4 * n_want + 8
        frames[kernel] = got
    grey = (s.tf[:, 0] == s.tf[:, 1]).all() and (s.tf[:, 0] == s.tf[:, 2]).all()
    if grey:  # the same bits with two-float colours
        for kernel in (11, 12):
            got, _, _ = orc.harness_render(s, kernel=kernel)
            assert (got == frames[kernel - 2]).all(), "%s k%d: grey form differs" % (name, kernel)


def test_trilinear_differs_from_nearest_on_noise():
    # the parity tolerance must be able to tell the two filters apart
    s = scenes.get("hash64_ert")
    near, _ = orc.oracle_render(s, threads=4)
    lin, _ = orc.oracle_render(s, threads=4, filter_mode=1)
    assert np.abs(near - lin).max() > 10 * scenes.MAX_ABS


def test_trilinear_nucleon_clamped_sampler():
    s = scenes.nucleon_scene()
    want, n_want = orc.oracle_render(s, threads=4, filter_mode=1)
    for kernel in (5, 6):
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want, "nucleon linear k%d" % kernel)
        assert n_got == n_want


U16_SCENES = {
    "hash64_spin_u16": dict(voxels=(64, 64, 64), block=16, viewport=(40, 56), volume="hash", spin=(0.5, 0.35), dtype="u16"),
    "hash64_ert_u16": dict(voxels=(64, 64, 64), block=16, viewport=(48, 48), volume="hash", spin=(0.3, -0.2), alpha=1.0, dtype="u16"),
    "mem_ragged_u16": dict(voxels=(96, 64, 32), block=16, viewport=(37, 29), spin=(0.2, 0.9), dtype="u16",
                           data_range=(0.0, 300.0)),
}


@pytest.mark.parametrize("name", sorted(U16_SCENES))
def test_uint16_extension_matches_oracle(name):
    # 16-bit voxels (extension: the reference CUDA kernel fetches unsigned char only): point
    # sampled and trilinear, classified per sample through the data range
    s = orc.build_scene(**U16_SCENES[name])
    assert s.atlas.dtype == np.uint16
    want, n_want = orc.oracle_render(s, threads=4)
    want_lin, n_lin = orc.oracle_render(s, threads=4, filter_mode=1)
    assert want[..., 3].max() > 0.05
    for kernel in (7, 8):
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want, "%s k%d" % (name, kernel))
        assert abs(n_got - n_want) <= 2e-4 * n_want + 8
    for kernel in (5, 6):
        got, n_got, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, want_lin, "%s k%d" % (name, kernel))
        assert abs(n_got - n_lin) <= 2e-4 * n_lin + 8
    # the trilinear filter through the tap-packed atlas of 16-bit voxels (32-bit texels, two 8-byte reads per sample):
    # reference order / grid walk, and the same bits with the two-float colours of a grey transfer function
    if min(s.vi.overlap[a] for a in range(3)) >= 1:
        frames = {}
        for kernel in (9, 10):
            got, n_got, _ = orc.harness_render(s, kernel=kernel)
            scenes.assert_parity(got, want_lin, "%s packed k%d" % (name, kernel))
            assert abs(n_got - n_lin) <= 2e-4 * n_lin + 8
            frames[kernel] = got
        if (s.tf[:, 0] == s.tf[:, 1]).all() and (s.tf[:, 0] == s.tf[:, 2]).all():
            for kernel in (11, 12):
                got, _, _ = orc.harness_render(s, kernel=kernel)
                assert (got == frames[kernel - 2]).all(), "%s k%d: grey form differs" % (name, kernel)


def test_per_sample_classification_equals_the_classified_table():
    # u8 point sampling through vrc_classify must agree with the 257-entry table path
    s = scenes.get("hash64_spin")
    table, n_t, _ = orc.harness_render(s, kernel=2)
    per_sample, n_p, _ = orc.harness_render(s, kernel=8)
    assert n_t == n_p
    assert np.abs(table - per_sample).max() < 1e-5


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_glraycaster_variant_matches_its_oracle(name):
    # the second parity target: the GLSL twin's semantics (fragRaycast.glsl:113-215) --
    # pixel centres, lattice-snapped first sample, per-brick clip planes
    s = scenes.get(name)
    want, n_want = orc.oracle_render(s, threads=4, variant=1)
    for kernel in (1, 2, 4):
        got, n_got, _ = orc.harness_render(s, kernel=kernel, variant=1)
        scenes.assert_parity(got, want, "%s gl k%d" % (name, kernel))
        assert abs(n_got - n_want) <= 3e-4 * n_want + 8


@pytest.mark.parametrize("name,spp", [("hash64_spin", 2), ("hash64_axis", 4), ("mem_ragged", 3), ("hash_clip", 2)])
def test_glraycaster_supersampling_matches_its_oracle(name, spp):
    # glRaycaster with nSamplesPerPixel > 1 (fragRaycast.glsl:121-129, :212-214): every brick marched by spp jittered
    # rays per pixel from the pixel's colour so far, the pixel their average; a sub-ray that misses discards the brick
    # for the pixel.  The reference-order loop is the form that renders it (the GLSL twin is one draw per brick).
    import ctypes as C
    s = scenes.get(name)
    s.render = orc.RenderData(s.render.samplesPerRay, spp, s.render.maxSamplesPerRay, s.render.datatype,
                              (C.c_float * 2)(*s.render.dataSourceRange))
    want, n_want = orc.oracle_render(s, threads=4, variant=1)
    one = scenes.get(name)
    want1, _ = orc.oracle_render(one, threads=4, variant=1)
    assert np.abs(want - want1).max() > 1e-3  # the jitter does something
    got, n_got, _ = orc.harness_render(s, kernel=1, variant=1)
    scenes.assert_parity(got, want, "%s gl spp %d" % (name, spp))
    assert abs(n_got - n_want) <= 3e-4 * n_want + 8
    # sub-sample 0 is the pixel centre (rand(0, 0) = 0): spp = 1 through the same code is the plain GL frame
    s.render.samplesPerPixel = 1
    got1, _, _ = orc.harness_render(s, kernel=1, variant=1)
    scenes.assert_parity(got1, want1, "%s gl spp 1" % name)


def test_oracle_still_matches_the_committed_frames():
    # tests/golden/frames.npz (tests/golden/make_golden.py): the oracle's frames of the named scenes -- the cudaRaycaster
    # rules, the glRaycaster twin with and without its jittered supersampling, the trilinear filter -- pinned between
    # rounds; runs without a GPU (tests/test_gpu_parity.py repeats the first part on the GPU box)
    import importlib.util
    import os
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(gdir, "make_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    golden = np.load(os.path.join(gdir, "frames.npz"))
    n_frames = 0
    for name in sorted(scenes.SCENES):
        fb, n = orc.oracle_render(scenes.get(name), threads=4)
        assert n == int(golden[name + "__samples"][0]), name
        assert np.allclose(fb, golden[name], atol=1e-6), name
        n_frames += 1
    fb, n = orc.oracle_render(scenes.nucleon_scene(), threads=4)
    assert n == int(golden["nucleon__samples"][0]) and np.allclose(fb, golden["nucleon"], atol=1e-6)
    for name, key, kw in gen.variants():
        fb, n = orc.oracle_render(gen.variant_scene(name, kw), threads=4, **{k: v for k, v in kw.items() if k != "spp"})
        assert n == int(golden[name + "__" + key + "_samples"][0]), (name, key)
        assert np.allclose(fb, golden[name + "__" + key], atol=1e-6), (name, key)
        n_frames += 1
    assert 2 * (n_frames + 1) == len(golden.files)


def test_the_two_reference_variants_differ():
    s = scenes.get("hash64_spin")
    cuda, _ = orc.oracle_render(s, threads=4)
    gl, _ = orc.oracle_render(s, threads=4, variant=1)
    assert np.abs(cuda - gl).max() > 10 * scenes.MAX_ABS


def _fuzz_scene(rng):
    vox = [int(rng.choice([32, 48, 64, 96])) for _ in range(3)]
    block = int(rng.choice([16, 32]))
    vox = [max(v, block) // block * block for v in vox]
    kw = dict(voxels=tuple(vox), block=block, viewport=(int(rng.integers(9, 40)), int(rng.integers(9, 40))),
              volume=str(rng.choice(["hash", "mem"])), spin=(float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.5, 1.5))),
              alpha=float(rng.choice([0.05, 0.3, 1.0])))
    if rng.random() < 0.3:  # eye inside or near the volume
        kw["eye"] = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.1, 0.9)))
    if rng.random() < 0.4:
        n = int(rng.integers(1, 4))
        planes = []
        for _ in range(n):
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            planes.append([float(nrm[0]), float(nrm[1]), float(nrm[2]), float(rng.uniform(0.05, 0.4))])
        kw["planes"] = planes
    if rng.random() < 0.3:
        kw["spr"] = int(rng.choice([97, 300, 700]))
    return kw


def _fuzz_parity(got, want, what):
    # the same rule as everywhere (tests/scenes.py): no widening for random geometry
    scenes.assert_parity(got, want, what)


@pytest.mark.parametrize("seed", range(64 * scenes.FUZZ_SCALE))
def test_random_views_all_kernel_forms_match_the_oracle(seed):
    # random volumes, cameras (also inside the volume), clip planes, viewports and step sizes:
    # reference order, grid DDA, fixed-point stepping, trilinear, glRaycaster rules
    rng = np.random.default_rng(1000 + seed)
    kw = _fuzz_scene(rng)
    s = orc.build_scene(**kw)
    want, n_want = orc.oracle_render(s, threads=4)
    for kernel in (1, 2, 4):
        got, n_got, grid_ok = orc.harness_render(s, kernel=kernel)
        _fuzz_parity(got, want, "seed %d k%d %r" % (seed, kernel, kw))
        # the same samples, one for one; with an opaque transfer function a ray may cross the early-exit
        # threshold a sample sooner or later where a tie (tests/scenes.py) falls the other way
        assert n_got == n_want or (kw.get("alpha", 0.05) >= 0.3 and abs(n_got - n_want) <= 1e-4 * n_want + 8), \
            (seed, kernel, kw, n_got, n_want)
    want_lin, _ = orc.oracle_render(s, threads=4, filter_mode=1)
    got, _, _ = orc.harness_render(s, kernel=6)
    _fuzz_parity(got, want_lin, "seed %d trilinear %r" % (seed, kw))
    if min(s.vi.overlap[a] for a in range(3)) >= 1 and max(s.slot_dim) <= 248 and s.atlas.dtype.itemsize == 1:
        got, _, grid_ok = orc.harness_render(s, kernel=9)
        _fuzz_parity(got, want_lin, "seed %d trilinear, tap-packed atlas %r" % (seed, kw))
        if grid_ok:
            got, _, _ = orc.harness_render(s, kernel=10)
            _fuzz_parity(got, want_lin, "seed %d trilinear, tap-packed atlas, grid walk %r" % (seed, kw))
    want_gl, _ = orc.oracle_render(s, threads=4, variant=1)
    got, _, _ = orc.harness_render(s, kernel=2, variant=1)
    _fuzz_parity(got, want_gl, "seed %d glRaycaster %r" % (seed, kw))


@pytest.mark.parametrize("name", ["hash64_axis", "hash64_spin", "hash_spr300", "hash64_ert"])
def test_parity_rule_rejects_a_biased_kernel(name):
    # NEGATIVE CONTROL of the parity rule (tests/scenes.py).  A host build of the kernel code whose brick segments start
    # 2e-7 world units early (VRC_DEV_BUILD + VRC_TEST_BIAS_ENTRY, vrc_core.h: vrc_brick_segment): the first sample of
    # every segment, which the reference puts exactly on the brick face (cuda/Renderer.cu:195-196, :208-214), then
    # ALWAYS reads the voxel on the near side of the face.  Every one of those flips lies inside the oracle's tie zone,
    # so the frame passes the per-pixel rule |d| <= E0 + 2 B -- a systematic error hiding in the budget.  The bias
    # check must throw it out; the unbiased build of the same code passes both on the same scene.
    s = scenes.get(name)
    want, _ = orc.oracle_render(s, threads=4)
    flipped, _ = orc.oracle_render(s, threads=4, entry_bias=orc.ENTRY_BIAS)
    assert np.abs(flipped - want).max() > 3 * scenes.E0  # the scene has ties that matter
    good, _, _ = orc.harness_render(s, kernel=2)
    scenes.assert_parity(good, want, name + " unbiased")
    assert abs(scenes.assert_no_tie_bias(good, want, flipped, name + " unbiased")) < 0.1
    biased, _, _ = orc.harness_render(s, kernel=2, sanitize="bias")
    tb = orc.budget_of(want)
    d = np.abs(biased.astype(np.float64) - want.astype(np.float64)).max(axis=-1)
    inside = float((d <= scenes.E0 + scenes.TIE_FACTOR * tb).mean())
    assert inside > 0.99, "the control is only meaningful while the per-pixel rule alone lets it through"
    assert scenes.tie_bias(biased, want, flipped) > 0.9
    with pytest.raises(AssertionError):
        scenes.assert_no_tie_bias(biased, want, flipped, name + " biased")


def test_the_parity_contract_is_frozen():
    # rounds 2-3 re-based the rule's constants after soak failures; since round 4 they are a contract.  A
    # change to any of them must change this test too, in the open (and DESIGN.md section 2's table with it).
    frozen = dict(E0=5e-5, TIE_FACTOR=2.0, MAX_ABS_CAP=6e-3, MEAN_ABS_CAP=3e-4, MEAN_E0=2e-5, BUDGET_USE=0.5, NEEDS_BUDGET=0.7,
                  STRONG_SAMPLE=1e-2, MAX_ABS_CAP_STRONG=3e-2, MEAN_ABS_CAP_STRONG=1.5e-3, NEEDS_BUDGET_STRONG=0.95,
                  TIE_BIAS_MAX=0.35, RAY_LOD_ALLOW=5e-4)
    for name, value in frozen.items():
        assert getattr(scenes, name) == value, name
    assert not hasattr(scenes, "OPAQUE_ALPHA")
    for name in frozen:
        assert ("%g" % frozen[name]) in scenes.rule_string() or name in ("TIE_FACTOR",), name
    # which frames get the looser caps: by the largest classified opacity of one sample alone
    s = scenes.get("hash64_spin")  # the alpha-0.05 ramp at the automatic 512 samples per ray: weak samples, tight caps
    a = float(np.asarray(s.tf).reshape(-1, 4)[:, 3].max())
    assert 1.0 - (1.0 - a) ** (32.0 / s.render.samplesPerRay) < scenes.STRONG_SAMPLE
    n = scenes.nucleon_scene()  # alpha 0.3 at 512: strong
    a = float(np.asarray(n.tf).reshape(-1, 4)[:, 3].max())
    assert 1.0 - (1.0 - a) ** (32.0 / n.render.samplesPerRay) > scenes.STRONG_SAMPLE


# ---- node lists that are not a brick grid (tests/nongrid.py) ---------------------------------------------------
# Overlapping lists (coarse bricks among the finer ones inside them: an asynchronous frame's cached ancestors) and the
# ragged UVF tree.  Every kernel form marches them with the reference-order loop; the grid walk refuses them.

NONGRID = sorted(nongrid.OVERLAPPING) + sorted(nongrid.RAGGED)


def nongrid_scene(name):
    if name in nongrid.RAGGED:
        from libre_amd import driver
        driver.load_library()
        return nongrid.uvf_scene(driver, name)
    return nongrid.overlapping_scene(name)


def colour_tf(alpha=0.3):
    """A transfer function whose red, green and blue differ (the four-float colour forms)."""
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.stack([i, 1 - i, i * i, np.float32(alpha) * i], axis=1).astype(np.float32))


def _list_order_forms(s):
    """(harness kernel, filter) of every list-order form that applies to the scene's voxel type: 1 / 3 classified
    table with float / fixed-point stepping (8-bit), 7 per-sample classification, 5 trilinear gathers, 9 / 11 the
    tap-packed atlas with four-float / (grey, alpha) colours."""
    u16 = s.atlas.dtype.itemsize == 2
    return ([] if u16 else [(1, 0), (3, 0)]) + [(7, 0), (5, 1), (9, 1), (11, 1)]


@pytest.mark.parametrize("name", NONGRID)
def test_non_grid_lists_every_list_order_form_matches_the_oracle(name):
    s = nongrid_scene(name)
    want = {f: orc.oracle_render(s, threads=4, filter_mode=f) for f in (0, 1)}
    frames = {}
    for kernel, f in _list_order_forms(s):
        got, n_got, grid_ok = orc.harness_render(s, kernel=kernel)
        assert not grid_ok, "%s: the list is not a grid" % name
        scenes.assert_parity(got, want[f][0], "%s k%d" % (name, kernel))
        assert abs(n_got - want[f][1]) <= 2e-4 * want[f][1] + 8, (name, kernel, n_got, want[f][1])
        frames[kernel] = got
    assert (frames[11] == frames[9]).all(), "%s: grey form of the packed march differs" % name
    with pytest.raises(RuntimeError):  # the grid walk refuses the list
        orc.harness_render(s, kernel=2)
    # glRaycaster rules, one and three samples per pixel (the brick-by-brick average), both filters
    for spp in (1, 3):
        s.render.samplesPerPixel = spp
        for kernel, f in ((1 if s.atlas.dtype.itemsize == 1 else 7, 0), (5, 1)):
            want_gl, n_gl = orc.oracle_render(s, threads=4, variant=1, filter_mode=f)
            got, n_got, _ = orc.harness_render(s, kernel=kernel, variant=1)
            scenes.assert_parity(got, want_gl, "%s glRaycaster spp %d k%d" % (name, spp, kernel))
            assert abs(n_got - n_gl) <= 3e-4 * n_gl + 8
    s.render.samplesPerPixel = 1
    # a coloured transfer function: the four-float forms
    s.tf = colour_tf()
    for kernel, f in _list_order_forms(s):
        if kernel == 11:
            continue  # the grey form is for grey tables only
        w, _ = orc.oracle_render(s, threads=4, filter_mode=f)
        got, _, _ = orc.harness_render(s, kernel=kernel)
        scenes.assert_parity(got, w, "%s colour k%d" % (name, kernel))


@pytest.mark.parametrize("seed", range(16 * scenes.FUZZ_SCALE))
def test_random_views_of_overlapping_lists_match_the_oracle(seed):
    # _fuzz_scene's volumes and views over random overlapping lists (tests/nongrid.py: fuzz_scene), u8 and u16,
    # split into random passes for the packed march
    rng = np.random.default_rng(21000 + seed)
    s, kw = nongrid.fuzz_scene(rng, dtype="u16" if seed % 4 == 3 else "u8",
                               **({"volume": "hash"} if seed % 4 == 3 else {}))
    want = {f: orc.oracle_render(s, threads=4, filter_mode=f) for f in (0, 1)}
    packed = min(s.vi.overlap[a] for a in range(3)) >= 1 and max(s.slot_dim) <= 248
    for kernel, f in _list_order_forms(s):
        if kernel in (9, 11) and not packed:
            continue
        got, n_got, grid_ok = orc.harness_render(s, kernel=kernel)
        assert not grid_ok
        _fuzz_parity(got, want[f][0], "seed %d k%d %r" % (seed, kernel, kw))
        assert n_got == want[f][1] or (kw.get("alpha", 0.05) >= 0.3 and
                                       abs(n_got - want[f][1]) <= 2e-4 * want[f][1] + 8), (seed, kernel, kw)
    want_gl, _ = orc.oracle_render(s, threads=4, variant=1)
    got, _, _ = orc.harness_render(s, kernel=1 if s.atlas.dtype.itemsize == 1 else 7, variant=1)
    _fuzz_parity(got, want_gl, "seed %d glRaycaster %r" % (seed, kw))
