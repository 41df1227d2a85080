"""VRC_OPT_UNIFORM_BRICKS on the GPU: frames and sample counts with the option on equal those with it off, bit for bit.
The off frames are the general march, which tests/test_gpu_parity.py holds to the oracle; no tolerance appears here.
(tests/test_uniform_bricks_cpu.py shows on the host build that the uniform march really does not read the voxels.)"""
import copy
import ctypes as C

import numpy as np
import pytest

import orc
from test_uniform_bricks_cpu import assert_split, mixed_scene, mixed_volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vrc():
    from libre_amd import vrc as v
    v.load_library()  # fails loudly when the HIP extension is missing
    return v


def _gpu(s):
    from gpu_run import GpuScene
    return GpuScene(s)


def _opt(vrc, g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def on_off(vrc, g, what, count=True, **kw):
    """Render with the option off and on; the frames (and counts) must be equal.  Returns the frame and the count."""
    _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, 0)
    off, n_off, st_off = g.render(count=count, **kw)
    _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, 1)
    on, n_on, st_on = g.render(count=count, **kw)
    assert st_on.kernel_variant == st_off.kernel_variant, what
    assert (on == off).all(), "%s: %d pixels differ" % (what, int((on != off).any(axis=-1).sum()))
    if count:
        assert n_on == n_off and n_on > 0, (what, n_on, n_off)
    return on, n_on


def all_uniform_scene(**kw):
    kw.setdefault("spin", (0.5, 0.35))
    kw.setdefault("viewport", (64, 64))
    return orc.build_scene(voxels=(64, 64, 64), block=16, **kw)  # mem: one value per brick, overlap included


def kernel_matrix(vrc, s, what):
    """Grey and four-float tables, grid walk and reference order, counted and not."""
    with _gpu(s) as g:
        for grey in (1, 0):
            _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
            for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
                for count in (True, False):
                    fb, _ = on_off(vrc, g, "%s grey %d kernel %d count %d" % (what, grey, kernel, count), count=count,
                                   kernel=kernel)
                    assert fb[..., 3].max() > 0.05
        _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
        # the float position chain (VRC_OPT_STEPPING = 0)
        on_off(vrc, g, what + " float stepping", stepping=0)
    return fb


@pytest.mark.parametrize("alpha", [0.05, 1.0])
def test_all_uniform_every_kernel_form(vrc, alpha):
    fb = kernel_matrix(vrc, all_uniform_scene(alpha=alpha), "mem alpha %g" % alpha)
    if alpha == 1.0:
        assert fb[..., 3].max() > 0.999  # early ray termination fires inside uniform bricks


@pytest.mark.parametrize("alpha", [0.05, 1.0])
def test_mixed_volume_every_kernel_form(vrc, alpha):
    s = mixed_scene(viewport=(64, 64), alpha=alpha)
    assert_split(s)
    kernel_matrix(vrc, s, "mixed alpha %g" % alpha)


def _special_forms(vrc, s, what):
    with _gpu(s) as g:
        # two passes: the second accumulates into pixels of which some are already past the early-exit threshold
        h = s.n_nodes // 2
        fb, _ = on_off(vrc, g, what + " two passes", passes=[(0, h), (h, s.n_nodes)])
        assert (fb[..., 3] > 0.999).any()
        # ray compaction
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 4)
        on_off(vrc, g, what + " ray compaction")
        _opt(vrc, g, vrc.OPT_ERT_COMPACTION, 0)
        # row bands
        rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, rows.ctypes.data, len(rows)))
        full = g.s
        g.s = copy.copy(full)
        g.s.H = len(rows)
        on_off(vrc, g, what + " row bands")
        g.s = full
        vrc.check(g.L, g.L.vrc_set_row_map(g.ctx, None, 0))
    thin = copy.copy(s)
    thin.tf = orc.linear_ramp_tf(0.05)
    with _gpu(thin) as g:  # depth split needs a frame in which early termination cannot occur
        _opt(vrc, g, vrc.OPT_DEPTH_SPLIT, 1)
        on_off(vrc, g, what + " depth split")


def test_all_uniform_clip_passes_bands_split_compaction(vrc):
    _special_forms(vrc, all_uniform_scene(alpha=1.0, planes=[[0.6, 0.0, 0.8, 0.2]]), "mem")


def test_mixed_volume_clip_passes_bands_split_compaction(vrc):
    _special_forms(vrc, mixed_scene(viewport=(64, 64), alpha=1.0, planes=[[0.6, 0.0, 0.8, 0.2]]), "mixed")


@pytest.mark.parametrize("volume", ["mem", "mixed"])
def test_per_ray_lod_gather_walk(vrc, volume):
    vi = orc.mem_volume_info(64, 64, 64, 16)
    kw = dict(voxels=(64, 64, 64), block=16, viewport=(64, 48), spin=(1.2, 0.3), ids=orc.all_level_ids(vi, None))
    if volume == "mixed":
        kw["volume"] = mixed_volume()
    s = orc.build_scene(**kw)
    with _gpu(s) as g:
        for sse in (0.5, 1.5, 1e3):
            lod = (sse, orc.world_space_per_pixel(s))
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                _, _ = on_off(vrc, g, "%s ray lod sse %g grey %d" % (volume, sse, grey), kernel=vrc.KERNEL_GRID_DDA,
                              ray_lod=lod)


@pytest.mark.parametrize("seed", range(12))
def test_random_views_of_the_mixed_volume(vrc, seed):
    rng = np.random.default_rng(32000 + seed)
    kw = dict(viewport=(int(rng.integers(9, 80)), int(rng.integers(9, 80))),
              spin=(float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.5, 1.5))),
              alpha=float(rng.choice([0.05, 0.3, 1.0])))
    if rng.random() < 0.3:  # eye inside or near the volume
        kw["eye"] = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.1, 0.9)))
    if rng.random() < 0.4:
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        kw["planes"] = [[float(nrm[0]), float(nrm[1]), float(nrm[2]), float(rng.uniform(0.05, 0.4))]]
    if rng.random() < 0.3:
        kw["spr"] = int(rng.choice([97, 300, 700]))
    s = mixed_scene(**kw)
    with _gpu(s) as g:
        for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                on_off(vrc, g, "seed %d kernel %d grey %d %r" % (seed, kernel, grey, kw), kernel=kernel)


def _reupload(vrc, g, t, device):
    """Replace every brick of g by scene t's (same geometry): release + upload takes the slot just released."""
    L = g.L
    hip = C.CDLL("libamdhip64.so")  # the HIP runtime libvrc_hip.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    for nid in t.ids:
        old = g.slots[nid]
        vrc.check(L, L.vrc_pool_release_slot(g.pool, vrc.f32x3(*old)))
        brick = t.bricks[nid]
        size = vrc.u32x3(brick.shape[2], brick.shape[1], brick.shape[0])
        slot = vrc.f32x3()
        if device:
            dev = C.c_void_p()
            assert hip.hipMalloc(C.byref(dev), brick.nbytes) == 0
            assert hip.hipMemcpy(dev, brick.ctypes.data, brick.nbytes, 1) == 0  # hipMemcpyHostToDevice
            vrc.check(L, L.vrc_pool_copy_to_slot_device(g.pool, dev, size, slot))  # returns when the repack has run
            assert hip.hipFree(dev) == 0
        else:
            vrc.check(L, L.vrc_pool_copy_to_slot(g.pool, brick.ctypes.data, size, slot))
        assert tuple(slot) == old
    g.s = t


@pytest.mark.parametrize("device", [False, True])
def test_the_word_follows_the_slot(vrc, device):
    kw = dict(viewport=(64, 64), spin=(1.2, 0.3), alpha=0.3)
    uni = all_uniform_scene(**kw)
    mix = mixed_scene(**kw)
    with _gpu(mix) as g:
        want_mix, n_mix = on_off(vrc, g, "mixed, fresh")
    with _gpu(uni) as g:
        want_uni, n_uni = on_off(vrc, g, "uniform, fresh")
        assert (want_uni != want_mix).any()
        for k in range(2):
            # uniform -> non-uniform in the same slots, and back
            _reupload(vrc, g, mix, device)
            fb, n = on_off(vrc, g, "mixed over uniform %d" % k)
            assert (fb == want_mix).all() and n == n_mix
            _reupload(vrc, g, uni, device)
            fb, n = on_off(vrc, g, "uniform over mixed %d" % k)
            assert (fb == want_uni).all() and n == n_uni


def test_the_word_follows_the_slot_through_the_plugin_cache(vrc, tmp_path):
    # the plugin's LRU path: a GPU cache smaller than the volume, so the passes of one frame upload uniform and
    # non-uniform bricks into the same slots in turn
    from libre_amd import driver as drv
    drv.load_library()
    path = tmp_path / "mixed.raw"
    vol = orc.hash_volume(128, 128, 128)
    vol[:, :, 56:] = 90
    vol[80:, :, 56:] = 0
    vol.tofile(str(path))
    uri = "raw://%s#128,128,128,uint8,32" % path
    frames = {}
    for cache in (1, 64):
        with drv.App(uri, 64, 64, synchronous=True, min_lod=2, max_lod=2, gpu_cache_mb=cache) as app:
            app.set_camera(spin=(1.2, 0.3))
            app.set_colormap(orc.linear_ramp_tf(0.3))
            for turn in range(2):
                for value in (0, 1, 0, 1):
                    app.set_option(vrc.OPT_UNIFORM_BRICKS, value)
                    fb, st = app.render_frame()
                    frames[(cache, turn, value)] = fb
                    if cache == 1:
                        assert st.n_passes > 1
                app.set_camera(spin=(1.2 + 0.4 * (turn + 1), 0.3))
    for cache in (1, 64):
        for turn in range(2):
            assert frames[(cache, turn, 0)][..., 3].max() > 0.05
            assert (frames[(cache, turn, 1)] == frames[(cache, turn, 0)]).all(), (cache, turn)


def test_one_voxel_is_enough(vrc):
    base = np.full((64, 64, 64), 90, dtype=np.uint8)
    odd = base.copy()
    odd[24, 24, 24] = 255  # interior of one brick
    edge = base.copy()
    edge[24, 24, 33] = 255  # interior of a brick, and in the overlap of its neighbour along x
    # (a viewport fine enough that every voxel column of the volume has a ray through it, a transfer function thin
    # enough that the rays get there)
    kw = dict(voxels=(64, 64, 64), block=16, viewport=(128, 128), spin=(0.0, 0.0), alpha=0.05)
    with _gpu(orc.build_scene(volume=base, **kw)) as g:
        plain, _ = on_off(vrc, g, "constant volume")
    with _gpu(orc.build_scene(volume=odd, **kw)) as g:
        fb, _ = on_off(vrc, g, "one odd voxel")
        assert (fb != plain).any()  # the brick took the general march and the voxel is seen
    with _gpu(orc.build_scene(volume=edge, **kw)) as g:
        on_off(vrc, g, "one odd voxel in a neighbour's overlap")


def test_the_option_reads_back_and_defaults_to_on(vrc):
    L = vrc.load_library()
    ctx = C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    v = C.c_int64(-1)
    vrc.check(L, L.vrc_get_option(ctx, vrc.OPT_UNIFORM_BRICKS, C.byref(v)))
    assert v.value == 1
    vrc.check(L, L.vrc_set_option(ctx, vrc.OPT_UNIFORM_BRICKS, 0))
    vrc.check(L, L.vrc_get_option(ctx, vrc.OPT_UNIFORM_BRICKS, C.byref(v)))
    assert v.value == 0
    L.vrc_ctx_destroy(ctx)
