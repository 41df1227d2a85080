"""Signed and float volumes through the plugin surface (libre_amd.driver.App) on the GPU: the typed pool behind
HipTexturePool, the default data ranges, raw:// and NRRD files bricked on demand with an LOD cut.  Files are held to
tests/ref64.py through affine images of a uint16 volume (tests/voxel_types.py) with test_ref64_cpu.check."""
import numpy as np
import pytest

import orc
import ref64
import scenes
import voxel_types as vt
from test_ref64_cpu import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from libre_amd import driver
    driver.load_library()
    return driver


def _q_volume():
    h = orc.hash_volume(64, 64, 64).astype(np.uint16)
    return h * np.uint16(257) ^ (h >> np.uint16(3))


def _level_grid_bricks(s, vol):
    """The scene's bricks as the raw:// source cuts them: a level above the finest takes every 2^k-th voxel and
    replicates its border in the LEVEL's own grid (tests/test_host.py::test_raw_data_source_bricked_out_of_core), where
    orc.brick_from_volume clamps in the file's grid.  The two differ only in overlap voxels outside the volume, which
    the trilinear filter reads at the volume's far faces.  ref64 samples s.bricks."""
    vi = s.vi
    ov = [vi.overlap[a] for a in range(3)]
    for nid, node in s.lod.items():
        shift = int(vi.depth) - 1 - int(orc.unpack(nid)[0])
        dims = [vol.shape[2 - a] for a in range(3)]
        for _ in range(shift):
            dims = [(d + 1) // 2 for d in dims]
        lo = [int(node.voxelBoxMin[a]) - ov[a] for a in range(3)]
        hi = [int(node.voxelBoxMax[a]) + ov[a] for a in range(3)]
        ix = [np.clip(np.arange(lo[a], hi[a]), 0, dims[a] - 1) << shift for a in range(3)]
        brick = np.ascontiguousarray(vol[np.ix_(ix[2], ix[1], ix[0])])
        assert brick.shape == s.bricks[nid].shape
        s.bricks[nid] = brick


def test_mem_int16_with_the_default_range_is_the_uint16_volume_with_the_same_range(drv):
    # mem:// computes the same brick values in either type; int16 defaults to (-32768, 32767).  The two frames classify
    # v + 32768 over (0, 65535) and v over (-32768, 32767): the same numbers up to float rounding, not the same bits,
    # hence assert_close_frames
    frames = []
    for datatype, rng in (("int16", None), ("uint16", (-32768.0, 32767.0)), ("int16", (-32768.0, 32767.0))):
        with drv.App("mem://?datatype=%s#64,64,64,16" % datatype, 48, 40, synchronous=True, gpu_cache_mb=16) as app:
            assert app.volume_info()["depth"] == 3
            app.set_camera(spin=(0.5, 0.35))
            app.set_colormap(orc.linear_ramp_tf(0.3))
            if rng:
                app.set_data_range(*rng)
            fb, _ = app.render_frame()
            frames.append(fb)
    assert frames[0][..., 3].max() > 0.05
    assert (frames[0] == frames[2]).all()  # the default IS (-32768, 32767)
    scenes.assert_close_frames(frames[0], frames[1], "mem:// int16 against uint16")


@pytest.mark.parametrize("kind", ["raw_float", "nrrd_int16"])
@pytest.mark.parametrize("level", [2, 1])
def test_files_bricked_on_demand_match_ref64(drv, tmp_path, kind, level):
    from libre_amd import vrc
    q = _q_volume()
    if kind == "raw_float":
        im = vt.IMAGES["float_narrow"]
        path = str(tmp_path / "vol.raw")
        im.apply(q).tofile(path)
        uri = "raw://%s#64,64,64,float,16" % path
    else:
        im = vt.IMAGES["int16"]
        path = str(tmp_path / "vol.nrrd")
        with open(path, "wb") as f:
            f.write(b"NRRD0004\ntype: short\ndimension: 3\nsizes: 64 64 64\nendian: little\nencoding: raw\n\n")
            f.write(im.apply(q).tobytes())
        uri = "raw://%s#16" % path
    with drv.App(uri, 48, 40, synchronous=True, min_lod=level, max_lod=level, gpu_cache_mb=16) as app:
        assert app.volume_info()["depth"] == 3
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        app.set_data_range(im.r0, im.r1)
        app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
        fb, _ = app.render_frame()
        n = int(app.stats().samples)
        ids = app.visible_set()
        assert len(ids) == (64 if level == 2 else 8)
        s = orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(48, 40), spin=(0.5, 0.35), volume=q, dtype="u16",
                            ids=ids, data_range=im.q_range())
        _level_grid_bricks(s, q)
        r = ref64.render(s)
        assert r.frame[..., 3].max() > 0.05
        check(s, fb, n, r, "%s, level %d" % (kind, level), "plugin")
        app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR)
        lin, _ = app.render_frame()
        check(s, lin, None, ref64.render(s, filter_mode=1), "%s, level %d, trilinear" % (kind, level), "plugin", count=False)


def test_a_float_volume_needs_a_data_range(drv):
    with drv.App("mem://?datatype=float#64,64,64,16", 32, 32, synchronous=True, gpu_cache_mb=16) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.3))
        with pytest.raises(drv.DriverError) as e:
            app.render_frame()
        assert "lvh_app_set_data_range" in str(e.value)
        with pytest.raises(drv.DriverError) as e:
            app.set_histogram(True)
        assert "not supported" in str(e.value)
        app.set_data_range(0.0, 255.0)  # ... and the same App renders once it has one
        fb, _ = app.render_frame()
        assert np.isfinite(fb).all() and fb[..., 3].max() > 0.05
