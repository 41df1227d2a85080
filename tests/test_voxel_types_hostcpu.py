"""Host side of the signed, 32-bit and float volumes, no GPU: the raw:// LOD pyramid keeps the voxel's own type, and the
plugin still links and runs against a device layer without vrc_pool_create_typed (tests/host_san/vrc_stub.cpp: the weak
symbol is NULL there and the pool comes from vrc_pool_create as before)."""
import os
import subprocess

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drv(built):
    from libre_amd import driver
    driver.load_library()
    return driver


def _volume(dtype):
    h = orc.hash_volume(96, 64, 128).astype(np.int64)  # (z, y, x) = (128, 64, 96): a ragged tree of depth 3
    if dtype == "int16":
        return (h * 257 - 32768).astype(np.int16)  # both signs, both bytes busy
    if dtype == "int8":
        return (h - 128).astype(np.int8)
    if dtype == "int32":
        return (h * 16843009 - 2 ** 31).astype(np.int32)
    return (h.astype(np.float32) - np.float32(127.5)) * np.float32(0.37)  # float: negative values and fractions


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "float"])
def test_raw_lod_pyramid_keeps_the_voxel_type(drv, tmp_path, dtype):
    vol = _volume(dtype)
    assert (vol < 0).any() and (vol > 0).any()
    path = str(tmp_path / "vol.raw")
    vol.tofile(path)
    uri = "raw://%s#96,64,128,%s,16" % (path, dtype)
    info = drv.datasource_info(uri)
    vi = orc.mem_volume_info(96, 64, 128, 16)
    assert info["depth"] == vi.depth == 3
    for nid in orc.leaf_ids(vi):
        want = orc.brick_from_volume(vol, vi, orc.lod_node(vi, nid))
        got = drv.datasource_brick(uri, nid).view(vol.dtype).reshape(want.shape)
        assert (got.view(np.uint8) == want.view(np.uint8)).all()
    # coarser levels: every 2^k-th voxel of the file, bit for bit in the voxel's own type (no averaging through
    # an unsigned or a wider type), border replicated in the level's own grid
    ov = 4
    dims = [vol.shape[2 - a] for a in range(3)]
    for up in (1, 2):
        dims = [(d + 1) // 2 for d in dims]
        nid = orc.pack(vi.depth - 1 - up, 0, 0, 0)
        node = orc.lod_node(vi, nid)
        lo = [int(node.voxelBoxMin[a]) - ov for a in range(3)]
        hi = [int(node.voxelBoxMax[a]) + ov for a in range(3)]
        ix = [np.clip(np.arange(lo[a], hi[a]), 0, dims[a] - 1) * (1 << up) for a in range(3)]
        want = vol[np.ix_(ix[2], ix[1], ix[0])]
        got = drv.datasource_brick(uri, nid).view(vol.dtype).reshape(want.shape)
        assert (got.view(np.uint8) == want.view(np.uint8)).all(), (dtype, up)


def test_plugin_links_and_runs_without_the_typed_pool(tmp_path):
    host = os.path.join(ROOT, "libre_amd", "host")
    srcs = [os.path.join(host, "src", n) for n in ("data.cpp", "datasources.cpp", "uvf_datasource.cpp", "render.cpp",
                                                   "hip_plugin.cpp", "driver.cpp")]
    srcs += [os.path.join(ROOT, "tests", "host_san", n) for n in ("pipeline_stress.cpp", "vrc_stub.cpp")]
    stub = open(os.path.join(ROOT, "tests", "host_san", "vrc_stub.cpp")).read()
    assert "vrc_pool_create_typed" not in stub
    exe = str(tmp_path / "pipeline_stub")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-pthread", "-I" + os.path.join(host, "include"), "-I" + os.path.join(ROOT, "include")] + srcs +
                          ["-o", exe, "-lz"])
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-2:] == ["w", "vrc_pool_create_typed"] for line in nm.splitlines()), "not bound weakly"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, LIVRE_HIP_UPLOAD_THREADS="2"))
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "DONE" in out.stdout, text
    assert "runtime error" not in text and "AddressSanitizer" not in text, text
    assert "sync 1 cache 2 MB: available 512 not available 0 passes 4" in text
