"""Argument errors of the frame-histogram entry points (vrc_pool_enable_histograms, vrc_frame_histogram,
vrc_get_frame_histogram, lvh_app_set_histogram, lvh_app_frame_histogram): reported as codes and messages before any
device call, so no GPU is needed."""
import pytest


def test_vrc_frame_histogram_argument_errors(built):
    from libre_amd import vrc
    L = vrc.load_library()
    assert L.vrc_pool_enable_histograms(None, 256, None) == vrc.VRC_EINVAL
    assert b"pool is NULL" in L.vrc_last_error()
    assert L.vrc_frame_histogram(None, None, None, None, 0, 0) == vrc.VRC_EINVAL
    assert b"NULL argument" in L.vrc_last_error()
    assert L.vrc_get_frame_histogram(None, None, 256) == vrc.VRC_EINVAL
    assert b"NULL argument" in L.vrc_last_error()


def test_lvh_histogram_argument_errors(built):
    from libre_amd import driver
    L = driver.load_library()
    assert L.lvh_app_set_histogram(None, 1) != 0
    assert b"NULL argument" in L.lvh_last_error()
    assert L.lvh_app_frame_histogram(None, None, 0, None, None, None, None) != 0
    assert b"NULL argument" in L.lvh_last_error()


def test_plugin_binds_the_histogram_entry_points_weakly():
    # the TSan harness links the plugin against a device stand-in without these symbols (tests/host_san/vrc_stub.cpp)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "libre_amd", "host", "src", "hip_plugin.cpp")).read()
    for name in ("vrc_pool_enable_histograms", "vrc_frame_histogram", "vrc_get_frame_histogram"):
        assert "#pragma weak %s" % name in src, name
    stub = open(os.path.join(root, "tests", "host_san", "vrc_stub.cpp")).read()
    assert "vrc_frame_histogram" not in stub


if __name__ == "__main__":
    pytest.main([__file__])
