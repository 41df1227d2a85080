"""Costs of the frame histogram on C2 (mem://#1024,1024,1024,128 uint8, 1024^2 viewport, the 512 leaf bricks of
136^3 voxels):
  1. the one-time binning of every resident brick when the histogram is turned on (vrc_pool_enable_histograms),
  2. the binning added to one brick's upload (512 uploads with the histograms on vs off),
  3. the reduction per frame (vrc_frame_histogram over the 512 rows),
  4. lvh_app_render_frame with the histogram on and off, alternating, in one run.
All times are host clocks around calls that end with a synchronisation: they include launch and wait latencies
(an upper bound of the kernels' own time).  Prints one line per measurement.

  python tools/dev_frame_histogram.py [--reps N]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(ts):
    return 1e3 * float(np.median(ts))


def device_layer(reps):
    from libre_amd import vrc
    L = vrc.load_library()
    ctx, pool = C.c_void_p(), C.c_void_p()
    vrc.check(L, L.vrc_ctx_create(0, C.byref(ctx)))
    dim = 136
    vrc.check(L, L.vrc_pool_create(ctx, 1, 0, 0, 1, vrc.u32x3(dim, dim, dim), 640 * dim ** 3, C.byref(pool)))
    rng = np.random.default_rng(1)
    brick = rng.integers(0, 256, size=(dim, dim, dim), dtype=np.uint8)
    slots = []
    for _ in range(512):
        s = vrc.f32x3()
        vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(dim, dim, dim), s))
        slots.append(s)
    vrc.check(L, L.vrc_pool_synchronize(pool))
    ov = vrc.u32x3(4, 4, 4)
    interior_bytes = 512 * 128 ** 3
    # 1. cold binning of the resident set
    ts = []
    for _ in range(reps):
        vrc.check(L, L.vrc_pool_enable_histograms(pool, 0, None))
        t0 = time.perf_counter()
        vrc.check(L, L.vrc_pool_enable_histograms(pool, 256, ov))
        vrc.check(L, L.vrc_pool_synchronize(pool))
        ts.append(time.perf_counter() - t0)
    ms = _median_ms(ts)
    print("cold binning of 512 resident bricks (enable, incl. table allocation): %.3f ms median of %d, "
          "%.2f GB/s of interior voxels" % (ms, reps, interior_bytes / ms / 1e6))
    # 2. the binning added to an upload: re-upload every brick with the histograms on and off
    def reupload():
        t0 = time.perf_counter()
        for i, s in enumerate(slots):
            vrc.check(L, L.vrc_pool_release_slot(pool, s))
            vrc.check(L, L.vrc_pool_copy_to_slot(pool, brick.ctypes.data, vrc.u32x3(dim, dim, dim), s))
        vrc.check(L, L.vrc_pool_synchronize(pool))
        return time.perf_counter() - t0
    on, off = [], []
    for _ in range(max(2, reps // 2)):
        vrc.check(L, L.vrc_pool_enable_histograms(pool, 256, ov))
        on.append(reupload())
        vrc.check(L, L.vrc_pool_enable_histograms(pool, 0, None))
        off.append(reupload())
    print("512 uploads: histograms on %.2f ms, off %.2f ms (medians): %+.2f us per brick" %
          (_median_ms(on), _median_ms(off), (np.median(on) - np.median(off)) / 512 * 1e6))
    # 3. the reduction per frame
    vrc.check(L, L.vrc_pool_enable_histograms(pool, 256, ov))
    flat = (C.c_float * (3 * 512))(*[v for s in slots for v in s])
    scales = (C.c_uint64 * 512)(*([1] * 512))
    vrc.check(L, L.vrc_frame_histogram(ctx, pool, flat, scales, 512, 0))
    vrc.check(L, L.vrc_synchronize(ctx))
    single = []
    for _ in range(50):
        t0 = time.perf_counter()
        vrc.check(L, L.vrc_frame_histogram(ctx, pool, flat, scales, 512, 0))
        vrc.check(L, L.vrc_synchronize(ctx))
        single.append(time.perf_counter() - t0)
    n = 200
    t0 = time.perf_counter()
    for _ in range(n):
        vrc.check(L, L.vrc_frame_histogram(ctx, pool, flat, scales, 512, 0))
    vrc.check(L, L.vrc_synchronize(ctx))
    back = (time.perf_counter() - t0) / n
    out = np.zeros(256, dtype=np.uint64)
    vrc.check(L, L.vrc_get_frame_histogram(ctx, out.ctypes.data, 256))
    assert int(out.sum()) == 512 * 128 ** 3
    print("reduction of 512 rows: %.1f us per call with its own synchronisation (median of 50), %.1f us per call "
          "back to back (%d calls)" % (_median_ms(single) * 1e3, back * 1e6, n))
    L.vrc_pool_destroy(pool)
    L.vrc_ctx_destroy(ctx)


def frames(reps):
    from libre_amd import driver
    import orc
    uri = "mem://#1024,1024,1024,128"
    with driver.App(uri, 1024, 1024, synchronous=True, min_lod=3, max_lod=3, gpu_cache_mb=3072) as app:
        app.set_camera(spin=(0.5, 0.35))
        app.set_colormap(orc.linear_ramp_tf(0.05))
        for _ in range(3):
            app.render_frame(readback=False)
        app.set_histogram(True)
        app.render_frame(readback=False)  # the cold binning happens here
        app.synchronize()
        on, off = [], []
        for k in range(2 * reps):
            enable = k % 2 == 0
            app.set_histogram(enable)
            app.synchronize()
            t0 = time.perf_counter()
            app.render_frame(readback=False)
            app.synchronize()
            (on if enable else off).append(time.perf_counter() - t0)
        print("C2 render_frame + synchronize, alternating: histogram on %.3f ms, off %.3f ms (medians of %d each)" %
              (_median_ms(on), _median_ms(off), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    device_layer(a.reps)
    frames(a.reps)


if __name__ == "__main__":
    main()
