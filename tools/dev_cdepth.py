"""Developer timing of the depth of a composite frame (VRC_OPT_COMPOSITE_DEPTH) against the plain gather kernel of the same
build, in one process and at the same cameras: the noise volume (hash://; --scheme mem: all uniform bricks, the volume
the walk cache replays) at the default camera and with the model spun by 30 / 20 degrees, point and trilinear samples,
marched by gathers (VRC_KERNEL_GRID_DDA).  Per camera and filter three rows, each timed --repeats times -- the spread
of those is what a ratio has to exceed to mean anything:
  plain   the option at 0, the walk cache off: the gather kernel the depth frame is compared with;
  depth   the option at --tau, the walk cache off;
  replay  the option at 0, the walk cache on: what a still view gives up while the option is set (a depth frame is not
          replayed).
Kernel ms from the library's HIP events (mean per frame over --steps frames after --warmup), samples from one counted
frame each, and for the depth row a pick at the centre and at a corner pixel (the read-back path, once).  The report goes to standard output and to --out
(profiles/r12_cdepth.txt).

Under rocprofv3 (a counter run is kept apart from any tracing) pass --only to keep the run to one row, e.g.
--only off_axis:nearest:depth --steps 1 --warmup 0 --repeats 1."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libre_amd import driver, vrc  # noqa: E402

CAMERAS = (("default", (0.0, 0.0)), ("off_axis", (0.5235988, 0.3490659)))
ROWS = (("plain", 0, 0), ("depth", 1, 0), ("replay", 0, 1))  # name, the option on, the walk cache on


def ramp(alpha):
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.stack([i, i, i, np.float32(alpha) * i], axis=1).astype(np.float32))


def time_kernel(app, n_warm, n_timed):
    for _ in range(n_warm):
        app.render_frame(readback=False)
    app.synchronize()
    app.stats()
    for _ in range(n_timed):
        app.render_frame(readback=False)
    app.synchronize()
    st = app.stats()
    return st.kernel_ms_sum / max(1, st.kernel_launches)


def count_samples(app):
    app.set_option(vrc.OPT_COUNT_SAMPLES, 1)
    app.render_frame(readback=False)
    n = int(app.stats().samples)
    app.set_option(vrc.OPT_COUNT_SAMPLES, 0)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="hash", help="hash (noise) or mem (every brick one value: the walk cache replays)")
    ap.add_argument("--voxels", type=int, default=1024)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--tau", type=int, default=500, help="VRC_OPT_COMPOSITE_DEPTH of the depth row, thousandths")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="camera:filter:row, e.g. off_axis:nearest:depth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_cdepth.txt"))
    a = ap.parse_args()
    driver.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# tools/dev_cdepth.py: " + a.scheme + ":// %d^3 voxels in %d^3 bricks, %dx%d viewport, alpha %.3g, tau %d / 1000, VRC_KERNEL_GRID_DDA, "
        "%d frames after %d warm-up, %d repeats" % (a.voxels, a.block, a.viewport, a.viewport, a.alpha, a.tau, a.steps, a.warmup,
                                                    a.repeats))
    say("# camera filter row: kernel, kernel ms per frame (mean of the repeats; min .. max), samples per frame, ms against plain")
    uri = "%s://#%d,%d,%d,%d" % (a.scheme, a.voxels, a.voxels, a.voxels, a.block)
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
        leaf = probe.volume_info()["depth"] - 1
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_GRID_DDA)
        app.set_colormap(ramp(a.alpha))
        for camera, spin in CAMERAS:
            app.set_camera(spin=spin)
            for flt in (0, 1):
                fname = "trilinear" if flt else "nearest"
                app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                results = {}
                for row, on, walk in ROWS:
                    if a.only and a.only != "%s:%s:%s" % (camera, fname, row):
                        continue
                    app.set_option(vrc.OPT_WALK_CACHE, walk)
                    app.set_composite_depth(a.tau if on else 0)
                    n = count_samples(app)
                    ms = [time_kernel(app, a.warmup, a.steps) for _ in range(a.repeats)]
                    crossed = ""
                    if on:
                        hits = sum(app.pick(x, y)[0] for x, y in ((a.viewport // 2, a.viewport // 2), (3, 3)))
                        crossed = " (centre and corner pixel: %d of 2 crossed)" % hits
                    results[row] = ((vrc.load_library().vrc_last_kernel() or b"").decode(), ms, n, crossed)
                app.set_composite_depth(0)
                app.set_option(vrc.OPT_WALK_CACHE, 1)
                base = results.get("plain")
                for row, (kernel, ms, n, crossed) in results.items():
                    mean = sum(ms) / len(ms)
                    say("%-8s %-9s %-6s %-66s %8.3f ms (%.3f .. %.3f) %13d samples %s%s" % (
                        camera, fname, row, kernel, mean, min(ms), max(ms), n,
                        "x%.3f" % (mean / (sum(base[1]) / len(base[1]))) if base else "-", crossed))
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
