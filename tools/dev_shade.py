"""Developer timing of the shaded composite frame (VRC_OPT_SHADING = 1) against the unshaded gather kernel of the same
build, in one process and at the same cameras: the noise volume (hash://; mem:// is all uniform bricks and would time
nothing) at the default camera and with the model spun by 30 / 20 degrees, point and trilinear samples, both marched by
gathers (VRC_KERNEL_GRID_DDA; the walk cache off, so that the unshaded frame is the gather kernel's and not the replay's).
Per camera and filter, with the plain ramp and with a ramp that is transparent over the lower half of its range (what
the gradient skip buys): the unshaded frame and the shaded frame, each timed --repeats times -- the spread of those is
what a ratio has to exceed to mean anything.  Kernel ms from the library's HIP events (mean per frame over --steps frames
after --warmup), samples from one counted frame each.  The report goes to standard output and to --out
(profiles/r11_shade.txt).

Under rocprofv3 (a counter run is kept apart from any tracing) pass --only to keep the run to one row, e.g.
--only off_axis:nearest:ramp:shaded --steps 1 --warmup 0 --repeats 1."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libre_amd import driver, vrc  # noqa: E402

CAMERAS = (("default", (0.0, 0.0)), ("off_axis", (0.5235988, 0.3490659)))


def ramp(alpha, transparent_below=0):
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    tf = np.stack([i, i, i, np.float32(alpha) * i], axis=1).astype(np.float32)
    tf[:transparent_below, 3] = 0.0
    return np.ascontiguousarray(tf)


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
    ap.add_argument("--voxels", type=int, default=1024)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--ambient", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="camera:filter:table:row, e.g. off_axis:nearest:ramp:shaded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_shade.txt"))
    a = ap.parse_args()
    driver.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# tools/dev_shade.py: hash:// %d^3 voxels in %d^3 bricks, %dx%d viewport, alpha %.3g, ambient %.3g, VRC_KERNEL_GRID_DDA, "
        "%d frames after %d warm-up, %d repeats" % (a.voxels, a.block, a.viewport, a.viewport, a.alpha, a.ambient, a.steps,
                                                    a.warmup, a.repeats))
    say("# camera filter table row: kernel, kernel ms per frame (mean of the repeats; min .. max), samples per frame, ms against unshaded")
    uri = "hash://#%d,%d,%d,%d" % (a.voxels, a.voxels, a.voxels, a.block)
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
        leaf = probe.volume_info()["depth"] - 1
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
        app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_GRID_DDA)
        app.set_option(vrc.OPT_WALK_CACHE, 0)
        for camera, spin in CAMERAS:
            app.set_camera(spin=spin)
            for flt in (0, 1):
                fname = "trilinear" if flt else "nearest"
                app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                for table, below in (("ramp", 0), ("half_transparent", 128)):
                    app.set_colormap(ramp(a.alpha, below))
                    results = {}
                    for row, on in (("unshaded", False), ("shaded", True)):
                        if a.only and a.only != "%s:%s:%s:%s" % (camera, fname, table, row):
                            continue
                        app.set_shading(on, a.ambient)
                        n = count_samples(app)
                        ms = [time_kernel(app, a.warmup, a.steps) for _ in range(a.repeats)]
                        results[row] = ((vrc.load_library().vrc_last_kernel() or b"").decode(), ms, n)
                    app.set_shading(False)
                    base = results.get("unshaded")
                    for row, (kernel, ms, n) in results.items():
                        mean = sum(ms) / len(ms)
                        say("%-8s %-9s %-16s %-8s %-62s %8.3f ms (%.3f .. %.3f) %13d samples %s" % (
                            camera, fname, table, row, kernel, mean, min(ms), max(ms), n,
                            "x%.3f" % (mean / (sum(base[1]) / len(base[1]))) if base else "-"))
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
