"""Developer timing of the pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1) against the plain gather kernel of
the same build, in one process and at the same cameras: the noise volume (hash://) and the mem:// volume (all uniform
bricks: with VRC_OPT_UNIFORM_BRICKS at its default both frames march from one table entry) at the default camera and
with the model spun by 30 / 20 degrees, point and trilinear samples, both marched by gathers (VRC_KERNEL_GRID_DDA; the walk
cache off, so that the plain frame is the gather kernel's and not the replay's).  Per camera and filter: the plain frame
and the pre-integrated frame, each timed --repeats times -- the spread of those is what a ratio has to exceed to mean
anything.  Kernel ms from the library's HIP events (mean per frame over --steps frames after --warmup), samples from one
counted frame each.

Then one table build, as a transfer-function edit, alone: wall-clock ms per frame of a loop that alternates between two
transfer functions every frame (vrc_update, render, synchronize), with the option at 0 (the 257-entry table is rebuilt)
and at 1 (the 256 x 256 table too), beside the same loop without the edit; VRC_OPT_PREINT_BUILDS says how many tables
the loop built.  The report goes to standard output and to --out (profiles/r13_preint.txt).

Under rocprofv3 (a counter run is kept apart from any tracing) pass --only to keep the run to one row, e.g.
--only hash:off_axis:nearest:preint --steps 1 --warmup 0 --repeats 1."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libre_amd import driver, vrc  # noqa: E402

CAMERAS = (("default", (0.0, 0.0)), ("off_axis", (0.5235988, 0.3490659)))


def ramp(alpha, shift=0.0):
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    tf = np.stack([i, i, i, np.float32(alpha) * np.clip(i + np.float32(shift), 0, 1)], axis=1).astype(np.float32)
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


def time_edits(app, tables, n_warm, n_timed):
    """wall ms per frame of (set_colormap, render, synchronize), cycling through `tables`"""
    for k in range(n_warm):
        app.set_colormap(tables[k % len(tables)])
        app.render_frame(readback=False)
    app.synchronize()
    t0 = time.perf_counter()
    for k in range(n_timed):
        app.set_colormap(tables[k % len(tables)])
        app.render_frame(readback=False)
        app.synchronize()
    return (time.perf_counter() - t0) * 1e3 / max(1, n_timed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=1024)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sources", default="hash,mem")
    ap.add_argument("--only", default=None, help="source:camera:filter:row, e.g. hash:off_axis:nearest:preint")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_preint.txt"))
    a = ap.parse_args()
    driver.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for source in a.sources.split(","):
        say("# tools/dev_preint.py: %s:// %d^3 voxels in %d^3 bricks, %dx%d viewport, alpha %.3g, VRC_KERNEL_GRID_DDA, "
            "%d frames after %d warm-up, %d repeats" % (source, a.voxels, a.block, a.viewport, a.viewport, a.alpha, a.steps,
                                                        a.warmup, a.repeats))
        say("# camera filter row: kernel, kernel ms per frame (mean of the repeats; min .. max), samples per frame, ms against plain")
        uri = "%s://#%d,%d,%d,%d" % (source, a.voxels, a.voxels, a.voxels, a.block)
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
            leaf = probe.volume_info()["depth"] - 1
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
            app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_GRID_DDA)
            app.set_option(vrc.OPT_WALK_CACHE, 0)
            app.set_colormap(ramp(a.alpha))
            for camera, spin in CAMERAS:
                app.set_camera(spin=spin)
                for flt in (0, 1):
                    fname = "trilinear" if flt else "nearest"
                    app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                    results = {}
                    for row, on in (("plain", 0), ("preint", 1)):
                        if a.only and a.only != "%s:%s:%s:%s" % (source, camera, fname, row):
                            continue
                        app.set_preintegration(on)
                        n = count_samples(app)
                        ms = [time_kernel(app, a.warmup, a.steps) for _ in range(a.repeats)]
                        results[row] = ((vrc.load_library().vrc_last_kernel() or b"").decode(), ms, n)
                    app.set_preintegration(0)
                    base = results.get("plain")
                    for row, (kernel, ms, n) in results.items():
                        mean = sum(ms) / len(ms)
                        say("%-8s %-9s %-6s %-62s %8.3f ms (%.3f .. %.3f) %13d samples %s" % (
                            camera, fname, row, kernel, mean, min(ms), max(ms), n,
                            "x%.3f" % (mean / (sum(base[1]) / len(base[1]))) if base else "-"))
            if not a.only:
                # one table build, as a transfer-function edit
                app.set_camera(spin=CAMERAS[0][1])
                say("# %s://, default camera: wall ms per frame of (vrc_update, render, synchronize), %d frames after %d; "
                    "edit = another transfer function every frame" % (source, a.steps, a.warmup))
                two = [ramp(a.alpha), ramp(a.alpha, 0.1)]
                for flt in (0, 1):
                    fname = "trilinear" if flt else "nearest"
                    app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                    for on in (0, 1):
                        app.set_preintegration(on)
                        builds0 = app.get_option(vrc.OPT_PREINT_BUILDS)
                        still = [time_edits(app, two[:1], a.warmup, a.steps) for _ in range(a.repeats)]
                        builds1 = app.get_option(vrc.OPT_PREINT_BUILDS)
                        edit = [time_edits(app, two, a.warmup, a.steps) for _ in range(a.repeats)]
                        builds2 = app.get_option(vrc.OPT_PREINT_BUILDS)
                        say("%-9s option %d: no edit %.3f ms (%.3f .. %.3f; %d tables built), edit %.3f ms (%.3f .. %.3f; %d tables "
                            "built in %d frames): an edit costs %.3f ms" % (
                                fname, on, sum(still) / len(still), min(still), max(still), builds1 - builds0,
                                sum(edit) / len(edit), min(edit), max(edit), builds2 - builds1,
                                a.repeats * (a.warmup + a.steps), sum(edit) / len(edit) - sum(still) / len(still)))
                    app.set_preintegration(0)
        say("")
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
