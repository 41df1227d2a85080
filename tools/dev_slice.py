"""Developer timing of a slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE) against the MIP frame of the same view,
in one session: the C2 volume (mem://, constant bricks) and the noise volume of the same size (hash://), the model spun by
30 / 20 degrees so that an axial, a coronal and an oblique plane through the centre all face the camera.  Per volume,
brick loop (VRC_KERNEL_REFERENCE_ORDER, VRC_KERNEL_GRID_DDA) and filter: the three slices and the MIP frame (maximum,
skipping on).  Every row is timed --rounds times, each the mean kernel time per frame from the library's HIP events
(vrc_stats) over --steps frames after --warmup warm ones; the report gives the range of the rounds, not their mean, and
each slice's largest round against the MIP frame's smallest.  Samples from one counted frame each.  The report goes to
standard output and to --out (profiles/r17_slice.txt).

Under rocprofv3 (a counter run is kept apart from any tracing) pass --only to keep the run to one row, e.g.
--only noise:dda:nearest:oblique --rounds 1 --steps 1 --warmup 0."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libre_amd import driver, vrc  # noqa: E402

SPIN = (0.5235988, 0.3490659)
PLANES = (("axial", (0.0, 0.0, 1.0)), ("coronal", (0.0, 1.0, 0.0)), ("oblique", (0.31, -0.42, 0.85)))
LOOPS = (("reforder", vrc.KERNEL_REFERENCE_ORDER), ("dda", vrc.KERNEL_GRID_DDA))


def linear_ramp(alpha):
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.stack([i, i, i, np.float32(alpha) * i], axis=1).astype(np.float32))


def time_kernel(app, n_warm, n_timed):
    for _ in range(n_warm):
        app.render_frame(readback=False)
    app.synchronize()
    app.stats()
    for _ in range(n_timed):
        app.render_frame(readback=False)
    app.synchronize()  # (the renderer's own stream; torch, imported after the library, would find no device)
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="volume:loop:filter:row, e.g. noise:dda:nearest:oblique")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "r17_slice.txt")
    driver.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# tools/dev_slice.py: %d^3 voxels in %d^3 bricks, %dx%d viewport, model spun by 30 / 20 degrees, alpha %.3g; "
        "%d rounds of %d frames after %d warm-up" % (a.voxels, a.block, a.viewport, a.viewport, a.alpha, a.rounds, a.steps, a.warmup))
    say("# volume loop filter row: kernel, kernel ms per frame (smallest .. largest round), samples per frame, "
        "largest round against the MIP frame's smallest")
    lost = 0
    for volume, scheme in (("C2", "mem"), ("noise", "hash")):
        uri = "%s://#%d,%d,%d,%d" % (scheme, a.voxels, a.voxels, a.voxels, a.block)
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
            leaf = probe.volume_info()["depth"] - 1
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
            app.set_colormap(linear_ramp(a.alpha))
            app.set_camera(spin=SPIN)
            for loop, kernel in LOOPS:
                app.set_option(vrc.OPT_KERNEL, kernel)
                for flt in (0, 1):
                    fname = "trilinear" if flt else "nearest"
                    app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                    results = []
                    for row, normal in (("mip", None),) + PLANES:
                        if a.only and a.only != "%s:%s:%s:%s" % (volume, loop, fname, row):
                            continue
                        if normal is None:
                            app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
                            app.set_option(vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MAX)
                            app.set_option(vrc.OPT_MIP_SKIP, 1)
                        else:
                            app.set_slice((0.0, 0.0, 0.0), normal)  # (before the projection can be selected)
                            app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_SLICE)
                        n = count_samples(app)
                        ms = [time_kernel(app, a.warmup, a.steps) for _ in range(a.rounds)]
                        name = (vrc.load_library().vrc_last_kernel() or b"").decode()
                        results.append((row, name, ms, n))
                    mip = [r for r in results if r[0] == "mip"]
                    for row, name, ms, n in results:
                        against = "-"
                        if mip and row != "mip":
                            against = "x%.3f" % (max(ms) / min(mip[0][2]))
                            lost += max(ms) > min(mip[0][2])
                        say("%-5s %-8s %-9s %-8s %-58s %8.4f .. %8.4f ms %13d samples %s" % (
                            volume, loop, fname, row, name, min(ms), max(ms), n, against))
                    app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
            app.set_option(vrc.OPT_FILTER, vrc.FILTER_NEAREST)
            app.set_option(vrc.OPT_KERNEL, vrc.KERNEL_AUTO)
    say("# slice rows slower than the MIP frame of their view: %d" % lost)
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
