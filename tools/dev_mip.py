"""Developer timing of the maximum-intensity projection (VRC_OPT_PROJECTION) against the composite kernel, in one
session and at the same cameras: the C2 volume (mem://, constant bricks) and the noise volume of the same size (hash://),
at the default camera and with the model spun by 30 / 20 degrees.  Per volume and camera: composite, MIP with
VRC_OPT_MIP_SKIP 0 and MIP with VRC_OPT_MIP_SKIP 1, point-sampled; the same three with the trilinear filter on the noise
volume.  Kernel ms from the library's HIP events (mean per frame over --steps frames after --warmup), samples from one
counted frame each.  The report goes to standard output and to --out (profiles/mip_projection.txt).

Under rocprofv3 (a counter run is kept apart from any tracing) pass --only to keep the run to one row, e.g.
--only noise:off_axis:nearest:mip_skip0 --steps 1 --warmup 0.

--fold (VRC_OPT_MIP_FOLD): the same workloads for the minimum and the mean beside the maximum.  Per volume, camera and
filter: composite, the maximum with skipping off three times (their spread is what a difference has to exceed to mean
anything), the minimum with skipping off and on, the mean; every row against the composite kernel and against the
first maximum run.  The report then goes to profiles/fold_projection.txt.

--depth (VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE): depth tracking against the same frame without it, all in this one
process.  Per volume (mem://, hash://), camera, filter (point and trilinear samples on both volumes) and fold (maximum,
minimum), skipping on: depth off three times (their spread is what a ratio has to exceed to mean anything), depth on,
depth on with a cue of 0.5; the last two against the first depth-off run.  A library without the two options (the
parent of the change that added them) runs the depth-off rows alone.  The report goes to profiles/mip_depth.txt.

--iso (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO): an isosurface frame against the MIP frame with depth tracking of the same
scene, on the noise volume (hash://) at both cameras, point and trilinear samples.  Per camera and filter three rows,
each timed --repeats times (the spread of those is what a difference has to exceed to mean anything): the isosurface
frame with VRC_OPT_MIP_SKIP 1, the same with 0, and the maximum with depth tracking and skipping on.  --iso-value gives
the isovalue; without it the tool bisects for the one about half of the window's rays hit (the share is reported).  The
report goes to profiles/iso_projection.txt."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libre_amd import driver, vrc  # noqa: E402

CAMERAS = (("default", (0.0, 0.0)), ("off_axis", (0.5235988, 0.3490659)))
# (row, VRC_OPT_PROJECTION, VRC_OPT_MIP_SKIP, VRC_OPT_MIP_FOLD)
ROWS = (("composite", vrc.PROJECTION_COMPOSITE, 1, vrc.MIP_FOLD_MAX), ("mip_skip0", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MAX),
        ("mip_skip1", vrc.PROJECTION_MIP, 1, vrc.MIP_FOLD_MAX))
FOLD_ROWS = (("composite", vrc.PROJECTION_COMPOSITE, 1, vrc.MIP_FOLD_MAX), ("max_skip0", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MAX),
             ("max_skip0_b", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MAX), ("max_skip0_c", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MAX),
             ("min_skip0", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MIN), ("min_skip1", vrc.PROJECTION_MIP, 1, vrc.MIP_FOLD_MIN),
             ("mean", vrc.PROJECTION_MIP, 0, vrc.MIP_FOLD_MEAN))
# (row, VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE)
DEPTH_ROWS = (("off", 0, 0), ("off_b", 0, 0), ("off_c", 0, 0), ("depth", 1, 0), ("depth_cue", 1, 500))
OPT_MIP_DEPTH, OPT_MIP_DEPTH_CUE = getattr(vrc, "OPT_MIP_DEPTH", 19), getattr(vrc, "OPT_MIP_DEPTH_CUE", 20)


def depth_report(a, say):
    """--depth: see the module's text."""
    say("# volume camera filter fold row: kernel, kernel ms per frame, samples per frame, ms against the first depth-off run")
    for volume, scheme in (("C2", "mem"), ("noise", "hash")):
        uri = "%s://#%d,%d,%d,%d" % (scheme, a.voxels, a.voxels, a.voxels, a.block)
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
            leaf = probe.volume_info()["depth"] - 1
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
            app.set_colormap(linear_ramp(a.alpha))
            app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
            app.set_option(vrc.OPT_MIP_SKIP, 1)
            try:
                app.set_option(OPT_MIP_DEPTH, 0)
                have = True
            except driver.DriverError:
                have = False
                say("# this library has no VRC_OPT_MIP_DEPTH: depth-off rows only")
            for camera, spin in CAMERAS:
                app.set_camera(spin=spin)
                for flt in (0, 1):
                    fname = "trilinear" if flt else "nearest"
                    app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                    for fold, foldname in ((vrc.MIP_FOLD_MAX, "max"), (vrc.MIP_FOLD_MIN, "min")):
                        app.set_option(vrc.OPT_MIP_FOLD, fold)
                        first = None
                        for row, depth, cue in DEPTH_ROWS:
                            if a.only and a.only != "%s:%s:%s:%s:%s" % (volume, camera, fname, foldname, row):
                                continue
                            if (depth or cue) and not have:
                                continue
                            if have:
                                app.set_option(OPT_MIP_DEPTH, depth)
                                app.set_option(OPT_MIP_DEPTH_CUE, cue)
                            n = count_samples(app)
                            ms = time_kernel(app, a.warmup, a.steps)
                            kernel = (vrc.load_library().vrc_last_kernel() or b"").decode()
                            first = ms if row == "off" else first
                            say("%-5s %-8s %-9s %-3s %-9s %-62s %8.3f ms %13d samples %s" % (
                                volume, camera, fname, foldname, row, kernel, ms, n, "x%.3f" % (ms / first) if first else "-"))
                        if have:
                            app.set_option(OPT_MIP_DEPTH, 0)
                            app.set_option(OPT_MIP_DEPTH_CUE, 0)


def hit_share(app):
    fb, _ = app.render_frame()
    return float((fb[..., 3] > 0).mean())


def iso_report(a, say):
    """--iso: see the module's text."""
    say("# camera filter row: kernel, kernel ms per frame (mean of the repeats; min .. max), samples per frame, ms against mip_depth")
    uri = "hash://#%d,%d,%d,%d" % (a.voxels, a.voxels, a.voxels, a.block)
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
        leaf = probe.volume_info()["depth"] - 1
    with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
        ramp = linear_ramp(a.alpha)
        ramp[:, 3] = np.maximum(ramp[:, 3], np.float32(1e-3))  # (a hit pixel has alpha > 0 whatever the isovalue: hit_share)
        app.set_colormap(ramp)
        for camera, spin in CAMERAS:
            app.set_camera(spin=spin)
            for flt in (0, 1):
                fname = "trilinear" if flt else "nearest"
                app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                iso = a.iso_value
                app.set_isosurface(128.0 if iso is None else iso, a.ambient)  # (before the projection can be selected)
                app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
                app.set_option(vrc.OPT_MIP_SKIP, 1)
                if iso is None:  # the isovalue about half of the rays hit
                    lo, hi = 0.0, 255.0
                    for _ in range(9):
                        iso = 0.5 * (lo + hi)
                        app.set_isosurface(iso, a.ambient)
                        lo, hi = (iso, hi) if hit_share(app) > 0.5 else (lo, iso)
                    iso = float(round(0.5 * (lo + hi)))
                app.set_isosurface(iso, a.ambient)
                say("# %s %s: isovalue %.1f, %.3f of the window's rays hit" % (camera, fname, iso, hit_share(app)))
                results = {}
                for row, projection, skip in (("iso_skip1", vrc.PROJECTION_ISO, 1), ("iso_skip0", vrc.PROJECTION_ISO, 0),
                                              ("mip_depth", vrc.PROJECTION_MIP, 1)):
                    if a.only and a.only != "%s:%s:%s" % (camera, fname, row):
                        continue
                    app.set_option(vrc.OPT_PROJECTION, projection)
                    app.set_option(vrc.OPT_MIP_SKIP, skip)
                    app.set_option(vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MAX)
                    app.set_option(OPT_MIP_DEPTH, 1)
                    n = count_samples(app)
                    ms = [time_kernel(app, a.warmup, a.steps) for _ in range(a.repeats)]
                    kernel = (vrc.load_library().vrc_last_kernel() or b"").decode()
                    results[row] = (kernel, ms, n)
                base = results.get("mip_depth")
                for row, (kernel, ms, n) in results.items():
                    mean = sum(ms) / len(ms)
                    say("%-8s %-9s %-9s %-46s %8.3f ms (%.3f .. %.3f) %13d samples %s" % (
                        camera, fname, row, kernel, mean, min(ms), max(ms), n,
                        "x%.3f" % (mean / (sum(base[1]) / len(base[1]))) if base else "-"))
                app.set_option(OPT_MIP_DEPTH, 0)
                app.set_option(vrc.OPT_MIP_SKIP, 1)
                app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)


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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None, help="volume:camera:filter:row, e.g. noise:off_axis:nearest:mip_skip0")
    ap.add_argument("--fold", action="store_true", help="the minimum and the mean beside the maximum (profiles/fold_projection.txt)")
    ap.add_argument("--depth", action="store_true", help="depth tracking against the same frames without it (profiles/mip_depth.txt)")
    ap.add_argument("--iso", action="store_true", help="an isosurface frame against the MIP frame with depth (profiles/iso_projection.txt)")
    ap.add_argument("--iso-value", type=float, default=None, help="--iso: the isovalue (default: the one about half of the rays hit)")
    ap.add_argument("--ambient", type=float, default=0.2, help="--iso: the ambient share of the shading")
    ap.add_argument("--repeats", type=int, default=3, help="--iso: timings per row")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = FOLD_ROWS if a.fold else ROWS
    a.out = a.out or os.path.join(ROOT, "profiles", "iso_projection.txt" if a.iso else "mip_depth.txt" if a.depth else "fold_projection.txt" if a.fold else "mip_projection.txt")
    driver.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# tools/dev_mip.py: %d^3 voxels in %d^3 bricks, %dx%d viewport, alpha %.3g, %d frames after %d warm-up" % (
        a.voxels, a.block, a.viewport, a.viewport, a.alpha, a.steps, a.warmup))
    if a.depth or a.iso:
        (iso_report if a.iso else depth_report)(a, say)
        if not a.only:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    say("# volume camera filter row: kernel, kernel ms per frame, samples per frame, Gsamples/s, ms against composite%s" % (
        ", ms against the first maximum run" if a.fold else ""))
    for volume, scheme, filters in (("C2", "mem", (0,)), ("noise", "hash", (0, 1))):
        uri = "%s://#%d,%d,%d,%d" % (scheme, a.voxels, a.voxels, a.voxels, a.block)
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, gpu_cache_mb=3072) as probe:
            leaf = probe.volume_info()["depth"] - 1
        with driver.App(uri, a.viewport, a.viewport, synchronous=True, min_lod=leaf, max_lod=leaf, gpu_cache_mb=3072) as app:
            app.set_colormap(linear_ramp(a.alpha))
            for camera, spin in CAMERAS:
                app.set_camera(spin=spin)
                for flt in filters:
                    fname = "trilinear" if flt else "nearest"
                    app.set_option(vrc.OPT_FILTER, vrc.FILTER_TRILINEAR if flt else vrc.FILTER_NEAREST)
                    base = first_max = None
                    for row, projection, skip, fold in rows:
                        if a.only and a.only != "%s:%s:%s:%s" % (volume, camera, fname, row):
                            continue
                        app.set_option(vrc.OPT_PROJECTION, projection)
                        app.set_option(vrc.OPT_MIP_SKIP, skip)
                        app.set_option(vrc.OPT_MIP_FOLD, fold)
                        n = count_samples(app)
                        ms = time_kernel(app, a.warmup, a.steps)
                        kernel = (vrc.load_library().vrc_last_kernel() or b"").decode()
                        base = ms if row == "composite" else base
                        first_max = ms if row == "max_skip0" else first_max
                        say("%-5s %-8s %-9s %-11s %-34s %8.3f ms %13d samples %7.2f Gsamples/s %s%s" % (
                            volume, camera, fname, row, kernel, ms, n, n / ms / 1e6,
                            "x%.3f" % (ms / base) if base else "-", " x%.3f" % (ms / first_max) if first_max else ""))
                    app.set_option(vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
                    app.set_option(vrc.OPT_MIP_SKIP, 1)
                    app.set_option(vrc.OPT_MIP_FOLD, vrc.MIP_FOLD_MAX)
            app.set_option(vrc.OPT_FILTER, vrc.FILTER_NEAREST)
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
