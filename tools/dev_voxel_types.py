"""Developer timing of the typed pools (vrc_pool_create_typed) on dev_bench.py's pattern: one noise volume as uint16,
as its int16 image (q - 32768) and as its float image (-1 + q / 32768), point-sampled and trilinear, at the default
camera and at 30 / 20 degrees; kernel ms and Gsamples/s per case, and the upload rate of the bricks.  Under rocprofv3
(counters only, e.g. --pmc TCC_EA0_RDREQ_128B) pass --types float --steps 1 to keep the run to the float form.
The uint16 rows are the comparison point: they go through vrc_pool_create_typed(UINT16), which is vrc_pool_create's pool."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402
import voxel_types as vt  # noqa: E402
from libre_amd import vrc  # noqa: E402

IMAGES = {
    "uint16": None,
    "int16": vt.IMAGES["int16"],
    "float": vt.IMAGES["float"],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=1024)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--types", nargs="*", default=["uint16", "int16", "float"])
    ap.add_argument("--filters", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--kernel", type=int, default=vrc.KERNEL_GRID_DDA, help="VRC_KERNEL_* (2: gathers for every type)")
    a = ap.parse_args()
    for spin in ((0.0, 0.0), (0.5236, 0.349)):
        t0 = time.time()
        s = orc.build_scene(voxels=(a.voxels,) * 3, block=a.block, viewport=(a.viewport,) * 2, volume="hash",
                            spin=spin, dtype="u16", data_range=(0.0, 65536.0))
        print("spin %s: scene built in %.1fs: %d nodes spr %d atlas %s" % (spin, time.time() - t0, s.n_nodes,
              s.render.samplesPerRay, s.atlas_dim), flush=True)
        for name in a.types:
            im = IMAGES[name]
            if im is None:
                t = vt.copy.copy(s)
                t.voxel_type = vrc.VOXEL_UINT16
            else:
                t = vt.typed_scene(s, im)
            t1 = time.time()
            with vt.typed_gpu_scene(t) as g:
                L = g.L
                vrc.check(L, L.vrc_pool_synchronize(g.pool))
                dt = time.time() - t1
                nbytes = sum(b.nbytes for b in t.bricks.values())
                print("%s: %d bricks, %.2f GB uploaded in %.2f s (%.1f GB/s, host copy included)"
                      % (name, len(t.bricks), nbytes / 1e9, dt, nbytes / 1e9 / dt), flush=True)
                view = C.cast(C.byref(t.view), C.POINTER(vrc.ViewData))
                render = C.cast(C.byref(t.render), C.POINTER(vrc.RenderData))
                nodes = C.cast(t.nodes, C.POINTER(vrc.NodeData))
                for flt in a.filters:
                    fb, n, st = g.render(kernel=a.kernel, filter_mode=flt, count=True)
                    vrc.check(L, L.vrc_set_option(g.ctx, vrc.OPT_COUNT_SAMPLES, 0))
                    ms = []
                    stt = vrc.Stats()
                    for i in range(a.steps + 2):
                        vrc.check(L, L.vrc_pre_render(g.ctx, view))
                        vrc.check(L, L.vrc_render(g.ctx, view, nodes, t.n_nodes, render, g.pool))
                        vrc.check(L, L.vrc_get_stats(g.ctx, C.byref(stt)))
                        if i >= 2:
                            ms.append(stt.kernel_ms)
                    ms = np.array(ms)
                    print("%s spin %s filter %d: %s: median %.3f ms min %.3f max %.3f -> %.1f Gsamples/s (%d samples, alpha max %.3f)"
                          % (name, spin, flt, L.vrc_last_kernel().decode(), np.median(ms), ms.min(), ms.max(),
                             n / np.median(ms) / 1e6, n, fb[..., 3].max()), flush=True)


if __name__ == "__main__":
    main()
