"""A/B of VRC_OPT_UNIFORM_BRICKS on one scene through the C ABI: the same frame with the option off and on (compared bit
for bit), then the raycast kernel timed from the library's HIP events (vrc_get_stats) in alternating rounds.
usage: python tools/uniform_ab.py [--volume mem|hash] [--steps 20] [--rounds 3] [--lib libvrc_hip.so]
A library that does not know the option (an older build) is timed once, as "off".
Forms of the uniform march against each other (the product carries no switch for them: they are builds,
tools/build_variants.sh NAME "-DVRC_UNIFORM_GROUP=8", or an older commit's library):
       python tools/uniform_ab.py --libs parent=variants/libvrc_hip_parent.so new=libre_amd/lib/libvrc_hip.so ...
renders the frame with every library, option on (compared bit for bit with the first one's, counts included), and
times them in alternating rounds in this one process; --walk-always sets VRC_OPT_WALK_CACHE = 2 in each of them, so
that a hash:// view is replayed (the gather path of the replay) instead of walked.
VRC_OPT_STREAM_MARKERS (what vrc_render puts on the stream besides the march) in one process:
       python tools/uniform_ab.py --markers [--steps 2000] [--rounds 3]
renders the frame with the option at 1 and at 0 (compared bit for bit), then in alternating rounds runs --steps frames
back to back and reports the wall time per frame of the synchronised loop beside the library's mean kernel time.  The
wall time is the figure to compare: the kernel time ends with a marker behind the march at 1 and with the dispatch itself at 0.
VRC_OPT_RAY_CACHE (rays computed every frame against rays loaded from the context's cache) the same way:
       python tools/uniform_ab.py --ray-cache [--steps 2000] [--rounds 3]
VRC_OPT_WALK_CACHE (the brick grid walked every frame against the march replayed from the context's recorded lists):
       python tools/uniform_ab.py --walk-cache [--steps 2000] [--rounds 3]
Frames and sample counts at 0 and 1 are compared bit for bit, and the option at 1 must have reached the replay
(VRC_OPT_WALK_CACHE_USED = 4), before anything is timed; the kernel instance of either side is reported.
VRC_OPT_STORE_THROUGH (the replayed frame's pixels stored plainly against written through the L2) the same way:
       python tools/uniform_ab.py --store-through [--steps 2000] [--rounds 3]
One context, one set of lists: frames and sample counts at 0 and 1 are compared bit for bit on replayed frames, with
VRC_OPT_STORE_THROUGH_USED reading what was asked, before the clock runs; the wall time per frame is the figure to compare.
VRC_OPT_FIRST_VISIT_TABLE (a ray's first uniform visit marched against taken from the context's table) the same way:
       python tools/uniform_ab.py --first-visit [--steps 2000] [--rounds 3]
The frames compared are uncounted replayed ones (a counted frame marches every visit), with
VRC_OPT_FIRST_VISIT_TABLE_USED reading what was asked before the clock runs and behind every timed loop.
VRC_OPT_LEAN_FREE_MARCH (a visit that cannot reach the exit threshold marched with the exit test against without) the same way:
       python tools/uniform_ab.py --free-march [--steps 2000] [--rounds 3]
Uncounted replayed frames again (the counted instances hold no such body), VRC_OPT_LEAN_FREE_MARCH_USED read as above.
VRC_OPT_WALK_RESOLVED (the uniform-only replay reading list and slot words against resolved visit words) the same way:
       python tools/uniform_ab.py --resolved [--steps 2000] [--rounds 3]
Uncounted replayed frames again (the counted instances read the lists), VRC_OPT_WALK_RESOLVED_USED read as above.
With --libs it times every library that knows the option at 0 and at 1 beside those that do not, as --uniform-only does.
With --steps of 200 or more, --libs reports the wall time per frame and the mean kernel time of such a loop as well.
VRC_OPT_WALK_UNIFORM_ONLY (the lean replay against its uniform-only instance) beside builds, in one process:
       python tools/uniform_ab.py --uniform-only --libs parent=variants/libvrc_hip_parent.so new=libre_amd/lib/libvrc_hip.so
times `new` with the option at 0 and at 1 (new@0, new@1) and `parent`, which does not know it, once; the frames
compared bit for bit are replayed ones, and on mem:// the option's read-back must say what was asked."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402
from gpu_run import GpuScene  # noqa: E402
from libre_amd import vrc  # noqa: E402


def frame_loop(g, s):
    """run(n): n frames back to back (vrc_pre_render + vrc_render, nothing read back), then a synchronise."""
    L = g.L
    view = C.cast(C.byref(s.view), C.POINTER(vrc.ViewData))
    render = C.cast(C.byref(s.render), C.POINTER(vrc.RenderData))
    nodes = C.cast(s.nodes, C.POINTER(vrc.NodeData))

    def run(n):
        for _ in range(n):
            vrc.check(L, L.vrc_pre_render(g.ctx, view))
            vrc.check(L, L.vrc_render(g.ctx, view, nodes, s.n_nodes, render, g.pool))
        vrc.check(L, L.vrc_synchronize(g.ctx))
    return run


def timed_loop(g, run, steps):
    """(wall ms per frame, mean kernel ms) of `steps` frames after a warm-up (clocks, the tile schedule, the ray cache)."""
    stats = vrc.Stats()
    run(max(40, steps // 10))
    vrc.check(g.L, g.L.vrc_get_stats(g.ctx, C.byref(stats)))
    t0 = time.perf_counter()
    run(steps)
    wall = (time.perf_counter() - t0) * 1e3 / steps
    vrc.check(g.L, g.L.vrc_get_stats(g.ctx, C.byref(stats)))
    assert stats.kernel_launches == steps
    return round(wall, 5), round(stats.kernel_ms_sum / stats.kernel_launches, 5)


def several(a):
    """--libs: the same frame, option on, through several builds of the library."""
    s = orc.build_scene(voxels=(a.voxels,) * 3, block=a.block, viewport=(a.viewport,) * 2, volume=a.volume,
                        spin=tuple(a.spin), spr=a.spr)
    names, scenes = [], {}
    for spec in a.libs:
        name, path = spec.split("=", 1)
        L = vrc.load_library(os.path.abspath(path))
        names.append(name)
        scenes[name] = GpuScene(s, lib=L)
        if a.walk_always:  # replay whatever the bricks hold: the gather path of the replay on hash://
            vrc.check(L, L.vrc_set_option(scenes[name].ctx, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS))
    # --uniform-only: a library that knows VRC_OPT_WALK_UNIFORM_ONLY is timed at 0 and at 1 (NAME@0, NAME@1: one context,
    # the same lists, the option set in front of every timed loop); one that does not is timed once, as NAME
    # --resolved with --libs: the same with VRC_OPT_WALK_RESOLVED (NAME@0 is the build without its resolved words)
    sided = a.uniform_only or a.resolved
    option = vrc.OPT_WALK_RESOLVED if a.resolved else vrc.OPT_WALK_UNIFORM_ONLY
    sides = []  # (label, library's name, value of the option or None)
    for name in names:
        g = scenes[name]
        if sided and g.L.vrc_set_option(g.ctx, option, 1) == 0:
            sides += [(name + "@0", name, 0), (name + "@1", name, 1)]
        else:
            sides.append((name, name, None))

    def select(side):
        g = scenes[side[1]]
        if side[2] is not None:
            vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, side[2]))
        return g
    first = None
    for side in sides:
        g = select(side)
        for _ in range(7 if sided else 1):  # (--uniform-only, --resolved: the frame compared is a replayed one)
            fb, n = g.render(count=True)[:2]
        if first is None:
            first = (fb, n)
        assert (fb == first[0]).all() and n == first[1], "%s: frame or count differs from %s" % (side[0], sides[0][0])
        if side[2] is not None and a.resolved:  # (the words serve uncounted frames: read back behind one)
            g.render(count=False)
            used = C.c_int64(-1)
            vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_WALK_RESOLVED_USED, C.byref(used)))
            assert used.value == side[2] or a.volume != "mem", "%s: VRC_OPT_WALK_RESOLVED_USED reads %d" % (side[0], used.value)
        elif side[2] is not None:
            used = C.c_int64(-1)
            vrc.check(g.L, g.L.vrc_get_option(g.ctx, vrc.OPT_WALK_UNIFORM_ONLY_USED, C.byref(used)))
            assert used.value == side[2] or a.volume != "mem", "%s: VRC_OPT_WALK_UNIFORM_ONLY_USED reads %d" % (side[0], used.value)
    ms = {side[0]: [] for side in sides}
    wall = {side[0]: [] for side in sides}
    mean = {side[0]: [] for side in sides}
    kernels = {}
    for _ in range(a.rounds):
        for side in sides:
            name = side[0]
            g = select(side)
            if a.steps >= 200:  # a loop long enough for a wall time
                for _ in range(6):  # synchronised frames: the tile schedule, the ray cache and the walk cache settle
                    g.render(count=False)
                w, k = timed_loop(g, frame_loop(g, s), a.steps)
                wall[name].append(w)
                mean[name].append(k)
                kernels[name] = g.L.vrc_last_kernel().decode()
                continue
            g.render(count=False)  # warm-up: the tile schedule
            best = None
            for _ in range(a.steps):
                _, _, st = g.render(count=False)
                best = st.kernel_ms if best is None else min(best, st.kernel_ms)
            ms[name].append(round(best, 4))
            kernels[name] = g.L.vrc_last_kernel().decode()
    print(json.dumps({"volume": a.volume, "spin": list(a.spin), "spr": s.render.samplesPerRay, "samples": first[1],
                      "kernel": kernels, "kernel_ms_min_per_round": ms, "wall_ms_per_frame": wall,
                      "kernel_ms_mean": mean, "frames_bit_identical": True}))
    for g in scenes.values():
        g.close()


def markers(a, option=None, names=("lean", "markers")):
    """--markers: VRC_OPT_STREAM_MARKERS 1 against 0, the same context and pool (--ray-cache: VRC_OPT_RAY_CACHE)."""
    option = vrc.OPT_STREAM_MARKERS if option is None else option
    s = orc.build_scene(voxels=(a.voxels,) * 3, block=a.block, viewport=(a.viewport,) * 2, volume=a.volume,
                        spin=tuple(a.spin), spr=a.spr)
    L = vrc.load_library(a.lib) if a.lib else vrc.load_library()
    g = GpuScene(s, lib=L)
    frames = {}
    walk = option == vrc.OPT_WALK_CACHE
    first = option in (vrc.OPT_FIRST_VISIT_TABLE, vrc.OPT_LEAN_FREE_MARCH, vrc.OPT_WALK_RESOLVED)  # (what serves uncounted frames alone)
    store = option == vrc.OPT_STORE_THROUGH or first  # (both sides are replayed frames: the option starts nothing over)
    read_back = {vrc.OPT_FIRST_VISIT_TABLE: vrc.OPT_FIRST_VISIT_TABLE_USED,
                 vrc.OPT_LEAN_FREE_MARCH: vrc.OPT_LEAN_FREE_MARCH_USED,
                 vrc.OPT_WALK_RESOLVED: vrc.OPT_WALK_RESOLVED_USED}.get(option, vrc.OPT_STORE_THROUGH_USED)
    on = vrc.WALK_CACHE_ALWAYS if walk else 1  # (the replay on any volume: at 1 a view that gathers keeps the walk)
    settle = 6 if walk or store else 3  # synchronised frames until the steady state (the ray cache: computed, stored,
    #                                     loaded; the walk cache: counted, recorded and replayed behind that)
    if store and a.volume != "mem":
        vrc.check(L, L.vrc_set_option(g.ctx, vrc.OPT_WALK_CACHE, vrc.WALK_CACHE_ALWAYS))

    def walk_mode():
        used = C.c_int64(-1)
        vrc.check(L, L.vrc_get_option(g.ctx, vrc.OPT_WALK_CACHE_USED, C.byref(used)))
        return used.value
    for v in (1, 0):
        vrc.check(L, L.vrc_set_option(g.ctx, option, on if v else 0))
        for _ in range(settle):
            frames[v] = g.render(count=not first)[:2]  # (the table serves uncounted frames alone)
        used = C.c_int64(0)
        if walk:
            assert walk_mode() == (4 if v else 0), "the frame compared was not replayed"
        if option == vrc.OPT_RAY_CACHE:
            vrc.check(L, L.vrc_get_option(g.ctx, vrc.OPT_RAY_CACHE_USED, C.byref(used)))
            assert used.value == (2 if v else 0), "the third frame did not load its rays"
        if store:
            vrc.check(L, L.vrc_get_option(g.ctx, read_back, C.byref(used)))
            assert walk_mode() == 4 and used.value == v, "mode %d, the option's read-back reads %d" % (walk_mode(), used.value)
    assert (frames[0][0] == frames[1][0]).all() and frames[0][1] == frames[1][1], "frames differ"
    g.render(count=False)
    run = frame_loop(g, s)
    wall = {1: [], 0: []}
    kernel = {1: [], 0: []}
    ran = {}
    for _ in range(a.rounds):
        for v in (1, 0):
            vrc.check(L, L.vrc_set_option(g.ctx, option, on if v else 0))
            if walk:  # the option starts the lists over: back to the replay before the clock runs
                for _ in range(settle):
                    g.render(count=False)
                assert walk_mode() == (4 if v else 0)
            w, k = timed_loop(g, run, a.steps)
            if walk:
                assert walk_mode() == (4 if v else 0)
            if store:
                vrc.check(L, L.vrc_get_option(g.ctx, read_back, C.byref(used)))
                assert walk_mode() == 4 and used.value == v
            wall[v].append(w)
            kernel[v].append(k)
            ran[names[v]] = L.vrc_last_kernel().decode()
    print(json.dumps({"volume": a.volume, "spin": list(a.spin), "samples": frames[0][1],
                      "kernel": ran if walk or store else L.vrc_last_kernel().decode(), "steps": a.steps,
                      "wall_ms_per_frame": {names[1]: wall[1], names[0]: wall[0]},
                      "kernel_ms_mean": {names[1]: kernel[1], names[0]: kernel[0]}, "frames_bit_identical": True}))
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--voxels", type=int, default=1024)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--volume", default="mem")
    ap.add_argument("--spin", type=float, nargs=2, default=(0.0, 0.0))
    ap.add_argument("--spr", type=int, default=0, help="samples per ray (0 = the automatic value)")
    ap.add_argument("--libs", nargs="+", default=None, metavar="NAME=PATH")
    ap.add_argument("--walk-always", action="store_true",
                    help="with --libs: VRC_OPT_WALK_CACHE = 2 in every context (a view that gathers is replayed too)")
    ap.add_argument("--uniform-only", action="store_true",
                    help="with --libs: time every library that knows VRC_OPT_WALK_UNIFORM_ONLY at 0 and at 1 (NAME@0, NAME@1)")
    ap.add_argument("--markers", action="store_true", help="A/B of VRC_OPT_STREAM_MARKERS instead (see above)")
    ap.add_argument("--ray-cache", action="store_true", help="A/B of VRC_OPT_RAY_CACHE instead (see above)")
    ap.add_argument("--walk-cache", action="store_true", help="A/B of VRC_OPT_WALK_CACHE instead (see above)")
    ap.add_argument("--store-through", action="store_true", help="A/B of VRC_OPT_STORE_THROUGH instead (see above)")
    ap.add_argument("--first-visit", action="store_true", help="A/B of VRC_OPT_FIRST_VISIT_TABLE instead (see above)")
    ap.add_argument("--free-march", action="store_true", help="A/B of VRC_OPT_LEAN_FREE_MARCH instead (see above)")
    ap.add_argument("--resolved", action="store_true", help="A/B of VRC_OPT_WALK_RESOLVED instead (see above)")
    a = ap.parse_args()
    if a.resolved and not a.libs:
        return markers(a, vrc.OPT_WALK_RESOLVED, ("lists", "resolved"))
    if a.first_visit:
        return markers(a, vrc.OPT_FIRST_VISIT_TABLE, ("marched", "table"))
    if a.free_march:
        return markers(a, vrc.OPT_LEAN_FREE_MARCH, ("tested", "free"))
    if a.markers:
        return markers(a)
    if a.ray_cache:
        return markers(a, vrc.OPT_RAY_CACHE, ("computed", "cached"))
    if a.walk_cache:
        return markers(a, vrc.OPT_WALK_CACHE, ("walked", "replayed"))
    if a.store_through:
        return markers(a, vrc.OPT_STORE_THROUGH, ("plain", "through"))
    if a.libs:
        return several(a)
    s = orc.build_scene(voxels=(a.voxels,) * 3, block=a.block, viewport=(a.viewport,) * 2, volume=a.volume,
                        spin=tuple(a.spin))
    L = vrc.load_library(a.lib) if a.lib else vrc.load_library()
    g = GpuScene(s, lib=L)
    known = L.vrc_set_option(g.ctx, vrc.OPT_UNIFORM_BRICKS, 0) == 0
    values = (0, 1) if known else (0,)
    frames = {}
    for v in values:
        if known:
            vrc.check(L, L.vrc_set_option(g.ctx, vrc.OPT_UNIFORM_BRICKS, v))
        frames[v] = g.render(count=True)[:2]
    if known:
        assert (frames[0][0] == frames[1][0]).all() and frames[0][1] == frames[1][1], "frames differ"
    ms = {v: [] for v in values}
    stats = vrc.Stats()
    for _ in range(a.rounds):
        for v in values:
            if known:
                vrc.check(L, L.vrc_set_option(g.ctx, vrc.OPT_UNIFORM_BRICKS, v))
            g.render(count=False)  # warm-up: the tile schedule
            best = None
            for _ in range(a.steps):
                _, _, st = g.render(count=False)
                best = st.kernel_ms if best is None else min(best, st.kernel_ms)
            ms[v].append(round(best, 4))
    kernel = L.vrc_last_kernel().decode() if hasattr(L, "vrc_last_kernel") else ""
    print(json.dumps({"volume": a.volume, "spin": list(a.spin), "samples": frames[0][1], "kernel": kernel,
                      "kernel_ms_min_per_round": {("on" if v else "off"): ms[v] for v in values},
                      "frames_bit_identical": bool(known)}))
    g.close()


if __name__ == "__main__":
    main()
