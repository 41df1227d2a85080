"""Tile culling of the reference-order kernels (libre_amd/csrc/vrc_core.h, "tile culling"): the host build of the
culling loop (tests/cpu_harness/cull_harness.cpp), an independent float64 statement of "some ray of this tile hits this
brick", and the scene helpers of tests/test_tile_cull_cpu.py and tests/test_tile_cull.py.  TEST INFRASTRUCTURE.

The thresholds of the culling's regimes are read from the host build (limits()); no test repeats them."""
import collections
import copy
import ctypes as C
import os
import subprocess

import numpy as np

import orc
import ref64

HARNESS_DIR = orc.HARNESS_DIR
SRC = os.path.join(HARNESS_DIR, "cull_harness.cpp")
SHORT, CULLED, OVERFLOW, LONG = 0, 1, 2, 3  # CULL_REGIME_* of the host build
HIT, STOP = 1, 2                            # bits of needed() and needed64()

Limits = collections.namedtuple("Limits", "candidates lower upper tile_w tile_h")


def build(flavour=""):
    """libcull_harness.so by g++ without contraction, or ("fma") by clang with -mfma and the pragmas of vrc_core.h honoured:
    the GPU build's floating-point mode on the host (tests/orc.py: build_harness)."""
    out = os.path.join(HARNESS_DIR, "libcull_harness%s.so" % ("_" + flavour if flavour else ""))
    deps = [SRC] + [os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
    if flavour == "fma":
        cmd = ["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma",
               "-ffp-contract=fast-honor-pragmas", "-Wno-unknown-pragmas", "-o", tmp, SRC]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", tmp, SRC]
    subprocess.check_call(cmd)
    os.replace(tmp, out)
    return out


_LIBS = {}
_SCENE_ARGS = [orc.u32x3, orc.u32x3, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(orc.ViewData), C.c_uint32,
               C.POINTER(orc.NodeData), C.POINTER(orc.RenderData), C.c_void_p, C.c_int, C.c_int, C.c_int]


def lib(flavour=""):
    if flavour not in _LIBS:
        L = C.CDLL(build(flavour))
        L.cull_limits.restype = None
        L.cull_limits.argtypes = [C.c_uint32 * 5]
        L.cull_tile_masks.restype = C.c_int
        L.cull_tile_masks.argtypes = _SCENE_ARGS + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cull_needed.restype = C.c_int
        L.cull_needed.argtypes = _SCENE_ARGS + [C.c_void_p, C.c_uint32, C.c_void_p]
        L.cull_render.restype = C.c_int
        L.cull_render.argtypes = ([C.c_void_p, C.c_uint32, orc.u32x3, orc.u32x3, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                   C.c_uint32, C.c_void_p] + _SCENE_ARGS[6:] +
                                  [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint64), C.c_void_p])
        _LIBS[flavour] = L
    return _LIBS[flavour]


def limits(flavour=""):
    out = (C.c_uint32 * 5)()
    lib(flavour).cull_limits(out)
    return Limits(*[int(v) for v in out])


def tiles_of(s, row_map=None):
    """(tilesX, tilesY) of the buffer the scene renders into (a row map: as many rows as it has entries)."""
    lim = limits()
    h = len(row_map) if row_map is not None else s.H
    return (s.W + lim.tile_w - 1) // lim.tile_w, (h + lim.tile_h - 1) // lim.tile_h


def _rows(row_map):
    return None if row_map is None else np.ascontiguousarray(row_map, dtype=np.uint32)


def _scene_args(s, rows, variant, pixel_off):
    h = len(rows) if rows is not None else s.H
    return [orc.u32x3(*s.atlas_dim), orc.u32x3(*s.slot_dim), s.W, h, s.planes.ctypes.data if len(s.planes) else None,
            len(s.planes), C.byref(s.view), s.n_nodes, s.nodes, C.byref(s.render), rows.ctypes.data if rows is not None else None,
            variant, pixel_off[0], pixel_off[1]]


def _tile_arg(s, rows, tiles):
    tx, ty = tiles_of(s, rows)
    if tiles is None:
        return None, tx * ty, None
    t = np.ascontiguousarray(tiles, dtype=np.uint32)
    return t, len(t), t.ctypes.data


def tile_masks(s, row_map=None, variant=0, pixel_off=(0, 0), tiles=None, flavour=""):
    """(kept[nTiles, n_nodes] bool, counts[nTiles], regimes[nTiles]) of the wave's culling loop, per tile (all of them in
    row-major order, or the tile indices `tiles`)."""
    rows = _rows(row_map)
    t, n, tp = _tile_arg(s, rows, tiles)
    kept = np.zeros((n, s.n_nodes), dtype=np.uint8)
    counts = np.zeros(n, dtype=np.uint32)
    regimes = np.zeros(n, dtype=np.int32)
    rc = lib(flavour).cull_tile_masks(*_scene_args(s, rows, variant, pixel_off), tp, n, kept.ctypes.data, counts.ctypes.data,
                                      regimes.ctypes.data)
    assert rc == 0, rc
    assert (kept.sum(axis=1) == counts).all()
    return kept.astype(bool), counts, regimes


def needed(s, row_map=None, variant=0, pixel_off=(0, 0), tiles=None, flavour=""):
    """needed[nTiles, n_nodes] uint8 of the kernel's own per-ray test (vrc_brick_segment, float32): HIT where some in-frame
    pixel's ray marches the brick, STOP where some ray's loop ends at it."""
    rows = _rows(row_map)
    t, n, tp = _tile_arg(s, rows, tiles)
    out = np.zeros((n, s.n_nodes), dtype=np.uint8)
    rc = lib(flavour).cull_needed(*_scene_args(s, rows, variant, pixel_off), tp, n, out.ctypes.data)
    assert rc == 0, rc
    return out


#: cull_render's modes: the forms of vrc_pixel_reference_order the host build instantiates
MODES = {"table": 0, "point": 1, "trilinear": 2, "shade": 3, "shade_trilinear": 4}


def render(s, mode="table", culled=True, row_map=None, variant=0, pixel_off=(0, 0), tiles=None, fb=None, ambient=0.25,
           flavour=""):
    """(frame, samples, regimes[nTiles]) of vrc_pixel_reference_order run tile by tile: with the candidates the culling
    gives, by the kernels' four-regime rule, or (culled=False) with candidates = nullptr in every tile."""
    rows = _rows(row_map)
    h = len(rows) if rows is not None else s.H
    if fb is None:
        fb = np.zeros((h, s.W, 4), dtype=np.float32)
    t, n, tp = _tile_arg(s, rows, tiles)
    regimes = np.zeros(n, dtype=np.int32)
    samples = C.c_uint64(0)
    a = _scene_args(s, rows, variant, pixel_off)
    rc = lib(flavour).cull_render(s.atlas.ctypes.data, s.atlas.dtype.itemsize, a[0], a[1], fb.ctypes.data, s.W, h, a[4], a[5],
                                  s.tf.ctypes.data, *a[6:], tp, n, MODES[mode], ambient, 1 if culled else 0, C.byref(samples),
                                  regimes.ctypes.data)
    assert rc == 0, rc
    return fb, int(samples.value), regimes


def pyramid_keeps(s, corners, boxes, variant=0, flavour=""):
    """vrc_pyramid_may_hit of the pyramid through the window positions corners = (x0, y0, x1, y1) of the scene's view, for
    boxes[n, 6] (min, size): bool[n]."""
    L = lib(flavour)
    L.cull_pyramid_keeps.restype = C.c_int
    L.cull_pyramid_keeps.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(orc.ViewData), C.POINTER(orc.RenderData), C.c_int] + \
        [C.c_float] * 4 + [C.c_void_p, C.c_uint32, C.c_void_p]
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(len(b), dtype=np.uint8)
    rc = L.cull_pyramid_keeps(s.W, s.H, C.byref(s.view), C.byref(s.render), variant, *[float(v) for v in corners], b.ctypes.data,
                              len(b), out.ctypes.data)
    assert rc == 0, rc
    return out.astype(bool)


def direction64(s, wx, wy):
    """The float64 direction (not normalised) from the eye through the window position (wx, wy): cuda/Renderer.cu:106-122."""
    view = s.view
    vp = [float(view.glViewport[i]) for i in range(4)]
    ndc = np.array([2.0 * (wx - vp[0] - vp[2] / 2.0) / vp[2], 2.0 * (wy - vp[1] - vp[3] / 2.0) / vp[3], 1.0, 1.0])
    eye4 = ref64._mat(view.invProjMatrix) @ ndc
    world = ref64._mat(view.invViewMatrix) @ (eye4 / eye4[3])
    return world[:3] - ref64._vec(view.eyePosition, 3)


# ---- the independent statement -------------------------------------------------------------------------------------------
def needed64(s, row_map=None, variant=0, pixel_off=(0, 0), tiles=None):
    """needed[nTiles, n_nodes] uint8 in float64 NumPy, from tests/ref64.py's reading of the ray set-up (cuda/Renderer.cu:40-51,
    :106-149) and of the node loop's slab test (:179-193): HIT where some in-frame pixel of the tile has a ray whose
    interval in the brick -- inside the global box, the clip planes and the near plane -- is longer than ref64.EXACT_TIE
    relative; STOP where a ray hits a brick that starts beyond the far end of its interval (:183-184).  Exact grazes are
    left to the float32 statement (needed()).

    variant 1 (glRaycaster): the ray through the pixel centre, the hit test of the same interval (the lattice snap of the
    first sample and samplesPerPixel are not restated: they only take samples away from a brick the ray crosses, and the
    sub-sample 0 is the centre ray)."""
    lim = limits()
    rows = np.arange(s.H) if row_map is None else np.asarray(row_map, dtype=np.int64)
    tx_n, ty_n = tiles_of(s, row_map)
    tiles = np.arange(tx_n * ty_n) if tiles is None else np.asarray(tiles, dtype=np.int64)
    view = s.view
    ly, lx = np.meshgrid(np.arange(lim.tile_h), np.arange(lim.tile_w), indexing="ij")
    px = (tiles % tx_n)[:, None] * lim.tile_w + lx.reshape(1, -1)   # [nTiles, 64] buffer columns
    py = (tiles // tx_n)[:, None] * lim.tile_h + ly.reshape(1, -1)  # buffer rows
    inside = (px < s.W) & (py < len(rows))
    centre = 0.5 if variant == 1 else 0.0
    wx = px.astype(np.float64) + pixel_off[0] + centre
    wy = rows[np.minimum(py, len(rows) - 1)].astype(np.float64) + pixel_off[1] + centre
    shape = wx.shape
    wx, wy = wx.reshape(-1), wy.reshape(-1)
    vp = [float(view.glViewport[i]) for i in range(4)]
    n = wx.size
    ndc = np.stack([2.0 * (wx - vp[0] - vp[2] / 2.0) / vp[2], 2.0 * (wy - vp[1] - vp[3] / 2.0) / vp[3], np.ones(n), np.ones(n)],
                   axis=1)
    eye4 = ndc @ ref64._mat(view.invProjMatrix).T
    eye4 = eye4 / eye4[:, 3:4]
    world = eye4 @ ref64._mat(view.invViewMatrix).T
    origin = ref64._vec(view.eyePosition, 3)
    d = world[:, :3] - origin
    d = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    d[d == 0.0] = ref64.EPSILON
    e3 = eye4[:, :3]
    t_near_plane = -float(view.nearPlane) / (e3[:, 2] / np.sqrt((e3 * e3).sum(axis=1)))
    tn_g, tf_g = ref64._slab(origin, d, ref64._vec(view.aabbMin, 3), ref64._vec(view.aabbMax, 3))
    alive = inside.reshape(-1) & (tf_g - tn_g > ref64.EXACT_TIE * np.maximum(1.0, np.abs(tn_g)))
    for plane in np.asarray(s.planes, dtype=np.float64).reshape(-1, 4):
        normal, dd = plane[:3], plane[3]
        rn = d @ normal
        rn = np.where(rn == 0.0, ref64.EPSILON, rn)
        t = -(normal @ origin + dd) / rn
        tn_g = np.where(rn > 0.0, np.maximum(tn_g, t), tn_g)
        tf_g = np.where(rn > 0.0, tf_g, np.minimum(tf_g, t))
    alive &= ~(tn_g > tf_g)

    out = np.zeros((len(tiles), s.n_nodes), dtype=np.uint8)
    lo_all = np.array([[float(s.nodes[i].aabbMin[a]) for a in range(3)] for i in range(s.n_nodes)]).reshape(-1, 3)
    size_all = np.array([[float(s.nodes[i].aabbSize[a]) for a in range(3)] for i in range(s.n_nodes)]).reshape(-1, 3)
    inv = 1.0 / d
    chunk = max(1, (1 << 21) // max(1, n))
    for c0 in range(0, s.n_nodes, chunk):
        lo = lo_all[c0:c0 + chunk, None, :]
        hi = lo + size_all[c0:c0 + chunk, None, :]
        t0, t1 = inv[None] * (lo - origin), inv[None] * (hi - origin)
        tn, tf = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)   # [chunk, rays]
        hit = alive[None] & (tf - tn > ref64.EXACT_TIE * np.maximum(1.0, np.abs(tn)))
        if variant == 1:
            stop = np.zeros_like(hit)
        else:
            stop = hit & (tn > tf_g[None])
            hit &= ~stop & ~(tf < tn_g[None])
        tn2 = np.maximum(np.maximum(t_near_plane[None], tn), tn_g[None])
        tf2 = np.minimum(tf, tf_g[None])
        hit &= tf2 - tn2 > ref64.EXACT_TIE * np.maximum(1.0, np.abs(tn2))
        k = hit.shape[0]
        bits = (hit.reshape(k, *shape).any(axis=-1) * HIT) | (stop.reshape(k, *shape).any(axis=-1) * STOP)
        out[:, c0:c0 + k] = bits.T
    return out


# ---- scene helpers ---------------------------------------------------------------------------------------------------------
def with_nodes(s, nodes):
    """The same scene (atlas, bricks, view, settings) over another node list (a sequence of orc.NodeData)."""
    t = copy.copy(s)
    t.n_nodes = len(nodes)
    t.nodes = (orc.NodeData * max(1, len(nodes)))()
    for k, nd in enumerate(nodes):
        C.memmove(C.byref(t.nodes, k * C.sizeof(orc.NodeData)), C.byref(nd), C.sizeof(orc.NodeData))
    return t


def first(s, n):
    """The scene over the first n entries of its list."""
    assert n <= s.n_nodes
    t = copy.copy(s)
    t.n_nodes = n
    t.nodes = (orc.NodeData * n)()
    C.memmove(t.nodes, s.nodes, n * C.sizeof(orc.NodeData))
    return t


def never_hit_entry(s):
    """A copy of the scene's first node moved far behind the eye: 2000 world units along the camera's backward axis (the
    unit volume spans one), outside the view frustum of every tile and outside the global box.  It keeps its slot, so a
    kernel that did march it would read valid voxels."""
    back = ref64._mat(s.view.invViewMatrix)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    back /= np.linalg.norm(back)
    eye = ref64._vec(s.view.eyePosition, 3)
    nd = orc.NodeData()
    C.memmove(C.byref(nd), C.byref(s.nodes, 0), C.sizeof(orc.NodeData))
    for a in range(3):
        nd.aabbMin[a] = float(eye[a] + 2000.0 * back[a] - 0.5 * float(nd.aabbSize[a]))
    return nd


def padded(s, total, where="end"):
    """The scene with never-hit entries (never_hit_entry) added until the list has `total` entries.  "end": behind the
    scene's own entries, which leaves the reference's loop over them unchanged statement for statement.  "interleaved":
    the scene's entries keep their order and are spread evenly over the list, the last one at index total - 1.
    The scene gets `real`: the indices of its own entries in the new list."""
    n = s.n_nodes
    assert total >= n and where in ("end", "interleaved")
    pad = never_hit_entry(s)
    size = C.sizeof(orc.NodeData)
    t = copy.copy(s)
    t.n_nodes = total
    t.nodes = (orc.NodeData * total)()
    one = np.frombuffer(bytes(pad), dtype=np.uint8)
    buf = np.frombuffer(t.nodes, dtype=np.uint8).reshape(total, size)
    buf[:] = one
    real = np.arange(n) if where == "end" else np.round(np.linspace(total - 1 - (n - 1) * ((total - 1) // max(1, n)), total - 1, n)).astype(np.int64)
    assert len(set(real.tolist())) == n and (np.diff(real) > 0).all() and real[-1] <= total - 1
    buf[real] = np.frombuffer(s.nodes, dtype=np.uint8)[:n * size].reshape(n, size)
    t.real = real
    return t


def passes_of(s, k=None):
    """The list cut into consecutive passes [(a, b)] of at most k entries (default: the lower bound of the culled regime,
    so that no pass is culled)."""
    if k is None:
        k = limits().lower
    return [(a, min(a + k, s.n_nodes)) for a in range(0, s.n_nodes, k)]


# ---- the scenes both test modules use ----------------------------------------------------------------------------------
ROW_MAP = [3, 4, 5, 17, 18, 30, 35]
BANDS = [(3, 5), (50, 13), (21, 7), (64, 8)]  # tests/test_gpu_host.py: row bands whose heights are no multiples of the tile's
CLIP_PLANES = [[-1, 0, 0, 0.2], [0.6, 0, 0.8, 0.35]]  # tests/mip_scenes.py

_SCENES = {}


def scene(name, dtype="u8"):
    """The scenes of the GPU matrix, built once (callers leave them unchanged)."""
    key = (name, dtype)
    if key in _SCENES:
        return _SCENES[key]
    hash64 = dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), volume="hash", spr=96, alpha=0.8, dtype=dtype)
    if name == "hash64":        # 64 bricks, partial tiles
        s = orc.build_scene(spin=(0.5, 0.35), **hash64)
    elif name == "hash64_clip":
        s = orc.build_scene(spin=(0.5, 0.35), planes=CLIP_PLANES, **hash64)
    elif name == "hash64_inside":
        s = orc.build_scene(eye=(0.1, 0.05, 0.2), **hash64)
    elif name == "dense8":      # 4096 bricks of 8^3 behind ONE tile: every brick survives the culling
        s = orc.build_scene(voxels=(128, 128, 128), block=8, viewport=(8, 8), volume="hash", spr=64, alpha=0.3, dtype=dtype)
    elif name == "dense8_wide":  # the same list behind 3 x 2 tiles, some of which keep more than the wave's array holds
        s = orc.with_viewport(scene("dense8", dtype), 24, 16)
    else:
        raise KeyError(name)
    _SCENES[key] = s
    return s
