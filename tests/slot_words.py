"""Scenes that pin the three words a brick upload leaves per slot -- the largest stored voxel, the smallest, the
uniformity word (libre_amd/csrc/vrc_kernels.hip: vrc_k_repack_u8x8, _generic, _padded) -- through nothing but the public
contract of include/vrc_hip.h, for tests/test_slot_words_cpu.py (the conditions below, without a GPU) and
tests/test_slot_words.py (the GPU).  NumPy only.

The words decide which bricks a ray never fetches, and the header promises that this changes vrc_stats.samples alone.
So the sample count of a frame IS the read-back of a word, if the scene is built so that one word decides the count:

  Probe A, the maximum (an isosurface frame of ONE brick, point samples).  The brick is noise in a low band with one
    voxel vmax above it, at a place no point sample reads.  iso_value = vmax: no sample hits and the slot can reach the
    threshold, so the ray marches -- the count is |S|, mip_ref's count of the brick.  iso_value = the next representable
    value above vmax: the slot cannot reach it -- the count is 0.  A word above vmax fails the second frame, a word
    below it (or one that missed the voxel) the first, a word of 0 ("nothing known") the second.
  Probe B, the minimum (a MinIP frame of TWO bricks, front then back along every ray).  The front brick holds the one
    value A; a ray holds no M before it, so it is always marched (or folded from its uniformity word).  The back brick
    is noise above A with one voxel vmin.  Per ray the back brick is marched iff the ray took no sample in front or
    vmin < A.  Expected count: the front brick's samples plus the back brick's over the rays that qualify, from
    mip_ref's per-ray counts of the two one-brick scenes.  The mirror under VRC_MIP_FOLD_MAX (noise below A, one voxel
    vmax) is a second witness of the maximum word and of "M >= word - 1".

Counts come from tests/mip_ref.py.  They do not depend on a voxel's value, only on the geometry: one mip_ref render per
geometry, of a MASK brick that is 1 at every place a test puts an extremum and 0 elsewhere, gives the counts and shows
that no sample -- certain or doubtful -- reads such a place (its maximum is 0 on every ray, no doubtful value above it).

A geometry is a volume of one brick (probe A) or of two bricks behind each other along z (probe B), seen along z from
(0, 0, 1.5) as tests/nonfinite.py's layers are; block 16 with an overlap of 4 fills its slot of 24^3 (the whole-slot
kernels), with an overlap of 1 it is 18^3 in 24^3 (the padding kernel), and a volume of 16 x 9 x 5 voxels gives the
ragged border brick 18 x 11 x 7 a bricking data source cuts.  Viewports: nonfinite.LAYERS_KW's 25 x 19 where mip_ref
leaves no sample of it in doubt; GEOMETRIES notes where it did not."""
import ctypes as C

import numpy as np

import mip_ref
import mip_scenes
import orc
from libre_amd import vrc

#: name -> (VRC_VOXEL_*, the dtype a brick is uploaded in)
TYPES = {
    "uint8": (vrc.VOXEL_UINT8, np.uint8), "uint16": (vrc.VOXEL_UINT16, np.uint16), "uint32": (vrc.VOXEL_UINT32, np.uint32),
    "int8": (vrc.VOXEL_INT8, np.int8), "int16": (vrc.VOXEL_INT16, np.int16), "int32": (vrc.VOXEL_INT32, np.int32),
    "float32": (vrc.VOXEL_FLOAT32, np.float32),
}
SPR = 96  # samples per ray, mip_scenes' "count96" and nonfinite's layers

#: name -> (voxels, block, overlap, viewport).  Probe A: one brick; probe B ("two_*"): two bricks along z.
GEOMETRIES = {
    "whole": ((16, 16, 16), 16, 4, (25, 19)),
    "padded": ((16, 16, 16), 16, 1, (25, 19)),
    "ragged": ((16, 9, 5), 16, 1, (25, 19)),
    # one brick of 136^3: the upload's grid-stride tail.  (17 x 15: with 16 x 16 one ray's last sample lies within
    # mip_ref's window of a whole number of steps, and float64 cannot say whether it is taken)
    "big": ((128, 128, 128), 128, 4, (17, 15)),
    # (49 x 37: the volume is half as wide as it is deep and fills a quarter of the frame; 25 x 19 leaves 48 rays that
    # reach the back brick, 51 x 39 has a column that looks along the volume's faces at x = -+1/4)
    "two_whole": ((16, 16, 32), 16, 4, (49, 37)),
    "two_padded": ((16, 16, 32), 16, 1, (49, 37)),
}


def _round8(n):
    return (n + 7) // 8 * 8


class Geometry:
    """vi, ids (front to back), lod, slot_dim, view, render, W, H, planes; shape[nid]: the brick's (z, y, x) shape;
    ref: mip_ref's result of the mask bricks; per_node[nid]: of that brick alone."""


_GEOM = {}


def brick_shape(g, nid):
    node, ov = g.lod[nid], [g.vi.overlap[a] for a in range(3)]
    n = [min(int(node.voxelBoxMax[a]), int(g.vi.voxels[a])) - int(node.voxelBoxMin[a]) + 2 * ov[a] for a in range(3)]
    return (n[2], n[1], n[0])


def positions(shape, eight_bit):
    """Where a test puts a brick's only extremum: {name: (x, y, z)}.  All of them lie in the overlap border."""
    sz, sy, sx = shape
    out = {"first": (0, 0, 0), "last": (sx - 1, sy - 1, sz - 1), "face": (0, sy // 2, sz // 2)}
    if eight_bit:  # the eight byte lanes of one uint2 of vrc_k_repack_u8x8, in the overlap row y = z = 0
        for k in range(8):
            out["lane%d" % k] = (8 + k, 0, 0)
    return out


def mask_brick(shape):
    m = np.zeros(shape, dtype=np.uint8)
    for x, y, z in positions(shape, True).values():
        m[z, y, x] = 1
    return m


def _scene(g, ids, bricks, voxel_type=vrc.VOXEL_UINT8, data_range=(0.0, 255.0), slots=None, atlas_dim=None):
    """A scene of the nodes `ids` (in the order given) of geometry g.  slots / atlas_dim: where a GPU pool put the
    bricks (None: the scene is for mip_ref, which does not read texture coordinates)."""
    L = orc.lib()
    s = orc.Scene()
    s.vi, s.ids, s.sorted_ids, s.lod = g.vi, list(ids), list(ids), g.lod
    s.slot_dim, s.W, s.H, s.view, s.planes = g.slot_dim, g.W, g.H, g.view, g.planes
    s.bricks = dict(bricks)
    s.atlas = np.zeros(1, dtype=next(iter(bricks.values())).dtype)  # (its dtype is all gpu_run.GpuScene reads of it)
    s.voxel_type = voxel_type
    s.nodes = (orc.NodeData * len(ids))()
    for k, nid in enumerate(ids):
        node, nd = g.lod[nid], s.nodes[k]
        tp, ts = orc.f32x3(), orc.f32x3()
        if slots is not None:
            L.orc_texture_object(C.byref(g.vi), C.byref(node), orc.f32x3(*slots[nid]), orc.u32x3(*atlas_dim), tp, ts)
        for a in range(3):
            nd.textureMin[a], nd.textureSize[a] = tp[a], ts[a]
            nd.aabbMin[a] = node.worldBoxMin[a]
            nd.aabbSize[a] = node.worldBoxMax[a] - node.worldBoxMin[a]
    s.n_nodes = len(ids)
    s.render = orc.RenderData(SPR, 1, 32, 0, (C.c_float * 2)(*data_range))
    s.tf = mip_scenes.colour_ramp_tf()
    return s


def geometry(name):
    if name in _GEOM:
        return _GEOM[name]
    voxels, block, overlap, viewport = GEOMETRIES[name]
    L = orc.lib()
    g = Geometry()
    g.name = name
    g.vi = vi = orc.VolumeInfo()
    for a in range(3):
        vi.voxels[a], vi.maximumBlockSize[a], vi.overlap[a] = voxels[a], block + 2 * overlap, overlap
    L.orc_fill_regular_volume_info(C.byref(vi))
    assert vi.depth == 1
    ids = orc.leaf_ids(vi)
    g.lod = {nid: orc.lod_node(vi, nid) for nid in ids}
    g.slot_dim = [_round8(vi.maximumBlockSize[a]) for a in range(3)]
    g.W, g.H = viewport
    g.mv, g.proj = orc.default_mv(), orc.default_proj()
    g.view = orc.ViewData()
    L.orc_make_view_data(g.mv, g.proj, (C.c_uint32 * 4)(0, 0, g.W, g.H), C.byref(vi), C.byref(g.view))
    arr = (C.c_uint64 * len(ids))(*ids)
    L.orc_sort_nodes_front_to_back(C.byref(vi), g.mv, arr, len(ids))
    g.ids = list(arr)
    g.planes = np.zeros((0, 4), dtype=np.float32)
    g.shape = {nid: brick_shape(g, nid) for nid in g.ids}
    masks = {nid: mask_brick(g.shape[nid]) for nid in g.ids}
    g.ref = mip_ref.render(_scene(g, g.ids, masks))
    g.per_node = {nid: mip_ref.render(_scene(g, [nid], masks)) for nid in g.ids} if len(g.ids) > 1 else {g.ids[0]: g.ref}
    _GEOM[name] = g
    return g


_TRILINEAR = {}


def trilinear_ref(name):
    """mip_ref's result of the geometry's mask bricks under the trilinear filter (the same sample positions: the same
    counts; its taps reach half a voxel further), and per brick."""
    if name not in _TRILINEAR:
        g = geometry(name)
        masks = {nid: mask_brick(g.shape[nid]) for nid in g.ids}
        _TRILINEAR[name] = (mip_ref.render(_scene(g, g.ids, masks), filter_mode=1),
                            {nid: mip_ref.render(_scene(g, [nid], masks), filter_mode=1) for nid in g.ids})
    return _TRILINEAR[name]


def pool_bytes(g, want):
    """Voxels of the smallest pool whose slot grid holds `want` bricks (as orc.build_scene sizes one)."""
    slot = g.slot_dim[0] * g.slot_dim[1] * g.slot_dim[2]
    slots, blocks = orc.u32x3(), want
    while True:
        orc.lib().orc_pool_slots(orc.u32x3(*g.slot_dim), slot, blocks * slot, orc.u32x3(4096, 4096, 4096), slots)
        if slots[0] * slots[1] * slots[2] >= want:
            return blocks * slot
        blocks += 1


def data_range(tname):
    """The type's own range for the integers (in float32, as vrc_render_data carries it), (-1, 1) for floats."""
    lim = _limits(tname)
    return (-1.0, 1.0) if lim is None else (float(np.float32(lim[0])), float(np.float32(lim[1])))


def gpu_scene(g, ids, bricks, tname, slots, atlas_dim):
    return _scene(g, ids, bricks, TYPES[tname][0], data_range(tname), slots, atlas_dim)


def upload_kernel(elem_bytes, size, slot_dim, aligned=True):
    """The repack kernel an upload takes (vrc_launch_repack_brick's dispatch, restated): size (x, y, z) against the
    pool's slot, the voxel's bytes, and whether the source is aligned to eight bytes."""
    if list(size) != list(slot_dim):
        return "padded"
    if elem_bytes == 1 and size[0] % 8 == 0 and aligned:
        return "u8x8"
    return "generic"


# ---- the numbers a word is tested with ---------------------------------------------------------------------------------
def stored_float(tname, v):
    """The value the library holds and reports for a voxel v of the type: itself, or -- 32-bit integers -- the float32
    NumPy converts it to (round to nearest even: 2^32 - 1 becomes 2^32)."""
    dt = TYPES[tname][1]
    return np.float32(np.array(v, dtype=dt)) if np.dtype(dt).itemsize == 4 else np.array(v, dtype=dt)


def next_above(tname, v):
    """The smallest isovalue above every voxel equal to v: v + 1 for the 8- and 16-bit types, the next float32 after the
    stored float for the others."""
    if np.dtype(TYPES[tname][1]).itemsize == 4:
        return float(np.nextafter(stored_float(tname, v), np.float32(np.inf)))
    return float(int(v) + 1)


def iso_of(tname, v):
    return float(stored_float(tname, v))


def _limits(tname):
    dt = np.dtype(TYPES[tname][1])
    if dt.kind == "f":
        return None
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def noise(tname, shape, lo, hi, seed):
    """Voxels in [lo, hi] (integers: inclusive, every value exact in float32 for the bands used here)."""
    dt = TYPES[tname][1]
    rng = np.random.default_rng(seed)
    if np.dtype(dt).kind == "f":
        return (lo + (hi - lo) * rng.random(shape)).astype(np.float32)
    return rng.integers(lo, hi, shape, dtype=np.int64, endpoint=True).astype(dt)


def with_voxel(brick, pos, v):
    out = brick.copy()
    x, y, z = pos
    out[z, y, x] = v
    return out


#: the maxima probe A plants, per type: at and next to the type's limit, and just above the noise
def maxima(tname):
    lim = _limits(tname)
    if lim is None:
        return [0.75, -0.25]  # (noise in [-0.9, -0.6])
    lo, hi = lim
    out = [hi, hi - 1, lo + (41 if hi < 2 ** 16 else 4096)]  # (int32: float32 is 128 apart at -2^31)
    if tname == "uint32":
        out += [16777217, 3000000001]  # neither is a float32: they are stored as 16777216 and 3000000000
    if tname == "int32":
        out += [-5, 16777217]
    return out


def max_noise(tname, shape, seed=3):
    """The low band under every maximum of maxima(tname)."""
    lim = _limits(tname)
    if lim is None:
        return noise(tname, shape, -0.9, -0.6, seed)
    return noise(tname, shape, lim[0], lim[0] + 40, seed)


def min_noise(tname, shape, seed=5):
    lim = _limits(tname)
    if lim is None:
        return noise(tname, shape, 0.6, 0.9, seed)
    return noise(tname, shape, lim[1] - 40, lim[1], seed)


#: 32-bit integers are held as the float32 NumPy converts them to: neighbours there are 128 or 256 apart at the type's
#: limits and 2 apart above 2^24, so "the next value" is chosen among the floats
FOLD_CASES_32 = {
    ("uint32", vrc.MIP_FOLD_MAX): [(2 ** 32 - 256, 2 ** 32 - 1, True), (2 ** 32 - 1, 2 ** 32 - 1, False),
                                   (2 ** 32 - 1, 2 ** 32 - 96, False),  # both round up to 2^32
                                   (16777216, 16777217, False), (16777216, 16777218, True)],
    ("uint32", vrc.MIP_FOLD_MIN): [(1, 0, True), (0, 0, False), (16777218, 16777217, True), (16777216, 16777217, False)],
    ("int32", vrc.MIP_FOLD_MAX): [(2 ** 31 - 128, 2 ** 31 - 1, True), (2 ** 31 - 1, 2 ** 31 - 1, False), (-5, -4, True),
                                  (-5, -5, False)],
    ("int32", vrc.MIP_FOLD_MIN): [(-2 ** 31 + 128, -2 ** 31, True), (-2 ** 31, -2 ** 31, False),
                                  (-16777216, -16777217, False), (-16777216, -16777218, True)],
}


def fold_cases(tname, fold):
    """Probe B: [(A, extremum of the back brick, marched?)] -- A - 1 (A + 1 under the maximum fold) is marched, A is
    skipped; at the type's limit and in the middle of its range."""
    if (tname, fold) in FOLD_CASES_32:
        return FOLD_CASES_32[tname, fold]
    lim = _limits(tname)
    if lim is None:
        a = np.float32(0.25)
        beyond = np.nextafter(a, np.float32(-np.inf if fold == vrc.MIP_FOLD_MIN else np.inf))
        return [(a, beyond, True), (a, a, False)]
    lo, hi = lim
    mid = (lo + hi) // 2
    if fold == vrc.MIP_FOLD_MIN:
        return [(lo + 1, lo, True), (lo, lo, False), (mid, mid - 1, True), (mid, mid, False)]
    return [(hi - 1, hi, True), (hi, hi, False), (mid, mid + 1, True), (mid, mid, False)]


def back_noise(tname, shape, fold):
    return min_noise(tname, shape) if fold == vrc.MIP_FOLD_MIN else max_noise(tname, shape)


def expected_two(g, marched):
    """Probe B's count: the front brick's samples, and the back brick's on the rays that march it."""
    front, back = g.ids
    cf, cb = g.per_node[front].counts, g.per_node[back].counts
    return int(cf.sum()) + int(cb[(cf == 0) | bool(marched)].sum())


# ---- float edges (FLOAT32 pool; probe A and the maximum-fold mirror of probe B) ----------------------------------------
FLT_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-45)  # the smallest positive float32
NAN = np.float32(np.nan)


def _up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def _down(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def float_edges_a(shape, pos):
    """name -> (brick, [(iso_value, marched?)]).  Marched: the count is |S|; not: 0."""
    neg = noise("float32", shape, -0.9, -0.6, 7)
    ninf = np.full(shape, -np.inf, dtype=np.float32)
    nan = np.full(shape, np.nan, dtype=np.float32)
    nan.view(np.uint32)[::2] = 0xFFC00001  # NaNs of both signs
    out = {
        "negative": (with_voxel(neg, pos, -0.5), [(-0.5, True), (float(_up(-0.5)), False)]),
        # -0.0 and +0.0 are one value: the contract compares ">= in float32", so a slot whose maximum is either zero
        # reaches an isovalue of either zero, although the word (a key ordered as the bit patterns are) tells them apart
        "minus_zero": (with_voxel(neg, pos, -0.0), [(0.0, True), (-0.0, True), (float(DENORMAL), False)]),
        "plus_zero": (with_voxel(neg, pos, 0.0), [(-0.0, True), (0.0, True), (float(DENORMAL), False)]),
        "denormal": (with_voxel(neg, pos, DENORMAL), [(float(DENORMAL), True), (float(_up(DENORMAL)), False)]),
        "flt_max": (with_voxel(neg, pos, FLT_MAX), [(float(FLT_MAX), True), (float("inf"), False)]),
        "minus_flt_max": (with_voxel(ninf, pos, -FLT_MAX), [(float(-FLT_MAX), True), (float(_up(-FLT_MAX)), False)]),
        "nan_but_one": (with_voxel(nan, pos, 0.3), [(float(np.float32(0.3)), True), (float(_up(0.3)), False)]),
        # nothing but NaN: the word is -infinity's, and any finite isovalue lies above it
        "all_nan": (nan, [(-3.0e38, False), (0.0, False), (3.0e38, False)]),
    }
    return out


def float_edges_b(shape, pos):
    """name -> (A of the uniform front brick, back brick, marched?) under VRC_MIP_FOLD_MAX: the back brick is marched
    iff its largest voxel that is not NaN exceeds A, compared as numbers."""
    neg = noise("float32", shape, -0.9, -0.6, 9)
    ninf = np.full(shape, -np.inf, dtype=np.float32)
    nan = np.full(shape, np.nan, dtype=np.float32)
    nan.view(np.uint32)[1::2] = 0xFFC00001
    return {
        "negative_above": (np.float32(-0.5), with_voxel(neg, pos, _up(-0.5)), True),
        "negative_equal": (np.float32(-0.5), with_voxel(neg, pos, -0.5), False),
        "plus_zero_over_minus_zero": (np.float32(-0.0), with_voxel(neg, pos, 0.0), False),  # equal as numbers
        "minus_zero_over_plus_zero": (np.float32(0.0), with_voxel(neg, pos, -0.0), False),
        "denormal_above_zero": (np.float32(0.0), with_voxel(neg, pos, DENORMAL), True),
        "denormal_equal": (DENORMAL, with_voxel(neg, pos, DENORMAL), False),
        "flt_max_above": (_down(FLT_MAX), with_voxel(neg, pos, FLT_MAX), True),
        "flt_max_equal": (FLT_MAX, with_voxel(neg, pos, FLT_MAX), False),
        "minus_flt_max_above": (np.float32(-np.inf), with_voxel(ninf, pos, -FLT_MAX), True),
        "minus_flt_max_equal": (-FLT_MAX, with_voxel(ninf, pos, -FLT_MAX), False),
        "nan_but_one_above": (np.float32(0.25), with_voxel(nan, pos, _up(0.25)), True),
        "nan_but_one_equal": (np.float32(0.25), with_voxel(nan, pos, 0.25), False),
        "all_nan": (np.float32(-3.0e38), nan, False),
    }


# ---- the words as NumPy computes them (tests/test_slot_words_cpu.py holds the host build of vrc_core.h to these) --------
def max_key(v):
    """vrc_slot_max_key: the float32's bits with the sign bit set (positive) or all bits flipped (negative)."""
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000).astype(np.uint32)
