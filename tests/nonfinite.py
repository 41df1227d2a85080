"""Float volumes with voxels that are not numbers, for tests/test_nonfinite_cpu.py and tests/test_nonfinite.py.

include/vrc_hip.h says what such voxels do: a NaN density classifies as the first texel of the transfer function,
+infinity as the last and -infinity as the first; a MIP ray drops its NaN samples (M = -infinity when all are NaN, which
is a hit pixel of texel 0, not the cleared value); the upload leaves per slot the largest voxel that is not NaN, and the
MIP march skips bricks by it without changing a bit of the frame.

No new reference and no new tolerance.  The scenes are uint16 volumes q under voxel_types.IMAGES["float_narrow"]
(v = -1 + q / 32768, dataSourceRange (-0.5, 0.75): q <= 16384 is v <= r0, q >= 57344 is v >= r1) with three values of q
reserved as MARKERS, which the base volumes are remapped to be free of:

    Q_NAN = 1      -> NaN (both signs, quiet and signalling payloads)
    Q_NINF = 2     -> -infinity
    Q_PINF = 65534 -> +infinity

The q scene ITSELF, markers left as the ordinary numbers they are, is what tests/ref64.py and tests/mip_ref.py render:
  * composite, point samples: NaN, -infinity and every density <= r0 classify as texel 0, +infinity and every density
    >= r1 as texel 255, and the markers lie outside [r0, r1] on the right sides;
  * MIP, point samples: a NaN sample drops out where the reference takes v(1); either way the pixel is texel 0 when no
    sample exceeds r0 and the maximum is unchanged otherwise.  +infinity gives texel 255, as v(65534) does;
  * trilinear (scenes with NaN only): every voxel within Chebyshev distance 2 of a NaN voxel holds some q <= 16384, so a
    sample with a NaN tap (NaN density: texel 0) has in the reference a density <= r0 (texel 0), also where float32 and
    float64 put it on different sides of a cell boundary.  Infinite taps are unspecified under the trilinear filter
    (inf * 0, inf - inf) and appear in no trilinear scene.

The "layers" scenes (the per-slot word) are built as float volumes directly; mip_ref gets their finite twin."""
import copy
import ctypes as C

import numpy as np

import mip_ref
import mip_scenes
import orc
import ref64
import voxel_types as vt
from libre_amd import vrc

Q_NAN, Q_NINF, Q_PINF = 1, 2, 65534
IMAGE = vt.IMAGES["float_narrow"]
Q_R0, Q_R1 = 16384, 57344
#: NaN patterns: quiet of both signs, signalling of both signs, all ones
NAN_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA00001, 0x7FFFFFFF], dtype=np.uint32)
NINF_BITS, PINF_BITS = np.uint32(0xFF800000), np.uint32(0x7F800000)


def _hash16(vx, vy, vz):
    """orc.build_scene's 16-bit hash volume, free of the markers (and of 0, so that a MIP maximum of Q_NAN means that
    every sample was one)."""
    vol = orc.hash_volume(vx, vy, vz)
    vol = vol.astype(np.uint16) * np.uint16(257) ^ (vol.astype(np.uint16) >> np.uint16(3))
    return _remap(vol)


def _remap(vol):
    vol = vol.copy()
    vol[vol <= 2] = 3
    vol[vol >= 65534] = 65533
    return vol


def _place(vol, placed):
    """Write the markers; placed: {marker: mask}.  The masks are kept with the volume for the tests."""
    for mark, mask in placed.items():
        assert not np.isin(vol, [Q_NAN, Q_NINF, Q_PINF])[mask].any(), "two markers on one voxel"
        vol[mask] = mark
    return vol


def _cube(shape, centre, half):
    """Mask of the (2 half + 1)^3 cube around centre = (x, y, z), clipped to the volume (z, y, x)."""
    m = np.zeros(shape, dtype=bool)
    x, y, z = centre
    m[max(0, z - half):z + half + 1, max(0, y - half):y + half + 1, max(0, x - half):x + half + 1] = True
    return m


def dilate(mask, r):
    """Every voxel within Chebyshev distance r of a voxel of the mask (no wrap-around)."""
    out = mask.copy()
    for ax in range(3):
        acc = out.copy()
        for k in range(1, r + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(k, None), slice(None, -k)
            acc[tuple(lo)] |= out[tuple(hi)]
            acc[tuple(hi)] |= out[tuple(lo)]
        out = acc
    return out


# ---- the volumes: (q volume (z, y, x), {marker: mask}, orc.build_scene keywords) ---------------------------------------
def _speckle():
    vol = _hash16(64, 64, 64)
    nan = (vol % 5) == 1  # a value class: about one voxel in seven
    pinf = np.zeros(vol.shape, dtype=bool)
    ninf = np.zeros(vol.shape, dtype=bool)
    # 2^3 clusters: inside a brick, across brick faces (overlap borders), at volume corners
    for x, y, z in ((20, 40, 50), (15, 31, 47), (62, 62, 62), (40, 8, 30)):
        pinf[z:z + 2, y:y + 2, x:x + 2] = True
    for x, y, z in ((44, 20, 52), (31, 15, 16), (0, 0, 0), (10, 50, 40)):
        ninf[z:z + 2, y:y + 2, x:x + 2] = True
    nan &= ~(pinf | ninf)
    return vol, {Q_NAN: nan, Q_PINF: pinf, Q_NINF: ninf}, dict(viewport=(40, 48), spin=(0.5, 0.35))


#: NaN cores of the "cores" volume: (centre (x, y, z), half): single voxels, 3^3 and 5^3 cubes -- inside bricks, across
#: the brick faces at 16 and 32 along every axis (so NaNs lie in overlap borders), at the volume's corners
CORES = [((8, 40, 24), 0), ((16, 8, 50), 0), ((40, 32, 16), 0), ((0, 0, 0), 0),
         ((16, 24, 40), 1), ((24, 16, 32), 1), ((50, 32, 16), 1), ((63, 63, 63), 1), ((32, 50, 52), 1),
         ((32, 16, 32), 2), ((50, 50, 40), 2), ((16, 48, 8), 2), ((1, 62, 62), 2)]


def _cores():
    vol = _remap(vt.smooth16())
    nan = np.zeros(vol.shape, dtype=bool)
    for centre, half in CORES:
        nan |= _cube(vol.shape, centre, half)
    shell = dilate(nan, 2) & ~nan
    z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
    low = (4000 + (x * 131 + y * 71 + z * 37) % 12000).astype(np.uint16)  # <= 16000 < r0 in q, varied
    vol[shell] = low[shell]
    return vol, {Q_NAN: nan}, dict(viewport=(40, 40), spin=(0.7, 0.4))


#: the brick of "allnan_brick": (1, 1, 3) of the 4^3 bricks, in the layer nearest the eye; with its overlap of 4 voxels
#: it spans [12, 36) x [12, 36) x [44, 68) and the NaN region two voxels more on every side
ALLNAN = (1, 1, 3)


def _allnan_brick():
    vol = _hash16(64, 64, 64)
    nan = np.zeros(vol.shape, dtype=bool)
    lo = [16 * b - 6 for b in ALLNAN]
    nan[max(0, lo[2]):lo[2] + 28, max(0, lo[1]):lo[1] + 28, max(0, lo[0]):lo[0] + 28] = True
    # the clip plane keeps z >= 0.26 (world): the front layer of bricks and nothing behind it, so the rays through the
    # NaN brick sample nothing else up to the plane
    return vol, {Q_NAN: nan}, dict(viewport=(44, 36), spin=(0.2, 0.1), planes=[[0.0, 0.0, 1.0, -0.26]])


def _ragged():
    vol = _hash16(48, 40, 56)  # (56, 40, 48): bricks reach past the volume on every axis and repeat its border plane
    z, y, x = np.meshgrid(np.arange(56), np.arange(40), np.arange(48), indexing="ij")
    outer = (x == 0) | (x == 47) | (y == 0) | (y == 39) | (z == 0) | (z == 55)
    nan = outer & ((x + y + z) % 3 != 1)
    return vol, {Q_NAN: nan}, dict(viewport=(40, 40), spin=(0.5, 0.35))


BUILDERS = {"speckle": _speckle, "cores": _cores, "allnan_brick": _allnan_brick, "ragged": _ragged}
NAMES = sorted(BUILDERS)
TRILINEAR = ("cores",)  # the scenes that hold no infinity and keep the shell property


def _image(q, nonfinite):
    """The float32 image of q with NaN / -infinity / +infinity at the markers (nonfinite), or with -1.0 (<= r0) in place
    of NaN and -infinity and +infinity kept (the low twin of the exact anchor)."""
    out = IMAGE.apply(q)
    u = out.view(np.uint32)  # written as bits: a signalling payload stays what it is
    nan = q == Q_NAN
    if nonfinite:
        u[nan] = NAN_BITS[np.arange(int(nan.sum())) % len(NAN_BITS)]
        u[q == Q_NINF] = NINF_BITS
    else:
        out[nan | (q == Q_NINF)] = -1.0
    u[q == Q_PINF] = PINF_BITS
    return out


def _typed(s, nonfinite):
    """voxel_types.typed_scene with the markers replaced, brick by brick and in the atlas."""
    t = vt.typed_scene(s, IMAGE)
    t.atlas = _image(s.atlas, nonfinite)
    t.bricks = {nid: _image(b, nonfinite) for nid, b in s.bricks.items()}
    return t


class Case:
    """q: the scene the references render; t: the float scene with NaN and infinities; low: t with -1.0 in place of NaN
    and -infinity.  mq / mt / mlow: the same with the transfer function of the MIP tests (its first texel is not the
    cleared value).  vol, placed: the q volume and the masks of its markers."""


_CASES = {}


def _mip_tf(s):
    m = copy.copy(s)
    m.tf = mip_scenes.colour_ramp_tf()
    return m


def case(name):
    if name not in _CASES:
        vol, placed, kw = BUILDERS[name]()
        vol = _place(vol, placed)
        c = Case()
        c.name, c.vol, c.placed = name, vol, placed
        c.q = orc.build_scene(voxels=vol.shape[::-1], block=16, dtype="u16", data_range=IMAGE.q_range(), volume=vol, **kw)
        c.t, c.low = _typed(c.q, True), _typed(c.q, False)
        c.mq, c.mt, c.mlow = _mip_tf(c.q), _mip_tf(c.t), _mip_tf(c.low)
        _CASES[name] = c
    return _CASES[name]


_REF = {}


def ref(name, filter_mode=0):
    """ref64's frame of the q scene, once per process; callers leave it unchanged."""
    key = ("composite", name, filter_mode)
    if key not in _REF:
        _REF[key] = ref64.render(case(name).q, filter_mode=filter_mode)
    return _REF[key]


def mref(name, filter_mode=0):
    """mip_ref's result for the q scene, once per process."""
    key = ("mip", name, filter_mode)
    if key not in _REF:
        _REF[key] = mip_ref.render(case(name).mq, filter_mode=filter_mode)
    return _REF[key]


def passes3(s):
    n = s.n_nodes
    return [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]


def mref_passes(name):
    key = ("mip3", name)
    if key not in _REF:
        _REF[key] = mip_ref.render_passes(case(name).mq, passes3(case(name).mq))
    return _REF[key]


def all_nan_rays(r):
    """Pixels whose every sample is surely a NaN voxel: the certain maximum is Q_NAN (the volumes hold no smaller q) and
    no doubtful sample could raise it."""
    return r.certain & (r.m == Q_NAN) & ~r.ambiguous()


# ---- layers: the per-slot word -------------------------------------------------------------------------------------------
#: variant -> (front value, finite stand-in of the front for mip_ref, back interval, dataSourceRange)
LAYERS = {
    "a": (0.25, 0.25, (-0.4, 0.2), (-1.0, 1.0)),
    "b": (-0.5, -0.5, (-0.9, -0.6), (-1.0, 1.0)),      # everything negative: the other half of the key's order
    "c": (np.inf, 2.0, (-0.4, 0.2), (-1.0, 1.0)),      # +infinity and every value >= r1 classify as the last texel
    # what "a" is swapped with in the same slots: noise in front, a constant ABOVE a's front behind it -- a word left
    # over from it would keep a's rays from skipping
    "swapped": (None, None, (-0.4, 0.2), (-1.0, 1.0)),
}
# mip_scenes.COUNT's volume and step, seen along z: every ray enters through the front layer.  25 columns: with 27 the
# columns 9 and 18 look exactly along the brick faces at x = -+1/6 and float64 cannot tell whether they graze a brick
LAYERS_KW = dict(voxels=(48, 48, 48), block=16, viewport=(25, 19), spr=96)
FRONT_Z = 32  # the front layer of bricks holds z >= 32; with its overlap it reads z >= 28


class Layers:
    """t: the float scene; twin: the same with its NaNs and its infinity replaced by numbers, for mip_ref; front: twin
    restricted to the bricks of the front layer.  ref / ref_front: mip_ref's results for twin / front.

    first: the samples a frame takes with VRC_OPT_MIP_SKIP on, to the sample.  A ray marches the first brick it has
    samples in -- it holds no maximum yet -- and after that holds the front value, which no brick exceeds: it skips
    every brick behind the front layer, and also a second brick OF the front layer where it crosses into one (the
    rays of this view spread outwards, and the slot's largest voxel equals the maximum the ray holds: "cannot beat").
    So the count is not the whole front layer's (ref_front.counts, which it may not exceed) but, per ray, that of the
    first front brick in list order that gives it a sample -- the order in which the ray meets them, as the bricks
    nearer the axis come first both in the list and along a ray that spreads outwards."""


_LAYERS = {}


def _float_scene(vol, rng_range):
    base = orc.build_scene(dtype="u16", data_range=(0.0, 65535.0), volume=np.full(vol.shape, 3, dtype=np.uint16),
                           **LAYERS_KW)
    s = copy.copy(base)
    s.bricks = {nid: orc.brick_from_volume(vol, s.vi, s.lod[nid]) for nid in s.ids}
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    s.atlas = np.zeros(base.atlas.shape, dtype=np.float32)
    for nid in s.ids:
        origin = orc.u32x3()
        orc.lib().orc_pool_slot_voxel_origin(orc.u32x3(*s.slots), orc.u32x3(*s.slot_dim), orc.f32x3(*s.slot_of[nid]), origin)
        s.atlas[origin[2]:origin[2] + mb[2], origin[1]:origin[1] + mb[1], origin[0]:origin[0] + mb[0]] = s.bricks[nid]
    r = base.render
    s.render = orc.RenderData(r.samplesPerRay, r.samplesPerPixel, r.maxSamplesPerRay, r.datatype, (C.c_float * 2)(*rng_range))
    s.voxel_type = vrc.VOXEL_FLOAT32
    s.tf = mip_scenes.colour_ramp_tf()
    return s


def _front_only(s):
    """The scene with its node list restricted to the bricks of the front layer, order kept."""
    keep = [i for i in range(s.n_nodes) if float(s.nodes[i].aabbMin[2]) > 0.1]
    f = copy.copy(s)
    f.nodes = (orc.NodeData * len(keep))()
    for k, i in enumerate(keep):
        C.memmove(C.byref(f.nodes, k * C.sizeof(orc.NodeData)), C.byref(s.nodes, i * C.sizeof(orc.NodeData)),
                  C.sizeof(orc.NodeData))
    f.n_nodes = len(keep)
    return f


def layers(variant):
    if variant not in _LAYERS:
        front, front_twin, (b0, b1), rng_range = LAYERS[variant]
        rng = np.random.RandomState(11)
        noise = (b0 + (b1 - b0) * rng.random_sample((48, 48, 48))).astype(np.float32)
        nan = rng.random_sample((48, 48, 48)) < 0.2
        bits = NAN_BITS[rng.randint(0, len(NAN_BITS), size=(48, 48, 48))]
        vol = noise.copy()
        vol.view(np.uint32)[nan] = bits[nan]
        twin = np.where(nan, np.float32(-1.0), noise).astype(np.float32)  # r0: a ray of NaN samples only shows texel 0
        if variant == "swapped":
            vol[:16 + 4], twin[:16 + 4] = 0.5, 0.5  # the layer farthest from the eye, its overlap included
        else:
            vol[FRONT_Z - 4:], twin[FRONT_Z - 4:] = front, front_twin
        L = Layers()
        L.vol, L.nan = vol, nan
        L.t, L.twin = _float_scene(vol, rng_range), _float_scene(twin, rng_range)
        L.front = _front_only(L.twin)
        L.ref, L.ref_front = mip_ref.render(L.twin), mip_ref.render(L.front)
        first = np.zeros((L.twin.H, L.twin.W), dtype=np.int64)
        for i in range(L.front.n_nodes):
            one = copy.copy(L.front)
            one.nodes = (orc.NodeData * 1)()
            C.memmove(one.nodes, C.byref(L.front.nodes, i * C.sizeof(orc.NodeData)), C.sizeof(orc.NodeData))
            one.n_nodes = 1
            r = mip_ref.render(one)
            assert (r.counts_lo == r.counts_hi).all()
            first = np.where(first == 0, r.counts, first)
        L.first = int(first.sum())
        _LAYERS[variant] = L
    return _LAYERS[variant]
