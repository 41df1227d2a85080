"""Scenes of the maximum-intensity tests (tests/test_mip_cpu.py checks every one against the conditions that keep the
acceptance rule of tests/mip_ref.py honest before tests/test_mip.py takes it to a GPU): the smallest at which the march
can still go wrong -- 2 to 4 bricks of 16^3 a side (orc.build_scene's volumes carry an overlap of 4 voxels, so a brick
is 24^3 in its slot), viewports with partial 8x8 tiles, 96 and 128 samples per ray (groups plus a tail, a float chain
and an integer step count)."""
import numpy as np

import orc


def colour_ramp_tf():
    """A second ramp, with colour: every channel moves by at most 1/255 from texel to texel, as orc.linear_ramp_tf's do."""
    i = np.arange(256, dtype=np.float32) / np.float32(255.0)
    tf = np.stack([i, np.float32(1.0) - i, np.float32(0.5) * i, np.float32(0.2) + np.float32(0.6) * i], axis=1)
    return np.ascontiguousarray(tf.astype(np.float32))


def skip_volume(n=48, dtype=np.uint8):
    """Noise of low amplitude, two constant bricks and one bright brick nearest the eye (the eye is on +z).  A brick is
    constant only if its overlap is too: brick i of an axis holds the voxels [16 i - OVERLAP, 16 i + 16 + OVERLAP) of the
    volume, clamped, so two constant bricks of different value cannot be neighbours, not even across a corner.  One
    value lies below the noise (a ray that saw noise first skips that brick), one above it (such a ray takes it, from
    the slot's word alone where uniform bricks are on)."""
    rng = np.random.RandomState(7)
    vol = rng.randint(1, 40, size=(n, n, n)).astype(np.uint8)  # (z, y, x)
    a, b = 16 + OVERLAP, n - 16 - OVERLAP
    vol[0:a, 0:a, 0:a] = 9                # brick (0, 0, 0), overlap included
    vol[0:a, b:n, b:n] = 60               # brick (2, 2, 0)
    c0, c1 = 16 - OVERLAP, 32 + OVERLAP
    vol[b:n, c0:c1, c0:c1] = rng.randint(180, 250, size=(n - b, c1 - c0, c1 - c0)).astype(np.uint8)  # brick (1, 1, 2)
    if dtype == np.uint16:  # spread over 16 bits as orc.build_scene's hash volume is: a constant brick stays constant
        vol = vol.astype(np.uint16) * np.uint16(257) ^ (vol.astype(np.uint16) >> np.uint16(3))
    return vol


OVERLAP = 4  # of every volume orc.build_scene makes (test_mip_cpu.py asserts it)


def uniform_and_mixed(s):
    """(number of bricks of the scene that are constant with their overlap, number that are not)."""
    u = sum(1 for b in s.bricks.values() if (b == b.flat[0]).all())
    return u, len(s.bricks) - u


SCENES = {
    # (along an axis the samples of a noise volume sit on voxel faces for whole segments: more than 5 % of its pixels
    # would be ambiguous; the mem:// volume's bricks are constant, so a face tie inside a brick decides nothing)
    "axis": dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), spr=128),
    "spin": dict(voxels=(48, 48, 48), block=16, viewport=(44, 36), volume="hash", spr=96, spin=(0.5, 0.35)),
    "inside": dict(voxels=(32, 32, 32), block=16, viewport=(28, 20), volume="hash", spr=96, eye=(0.1, 0.05, 0.2)),
    "clip": dict(voxels=(48, 48, 48), block=16, viewport=(36, 28), volume="hash", spr=128, spin=(0.5, 0.35),
                 planes=[[-1, 0, 0, 0.2], [0.6, 0, 0.8, 0.35]]),
    "skip": dict(voxels=(48, 48, 48), block=16, viewport=(44, 36), spr=128, spin=(0.2, 0.1)),
    # scenes in which float64 leaves no sample of any ray in doubt (test_mip_cpu.py asserts it): the sample count of
    # the whole frame is then one number.  (Odd viewports: the middle row of an even one looks along brick faces.)
    "count96": dict(voxels=(48, 48, 48), block=16, viewport=(27, 19), volume="hash", spr=96, spin=(0.27, 0.58)),
    "count128": dict(voxels=(48, 48, 48), block=16, viewport=(27, 19), volume="hash", spr=128, spin=(0.48, 0.29)),
    "countclip": dict(voxels=(48, 48, 48), block=16, viewport=(27, 19), volume="hash", spr=128, spin=(0.63, 0.37),
                      planes=[[-1, 0, 0, 0.2], [0.6, 0, 0.8, 0.35]]),
    "skip16": dict(voxels=(48, 48, 48), block=16, viewport=(44, 36), spr=128, spin=(0.2, 0.1)),  # 16-bit voxels
}
COUNT = ("count96", "count128", "countclip")
COLOUR = ("spin",)  # rendered with colour_ramp_tf


def get(name, dtype="u8"):
    kw = dict(SCENES[name])
    if name == "skip":
        kw["volume"] = skip_volume(48)
    elif name == "skip16":
        kw["volume"], dtype = skip_volume(48, np.uint16), "u16"
    s = orc.build_scene(dtype=dtype, alpha=0.8, **kw)
    if name in COLOUR:
        s.tf = colour_ramp_tf()
    return s


_TYPED = {}
TYPED_IMAGES = ("uint16", "int16", "float")


def typed(image):
    """(the scene mip_ref reads: uint16 voxels q, the range carried back to q; the scene that is rendered; a dict for
    its references), once."""
    import voxel_types
    if image not in _TYPED:
        if image == "uint16":
            q = orc.build_scene(voxels=(64, 64, 64), dtype="u16", **dict(voxel_types.BASES["hash16"], viewport=(36, 28)))
            t = q
        else:
            q = voxel_types.q_scene("hash16", voxel_types.IMAGES[image], viewport=(36, 28))
            t = voxel_types.typed_scene(q, voxel_types.IMAGES[image])
        q.tf = t.tf = orc.linear_ramp_tf(0.8)
        _TYPED[image] = (q, t, {})
    return _TYPED[image]


def typed_ref(image, filter_mode):
    import mip_ref
    q, _, refs = typed(image)
    if filter_mode not in refs:
        refs[filter_mode] = mip_ref.render(q, filter_mode=filter_mode)
    return refs[filter_mode]


# ---- the scenes tests/test_mip_host.py renders through the plugin ------------------------------------------------------
HOST_MEM = dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), spin=(0.5, 0.35), alpha=0.8)
HOST_NUCLEON = dict(viewport=(44, 36), spin=(0.4, 0.3), alpha=0.8)


def host_mem_scene(ids=None, spr=0):
    """mem://#64,64,64,16 at its finest level; ids: the plugin's visible set (the 64 leaves, which is the default)."""
    return orc.build_scene(ids=ids, spr=spr, **HOST_MEM)


def host_nucleon_scene():
    import scenes
    return scenes.nucleon_scene(**HOST_NUCLEON)


_REF = {}


def ref(name, filter_mode=0, dtype="u8"):
    """mip_ref of a scene, computed once and shared; callers leave it unchanged."""
    import mip_ref
    key = (name, filter_mode, dtype)
    if key not in _REF:
        _REF[key] = mip_ref.render(get(name, dtype), filter_mode=filter_mode)
    return _REF[key]


# ---- the host build of the MIP per-ray code (tests/cpu_harness/mip_harness.cpp), built as typed_harness.cpp is ---------
GRID, FIXED, TRILINEAR, SKIP, UNIFORM = 1, 2, 8, 16, 32
_H = None


def harness():
    import ctypes as C
    import os
    import subprocess
    global _H
    if _H is None:
        here = os.path.dirname(os.path.abspath(__file__))
        src = os.path.join(here, "cpu_harness", "mip_harness.cpp")
        out = os.path.join(here, "cpu_harness", "libmip_harness.so")
        deps = [src, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, src])
            os.replace(tmp, out)
        _H = C.CDLL(out)
    return _H


def harness_render(s, form, passes=None, frac_bits=8, per_pixel=None):
    """(frame, samples) of the host build; passes: [(a, b)] of s.nodes, meeting in the running maxima.  per_pixel: an
    H x W int64 array that receives every pixel's sample count, summed over the passes."""
    import ctypes as C
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    run = np.zeros((s.H, s.W), dtype=np.uint32)
    total = 0
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().mip_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(fb.ctypes.data), C.c_void_p(run.ctypes.data),
            C.c_uint32(s.W), C.c_uint32(s.H), C.c_void_p(s.planes.ctypes.data if len(s.planes) else None),
            C.c_uint32(len(s.planes)), C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes,
            C.byref(s.render), C.c_int(form), C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.byref(samples),
            C.c_void_p(each.ctypes.data))
        assert rc == 0, "mip_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        if per_pixel is not None:
            per_pixel += each
        total += int(samples.value)
    return fb, total
