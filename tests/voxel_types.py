"""Scenes of signed, 32-bit and float voxels (vrc_pool_create_typed, include/vrc_hip.h) for tests/test_voxel_types*.py.

tests/ref64.py point-samples through a table indexed by the voxel, so it takes 8- and 16-bit bricks only.  The typed
scenes are therefore AFFINE IMAGES of scenes it does take: the volume is v = a + b q of a uint16 (or uint8) volume q,
with a and b chosen so that every v is exact in the voxel type and in float32, and a dataSourceRange (r0, r1) in the
volume's values.  Classification depends on (v - r0) / (r1 - r0) alone, so ref64's frame of the q scene with
dataSourceRange ((r0 - a) / b, (r1 - a) / b) is the frame the typed volume must give -- under the frozen rule of
tests/scenes.py with ref64's own tie budget, exactly as tests/test_ref64_cpu.py::check applies it.  ref64 itself is
untouched."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

import orc
import ref64
from libre_amd import vrc

HERE = os.path.dirname(os.path.abspath(__file__))


class Image:
    """v = a + b q in `dtype`; (r0, r1): the dataSourceRange in v's values.  base: the dtype of q ("u16" / "u8")."""

    def __init__(self, name, voxel_type, dtype, a, b, r0, r1, base="u16"):
        self.name, self.voxel_type, self.dtype, self.a, self.b, self.r0, self.r1, self.base = (
            name, voxel_type, np.dtype(dtype), a, b, r0, r1, base)

    def apply(self, q):
        v = (np.float64(self.a) + np.float64(self.b) * q.astype(np.float64))
        out = v.astype(self.dtype)
        assert (out.astype(np.float64) == v).all(), "%s: the image is not exact in %s" % (self.name, self.dtype)
        assert (out.astype(np.float32).astype(np.float64) == v).all(), "%s: the image is not exact in float32" % self.name
        return np.ascontiguousarray(out)

    def q_range(self):
        q0, q1 = (self.r0 - self.a) / self.b, (self.r1 - self.a) / self.b
        for x in (q0, q1, self.r0, self.r1):  # both ranges travel as float32 (vrc_render_data)
            assert float(np.float32(x)) == x, (self.name, x)
        return q0, q1


IMAGES = {i.name: i for i in [
    # float: -1 + q / 32768, the whole interval and a narrower range that clamps at both ends
    Image("float", vrc.VOXEL_FLOAT32, np.float32, -1.0, 1.0 / 32768.0, -1.0, 1.0),
    Image("float_narrow", vrc.VOXEL_FLOAT32, np.float32, -1.0, 1.0 / 32768.0, -0.5, 0.75),
    Image("int32", vrc.VOXEL_INT32, np.int32, -4000000, 128, -4000000, -4000000 + 128 * 65535),
    Image("uint32", vrc.VOXEL_UINT32, np.uint32, 1000, 128, 1000, 1000 + 128 * 65535),
    Image("int16", vrc.VOXEL_INT16, np.int16, -32768, 1, -32768, 32767),
    Image("int8", vrc.VOXEL_INT8, np.int8, -128, 1, -128, 127, base="u8"),
]}
FOUR_BYTE = ["float", "float_narrow", "int32", "uint32"]


def smooth16(n=64):
    """The smooth volume of tests/test_ref64_cpu.py in 16 bits: neighbours differ by a few hundred of 65536 levels, so
    one flipped sample moves a pixel by less than E0 and the tie budget cannot be what makes a comparison pass."""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    v = 20480.0 + 512.0 * (np.sin(2 * np.pi * x / 61.0 + 0.3) + np.sin(2 * np.pi * y / 47.0 + 1.1) +
                           np.sin(2 * np.pi * z / 53.0 + 2.0))
    return np.floor(v + 0.5).astype(np.uint16)


#: the q scenes (orc.build_scene keywords; 64^3 voxels, viewports of at most 64^2)
BASES = {
    "hash16": dict(volume="hash", block=16, viewport=(40, 48), spin=(0.5, 0.35)),
    "smooth16": dict(volume="smooth16", block=16, viewport=(40, 40), spin=(0.7, 0.4)),
    "hash32_clip": dict(volume="hash", block=32, viewport=(48, 40), spin=(2.6, 0.9), planes=[[0.6, 0.0, 0.8, 0.3]]),
    "hash16_ert": dict(volume="hash", block=16, viewport=(36, 36), spin=(0.3, -0.2), alpha=1.0),
}


def q_scene(base, image, **over):
    """The scene ref64 renders: uint16 / uint8 voxels q with the image's range carried back to q."""
    kw = dict(BASES[base], **over)
    if kw.get("volume") == "smooth16":
        kw["volume"] = smooth16() if image.base == "u16" else (smooth16() >> 8).astype(np.uint8)
    return orc.build_scene(voxels=(64, 64, 64), dtype=image.base, data_range=image.q_range(), **kw)


def typed_scene(s, image):
    """The same scene with its voxels replaced by their image and the range in the image's values."""
    t = copy.copy(s)
    t.atlas = image.apply(s.atlas)
    t.bricks = {nid: image.apply(b) for nid, b in s.bricks.items()}
    r = s.render
    t.render = orc.RenderData(r.samplesPerRay, r.samplesPerPixel, r.maxSamplesPerRay, r.datatype,
                              (C.c_float * 2)(image.r0, image.r1))
    t.voxel_type = image.voxel_type
    return t


_REF = {}


def ref(base, image, filter_mode=0, frac_bits=8, **over):
    """(q scene, typed scene, ref64's frame of the q scene), once per process."""
    key = (base, image.name, filter_mode, frac_bits, tuple(sorted(over.items())))
    skey = key[:2] + key[4:]
    if skey not in _REF:
        s = q_scene(base, image, **over)
        _REF[skey] = (s, typed_scene(s, image))
    if key not in _REF:
        _REF[key] = ref64.render(_REF[skey][0], filter_mode=filter_mode, frac_bits=frac_bits)
    return _REF[skey][0], _REF[skey][1], _REF[key]


# ---- the host build of the kernel code over the typed atlases ------------------------------------------------------
SRC = os.path.join(HERE, "cpu_harness", "typed_harness.cpp")
OUT = os.path.join(HERE, "cpu_harness", "libtyped_harness.so")
GRID, FIXED, GREY, TRILINEAR = 1, 2, 4, 8
_H = None


def harness():
    global _H
    if _H is None:
        deps = [SRC, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (OUT, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, OUT)
        _H = C.CDLL(OUT)
    return _H


def harness_render(t, form, frac_bits=8, fb=None):
    clear_first = fb is None
    if fb is None:
        fb = np.zeros((t.H, t.W, 4), dtype=np.float32)
    samples = C.c_uint64(0)
    rc = harness().typed_harness_render(
        C.c_void_p(t.atlas.ctypes.data), C.c_int(t.voxel_type), orc.u32x3(*t.atlas_dim), orc.u32x3(*t.slot_dim),
        C.c_void_p(fb.ctypes.data), C.c_uint32(t.W), C.c_uint32(t.H),
        C.c_void_p(t.planes.ctypes.data if len(t.planes) else None), C.c_uint32(len(t.planes)),
        C.c_void_p(t.tf.ctypes.data), C.byref(t.view), C.c_uint32(t.n_nodes), t.nodes, C.byref(t.render), C.c_int(form),
        C.c_int(frac_bits), C.c_int(1 if clear_first else 0), C.byref(samples))
    assert rc == 0, "typed_harness_render: %d" % rc
    return fb, int(samples.value)


def harness_xform(src, voxel_type, out_dtype):
    src = np.ascontiguousarray(src)
    dst = np.empty(src.shape, dtype=out_dtype)
    assert dst.itemsize == src.itemsize
    rc = harness().typed_harness_xform(C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data), C.c_uint64(src.size),
                                       C.c_int(voxel_type))
    assert rc == 0
    return dst


def harness_classify(tf, d, r0, r1, alpha_correction=1.0, frac_bits=8):
    d = np.ascontiguousarray(d, dtype=np.float32)
    out = np.empty((d.size, 4), dtype=np.float32)
    rc = harness().typed_harness_classify(C.c_void_p(tf.ctypes.data), C.c_void_p(d.ctypes.data), C.c_uint32(d.size),
                                          C.c_float(r0), C.c_float(r1), C.c_float(alpha_correction), C.c_int(frac_bits),
                                          C.c_void_p(out.ctypes.data))
    assert rc == 0, "typed_harness_classify: %d" % rc
    return out


# ---- the GPU through the C ABI -------------------------------------------------------------------------------------
def typed_gpu_scene(t, device=0, voxel_type=None):
    """tests/gpu_run.py's GpuScene with its pool made by vrc_pool_create_typed."""
    from gpu_run import GpuScene

    class TypedGpuScene(GpuScene):
        def __init__(self, s):
            self.L = L = vrc.load_library()
            self.s = s
            self.ctx = C.c_void_p()
            self.pool = C.c_void_p()
            vrc.check(L, L.vrc_ctx_create(device, C.byref(self.ctx)))
            mb = vrc.u32x3(*[s.vi.maximumBlockSize[a] for a in range(3)])
            self.voxel_bytes = s.atlas.dtype.itemsize
            vt = s.voxel_type if voxel_type is None else voxel_type
            try:
                vrc.check(L, L.vrc_pool_create_typed(self.ctx, vt, mb, s.pool_bytes * self.voxel_bytes,
                                                     C.byref(self.pool)))
                self.slots = {}
                for nid in s.ids:
                    brick = s.bricks[nid]
                    slot = vrc.f32x3()
                    size = vrc.u32x3(brick.shape[2], brick.shape[1], brick.shape[0])
                    vrc.check(L, L.vrc_pool_copy_to_slot(self.pool, brick.ctypes.data, size, slot))
                    self.slots[nid] = (slot[0], slot[1], slot[2])
            except Exception:
                self.close()
                raise

    return TypedGpuScene(t)
