"""A float64 restatement of a slice frame (include/vrc_hip.h, "A slice frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py, tests/mip_ref.py, tests/depth_ref.py and tests/mip_scenes.py (imported,
none is edited); it shares nothing with libre_amd/csrc/vrc_core.h.

A pixel's ray meets the plane (n, d), n.x + d = 0, at t_p = -(n.origin + d) / (n.dir); it takes its one sample there if
the ray hits the global box and max(tNearGlobal, tNearPlane) <= t_p <= tFarGlobal, from a node of the pass whose box holds
P = origin + t_p dir.  All of it in float64.

Float64 cannot say how float32 decides a tie, so a pixel gets a finite set of CANDIDATES: "unsampled", or (V, t).
  w = ref64.REL_WINDOW x max(1, |t_p|) / |cos(dir, n)| is how far float32 may move t_p: the window the contract gives a
    ray parameter, over the cosine the division by n.dir magnifies it by.
  A node is a candidate if its float64 interval of the slab test, widened by w, contains t_p.
  "Unsampled" is a candidate only if t_p is within w of leaving the ray's interval or the union of the pass's boxes
    (on the ray: the union of the nodes' intervals).
  A point sample's candidate voxels are those within orc.TIE_DELTA + w |dir_a| voxPerWorld_a of l_a per axis.
  A trilinear sample's V is accepted within depth_ref.tolerance plus (spread of its eight taps) x (sum of those per-axis
    margins): an interpolant moves by at most the spread per voxel along each axis.

A pixel with count 0 passes if "unsampled" is a candidate, D is +infinity and the pixel is cleared.  A pixel with count 1
passes if some candidate matches V -- exactly for point samples of integer atlases, to tolerance otherwise -- and D lies
within w of that candidate's t.  The frame's pixel is then held to mip_ref.classify64(V) within scenes.E0.

own() is what a renderer that agrees with float64 everywhere reads back; `mutate` gives deliberate misreadings of it,
for tests/test_slice_cpu.py alone.
"""
import numpy as np

import depth_ref
import mip_ref
import mip_scenes
import orc
import scenes
from ref64 import EPSILON, EXACT_TIE, REL_WINDOW, _Ctx, _mat, _slab, _trilinear, _vec, node_ids

MUTATIONS = ("lattice_sample", "plane_negated", "unclipped", "neighbour_brick", "depth_half_step", "later_pass_overwrites")
#: at most this share of a scene's covered pixels may have more than one candidate value (the issue's condition; a scene
#: that exceeds it is replaced, the cap is not raised)
MULTI_CAP = 0.05
#: every scene under the cap keeps |cos(dir, n)| at or above this over the viewport
MIN_COS = 0.2


def plane_through(point, normal):
    """(nx, ny, nz, d) of the plane through `point` with normal `normal`, as float32 -- what vrc_set_slice is given."""
    n = np.asarray(normal, dtype=np.float64)
    return np.array([n[0], n[1], n[2], -float(n @ np.asarray(point, dtype=np.float64))], dtype=np.float32)


class Result:
    """Per pixel (H x W): t the float64 ray parameter of the plane (NaN: the ray lies in it), w its window, cos;
    sure: a sample surely taken; none: "unsampled" is a candidate; cands[(y, x)]: [(V, t, node)], the first of a node the
    pixel's own reading of it; tolv[(y, x)]: what V may differ by."""

    def __init__(self, s, plane, filter_mode):
        self.s, self.H, self.W, self.plane, self.filter_mode = s, s.H, s.W, plane, filter_mode
        self.cands, self.tolv = {}, {}

    def covered(self):
        """pixels with a sample among their candidates"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            out[key] = bool(c)
        return out

    def multi(self):
        """pixels with more than one candidate value"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            out[key] = len({q[0] for q in c}) > 1
        return out

    def share(self):
        return float(self.multi().sum()) / max(int(self.covered().sum()), 1)

    def single_node(self):
        """pixels that surely take their sample, from one node only"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            out[key] = bool(c) and len({q[2] for q in c}) == 1
        return out & self.sure

    def own(self, mutate=None):
        """(values, counts, depths) of the certain answer of every pixel that has one."""
        assert mutate is None or mutate in MUTATIONS, mutate
        s = self.s
        if mutate == "plane_negated":  # the plane mirrored through the origin: (n, -d)
            p = self.plane.astype(np.float64).copy()
            p[3] = -p[3]
            return render(s, p.astype(np.float32), self.filter_mode).own()
        if mutate == "unclipped":
            import copy
            t = copy.copy(s)
            t.planes = np.zeros((0, 4), dtype=np.float32)
            return render(t, self.plane, self.filter_mode).own()
        values = np.zeros((self.H, self.W))
        counts = np.zeros((self.H, self.W), dtype=np.uint32)
        depths = np.full((self.H, self.W), np.inf)
        step = 1.0 / float(s.render.samplesPerRay)
        for y, x in zip(*np.nonzero(self.sure)):
            v, t, node = self.cands[(y, x)][0]
            if mutate == "lattice_sample":  # the nearest sample of the ray's step lattice from tNearGlobal
                t0 = self.t_lo[y, x]
                t = t0 + np.round((t - t0) / step) * step
                v = self._value_at(y, x, node, t)
            elif mutate == "neighbour_brick":  # the right local coordinate in the wrong slot
                v = self._value_at(y, x, (node + 1) % s.n_nodes, t, local_of=node)
            elif mutate == "depth_half_step":
                t = t + 0.5 * step
            counts[y, x], values[y, x], depths[y, x] = 1, v, t
        return values, counts, depths

    def _value_at(self, y, x, node, t, local_of=None):
        s = self.s
        P = self.origin + self.dir[y, x] * t
        c = _coords(s, node if local_of is None else local_of, P[None, :])
        brick = s.bricks[node_ids(s)[node]]
        return float(_value(s, brick, c, self.filter_mode)[0])


def _coords(s, i, P):
    nid = node_ids(s)[i]
    nd = s.nodes[i]
    lo, size = _vec(nd.aabbMin, 3), _vec(nd.aabbSize, 3)
    ov = np.array([float(s.vi.overlap[a]) for a in range(3)])
    bs = np.array([float(s.lod[nid].blockSize[a]) for a in range(3)])
    return ov + (P - lo) / size * bs


def _clamp(s, c):
    """the contract's clamp of the slot-local coordinate: [0, slotDim - 1] (a slot is at least its brick; the voxels of a
    slot beyond its brick repeat the brick's last, so an index is clamped to the brick)"""
    return np.clip(c, 0.0, np.array([float(v) for v in s.slot_dim]) - 1.0)


def _value(s, brick, c, filter_mode):
    dims = brick.shape[::-1]
    c = _clamp(s, c)
    if filter_mode:
        cx = _Ctx()
        cx.mutate = None
        return _trilinear(cx, brick, c)
    idx = [np.clip(np.floor(c[..., a]), 0, dims[a] - 1).astype(np.intp) for a in range(3)]
    return brick[idx[2], idx[1], idx[0]].astype(np.float64)


def render(s, plane, filter_mode=0, tol=None, nodes=None):
    """The candidates of every pixel for the pass over nodes = (a, b) of s.nodes (default: all)."""
    view = s.view
    plane = np.asarray(plane, dtype=np.float32)
    if tol is None:
        tol = depth_ref.tolerance(s, filter_mode)
    res = Result(s, plane, filter_mode)
    ys, xs = np.arange(s.H), np.arange(s.W)
    py, px = [g.reshape(-1).astype(np.float64) for g in np.meshgrid(ys, xs, indexing="ij")]
    vp = [float(view.glViewport[i]) for i in range(4)]
    n = px.size
    ndc = np.stack([2.0 * (px - vp[0] - vp[2] / 2.0) / vp[2], 2.0 * (py - vp[1] - vp[3] / 2.0) / vp[3],
                    np.ones(n), np.ones(n)], axis=1)
    eye4 = ndc @ _mat(view.invProjMatrix).T
    eye4 = eye4 / eye4[:, 3:4]
    world = eye4 @ _mat(view.invViewMatrix).T
    origin = _vec(view.eyePosition, 3)
    d = world[:, :3] - origin
    d = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    d[d == 0.0] = EPSILON
    e3 = eye4[:, :3]
    t_near_plane = -float(view.nearPlane) / (e3[:, 2] / np.sqrt((e3 * e3).sum(axis=1)))
    tn_g, tf_g = _slab(origin, d, _vec(view.aabbMin, 3), _vec(view.aabbMax, 3))
    for pl in np.asarray(s.planes, dtype=np.float64).reshape(-1, 4):
        normal, dd = pl[:3], pl[3]
        rn = d @ normal
        rn = np.where(rn == 0.0, EPSILON, rn)
        t = -(normal @ origin + dd) / rn
        tn_g = np.where(rn > 0.0, np.maximum(tn_g, t), tn_g)
        tf_g = np.where(rn > 0.0, tf_g, np.minimum(tf_g, t))

    normal, dd = plane[:3].astype(np.float64), float(plane[3])
    rn = d @ normal
    cos = np.abs(rn) / np.sqrt(normal @ normal)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.where(rn != 0.0, -(normal @ origin + dd) / rn, np.nan)
        w = REL_WINDOW * np.maximum(1.0, np.abs(tp)) / cos
    lo = np.maximum(tn_g, t_near_plane)
    # the ray's interval: surely inside, possibly inside (a box the ray barely misses in float64 may be hit in float32)
    with np.errstate(invalid="ignore"):
        in_sure = (tf_g - tn_g > w) & (tp >= lo + w) & (tp <= tf_g - w)
        in_maybe = (tf_g - tn_g >= -w) & (tp >= lo - w) & (tp <= tf_g + w)
    res.origin, res.dir = origin, d.reshape(s.H, s.W, 3)
    res.t, res.w, res.cos = tp.reshape(s.H, s.W), w.reshape(s.H, s.W), cos.reshape(s.H, s.W)
    res.t_lo = tn_g.reshape(s.H, s.W)

    a, b = nodes if nodes is not None else (0, s.n_nodes)
    ids = node_ids(s)
    P = origin + d * np.where(np.isfinite(tp), tp, 0.0)[:, None]
    iv = []
    for i in range(a, b):
        nd = s.nodes[i]
        blo, size = _vec(nd.aabbMin, 3), _vec(nd.aabbSize, 3)
        tn, tf = _slab(origin, d, blo, blo + size)
        iv.append((i, tn, tf))
    # the union of the nodes' intervals around t_p: does it cover [t_p - w, t_p + w]?
    reach = tp - w
    for _ in range(len(iv) + 1):
        before = reach.copy()
        for i, tn, tf in iv:
            with np.errstate(invalid="ignore"):
                ok = (tf >= tn) & (tn <= reach + 0.25 * w) & (tf > reach)
            reach = np.where(ok, tf, reach)
        if np.array_equal(before, reach, equal_nan=True):
            break
    with np.errstate(invalid="ignore"):
        in_union = reach >= tp + w
    sure = in_sure & in_union
    res.sure = sure.reshape(s.H, s.W)
    res.none = ~res.sure
    for key in zip(*np.nonzero(np.ones((s.H, s.W), dtype=bool))):
        res.cands[(int(key[0]), int(key[1]))] = []
    for i, tn, tf in iv:
        with np.errstate(invalid="ignore"):
            cand = in_maybe & (tf - tn >= -w) & (tp >= tn - w) & (tp <= tf + w)
        p = np.nonzero(cand)[0]
        if p.size == 0:
            continue
        nid = ids[i]
        brick = s.bricks[nid]
        dims = np.array(brick.shape[::-1], dtype=np.float64)
        size = _vec(s.nodes[i].aabbSize, 3)
        bs = np.array([float(s.lod[nid].blockSize[k]) for k in range(3)])
        vpw = bs / size
        c = _clamp(s, _coords(s, i, P[p]))
        margin = orc.TIE_DELTA + w[p, None] * np.abs(d[p]) * vpw[None, :]
        own = _value(s, brick, c, filter_mode)
        if filter_mode:
            # the eight taps around the sample, and the voxels a margin reaches
            cc = c - 0.5
            f0 = np.floor(cc)
            taps = []
            for m in range(8):
                q = [np.clip(f0[:, k] + ((m >> k) & 1), 0, dims[k] - 1).astype(np.intp) for k in range(3)]
                taps.append(brick[q[2], q[1], q[0]].astype(np.float64))
            taps = np.stack(taps, axis=1)
            spread = taps.max(axis=1) - taps.min(axis=1)
            tolv = tol + spread * margin.sum(axis=1)
            for j in range(p.size):
                key = (int(p[j]) // s.W, int(p[j]) % s.W)
                res.cands[key].append((float(own[j]), float(tp[p[j]]), i))
                res.tolv[key] = max(res.tolv.get(key, 0.0), float(tolv[j]))
            continue
        fr = c - np.floor(c)
        off = np.where(fr < margin, -1, 0) + np.where(fr > 1.0 - margin, 1, 0)
        idx = np.clip(np.floor(c), 0, dims - 1).astype(np.intp)
        for j in range(p.size):
            key = (int(p[j]) // s.W, int(p[j]) % s.W)
            res.cands[key].append((float(own[j]), float(tp[p[j]]), i))
            res.tolv[key] = tol
            if not off[j].any():
                continue
            for m in range(1, 8):
                use = [(m >> k) & 1 for k in range(3)]
                if any(use[k] and off[j, k] == 0 for k in range(3)):
                    continue
                q = [int(np.clip(idx[j, k] + use[k] * off[j, k], 0, dims[k] - 1)) for k in range(3)]
                res.cands[key].append((float(brick[q[2], q[1], q[0]]), float(tp[p[j]]), i))
    return res


def check(res, values, counts, depths, frame=None, cleared=None):
    """The acceptance rule.  values in the scene's own units; frame: H x W x 4 or None; cleared: what an unsampled pixel
    of the frame holds (default zeros).  Returns the number of failing pixels."""
    values, counts = np.asarray(values, dtype=np.float64), np.asarray(counts)
    depths = np.asarray(depths, dtype=np.float64)
    bad = 0
    for y in range(res.H):
        for x in range(res.W):
            if counts[y, x] == 0:
                ok = bool(res.none[y, x]) and np.isposinf(depths[y, x])
                if frame is not None:
                    ok = ok and np.array_equal(frame[y, x], np.zeros(4) if cleared is None else cleared[y, x])
                bad += not ok
                continue
            if counts[y, x] != 1:
                bad += 1
                continue
            v, t = values[y, x], depths[y, x]
            tolv = res.tolv.get((y, x), 0.0)
            ok = any((v == q[0] or abs(v - q[0]) <= tolv or (np.isnan(v) and np.isnan(q[0]))) and
                     abs(t - q[1]) <= res.w[y, x] for q in res.cands[(y, x)])
            if ok and frame is not None and not np.isnan(v):
                ok = bool(np.abs(np.asarray(frame[y, x], dtype=np.float64) - mip_ref.classify64(res.s, v)).max() <= scenes.E0)
            bad += not ok
    return bad


def merge(first, second):
    """own()-style read-backs of two passes met as the contract says: the later pass sets only unsampled pixels."""
    v0, c0, d0 = first
    v1, c1, d1 = second
    take = (c0 == 0) & (c1 != 0)
    return np.where(take, v1, v0), np.where(take, c1, c0), np.where(take, d1, d0)


# ---- the scenes of tests/test_slice_cpu.py and tests/test_slice.py, and their references, computed once ------------------
#: 64^3 voxels in bricks of 16^3 in the unit cube around the origin: 64 voxels per world unit, layer k of an axis spans
#: [-0.5 + k / 64, -0.5 + (k + 1) / 64)
VOXELS, BLOCK = 64, 16
AXIAL_LAYER = 37


def layer_centre(k):
    return -0.5 + (k + 0.5) / VOXELS


OBLIQUE_N = (0.31, -0.42, 0.85)
#: name -> (orc.build_scene keywords, plane)
SCENES = {
    "axial": (dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), volume="hash", spin=(0.23, 0.31)),
              plane_through((0.0, 0.0, layer_centre(AXIAL_LAYER)), (0.0, 0.0, 1.0))),
    "oblique": (dict(voxels=(64, 64, 64), block=16, viewport=(48, 40), volume="hash", spin=(0.5, 0.35)),
                plane_through((0.0, 0.0, 0.0), OBLIQUE_N)),
    "clip": (dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), volume="hash", spin=(0.5, 0.35),
                  planes=[[-1, 0, 0, 0.2], [0.6, 0, 0.8, 0.35]]),
             plane_through((0.05, 0.0, 0.07), OBLIQUE_N)),  # (off the centre: the sign of d matters)
}
#: eye inside the box: one plane in front of it (sampled), one behind it (the frame stays cleared)
INSIDE = dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), volume="hash", eye=(0.1, 0.05, 0.2))
INSIDE_FRONT = plane_through((0.0, 0.0, -0.2), (0.1, 0.2, 1.0))
INSIDE_BEHIND = plane_through((0.0, 0.0, 0.45), (0.1, 0.2, 1.0))
OUTSIDE = plane_through((0.0, 0.0, 2.0), (0.0, 0.3, 1.0))  # misses the box
#: exactly on the face between the bricks of z layers 31 | 32, seen from a spun camera
FACE = plane_through((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
_SCENES, _REFS = {}, {}


def scene(name):
    if name not in _SCENES:
        if name in SCENES:
            kw = SCENES[name][0]
        elif name in ("inside", "behind"):
            kw = INSIDE
        elif name in ("outside", "face"):
            kw = SCENES["axial"][0]
        elif name == "edge-on":
            kw = dict(SCENES["axial"][0], spin=(0.0, 0.0))
        elif name == "mem":
            kw = dict(voxels=(64, 64, 64), block=16, viewport=(44, 36), spin=(0.5, 0.35))
        elif name == "zindex":
            z = np.arange(64, dtype=np.uint8)[:, None, None]
            kw = dict(SCENES["axial"][0], volume=np.ascontiguousarray(np.broadcast_to(z, (64, 64, 64))))
        else:
            raise KeyError(name)
        _SCENES[name] = orc.build_scene(dtype="u8", alpha=0.8, **kw)
    return _SCENES[name]


def plane(name):
    if name in SCENES:
        return SCENES[name][1]
    if name == "edge-on":
        # contains the central ray of the unspun camera on +z: n.dir = 0 there and small around it
        return plane_through((0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    return {"inside": INSIDE_FRONT, "behind": INSIDE_BEHIND, "outside": OUTSIDE, "face": FACE,
            "mem": SCENES["oblique"][1], "zindex": SCENES["axial"][1]}[name]


#: the scenes held to the cap and the candidate rule
RULE_SCENES = ("axial", "oblique", "clip", "inside")


def ref(name, filter_mode=0):
    """render of a scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode)
    if key not in _REFS:
        _REFS[key] = render(scene(name), plane(name), filter_mode)
    return _REFS[key]


def nucleon_scene():
    if "nucleon" not in _SCENES:
        _SCENES["nucleon"] = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    return _SCENES["nucleon"]


NUCLEON_PLANE = plane_through((0.0, 0.0, 0.013), (0.2, -0.3, 1.0))


def nucleon_ref(filter_mode=0):
    key = ("nucleon", filter_mode)
    if key not in _REFS:
        _REFS[key] = render(nucleon_scene(), NUCLEON_PLANE, filter_mode)
    return _REFS[key]


def lod_scene():
    """a cut of mixed brick sizes, for the reference-order loop (tests/nongrid.py)"""
    import nongrid
    if "lod" not in _SCENES:
        s = nongrid.overlapping_scene("hash_parents_some_children", viewport=(36, 28))
        s.tf = orc.linear_ramp_tf(0.8)
        _SCENES["lod"] = s
    return _SCENES["lod"]


def typed_ref(image, filter_mode):
    key = ("typed", image, filter_mode)
    if key not in _REFS:
        q = mip_scenes.typed(image)[0]
        tol = 0.0 if (not filter_mode and image != "float") else scenes.E0 * (
            float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
        _REFS[key] = render(q, TYPED_PLANE, filter_mode, tol=tol)
    return _REFS[key]


TYPED_PLANE = plane_through((0.0, 0.0, 0.0), OBLIQUE_N)
#: tests/nonfinite.py's brick of NaNs (voxels 10 .. 37 across, z from 42 on, in front of its clip plane), cut along z
NAN_PLANE = plane_through((0.0, 0.0, layer_centre(54)), (0.0, 0.0, 1.0))


def nan_ref():
    """the q scene of nonfinite.case("allnan_brick") (Q_NAN where the rendered volume holds NaN) on NAN_PLANE"""
    import nonfinite
    if "nan" not in _REFS:
        q = nonfinite.case("allnan_brick").mq
        _REFS["nan"] = render(q, NAN_PLANE, 0, tol=scenes.E0 * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0])))
    return _REFS["nan"]

# ---- the host build of the per-pixel code (tests/cpu_harness/slice_harness.cpp), built as iso_harness.cpp is ------------
GRID, TRILINEAR, UNIFORM = mip_scenes.GRID, mip_scenes.TRILINEAR, mip_scenes.UNIFORM
_H = {}


def harness_paths():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "cpu_harness", "slice_harness.cpp")
    deps = [src, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
        os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
    return here, src, deps


def _clang():
    """the clang++ beside hipcc: a host compiler that honours the contraction pragmas of vrc_core.h, as the device's does"""
    import os
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    root = os.path.dirname(os.path.dirname(hipcc))
    for c in (os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++"),
              "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(c):
            return c
    raise FileNotFoundError("no clang++ beside %s" % hipcc)


def harness(fused=False):
    """fused: the build that evaluates vrc_classify_mip as the device does -- clang++, whose VRC_FAST_FP contracts a
    product and a sum where the device's contracts them, fused multiply-add instructions, and VRC_LERP2 in the device's
    form -- for the comparison of frames bit for bit (tests/test_slice.py); everything under VRC_STRICT_FP is the same."""
    import ctypes as C
    import os
    import subprocess
    if fused not in _H:
        here, src, deps = harness_paths()
        out = os.path.join(here, "cpu_harness", "libslice_harness_fused.so" if fused else "libslice_harness.so")
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
            if fused:
                cmd = [_clang(), "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-DVRC_HOST_FUSED_LERP", "-o", tmp, src]
            else:
                cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", tmp, src]
            subprocess.check_call(cmd)
            os.replace(tmp, out)
        _H[fused] = C.CDLL(out)
    return _H[fused]


def harness_render(s, form, pl, passes=None, frac_bits=8, fused=False):
    """(frame, samples, values, counts, depths) of the host build; passes: [(a, b)] of s.nodes, meeting in the running
    state."""
    import ctypes as C
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    run = np.zeros((s.H, s.W), dtype=np.uint32)
    dep = np.full((s.H, s.W), np.nan, dtype=np.float32)
    values = np.zeros((s.H, s.W), dtype=np.float32)
    counts = np.zeros((s.H, s.W), dtype=np.uint32)
    pl = np.ascontiguousarray(pl, dtype=np.float32)
    total = 0
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness(fused).slice_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(fb.ctypes.data), C.c_void_p(run.ctypes.data),
            C.c_void_p(dep.ctypes.data), C.c_void_p(pl.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.byref(samples), C.c_void_p(values.ctypes.data),
            C.c_void_p(counts.ctypes.data))
        assert rc == 0, "slice_harness_render: %d" % rc
        total += int(samples.value)
    return fb, total, values, counts, dep
