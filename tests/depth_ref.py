"""A float64 restatement of the depth of a MIP frame (include/vrc_hip.h, "The depth of a MIP frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/mip_ref.py, tests/fold_ref.py and tests/ref64.py (imported, none is edited); it
shares nothing with libre_amd/csrc/vrc_core.h.

The sample set S of a ray is mip_ref.render's (its geometry is restated here because mip_ref keeps no positions): sample
k of a brick segment lies at t = tNear + k x step, in float64.  The ray's pair is (M, D): M the maximum (minimum) over S,
D the smallest t over the samples whose value equals M.

Float64 cannot say which way a float kernel decides a tie, so a pixel gets a finite set of CANDIDATE PAIRS (M, D).  A
sample's possible readings are mip_ref._values' (point samples within the contract's window of a voxel face may read
the voxel across it); doubtful samples are mip_ref's (a grazed brick's, a barely-taken last or barely-not-taken next
one): the same windows, no new numbers.  The certain maximum is the largest over the certain samples of their smallest
reading.  A pair (c, t) is a candidate when some sample at t could read c, c is not below the certain maximum, and no
certain sample before t reads c and nothing else.  Trilinear samples (compared to `tol`, the tolerance the value tests
use) cannot be called equal or not, so every sample within tol of the certain maximum gives a pair; point samples of a
float atlas are equal or not as their voxels are, and only the value is compared to tol.  A ray whose samples may all be NaN (nan_q: the stand-in the q scene holds for NaN, which loses
every comparison) has the pair (-inf, +inf).

The minimum is the maximum of the complemented scene (fold_ref.complemented), values carried back as top - value.

A pixel passes if its (value, depth) matches one candidate: the value as the value tests match it (exactly, or to tol),
the depth within step / 4 of the candidate's t -- a condition, not a measurement: a wrong sample index is off by a whole
step, float32 rounding of t by four orders of magnitude less.  Pixels with an empty S must read +infinity.

own() is the frame a renderer that agrees with float64 everywhere reads back; `mutate` gives deliberate misreadings of
it, for tests/test_depth_cpu.py alone.
"""
import copy

import numpy as np

import fold_ref
import mip_ref
import mip_scenes
import orc
import scenes
from ref64 import EPSILON, EXACT_TIE, REL_WINDOW, _mat, _slab, _vec, node_ids

FOLD_MAX, FOLD_MIN = fold_ref.FOLD_MAX, fold_ref.FOLD_MIN
MUTATIONS = ("last_tie", "segment_start", "off_by_one", "later_brick")


class Sample:
    __slots__ = ("t", "readings", "sure", "seg", "brick")

    def __init__(self, t, readings, sure, seg, brick):
        self.t, self.readings, self.sure, self.seg, self.brick = t, readings, sure, seg, brick


class Result:
    """Per pixel (H x W): certain[bool] S surely not empty; maybe[bool] S not empty only if a doubtful sample is taken;
    m the certain maximum in the scene's own values (fold MIN: minimum); cands[(y, x)] the candidate pairs (M, t);
    samples[(y, x)] the samples that could attain a candidate M, in the maximum's space (m_max: the certain maximum
    there; back(): to the scene's values)."""

    def __init__(self, h, w, step, fold, top):
        self.H, self.W, self.step, self.fold, self.top = h, w, step, fold, top
        self.certain = np.zeros((h, w), dtype=bool)
        self.maybe = np.zeros((h, w), dtype=bool)
        self.m_max = np.full((h, w), -np.inf)
        self.samples, self.cands = {}, {}

    def back(self, v):
        return self.top - v if self.fold == FOLD_MIN else v

    def hit(self):
        return self.certain | self.maybe

    def multi(self):
        """pixels with more than one candidate depth"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            ts = sorted({t for _, t in c})
            out[key] = any(b - a > 0.25 * self.step for a, b in zip(ts, ts[1:]))
        return out

    def own(self, mutate=None):
        """(values, counts, depths) of the certain pair of every pixel with a certain sample."""
        assert mutate is None or mutate in MUTATIONS, mutate
        values = np.zeros((self.H, self.W))
        counts = np.zeros((self.H, self.W), dtype=np.uint32)
        depths = np.full((self.H, self.W), np.inf)
        for y, x in zip(*np.nonzero(self.certain)):
            m = self.m_max[y, x]
            counts[y, x] = 1
            values[y, x] = self.back(m)
            ties = sorted((s for s in self.samples.get((y, x), ()) if s.sure and s.readings and min(s.readings) == m),
                          key=lambda s: s.t)
            if not ties:
                continue  # (every sample NaN: D = +infinity)
            first = ties[0]
            t = first.t
            if mutate == "last_tie":
                t = ties[-1].t
            elif mutate == "segment_start":
                t = first.seg
            elif mutate == "off_by_one":
                t = first.t + self.step
            elif mutate == "later_brick":
                later = [s for s in ties if s.brick != first.brick]
                t = later[0].t if later else t
            depths[y, x] = t
        return values, counts, depths


def _march(s, filter_mode, tol, nan_q, res):
    """mip_ref.render's geometry; fills res (in the maximum's space)."""
    view, rd = s.view, s.render
    step = 1.0 / float(rd.samplesPerRay)
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
    alive = tf_g - tn_g > EXACT_TIE * np.maximum(1.0, np.abs(tn_g))
    for plane in np.asarray(s.planes, dtype=np.float64).reshape(-1, 4):
        normal, dd = plane[:3], plane[3]
        rn = d @ normal
        rn = np.where(rn == 0.0, EPSILON, rn)
        t = -(normal @ origin + dd) / rn
        tn_g = np.where(rn > 0.0, np.maximum(tn_g, t), tn_g)
        tf_g = np.where(rn > 0.0, tf_g, np.minimum(tf_g, t))
    alive &= ~(tn_g > tf_g)
    res.origin, res.dir, res.tn_g, res.tf_g = origin, d.reshape(s.H, s.W, 3), tn_g.reshape(s.H, s.W), tf_g.reshape(s.H, s.W)

    certain, maybe, m = res.certain.reshape(n), res.maybe.reshape(n), res.m_max.reshape(n)

    def readings(brick, c, k, vpw):
        vlo, others = mip_ref._values(brick, c, k, vpw, filter_mode)
        r = [vlo] + [np.where(mask, there, np.nan) for mask, there in others]
        if nan_q is not None:
            r = [np.where(a == nan_q, -np.inf, a) for a in r]
        return r

    recs = []
    done = ~alive
    ov = np.array([float(s.vi.overlap[a]) for a in range(3)])
    for i, nid in enumerate(node_ids(s)):
        if done.all():
            break
        nd = s.nodes[i]
        lo, size = _vec(nd.aabbMin, 3), _vec(nd.aabbSize, 3)
        brick = s.bricks[nid]
        bs = np.array([float(s.lod[nid].blockSize[a]) for a in range(3)])
        vpw = bs / size
        tn, tf = _slab(origin, d, lo, lo + size)

        def coords(p):
            return ov + (p - lo) / size * bs

        win = REL_WINDOW * np.maximum(1.0, np.abs(tn))
        graze = (~done & (np.abs(tf - tn) <= win) & (tf >= tn_g - win) & (tn <= tf_g + win) & (tf >= t_near_plane - win))
        hit = ~done & (tf - tn > EXACT_TIE * np.maximum(1.0, np.abs(tn)))
        ended = hit & (tn > tf_g)
        done |= ended
        hit &= ~ended & ~(tf < tn_g)
        tn = np.maximum(np.maximum(t_near_plane, tn), tn_g)
        tf = np.minimum(tf, tf_g)
        hit &= ~(tn > tf)
        g = np.nonzero(graze & ~hit)[0]
        if g.size:  # one sample or none
            r = readings(brick, coords(origin + d[g] * tn[g, None])[:, None, :], 0.0, vpw)
            recs.append((i, g, tn[g], np.ones(g.size, dtype=np.int64), np.zeros(g.size, dtype=np.int64), r))
            maybe[g] = True
        p = np.nonzero(hit)[0]
        if p.size == 0:
            continue
        start = origin + d[p] * tn[p, None]
        diff = (origin + d[p] * tf[p, None]) - start
        dist = np.sqrt((diff * diff).sum(axis=1))
        ratio = dist / step
        whole = np.round(ratio)
        ratio = np.where(np.abs(ratio - whole) <= EXACT_TIE * np.maximum(1.0, whole), whole, ratio)
        count = np.where(dist > 0.0, np.ceil(ratio).astype(np.int64), 0)
        if count.max() == 0:
            continue
        unit = diff / np.where(dist > 0.0, dist, 1.0)[:, None]
        kk = np.arange(int(count.max()) + 1, dtype=np.float64)
        pos = start[:, None, :] + kk[None, :, None] * (unit * step)[:, None, :]
        r = readings(brick, coords(pos), kk[None, :], vpw)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)
        next_tie = (count > 0) & (dist - count * step > -end_eps)
        n_sure = np.where(graze[p], 0, count - last_tie)
        kidx = np.arange(kk.size)[None, :]
        sure = kidx < n_sure[:, None]
        seg_max = np.where(sure, r[0], -np.inf).max(axis=1)
        m[p] = np.where(n_sure > 0, np.fmax(m[p], seg_max), m[p])
        certain[p] |= n_sure > 0
        maybe[p[(count + next_tie) > n_sure]] = True
        recs.append((i, p, tn[p], count + next_tie, n_sure, r))

    for i, p, tn, taken, n_sure, r in recs:
        stack = np.stack(r)  # readings x P x K
        with np.errstate(invalid="ignore"):
            vhi = np.nanmax(np.where(np.isnan(stack), -np.inf, stack), axis=0)
        kidx = np.arange(stack.shape[2])[None, :]
        keep = (kidx < taken[:, None]) & (vhi >= m[p][:, None] - tol) & (vhi > -np.inf)
        for a, k in zip(*np.nonzero(keep)):
            vals = tuple(sorted({float(v) for v in stack[:, a, k] if v == v and v > -np.inf}))
            key = (int(p[a]) // s.W, int(p[a]) % s.W)
            res.samples.setdefault(key, []).append(Sample(float(tn[a]) + float(k) * step, vals, bool(k < n_sure[a]), float(tn[a]), i))


def render(s, fold=FOLD_MAX, filter_mode=0, tol=0.0, nan_q=None):
    """The candidate pairs of every pixel.  tol: 0 where values compare exactly (point samples of the integer atlases),
    else the value tests' tolerance.  nan_q: the value the scene's bricks hold where the rendered volume holds NaN."""
    assert fold in (FOLD_MAX, FOLD_MIN), fold
    top = 0.0
    if fold == FOLD_MIN:
        top = fold_ref.top_of(s)
        if nan_q is not None:  # a NaN loses every comparison: the largest value there is, whose complement is 0
            s = copy.copy(s)
            s.bricks = {k: np.where(b == nan_q, b.dtype.type(top), b).astype(b.dtype) for k, b in s.bricks.items()}
            nan_q = 0.0
        s = fold_ref.complemented(s)
    res = Result(s.H, s.W, 1.0 / float(s.render.samplesPerRay), fold, top)
    _march(s, filter_mode, tol, nan_q, res)
    exact = not filter_mode  # point samples: two samples are equal or not, whatever the value's image is compared to
    for key in zip(*np.nonzero(res.hit())):
        key = (int(key[0]), int(key[1]))
        m = res.m_max[key]
        smp = sorted(res.samples.get(key, ()), key=lambda q: q.t)
        first_certain = {}
        if exact:
            for q in smp:
                if q.sure and len(q.readings) == 1:
                    first_certain.setdefault(q.readings[0], q.t)
        pairs = set()
        for q in smp:
            for c in q.readings:
                if c >= m - tol and q.t <= first_certain.get(c, np.inf):
                    pairs.add((res.back(c), q.t))
        if m == -np.inf:  # no certain sample, or every certain one a NaN: the fold's identity, attained nowhere
            pairs.add((np.inf if fold == FOLD_MIN else -np.inf, np.inf))
        res.cands[key] = sorted(pairs)
    res.m = np.where(res.certain, res.back(res.m_max), np.nan)
    return res


def check(res, values, counts, depths, tol=0.0):
    """The acceptance rule.  values in the scene's own units (what res was rendered from).  Returns (failing pixels,
    worst depth error over the matched pixels in steps)."""
    values, counts, depths = np.asarray(values, dtype=np.float64), np.asarray(counts), np.asarray(depths, dtype=np.float64)
    bad, worst = 0, 0.0
    for y in range(res.H):
        for x in range(res.W):
            if counts[y, x] == 0:
                bad += bool(res.certain[y, x]) or not np.isposinf(depths[y, x])
                continue
            if not (res.certain[y, x] or res.maybe[y, x]) or counts[y, x] != 1:
                bad += 1
                continue
            v, t, best = values[y, x], depths[y, x], np.inf
            for c, ct in res.cands.get((y, x), ()):
                if not (v == c or abs(v - c) <= tol):
                    continue
                err = 0.0 if t == ct else abs(t - ct)  # (+infinity matches +infinity)
                best = min(best, err)
            if not best <= 0.25 * res.step:
                bad += 1
            else:
                worst = max(worst, best / res.step)
    return bad, worst


def multi_share(res):
    """The share of the hit pixels that have more than one candidate depth."""
    hit = int(res.hit().sum())
    return float(res.multi().sum()) / max(hit, 1)


def rays32(s):
    """The float32 rays of the host build: H x W x 8 -- tNearGlobal, tFarGlobal, origin, direction."""
    harness_render(s, 0, FOLD_MAX, depth=0)
    return harness_render.interval.copy()


def xyz32(depths, rays):
    """origin + D x dir in float32, the product and the sum each rounded, from read-back depths and rays32()."""
    d = np.asarray(depths, dtype=np.float32)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        return (rays[..., 2:5] + (d * rays[..., 5:8]).astype(np.float32)).astype(np.float32)


def cue_weight(depths, interval, strength):
    """w of the depth cue, in float32 and in the order the contract writes it, from read-back depths (H x W) and the
    rays' float32 intervals (H x W x 2 or more: tNearGlobal, tFarGlobal first)."""
    f = np.float32
    d = np.asarray(depths, dtype=f)
    tn, tf = np.asarray(interval[..., 0], dtype=f), np.asarray(interval[..., 1], dtype=f)
    span = (tf - tn).astype(f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = ((d - tn).astype(f) / span).astype(f)
    u = np.where(u > 0, u, f(0))
    u = np.where(u < 1, u, f(1)).astype(f)
    u = np.where(span > 0, u, f(0)).astype(f)
    return (f(1) - (f(strength) * u).astype(f)).astype(f)


# ---- the scenes of tests/test_depth_cpu.py and tests/test_depth.py, and their references, computed once ---------------------
#: the share of hit pixels that may have more than one candidate depth (the issue's condition; not to be raised: a scene
#: that exceeds it is replaced)
MULTI_CAP = 0.5
_SCENES, _REFS = {}, {}


def scene(name, filter_mode=0, fold=FOLD_MAX):
    """The scene of that name.  Replaced where the cap asks for it: trilinear samples of "axis" -- whose bricks are
    constant, so that every sample of a brick equals M up to rounding and every pixel has as many candidate depths as
    samples (share 1.0) -- take the axis view of the hash volume.  The minimum of "skip" / "skip16" takes the complemented
    volume, in which the minimum is what has something to skip."""
    if name == "axis" and filter_mode:
        key = ("axis", "hash")
        if key not in _SCENES:
            _SCENES[key] = orc.build_scene(dtype="u8", alpha=0.8, **dict(mip_scenes.SCENES["axis"], volume="hash"))
        return _SCENES[key]
    if name in ("skip", "skip16") and fold == FOLD_MIN:
        return fold_ref.complemented_scene(name)
    key = (name, None)
    if key not in _SCENES:
        _SCENES[key] = mip_scenes.get(name)
    return _SCENES[key]


def tolerance(s, filter_mode):
    """What a value may differ by: nothing for point samples of the integer atlases, else the value tests' E0 x range."""
    if not filter_mode and next(iter(s.bricks.values())).dtype != np.float32:
        return 0.0
    return scenes.E0 * (float(s.render.dataSourceRange[1]) - float(s.render.dataSourceRange[0]))


def ref(name, filter_mode, fold):
    """depth_ref.render of a scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode, fold)
    if key not in _REFS:
        s = scene(name, filter_mode, fold)
        _REFS[key] = render(s, fold=fold, filter_mode=filter_mode, tol=tolerance(s, filter_mode))
    return _REFS[key]


def two_blocks(complement=False):
    """The known answer: "axis" geometry, 64^3 in bricks of 16^3, zero but for two 4 x 4 x 4 blocks of one value on the
    same rays (the view looks along z) in different bricks."""
    key = ("two blocks", complement)
    if key not in _SCENES:
        vol = np.zeros((64, 64, 64), dtype=np.uint8)  # (z, y, x)
        for z0 in NEAR_FAR_Z:
            vol[z0:z0 + 4, BLOCK_XY:BLOCK_XY + 4, BLOCK_XY:BLOCK_XY + 4] = BLOCK_VALUE
        if complement:
            vol = np.uint8(255) - vol
        _SCENES[key] = orc.build_scene(dtype="u8", alpha=0.8, **dict(mip_scenes.SCENES["axis"], volume=vol))
    return _SCENES[key]


NEAR_FAR_Z = (50, 10)
BLOCK_VALUE = 200
BLOCK_XY = 28  # next to the axis: the view is a perspective, and rays farther out leave a 4-voxel column between the blocks


# ---- the host build of the depth-tracking per-ray code (tests/cpu_harness/depth_harness.cpp), built as fold_harness is ---
_H = None


def harness():
    import ctypes as C
    import os
    import subprocess
    global _H
    if _H is None:
        here = os.path.dirname(os.path.abspath(__file__))
        src = os.path.join(here, "cpu_harness", "depth_harness.cpp")
        out = os.path.join(here, "cpu_harness", "libdepth_harness.so")
        deps = [src, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, src])
            os.replace(tmp, out)
        _H = C.CDLL(out)
    return _H


def harness_render(s, form, fold, depth=1, cue=0, passes=None, frac_bits=8):
    """(frame, samples, values, counts, depths, xyz) of the host build; passes: [(a, b)] of s.nodes, meeting in the running
    state; depth = 0: the instances without depth tracking (depths and xyz are then None)."""
    import ctypes as C
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    run = np.zeros((s.H, s.W), dtype=np.uint32)
    dep = np.full((s.H, s.W), np.nan, dtype=np.float32)
    xyz = np.full((s.H, s.W, 3), np.nan, dtype=np.float32)
    interval = np.zeros((s.H, s.W, 8), dtype=np.float32)
    values = np.zeros((s.H, s.W), dtype=np.float32)
    counts = np.zeros((s.H, s.W), dtype=np.uint32)
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    total = 0
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().depth_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(fb.ctypes.data), C.c_void_p(run.ctypes.data),
            C.c_void_p(dep.ctypes.data), C.c_int(depth), C.c_int(cue), C.c_void_p(xyz.ctypes.data), C.c_void_p(interval.ctypes.data),
            C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(fold), C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.byref(samples),
            C.c_void_p(each.ctypes.data), C.c_void_p(values.ctypes.data), C.c_void_p(counts.ctypes.data))
        assert rc == 0, "depth_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        total += int(samples.value)
    harness_render.interval = interval  # (of the last call: what tests/test_depth_cpu.py recomputes the cue from)
    return fb, total, values, counts, (dep if depth else None), (xyz if depth else None)
