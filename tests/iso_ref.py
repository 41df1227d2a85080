"""A float64 restatement of an isosurface frame (include/vrc_hip.h, "An isosurface frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py, tests/mip_ref.py and tests/depth_ref.py (imported, none is edited); it
shares nothing with libre_amd/csrc/vrc_core.h.

The sample set S of a ray is mip_ref.render's, with depth_ref's positions: sample k of a brick segment lies at
t = tNear + k x step, in float64.  A sample hits when its value is >= iso; the ray's answer is the hit of the smallest t:
its value V, its depth D = t, and the gradient G of the voxel it was read from -- central differences of the brick's
voxels, indices clamped, times the brick's voxels per world unit.

Float64 cannot say which way a float kernel decides a tie, so a pixel gets a finite set of CANDIDATES: "miss", or
(V, t, G).  A sample's possible readings are mip_ref._values' (a point sample within the contract's window of a voxel
face may read the voxel across it -- here each reading keeps the voxel it comes from; a trilinear sample that close to a
face keeps its value and may take either voxel's gradient); doubtful samples are mip_ref's (a grazed brick's, a
barely-taken last or barely-not-taken next one): the same windows, no new numbers.  A sample at t with a reading
c >= iso - tol is a candidate, with the gradient of the voxel that reading comes from, unless a certain sample before t
(by more than ref64.REL_WINDOW, which is how close two bricks' samples can lie without float32 telling them apart) has
all its readings >= iso + tol.  "Miss" is a candidate unless some certain sample surely hits.  tol is 0 for point samples
of integer atlases, else depth_ref.tolerance.

A pixel with count 0 passes if "miss" is a candidate and D is +infinity.  A pixel with count 1 passes if one candidate
matches all three: V exactly or to tol; D within step / 4 (depth_ref's condition: a wrong index is off by a whole step);
every component of G within 1e-5 x the candidate's largest |component| (integer differences are exact; the margin covers
the one float32 multiply), a NaN component where the candidate's is NaN.

own() is what a renderer that agrees with float64 everywhere reads back; `mutate` gives deliberate misreadings of it,
for tests/test_iso_cpu.py alone.
"""
import numpy as np

import depth_ref
import mip_scenes
import orc
from ref64 import DRIFT, EPSILON, EXACT_TIE, REL_WINDOW, _Ctx, _mat, _nearest, _slab, _trilinear, _vec, node_ids

MUTATIONS = ("last_crossing", "segment_start", "off_by_one", "later_brick", "gradient_negated", "gradient_neighbour")
G_REL = 1e-5
#: the share of all pixels for which both "miss" and a hit may be candidates (the issue's condition; not to be raised)
BOTH_CAP = 0.1
MULTI_CAP = depth_ref.MULTI_CAP


class Cand:
    __slots__ = ("v", "t", "g", "sure", "primary", "seg", "brick", "idx")

    def __init__(self, v, t, g, sure, primary, seg, brick, idx):
        self.v, self.t, self.g, self.sure, self.primary, self.seg, self.brick, self.idx = v, t, g, sure, primary, seg, brick, idx


class Result:
    """Per pixel (H x W): t_sure the depth of the first certain sample that surely hits (+inf without one: "miss" is a
    candidate); t_last the last such; cands[(y, x)] the candidates; later[(y, x)] the first sure hit of every brick."""

    def __init__(self, s, iso, step):
        self.s, self.H, self.W, self.iso, self.step = s, s.H, s.W, iso, step
        self.t_sure = np.full((s.H, s.W), np.inf)
        self.t_last = np.full((s.H, s.W), -np.inf)
        self.cands, self.later = {}, {}

    def miss(self):
        return np.isposinf(self.t_sure)

    def hit(self):
        """pixels with a hit among their candidates"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            out[key] = bool(c)
        return out

    def multi(self):
        """pixels with more than one candidate depth"""
        out = np.zeros((self.H, self.W), dtype=bool)
        for key, c in self.cands.items():
            ts = sorted({q.t for q in c})
            out[key] = any(b - a > 0.25 * self.step for a, b in zip(ts, ts[1:]))
        return out

    def shares(self):
        """(share of the hit pixels with more than one candidate depth, share of all pixels with "miss" and a hit)"""
        hit = self.hit()
        return (float(self.multi().sum()) / max(int(hit.sum()), 1), float((hit & self.miss()).sum()) / float(self.H * self.W))

    def own(self, mutate=None):
        """(values, counts, depths, gradients) of the certain answer of every pixel that has one."""
        assert mutate is None or mutate in MUTATIONS, mutate
        values = np.zeros((self.H, self.W))
        counts = np.zeros((self.H, self.W), dtype=np.uint32)
        depths = np.full((self.H, self.W), np.inf)
        grads = np.zeros((self.H, self.W, 3))
        for y, x in zip(*np.nonzero(~self.miss())):
            mine = [q for q in self.cands[(y, x)] if q.sure and q.primary and q.t == self.t_sure[y, x]]
            q = mine[0]
            v, t, g = q.v, q.t, np.array(q.g)
            if mutate == "last_crossing":
                t = self.t_last[y, x]
            elif mutate == "segment_start":
                t = q.seg
            elif mutate == "off_by_one":
                t = q.t + self.step
            elif mutate == "later_brick":
                other = [tt for b, tt in self.later[(y, x)].items() if b != q.brick]
                t = min(other) if other else t
            elif mutate == "gradient_negated":
                a = int(np.nanargmax(np.abs(g))) if np.isfinite(g).any() else 0
                g[a] = -g[a]
            elif mutate == "gradient_neighbour":
                brick, vpw = self._brick(q.brick)
                g = _gradient(brick, [np.array([min(q.idx[0] + 1, brick.shape[2] - 1)]), np.array([q.idx[1]]),
                                      np.array([q.idx[2]])], vpw, None)[0]
            counts[y, x], values[y, x], depths[y, x], grads[y, x] = 1, v, t, g
        return values, counts, depths, grads

    def _brick(self, i):
        s = self.s
        nid = node_ids(s)[i]
        size = _vec(s.nodes[i].aabbSize, 3)
        bs = np.array([float(s.lod[nid].blockSize[a]) for a in range(3)])
        return s.bricks[nid], bs / size


def _gradient(brick, idx, vpw, nan_q):
    """central differences of the brick's voxels at idx = [x, y, z] arrays, indices clamped, times voxels per world unit"""
    dims = brick.shape[::-1]
    b = brick.astype(np.float64)
    if nan_q is not None:
        b = np.where(b == nan_q, np.nan, b)
    out = np.zeros((len(idx[0]), 3))
    for a in range(3):
        hi = [np.clip(idx[c] + (1 if c == a else 0), 0, dims[c] - 1) for c in range(3)]
        lo = [np.clip(idx[c] - (1 if c == a else 0), 0, dims[c] - 1) for c in range(3)]
        out[:, a] = (b[hi[2], hi[1], hi[0]] - b[lo[2], lo[1], lo[0]]) * vpw[a]
    return out


def _readings(brick, c, k, vpw, filter_mode):
    """mip_ref._values with the voxel of every reading: [(mask, value, [x, y, z])], the first the sample's own."""
    v, idx = _nearest(brick, c)
    v = v.astype(np.float64)
    if filter_mode:
        cx = _Ctx()
        cx.mutate = None
        v = _trilinear(cx, brick, c)
    dims = brick.shape[::-1]
    off = []
    for a in range(3):
        fr = c[..., a] - np.floor(c[..., a])
        delta = orc.TIE_DELTA + k * DRIFT * vpw[a]
        off.append(np.where(fr < delta, -1, 0) + np.where(fr > 1.0 - delta, 1, 0))
    out = [(np.ones(v.shape, dtype=bool), v, idx)]
    if not ((off[0] != 0) | (off[1] != 0) | (off[2] != 0)).any():
        return out
    for m in range(1, 8):
        use = [(m >> a) & 1 for a in range(3)]
        valid = np.ones(v.shape, dtype=bool)
        for a in range(3):
            if use[a]:
                valid &= off[a] != 0
        if not valid.any():
            continue
        q = [np.clip(idx[a] + use[a] * off[a], 0, dims[a] - 1) for a in range(3)]
        there = v if filter_mode else brick[q[2], q[1], q[0]].astype(np.float64)
        out.append((valid, there, q))
    return out


def render(s, iso, filter_mode=0, tol=0.0, nan_q=None):
    """The candidates of every pixel.  iso in the scene's own values; nan_q: the value the scene's bricks hold where the
    rendered volume holds NaN (such a sample never hits, such a tap makes a NaN component)."""
    view, rd = s.view, s.render
    step = 1.0 / float(rd.samplesPerRay)
    res = Result(s, iso, step)
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
    res.origin, res.dir = origin, d.reshape(s.H, s.W, 3)

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
            r = _readings(brick, coords(origin + d[g] * tn[g, None])[:, None, :], 0.0, vpw, filter_mode)
            recs.append((i, g, tn[g], np.ones(g.size, dtype=np.int64), np.zeros(g.size, dtype=np.int64), r, brick, vpw))
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
        r = _readings(brick, coords(pos), kk[None, :], vpw, filter_mode)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)
        next_tie = (count > 0) & (dist - count * step > -end_eps)
        n_sure = np.where(graze[p], 0, count - last_tie)
        recs.append((i, p, tn[p], count + next_tie, n_sure, r, brick, vpw))

    def hits(val):
        return np.where(val == nan_q, -np.inf, val) if nan_q is not None else val

    t_sure, t_last = res.t_sure.reshape(n), res.t_last.reshape(n)
    per_brick = []
    for i, p, tn, taken, n_sure, r, brick, vpw in recs:
        kidx = np.arange(r[0][1].shape[1])[None, :]
        t = tn[:, None] + kidx * step
        vmin = hits(r[0][1]).copy()
        for mask, val, _ in r[1:]:
            vmin = np.where(mask, np.minimum(vmin, hits(val)), vmin)
        sure = (kidx < n_sure[:, None]) & (vmin >= iso + tol)
        first = np.where(sure, t, np.inf).min(axis=1)
        t_sure[p] = np.minimum(t_sure[p], first)
        t_last[p] = np.maximum(t_last[p], np.where(sure, t, -np.inf).max(axis=1))
        per_brick.append((i, p, first, sure))
    for i, p, first, _ in per_brick:
        for a in np.nonzero(np.isfinite(first))[0]:
            key = (int(p[a]) // s.W, int(p[a]) % s.W)
            at = res.later.setdefault(key, {})
            at[i] = min(at.get(i, np.inf), float(first[a]))
    for key in zip(*np.nonzero(np.ones((s.H, s.W), dtype=bool))):
        res.cands[(int(key[0]), int(key[1]))] = []
    for (i, p, tn, taken, n_sure, r, brick, vpw), (_, _, _, sure) in zip(recs, per_brick):
        kidx = np.arange(r[0][1].shape[1])[None, :]
        t = tn[:, None] + kidx * step
        limit = t_sure[p] + REL_WINDOW * np.maximum(1.0, np.abs(t_sure[p]))
        for which, (mask, val, idx) in enumerate(r):
            cand = mask & (kidx < taken[:, None]) & (hits(val) >= iso - tol) & (t <= limit[:, None])
            a, k = np.nonzero(cand)
            if a.size == 0:
                continue
            at = [np.broadcast_to(idx[c], cand.shape)[a, k] for c in range(3)]
            g = _gradient(brick, at, vpw, nan_q)
            vv = np.broadcast_to(val, cand.shape)[a, k]
            for j in range(a.size):
                key = (int(p[a[j]]) // s.W, int(p[a[j]]) % s.W)
                res.cands[key].append(Cand(float(vv[j]), float(t[a[j], k[j]]), tuple(g[j]), bool(sure[a[j], k[j]]),
                                           which == 0, float(tn[a[j]]), i, (int(at[0][j]), int(at[1][j]), int(at[2][j]))))
    return res


def check(res, values, counts, depths, grads, tol=0.0):
    """The acceptance rule.  values in the scene's own units.  Returns (failing pixels, worst depth error over the matched
    pixels in steps)."""
    values, counts = np.asarray(values, dtype=np.float64), np.asarray(counts)
    depths, grads = np.asarray(depths, dtype=np.float64), np.asarray(grads, dtype=np.float64)
    miss = res.miss()
    bad, worst = 0, 0.0
    for y in range(res.H):
        for x in range(res.W):
            if counts[y, x] == 0:
                bad += (not miss[y, x]) or not np.isposinf(depths[y, x]) or bool(np.any(grads[y, x] != 0.0))
                continue
            if counts[y, x] != 1:
                bad += 1
                continue
            v, t, g, best = values[y, x], depths[y, x], grads[y, x], np.inf
            for q in res.cands[(y, x)]:
                if not (v == q.v or abs(v - q.v) <= tol) or not abs(t - q.t) <= 0.25 * res.step:
                    continue
                want = np.array(q.g)
                fin = np.isfinite(want)
                top = float(np.abs(want[fin]).max()) if fin.any() else 0.0
                if np.array_equal(np.isnan(g), ~fin) and (np.abs(g[fin] - want[fin]) <= G_REL * top).all():
                    best = min(best, abs(t - q.t))
            if not best <= 0.25 * res.step:
                bad += 1
            else:
                worst = max(worst, best / res.step)
    return bad, worst


def shade32(grads, dirs, ambient):
    """s of the contract in float32, in the order written, from read-back G (H x W x 3) and float32 ray directions."""
    f = np.float32
    g, d, amb = np.asarray(grads, dtype=f), np.asarray(dirs, dtype=f), f(ambient)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sq = (g * g).astype(f)
        ln = np.sqrt(((sq[..., 0] + sq[..., 1]).astype(f) + sq[..., 2]).astype(f)).astype(f)
        pr = (g * d).astype(f)
        dot = np.abs(((pr[..., 0] + pr[..., 1]).astype(f) + pr[..., 2]).astype(f))
        sh = (amb + (((f(1) - amb) * dot).astype(f) / ln).astype(f)).astype(f)
    return np.where((ln > 0) & np.isfinite(ln), sh, f(1)).astype(f)


# ---- the scenes and isovalues of tests/test_iso_cpu.py and tests/test_iso.py, and their references, computed once -------
#: the isovalue of every scene the GPU tests render (tests/test_iso_cpu.py asserts the caps and the pixel counts for each)
ISO = {"axis": 150.0, "spin": 150.0, "inside": 150.0, "clip": 150.0, "skip": 100.0, "skip16": 25700.0, "two blocks": 200.0}
_REFS, _SCENES = {}, {}
#: "two blocks" is depth_ref.two_blocks with blocks wide enough across the view for a hundred pixels to hit them (its
#: own are 4 x 4 voxels, nine pixels): 28 x 28 voxels, still 4 thick, in the same two z ranges, crossing brick borders
BLOCK_LO, BLOCK_HI = 18, 46


def two_blocks():
    if "two blocks" not in _SCENES:
        vol = np.zeros((64, 64, 64), dtype=np.uint8)  # (z, y, x)
        for z0 in depth_ref.NEAR_FAR_Z:
            vol[z0:z0 + 4, BLOCK_LO:BLOCK_HI, BLOCK_LO:BLOCK_HI] = depth_ref.BLOCK_VALUE
        _SCENES["two blocks"] = orc.build_scene(dtype="u8", alpha=0.8, **dict(mip_scenes.SCENES["axis"], volume=vol))
    return _SCENES["two blocks"]


def scene(name, filter_mode=0):
    """"axis" is the axis view of the hash volume (depth_ref's trilinear one) for both filters."""
    if name == "two blocks":
        return two_blocks()
    return depth_ref.scene(name, 1 if name == "axis" else 0)


def tolerance(s, filter_mode):
    return depth_ref.tolerance(s, filter_mode)


def ref(name, filter_mode):
    key = (name, filter_mode)
    if key not in _REFS:
        s = scene(name, filter_mode)
        _REFS[key] = render(s, ISO[name], filter_mode=filter_mode, tol=tolerance(s, filter_mode))
    return _REFS[key]


# the typed scenes of mip_scenes.typed (uint16 voxels q behind every image v = a + b q), the NaN brick and the nucleon
TYPED_ISO_Q = {"uint16": 37000.0, "int16": 32700.0, "float": 37000.0}
NAN_ISO_Q = 37000.0
NUCLEON_ISO = 100.0


def typed_iso(image):
    """(the isovalue in q, the isovalue of the rendered volume: a + b q, a negative one for int16)"""
    import voxel_types
    q = TYPED_ISO_Q[image]
    if image == "uint16":
        return q, q
    im = voxel_types.IMAGES[image]
    return q, float(np.float32(im.a + im.b * q))


def typed_tolerance(image, filter_mode):
    q = mip_scenes.typed(image)[0]
    if not filter_mode and image != "float":
        return 0.0
    return scenes_e0() * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))


def scenes_e0():
    import scenes
    return scenes.E0


def typed_ref(image, filter_mode):
    key = ("typed", image, filter_mode)
    if key not in _REFS:
        _REFS[key] = render(mip_scenes.typed(image)[0], TYPED_ISO_Q[image], filter_mode=filter_mode,
                            tol=typed_tolerance(image, filter_mode))
    return _REFS[key]


def nan_ref():
    import nonfinite
    if "nan" not in _REFS:
        q = nonfinite.case("allnan_brick").mq
        tol = scenes_e0() * (float(q.render.dataSourceRange[1]) - float(q.render.dataSourceRange[0]))
        _REFS["nan"] = render(q, NAN_ISO_Q, tol=tol, nan_q=nonfinite.Q_NAN)
    return _REFS["nan"]


def nucleon_scene():
    import scenes
    if "nucleon" not in _SCENES:
        _SCENES["nucleon"] = scenes.nucleon_scene(viewport=(44, 36), alpha=0.8)
    return _SCENES["nucleon"]


def nucleon_ref():
    if "nucleon" not in _REFS:
        _REFS["nucleon"] = render(nucleon_scene(), NUCLEON_ISO)
    return _REFS["nucleon"]


# ---- the host build of the per-ray code (tests/cpu_harness/iso_harness.cpp), built as depth_harness.cpp is --------------
GRID, FIXED, TRILINEAR, SKIP, UNIFORM = mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.TRILINEAR, mip_scenes.SKIP, mip_scenes.UNIFORM
_H = None


def harness():
    import ctypes as C
    import os
    import subprocess
    global _H
    if _H is None:
        here = os.path.dirname(os.path.abspath(__file__))
        src = os.path.join(here, "cpu_harness", "iso_harness.cpp")
        out = os.path.join(here, "cpu_harness", "libiso_harness.so")
        deps = [src, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, src])
            os.replace(tmp, out)
        _H = C.CDLL(out)
    return _H


def harness_render(s, form, iso, ambient=0.25, passes=None, frac_bits=8):
    """(frame, samples, values, counts, depths, gradients) of the host build; passes: [(a, b)] of s.nodes, meeting in the
    running state.  harness_render.rays: H x W x 8 -- tNearGlobal, tFarGlobal, origin, direction in float32."""
    import ctypes as C
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    run = np.zeros((s.H, s.W), dtype=np.uint32)
    dep = np.full((s.H, s.W), np.nan, dtype=np.float32)
    grad = np.full((s.H, s.W, 3), np.nan, dtype=np.float32)
    rays = np.zeros((s.H, s.W, 8), dtype=np.float32)
    values = np.zeros((s.H, s.W), dtype=np.float32)
    counts = np.zeros((s.H, s.W), dtype=np.uint32)
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    total = 0
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().iso_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(fb.ctypes.data), C.c_void_p(run.ctypes.data),
            C.c_void_p(dep.ctypes.data), C.c_void_p(grad.ctypes.data), C.c_float(iso), C.c_float(ambient),
            C.c_void_p(rays.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.byref(samples),
            C.c_void_p(each.ctypes.data), C.c_void_p(values.ctypes.data), C.c_void_p(counts.ctypes.data))
        assert rc == 0, "iso_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        total += int(samples.value)
    harness_render.rays = rays
    return fb, total, values, counts, dep, grad
