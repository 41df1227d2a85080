"""Float64 references of the other folds of a MIP frame (include/vrc_hip.h, "The folds of a MIP frame"): the minimum and
the mean, with the acceptance rules of their frames and of the values vrc_get_projection_values returns.

TEST INFRASTRUCTURE.  Built on tests/mip_ref.py and tests/ref64.py (imported, neither is edited); it shares nothing with
libre_amd/csrc/vrc_core.h.

MINIMUM.  min over S of v = top - max over S of (top - v): mip_ref.render on a copy of the scene whose bricks are
complemented (255 - v, 65535 - v), certain values and candidates carried back as top - value.  A doubtful sample
matters where it could LOWER the certain minimum; the acceptance rule is mip_ref.check_frame itself, handed a result
whose comparisons are mirrored.  Same windows, same scenes.E0: no new constant.

MEAN.  The same geometry once more (mip_ref.render's, restated here because it keeps no per-sample values), summing
instead.  Float64 cannot say which way a float kernel decides a tie, so a pixel gets an INTERVAL [lo, hi] for the mean
and one for the count: every doubtful reading (a point sample within the contract's window of a voxel face) at its
smallest and at its largest, every doubtful sample (a grazed brick's, a barely-taken last or barely-not-taken next one)
both taken and not taken.  A pixel is SETTLED when lo = hi and its count is certain.  `_mutate` is for
tests/test_fold_cpu.py alone.

Acceptance of read-back values: settled pixels of integer point samples within 1 ulp of the float32 result (the sum is
exact, the quotient is rounded once); the float atlas and trilinear samples within scenes.E0 x (r1 - r0), the accuracy
the MIP rule already asks of every single trilinear sample (a frame within E0 of the classification of a value is a
value within E0 x the range where the transfer function has unit slope); unsettled pixels inside [lo, hi] widened by
the same amount; counts equal where certain, inside their interval elsewhere.  Acceptance of frames, every fold: a
pixel with a non-zero count is within scenes.E0 of mip_ref.classify64 of its READ-BACK value, a pixel with count 0
holds the cleared value.
"""
import copy

import numpy as np

import mip_ref
import mip_scenes
import orc
import scenes
from ref64 import DRIFT, EPSILON, EXACT_TIE, REL_WINDOW, _mat, _slab, _vec, node_ids  # noqa: F401

FOLD_MAX, FOLD_MIN, FOLD_MEAN = 0, 1, 2  # VRC_MIP_FOLD_*
_SCENES, _MEAN_REF, _MIN_REF = {}, {}, {}
MUTATIONS = mip_ref.MUTATIONS


# ---- minimum ------------------------------------------------------------------------------------------------------------
def top_of(s):
    """The value the complement turns about: the largest of the bricks' type."""
    dt = next(iter(s.bricks.values())).dtype
    assert dt in (np.uint8, np.uint16), dt
    return float(np.iinfo(dt).max)


def complemented(s):
    """A copy of the scene whose bricks hold top - v (what mip_ref.render reads; the atlas is not touched)."""
    c = copy.copy(s)
    top = np.iinfo(next(iter(s.bricks.values())).dtype).max
    c.bricks = {k: (top - b).astype(b.dtype) for k, b in s.bricks.items()}
    return c


def complemented_scene(name):
    """A renderable scene: mip_scenes' geometry of that name around the complement of its volume (top - v)."""
    key = (name, "volume complement")
    if key not in _SCENES:
        kw, dtype = dict(mip_scenes.SCENES[name]), "u8"
        if name == "skip":
            vol = mip_scenes.skip_volume(48)
        elif name == "skip16":
            vol, dtype = mip_scenes.skip_volume(48, np.uint16), "u16"
        else:
            assert kw["volume"] == "hash", name
            vol = orc.hash_volume(*kw["voxels"])
        kw["volume"] = (np.iinfo(vol.dtype).max - vol).astype(vol.dtype)
        _SCENES[key] = orc.build_scene(dtype=dtype, alpha=0.8, **kw)
    return _SCENES[key]


class MinResult:
    """mip_ref.Result read in a mirror: m the certain minimum (+inf without one), extra the doubtful values BELOW it."""

    def __init__(self, rc, top):
        self.certain, self.maybe = rc.certain, rc.maybe
        self.m = np.where(rc.certain, top - rc.m, np.inf)
        self.extra = {k: [top - v for v in vals] for k, vals in rc.extra.items()}
        self.counts, self.counts_lo, self.counts_hi = rc.counts, rc.counts_lo, rc.counts_hi

    def candidates(self, y, x):
        out = [self.m[y, x]] if self.certain[y, x] else []
        out += sorted(v for v in self.extra.get((y, x), ()) if v < self.m[y, x])
        return out

    def ambiguous(self):
        a = self.maybe & ~self.certain
        for (y, x), vals in self.extra.items():
            if any(v < self.m[y, x] for v in vals):
                a[y, x] = True
        return a

    def hit(self):
        return self.certain | self.maybe


def min_render(s, filter_mode=0, passes=None, _mutate=None):
    c = complemented(s)
    if passes is None:
        rc = mip_ref.render(c, filter_mode=filter_mode, _mutate=_mutate)
    else:
        rc = mip_ref.render_passes(c, passes, filter_mode=filter_mode)
    return MinResult(rc, top_of(s))


def check_min_frame(s, res, frame, frac_bits=8, cleared=0.0):
    """mip_ref.check_frame: the rule is the same, the comparisons are res's."""
    return mip_ref.check_frame(s, res, frame, frac_bits=frac_bits, cleared=cleared)


def check_candidates(res, values, counts, shift=0.0, tol=0.0):
    """Read-back values of the maximum or the minimum against a candidate set.  Returns the number of failing pixels."""
    bad = 0
    values, counts = np.asarray(values, dtype=np.float64) + shift, np.asarray(counts)
    for y in range(values.shape[0]):
        for x in range(values.shape[1]):
            if counts[y, x] == 0:
                bad += bool(res.certain[y, x])
                continue
            if not (res.certain[y, x] or res.maybe[y, x]) or counts[y, x] != 1:
                bad += 1
                continue
            cands = res.candidates(y, x)
            bad += not any(abs(values[y, x] - c) <= tol or values[y, x] == c for c in cands)
    return bad


# ---- mean ---------------------------------------------------------------------------------------------------------------
def face_matched_noise(n=48, block=16, seed=11):
    """uint8 noise in which the two voxel planes either side of every brick face are equal (plane 16 i - 1 := plane 16 i,
    axis by axis): the first sample of every brick segment lies on the brick's entry face, the contract calls which of
    the two voxels it reads a tie, and in noise that leaves every pixel's mean unsettled.  Here both readings agree."""
    rng = np.random.RandomState(seed)
    vol = rng.randint(0, 256, size=(n, n, n)).astype(np.uint8)  # (z, y, x)
    for axis in range(3):
        for i in range(1, n // block):
            sel = [slice(None)] * 3
            src = list(sel)
            sel[axis], src[axis] = block * i - 1, block * i
            vol[tuple(sel)] = vol[tuple(src)]
    return vol


MEAN_SCENES = ("spin", "inside", "clip", "count96", "count128")


def mean_scene(name, complement=False):
    """mip_scenes' geometry of that name around the face-matched noise volume (or its complement, 255 - v: the same
    slots, the same sample positions)."""
    key = (name, complement)
    if key not in _SCENES:
        kw = dict(mip_scenes.SCENES[name])
        n = kw["voxels"][0]
        vol = face_matched_noise(n, kw["block"])
        kw["volume"] = (np.uint8(255) - vol) if complement else vol
        _SCENES[key] = orc.build_scene(dtype="u8", alpha=0.8, **kw)
    return _SCENES[key]


class MeanResult:
    """Per pixel (H x W): sum_lo / sum_hi and n the sums (every doubtful reading at its smallest / largest) and number of
    the samples that are surely taken; doubt[(y, x)] the (smallest, largest) readings of the samples that may be taken
    or not.  finish() derives lo, hi (the interval of the mean; nan where no sample is certain or doubtful), count_lo,
    count_hi and settled."""

    def __init__(self, h, w):
        self.sum_lo = np.zeros((h, w))
        self.sum_hi = np.zeros((h, w))
        self.n = np.zeros((h, w), dtype=np.int64)
        self.doubt = {}

    def finish(self):
        h, w = self.n.shape
        self.count_lo = self.n.copy()
        self.count_hi = self.n.copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            self.lo = np.where(self.n > 0, self.sum_lo / self.n, np.nan)
            self.hi = np.where(self.n > 0, self.sum_hi / self.n, np.nan)
        for (y, x), d in self.doubt.items():
            self.count_hi[y, x] += len(d)
            # the smallest mean: take doubtful samples, smallest first, while they lower it (the largest: mirrored)
            for sign, which, out, total in ((1.0, 0, self.lo, self.sum_lo[y, x]), (-1.0, 1, self.hi, self.sum_hi[y, x])):
                t, k = sign * total, int(self.n[y, x])
                for v in sorted(sign * r[which] for r in d):
                    if k == 0 or v < t / k:
                        t, k = t + v, k + 1
                out[y, x] = sign * t / k
        self.settled = (self.lo == self.hi) & (self.count_lo == self.count_hi) & (self.n > 0)
        return self

    def hit(self):
        return self.count_hi > 0


def mean_render(s, filter_mode=0, prev=None, _mutate=None, _finish=True):
    """One pass over s.nodes[:s.n_nodes]; prev: the (unfinished) MeanResult of the passes before it."""
    assert _mutate is None or _mutate in MUTATIONS, _mutate
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

    res = MeanResult(s.H, s.W)
    if prev is not None:
        res.sum_lo, res.sum_hi, res.n = prev.sum_lo.copy(), prev.sum_hi.copy(), prev.n.copy()
        res.doubt = {k: list(v) for k, v in prev.doubt.items()}
    sum_lo, sum_hi, cnt = res.sum_lo.reshape(n), res.sum_hi.reshape(n), res.n.reshape(n)

    def doubt(pix, vlo, vhi):
        for p_, a_, b_ in zip(pix, vlo, vhi):
            res.doubt.setdefault((int(p_) // s.W, int(p_) % s.W), []).append((float(a_), float(b_)))

    def readings(brick, c, k, vpw):
        vlo, others = mip_ref._values(brick, c, k, vpw, filter_mode)
        vhi = vlo.copy()
        for mask, there in others:
            vhi = np.where(mask, np.maximum(vhi, there), vhi)
        return vlo, vhi

    done = ~alive
    ov = np.array([float(s.vi.overlap[a]) for a in range(3)])
    for i, nid in enumerate(node_ids(s)):
        if done.all() or (_mutate == "first_brick_only" and i > 0):
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
            vlo, vhi = readings(brick, coords(origin + d[g] * tn[g, None]), 0.0, vpw)
            doubt(g, vlo, vhi)
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
        vlo, vhi = readings(brick, coords(pos), kk[None, :], vpw)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)
        next_tie = (count > 0) & (dist - count * step > -end_eps)
        if _mutate == "drop_last_sample":
            count = count - 1
            last_tie[:] = False
            next_tie[:] = False
        kidx = np.arange(kk.size)[None, :]
        # a grazed brick that float64 calls hit: its sample(s) are doubtful all the same
        n_sure = np.where(graze[p], 0, count - last_tie)
        sure = kidx < n_sure[:, None]
        sum_lo[p] += np.where(sure, vlo, 0.0).sum(axis=1)
        sum_hi[p] += np.where(sure, vhi, 0.0).sum(axis=1)
        cnt[p] += n_sure
        n_doubt = np.where(graze[p], count, last_tie.astype(np.int64)) + next_tie
        for r in np.nonzero(n_doubt)[0]:
            ks = np.arange(n_sure[r], n_sure[r] + n_doubt[r])
            doubt([p[r]] * ks.size, vlo[r, ks], vhi[r, ks])
    return res.finish() if _finish else res


def mean_render_passes(s, passes, **kw):
    import nongrid
    r = None
    for t in nongrid.passes_of(s, passes):
        r = mean_render(t, prev=r, _finish=False, **kw)
    return r.finish()


def mean_ref(name, filter_mode=0):
    """mean_render of a MEAN scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode)
    if key not in _MEAN_REF:
        _MEAN_REF[key] = mean_render(mean_scene(name), filter_mode=filter_mode)
    return _MEAN_REF[key]


def min_ref(name, filter_mode=0, dtype="u8"):
    """min_render of a mip_scenes scene, computed once and shared."""
    key = (name, filter_mode, dtype)
    if key not in _MIN_REF:
        _MIN_REF[key] = min_render(mip_scenes.get(name, dtype), filter_mode=filter_mode)
    return _MIN_REF[key]


def value_tolerance(s, mean64, exact):
    """What a read-back mean may differ by: 1 ulp of the float32 result (exact: integer point samples), else E0 x range."""
    if exact:
        with np.errstate(invalid="ignore"):
            return np.spacing(np.abs(np.nan_to_num(mean64)).astype(np.float32)).astype(np.float64)
    r0, r1 = float(s.render.dataSourceRange[0]), float(s.render.dataSourceRange[1])
    return np.full(np.shape(mean64), scenes.E0 * (r1 - r0))


def check_mean_values(s, res, values, counts, exact, shift=0.0):
    """The acceptance rule of read-back means and counts.  shift: added to the values before they are compared (a signed
    volume read through its unsigned twin).  Returns (failing pixels, worst excess over the tolerance, settled pixels)."""
    values = np.asarray(values, dtype=np.float64) + shift
    counts = np.asarray(counts, dtype=np.int64)
    ok_count = (res.count_lo <= counts) & (counts <= res.count_hi)
    has = counts > 0
    lo, hi = np.nan_to_num(res.lo), np.nan_to_num(res.hi)
    tol = np.maximum(value_tolerance(s, lo, exact), value_tolerance(s, hi, exact))
    excess = np.maximum(lo - tol - values, values - (hi + tol))
    ok = ok_count & (~has | (excess <= 0.0))
    worst = float(excess[has & ok_count].max()) if (has & ok_count).any() else 0.0
    return int((~ok).sum()), max(worst, 0.0), int(res.settled.sum())


def check_frame_against_values(s, frame, values, counts, frac_bits=8, cleared=0.0, shift=0.0):
    """The frame rule of every fold: a pixel with samples is the classification of its read-back value, to E0; a pixel
    without holds the cleared value.  Returns (failing pixels, worst excess over E0)."""
    frame = np.asarray(frame, dtype=np.float64)
    counts = np.asarray(counts)
    v = np.where(counts > 0, np.asarray(values, dtype=np.float64) + shift, 0.0)
    err = np.abs(frame - mip_ref.classify64(s, v, frac_bits)).max(axis=-1)
    ok = np.where(counts > 0, err <= scenes.E0, np.all(frame == cleared, axis=-1))
    worst = float((err[counts > 0] - scenes.E0).max()) if (counts > 0).any() else 0.0
    return int((~ok).sum()), max(worst, 0.0)


def check_mean_frame(s, res, frame, exact, frac_bits=8, cleared=0.0):
    """The mean's rule for a frame that comes without a read-back (the plugin surface): every channel of a hit pixel lies
    within E0 of what mip_ref.classify64 makes of the interval [lo, hi], widened as read-back values are (17 points of
    it: the transfer functions of the tests move by less than E0 between two of them); a pixel that may be empty may be
    cleared, one that is empty must be.  Returns (failing pixels, worst excess over E0)."""
    frame = np.asarray(frame, dtype=np.float64)
    lo, hi = np.nan_to_num(res.lo), np.nan_to_num(res.hi)
    tol = np.maximum(value_tolerance(s, lo, exact), value_tolerance(s, hi, exact))
    w = np.linspace(0.0, 1.0, 17)[:, None, None]
    cls = mip_ref.classify64(s, (lo - tol)[None] * (1.0 - w) + (hi + tol)[None] * w, frac_bits)  # 17 x H x W x 4
    excess = np.maximum(cls.min(axis=0) - frame, frame - cls.max(axis=0)).max(axis=-1) - scenes.E0
    empty = np.all(frame == cleared, axis=-1)
    ok = np.where(res.count_lo > 0, excess <= 0.0, np.where(res.count_hi > 0, empty | (excess <= 0.0), empty))
    worst = float(excess[res.count_lo > 0].max()) if (res.count_lo > 0).any() else 0.0
    return int((~ok).sum()), max(worst, 0.0)


#: the scenes tests/test_fold_host.py renders through the plugin beside mip_scenes.HOST_MEM: the same volume through a taller
#: viewport (row bands), and mem:// at 128^3 in bricks of 32^3, whose 64 bricks of 40^3 voxels do not fit a pool of 1 MiB
BANDS_MEM = dict(mip_scenes.HOST_MEM, viewport=(48, 64))
PASSES_MEM = dict(voxels=(128, 128, 128), block=32, viewport=(40, 40), spin=(0.5, 0.35), alpha=0.8)


def band_rows(res, rows):
    """The reference of a pixel buffer that holds the given frame rows, in that order (sort-first row bands): a MinResult
    or a finished MeanResult cut to them."""
    rows = np.asarray(rows, dtype=np.int64)
    out = copy.copy(res)
    for name, a in vars(res).items():
        if isinstance(a, np.ndarray):
            setattr(out, name, a[rows])
    for name in ("extra", "doubt"):
        if hasattr(res, name):
            d = getattr(res, name)
            setattr(out, name, {(k, x): d[(int(y), x)] for k, y in enumerate(rows) for x in range(res.certain.shape[1] if hasattr(res, "certain") else res.n.shape[1]) if (int(y), x) in d})
    return out


def own_mean(res):
    """(values, counts) a renderer that agrees with float64 everywhere would read back: every doubt at its low end."""
    return np.where(res.count_lo > 0, np.nan_to_num(res.lo), 0.0).astype(np.float32), res.count_lo.copy()


# ---- the host build of every fold's per-ray code (tests/cpu_harness/fold_harness.cpp), built as mip_harness.cpp is ---------
_H = None


def harness():
    import ctypes as C
    import os
    import subprocess
    global _H
    if _H is None:
        here = os.path.dirname(os.path.abspath(__file__))
        src = os.path.join(here, "cpu_harness", "fold_harness.cpp")
        out = os.path.join(here, "cpu_harness", "libfold_harness.so")
        deps = [src, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
            os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, src])
            os.replace(tmp, out)
        _H = C.CDLL(out)
    return _H


def harness_render(s, form, fold, passes=None, frac_bits=8):
    """(frame, samples, values, counts) of the host build; passes: [(a, b)] of s.nodes, meeting in the running state."""
    import ctypes as C
    fb = np.zeros((s.H, s.W, 4), dtype=np.float32)
    run = np.zeros((s.H, s.W), dtype=np.uint32)
    msum = np.zeros((s.H, s.W), dtype=np.uint64)
    mcnt = np.zeros((s.H, s.W), dtype=np.uint32)
    values = np.zeros((s.H, s.W), dtype=np.float32)
    counts = np.zeros((s.H, s.W), dtype=np.uint32)
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    total = 0
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().fold_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(fb.ctypes.data), C.c_void_p(run.ctypes.data),
            C.c_void_p(msum.ctypes.data), C.c_void_p(mcnt.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(fold), C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.byref(samples),
            C.c_void_p(each.ctypes.data), C.c_void_p(values.ctypes.data), C.c_void_p(counts.ctypes.data))
        assert rc == 0, "fold_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        total += int(samples.value)
    return fb, total, values, counts
