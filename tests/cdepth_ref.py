"""A float64 restatement of the depth of a composite frame (include/vrc_hip.h, "The depth of a composite frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py, tests/mip_ref.py and tests/shade_ref.py (imported, none is edited); it
shares nothing with libre_amd/csrc/vrc_core.h.

render() is ref64.render's march, statement for statement -- its own copy of the loop, because it needs the running
alpha -- and beside the frame it keeps, per pixel, where the alpha crosses tau.  Float64 cannot say which sample a float
kernel crosses at, so a pixel gets a WINDOW of candidate samples, built as ref64 builds the window around the early exit,
with tau in place of 0.999: with eps = scenes.E0 + scenes.TIE_FACTOR x (the running budget), the window opens at the first
sample with A64 > tau - eps and closes at the first with A64 >= tau + eps, both included.  While the window is open (or
would open with them) mip_ref's doubtful samples are candidates too: the one sample of a grazed brick and the
barely-not-taken next sample of a segment; a barely-taken last sample is a sample of the loop anyway.  A candidate is
(t, readings): t = tNear + k x step in float64, readings = the values the sample can come out as (mip_ref._values: a point
sample within the contract's window of a voxel face may read the voxel across it).

A pixel passes (check) when
  * its window never opened and it reads D = +infinity, count 0;
  * or it reads a finite D within step / 4 of a candidate's t -- a condition, not a measurement: a wrong index is off by
    a whole step -- with a V that matches one of that candidate's readings, exactly or to tol, and count 1;
  * or its window opened, never closed, and it reads +infinity, count 0.
A pixel whose window closed must read a finite D.

own() is the read-back of a renderer that agrees with float64 everywhere: the first sample with A64 >= tau; `mutate` gives
deliberate misreadings of it, for tests/test_cdepth_cpu.py alone.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import mip_ref
import mip_scenes
import nongrid
import orc
import scenes
import shade_ref
from depth_ref import tolerance  # noqa: F401  (what a read-back value may differ by)
from ref64 import (EARLY_EXIT, EPSILON, EXACT_TIE, REL_WINDOW, _Ctx, _classify, _face_ties, _mat, _sample, _slab, _vec,
                   node_ids)

MUTATIONS = ("off_by_one", "before_composite", "segment_start", "first_opaque", "later_pass")
MAX_WINDOW = 4      # a cap, not a measurement: no window may be longer (in samples)
MAX_MULTI = 0.15    # a cap: the share of a rule test's crossing pixels with more than one candidate


class Result:
    """frame, samples, budget, counts: ref64's.  Per pixel: opened / closed[H, W] bool; cands[(y, x)] = [(t, readings)];
    own_t / own_v / own_hit: the first sample with A64 >= tau (own_seg: its segment's tNear; own_first: the first sample
    with alpha' > 0; own_before: the first sample with A64 >= tau BEFORE it is added -- for the mutations)."""

    def __init__(self, h, w, step, tau):
        self.H, self.W, self.step, self.tau = h, w, step, tau
        self.opened = np.zeros((h, w), dtype=bool)
        self.closed = np.zeros((h, w), dtype=bool)
        self.cands = {}
        self.own_hit = np.zeros((h, w), dtype=bool)
        self.own_t = np.full((h, w), np.inf)
        self.own_v = np.zeros((h, w))
        self.own_seg = np.full((h, w), np.inf)
        self.own_first = np.full((h, w), np.inf)
        self.own_before = np.full((h, w), np.inf)
        self.frame = self.budget = self.counts = None
        self.samples = 0

    def windows(self):
        """candidates per pixel, counted as distinct depths (two readings of one sample are one depth)"""
        out = np.zeros((self.H, self.W), dtype=np.int64)
        for key, c in self.cands.items():
            ts = sorted(t for t, _ in c)
            out[key] = (1 + sum(1 for a, b in zip(ts, ts[1:]) if b - a > 0.25 * self.step)) if ts else 0
        return out

    def multi_share(self):
        """the share of the crossing pixels (window opened) with more than one candidate depth"""
        return float((self.windows() > 1).sum()) / max(int(self.opened.sum()), 1)

    def longest(self):
        return int(self.windows().max()) if self.cands else 0

    def own(self, mutate=None, earlier=None):
        """(values, counts, depths) of the read-back.  earlier: the Result of the passes before this one, for `later_pass`."""
        assert mutate is None or mutate in MUTATIONS, mutate
        t = self.own_t.copy()
        if mutate == "off_by_one":
            t = t + self.step
        elif mutate == "before_composite":
            t = np.where(self.own_hit, self.own_before, t)
        elif mutate == "segment_start":
            t = np.where(self.own_hit, self.own_seg, t)
        elif mutate == "first_opaque":
            t = np.where(self.own_hit, self.own_first, t)
        elif mutate == "later_pass":
            assert earlier is not None
            t = np.where(earlier.own_hit & np.isfinite(self.last_t), self.last_t, t)
        return self.own_v.copy(), self.own_hit.astype(np.uint32), np.where(self.own_hit, t, np.inf)


def _add(res, key, t, readings):
    res.cands.setdefault(key, []).append((float(t), tuple(sorted({float(v) for v in readings if v == v}))))


def render(s, tau, fb=None, budget=None, frac_bits=8, filter_mode=0, prev=None):
    """One pass over s.nodes[:s.n_nodes].  prev: the Result of the passes before (its frame and budget come in as fb /
    budget do in ref64; a pixel whose window closed there keeps its candidates and takes no new ones; one whose window
    opened there and did not close goes on collecting)."""
    assert s.render.samplesPerPixel == 1
    tau = float(np.float32(tau))
    view, rd = s.view, s.render
    cx = _Ctx()
    cx.mutate, cx.frac_bits, cx.filter_mode = None, int(frac_bits), int(filter_mode)
    cx.tf = np.asarray(s.tf, dtype=np.float64).reshape(256, 4)
    r0, r1 = float(rd.dataSourceRange[0]), float(rd.dataSourceRange[1])
    cx.mult, cx.add = 1.0 / (r1 - r0), -r0 / (r1 - r0)
    spr = float(rd.samplesPerRay)
    cx.corr = float(rd.maxSamplesPerRay) / spr
    cx.alpha_max = 255.0 / 256.0
    step = 1.0 / spr
    some_brick = next(iter(s.bricks.values()))
    if not filter_mode:
        cx.table = _classify(cx, np.arange(256 if some_brick.dtype.itemsize == 1 else 65536, dtype=np.float64))
    if prev is not None:
        fb, budget = prev.frame, prev.budget

    # ---- rays (cuda/Renderer.cu:40-51, :106-122)
    h, w = s.H, s.W
    py, px = [g.reshape(-1).astype(np.float64) for g in np.meshgrid(np.arange(h), np.arange(w), indexing="ij")]
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

    # ---- global box and clip planes (:124-149)
    tn_g, tf_g = _slab(origin, d, _vec(view.aabbMin, 3), _vec(view.aabbMax, 3))
    alive = tf_g - tn_g > EXACT_TIE * np.maximum(1.0, np.abs(tn_g))
    for plane in np.asarray(s.planes, dtype=np.float64).reshape(-1, 4):
        normal, dd = plane[:3], plane[3]
        rn = d @ normal
        rn = np.where(rn == 0.0, EPSILON, rn)
        t = -(normal @ origin + dd) / rn
        lower = rn > 0.0
        tn_g = np.where(lower, np.maximum(tn_g, t), tn_g)
        tf_g = np.where(lower, tf_g, np.minimum(tf_g, t))
    alive &= ~(tn_g > tf_g)

    col = np.zeros((n, 4)) if fb is None else np.asarray(fb, dtype=np.float64).reshape(n, 4).copy()
    bud = np.zeros(n) if budget is None else np.asarray(budget, dtype=np.float64).reshape(n).copy()
    alive &= ~(col[:, 3] > EARLY_EXIT)  # :151-155

    res = Result(h, w, step, tau)
    res.origin, res.dir = origin, d.reshape(h, w, 3)
    opened, closed = res.opened.reshape(n), res.closed.reshape(n)
    own_hit, own_t, own_v = res.own_hit.reshape(n), res.own_t.reshape(n), res.own_v.reshape(n)
    own_seg, own_first, own_before = res.own_seg.reshape(n), res.own_first.reshape(n), res.own_before.reshape(n)
    res.last_t = np.full((h, w), np.inf)   # (`later_pass`: the first crossing-or-later sample of THIS pass)
    last_t = res.last_t.reshape(n)
    if prev is not None:
        opened[:], closed[:] = prev.opened.reshape(n), prev.closed.reshape(n)
        own_hit[:], own_t[:], own_v[:] = prev.own_hit.reshape(n), prev.own_t.reshape(n), prev.own_v.reshape(n)
        own_seg[:], own_first[:], own_before[:] = prev.own_seg.reshape(n), prev.own_first.reshape(n), prev.own_before.reshape(n)
        res.cands = {k: list(v) for k, v in prev.cands.items()}

    def values(brick, c, k, vpw):
        vlo, others = mip_ref._values(brick, c, k, vpw, filter_mode)
        return [vlo] + [np.where(mask, there, np.nan) for mask, there in others]

    def eps_of(b):
        return scenes.E0 + scenes.TIE_FACTOR * b

    done = ~alive
    shadow = np.zeros(n, dtype=bool)
    sh_a = np.zeros(n)
    ert_lo = np.full(n, -1.0)
    ert_eps = np.zeros(n)
    counts = np.zeros(n, dtype=np.int64)
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

        # budget, part 2: a brick the ray grazes gets one sample, or none -- a doubtful sample of the window
        graze = (~done & ~shadow & (np.abs(tf - tn) <= REL_WINDOW * np.maximum(1.0, np.abs(tn))) &
                 (tf >= tn_g) & (tn <= tf_g) & (tf >= t_near_plane))
        if graze.any():
            g = np.nonzero(graze)[0]
            tg = np.maximum(np.maximum(t_near_plane[g], tn[g]), tn_g[g])
            cg = coords(origin + d[g] * tn[g, None])
            cls, _, _ = _sample(cx, brick, cg)
            bud[g] += cls.max(axis=-1) * (1.0 - col[g, 3])
            would = col[g, 3] + cls[:, 3] * (1.0 - col[g, 3])
            take = ~closed[g] & (opened[g] | (would > tau - eps_of(bud[g])))
            if take.any():
                r = values(brick, cg[:, None, :], 0.0, vpw)
                for a in np.nonzero(take)[0]:
                    _add(res, (int(g[a]) // w, int(g[a]) % w), tg[a], [q[a, 0] for q in r])
                opened[g[take]] = True

        hit = ~done & (tf - tn > EXACT_TIE * np.maximum(1.0, np.abs(tn)))   # :180-181
        ended = hit & (tn > tf_g)            # :183-184
        done |= ended
        hit &= ~ended & ~(tf < tn_g)         # :186-187
        tn = np.maximum(np.maximum(t_near_plane, tn), tn_g)   # :189-190
        tf = np.minimum(tf, tf_g)
        hit &= ~(tn > tf)                    # :192-193
        p = np.nonzero(hit)[0]
        if p.size == 0:
            continue

        # ---- the samples of this brick, for all its rays at once (:195-216)
        start = origin + d[p] * tn[p, None]
        diff = (origin + d[p] * tf[p, None]) - start
        dist = np.sqrt((diff * diff).sum(axis=1))
        ratio = dist / step
        whole = np.round(ratio)
        ratio = np.where(np.abs(ratio - whole) <= EXACT_TIE * np.maximum(1.0, whole), whole, ratio)
        count = np.ceil(ratio).astype(np.int64)
        count = np.where(dist > 0.0, count, 0)
        if count.max() == 0:
            continue
        unit = diff / np.where(dist > 0.0, dist, 1.0)[:, None]
        kk = np.arange(int(count.max()) + 1, dtype=np.float64)   # one more: the sample that was barely not taken
        pos = start[:, None, :] + kk[None, :, None] * (unit * step)[:, None, :]
        cc = coords(pos)
        cls, idx, c = _sample(cx, brick, cc)
        reads = values(brick, cc, kk[None, :], vpw)
        own_val = reads[0] if filter_mode else brick[idx[2], idx[1], idx[0]].astype(np.float64)
        heavy = cls.max(axis=-1)
        ties = None if filter_mode else _face_ties(cx, brick, c, idx, cls, kk[None, :], vpw)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)   # barely taken
        next_tie = (count > 0) & (dist - count * step > -end_eps)          # barely not

        # ---- front to back, sample by sample (:208-226)
        c_col, c_bud = col[p], bud[p]
        c_done, c_shadow, c_sha = done[p], shadow[p], sh_a[p]
        c_lo, c_eps, c_n = ert_lo[p], ert_eps[p], counts[p]
        c_open, c_closed = opened[p], closed[p]
        c_hit, c_t, c_v = own_hit[p], own_t[p], own_v[p]
        c_seg, c_first, c_before, c_last = own_seg[p], own_first[p], own_before[p], last_t[p]

        def candidates(sel, k):
            for a in np.nonzero(sel)[0]:
                _add(res, (int(p[a]) // w, int(p[a]) % w), tn[p[a]] + k * step, [q[a, k] for q in reads])

        for k in range(kk.size):
            normal = ~c_done & ~c_shadow
            extra = normal & (count == k) & next_tie
            if extra.any():
                c_bud[extra] += heavy[extra, k] * (1.0 - c_col[extra, 3])
                would = c_col[:, 3] + cls[:, k, 3] * (1.0 - c_col[:, 3])
                take = extra & ~c_closed & (c_open | (would > tau - eps_of(c_bud)))
                candidates(take, k)
                c_open |= take
            act = ~c_done & (k < count)
            if not act.any():
                break
            normal &= act
            trans = 1.0 - c_col[:, 3]
            if ties is not None:
                c_bud += np.where(normal, ties[:, k] * trans, 0.0)
            if k > 0:
                c_bud += np.where(normal & last_tie & (count == k + 1), heavy[:, k] * trans, 0.0)
            a_before = np.where(c_shadow, c_sha, c_col[:, 3])
            c_col += np.where(normal[:, None], cls[:, k, :] * trans[:, None], 0.0)   # :83-93
            c_n += normal
            follow = act & c_shadow
            c_sha = np.where(follow, c_sha + cls[:, k, 3] * (1.0 - c_sha), c_sha)
            acc = np.where(c_shadow, c_sha, c_col[:, 3])
            # ---- the crossing: the window of candidates, and the read-back of a renderer that agrees with float64
            eps = eps_of(c_bud)
            c_open |= act & ~c_closed & (acc > tau - eps)
            inside = act & c_open & ~c_closed
            candidates(inside, k)
            c_closed |= inside & (acc >= tau + eps)
            tk = tn[p] + k * step
            c_first = np.where(normal & (cls[:, k, 3] > 0.0) & ~np.isfinite(c_first), tk, c_first)
            c_before = np.where(normal & (a_before >= tau) & ~np.isfinite(c_before), tk, c_before)
            c_last = np.where(normal & (acc >= tau) & ~np.isfinite(c_last), tk, c_last)
            cross = normal & ~c_hit & (acc >= tau)
            c_t, c_v, c_seg = np.where(cross, tk, c_t), np.where(cross, own_val[:, k], c_v), np.where(cross, tn[p], c_seg)
            c_hit |= cross
            # budget, part 4: the window around the early exit
            unset = act & (c_lo < 0.0)
            c_eps = np.where(unset, scenes.E0 + scenes.TIE_FACTOR * c_bud, c_eps)
            c_lo = np.where(unset & (acc > EARLY_EXIT - c_eps), acc, c_lo)
            c_done |= follow & (c_sha > EARLY_EXIT + c_eps)
            leave = normal & (c_col[:, 3] > EARLY_EXIT)                              # :219-226
            stay = leave & (c_col[:, 3] <= EARLY_EXIT + c_eps)
            c_sha = np.where(stay, c_col[:, 3], c_sha)
            c_shadow |= stay
            c_done |= leave & ~stay
        col[p], bud[p] = c_col, c_bud
        done[p], shadow[p], sh_a[p] = c_done, c_shadow, c_sha
        ert_lo[p], ert_eps[p], counts[p] = c_lo, c_eps, c_n
        opened[p], closed[p] = c_open, c_closed
        own_hit[p], own_t[p], own_v[p] = c_hit, c_t, c_v
        own_seg[p], own_first[p], own_before[p], last_t[p] = c_seg, c_first, c_before, c_last

    acc = np.where(shadow, sh_a, col[:, 3])
    bud += np.where(ert_lo >= 0.0, np.maximum(0.0, acc - ert_lo), 0.0)
    res.frame, res.samples, res.budget, res.counts = col.reshape(h, w, 4), int(counts.sum()), bud.reshape(h, w), counts.reshape(h, w)
    return res


def table_alpha(s, value, frac_bits=8):
    """alpha' of a point sample of this value, in float64 (ref64._classify)"""
    cx = _Ctx()
    cx.mutate, cx.frac_bits, cx.filter_mode = None, int(frac_bits), 0
    cx.tf = np.asarray(s.tf, dtype=np.float64).reshape(256, 4)
    r0, r1 = float(s.render.dataSourceRange[0]), float(s.render.dataSourceRange[1])
    cx.mult, cx.add = 1.0 / (r1 - r0), -r0 / (r1 - r0)
    cx.corr = float(s.render.maxSamplesPerRay) / float(s.render.samplesPerRay)
    cx.alpha_max = 255.0 / 256.0
    return float(_classify(cx, np.array([float(value)]))[0, 3])


def render_passes(s, tau, passes, **kw):
    """The list rendered in passes [(a, b)] of its nodes into one buffer; the Result after every pass."""
    out, prev = [], None
    for t in nongrid.passes_of(s, passes):
        prev = render(t, tau, prev=prev, **kw)
        out.append(prev)
    return out


def check(res, values, counts, depths, tol=0.0):
    """The acceptance rule.  values in the units res was rendered from.  Returns (failing pixels, worst depth error over
    the matched pixels in steps)."""
    values, counts, depths = np.asarray(values, dtype=np.float64), np.asarray(counts), np.asarray(depths, dtype=np.float64)
    bad, worst = 0, 0.0
    for y in range(res.H):
        for x in range(res.W):
            t = depths[y, x]
            if counts[y, x] == 0 or not np.isfinite(t):
                # never crossed: allowed where the window did not close; the pair must say so both ways
                bad += bool(res.closed[y, x]) or counts[y, x] != 0 or not np.isposinf(t)
                continue
            if not res.opened[y, x] or counts[y, x] != 1:
                bad += 1
                continue
            v, best = values[y, x], np.inf
            for ct, readings in res.cands.get((y, x), ()):
                if any(v == c or abs(v - c) <= tol for c in readings):
                    best = min(best, abs(t - ct))
            if not best <= 0.25 * res.step:
                bad += 1
            else:
                worst = max(worst, best / res.step)
    return bad, worst


# ---- the scenes of tests/test_cdepth_cpu.py, tests/test_cdepth.py and tests/test_cdepth_host.py, and their references ---
RULE_SCENES = ("axis", "spin", "inside", "clip")
RULE_TAUS = (100, 500)
IDENTITY_TAUS = (1, 100, 500, 900, 999)
_REFS = {}


def tau_of(k):
    """tau as the contract forms it: one rounded float32 division"""
    return np.float32(k) / np.float32(1000)


def scene(name):
    return shade_ref.scene(name)


def rule_cases():
    """(scene, filter, thousandths) of the rule tests: shade_ref's scenes under both filters and the nucleon under the
    trilinear one, at tau 0.1 and 0.5"""
    out = [(name, f, k) for name in RULE_SCENES for f in (0, 1) for k in RULE_TAUS]
    return out + [("nucleon", 1, k) for k in RULE_TAUS]


def ref(name, filter_mode, k):
    """cdepth_ref's Result of a scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode, k)
    if key not in _REFS:
        _REFS[key] = render(scene(name), tau_of(k), filter_mode=filter_mode)
    return _REFS[key]


def typed_ref(image, filter_mode, k):
    """of the uint16 scene q behind a typed image v = a + b q"""
    key = ("typed", image, filter_mode, k)
    if key not in _REFS:
        _REFS[key] = render(mip_scenes.typed(image)[0], tau_of(k), filter_mode=filter_mode)
    return _REFS[key]


def assert_rule(res, values, counts, depths, what, tol=0.0):
    bad, worst = check(res, values, counts, depths, tol=tol)
    print("%s: %d crossing pixels (window opened), %.1f %% with more than one candidate, longest window %d; %d failing, worst "
          "depth error %.3g steps" % (what, int(res.opened.sum()), 100.0 * res.multi_share(), res.longest(), bad, worst))
    assert bad == 0, "%s: %d pixels outside the rule" % (what, bad)


# ---- the host build of the per-ray code (tests/cpu_harness/cdepth_harness.cpp), built as shade_harness.cpp is ------------
GRID, FIXED, TRILINEAR, UNIFORM = mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.TRILINEAR, mip_scenes.UNIFORM
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "cdepth_harness.cpp")
DEPS = [SRC, os.path.join(orc.ROOT, "include", "vrc_hip.h")] + [
    os.path.join(orc.ROOT, "libre_amd", "csrc", f) for f in ("vrc_core.h", "vrc_tables.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_H = None


def build(out, extra):
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = "%s.%d.tmp" % (out, os.getpid())  # several test workers may build at once: rename is atomic
        subprocess.check_call(["g++", "-O2"] + FLAGS + extra + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def harness():
    global _H
    if _H is None:
        _H = C.CDLL(build(os.path.join(HERE, "cpu_harness", "libcdepth_harness.so"), ["-fPIC", "-shared"]))
    return _H


class Host:
    """frame, samples, samples per pixel; depths, values, counts: the read-backs (values in the atlas's stored units);
    after[k]: (frame, depths) after pass k; rays[H, W, 3]"""

    def __init__(self, s):
        self.frame = np.zeros((s.H, s.W, 4), dtype=np.float32)
        self.samples = 0
        self.each = np.zeros((s.H, s.W), dtype=np.int64)
        self.depths = np.full((s.H, s.W), np.inf, dtype=np.float32)
        self.bits = np.full((s.H, s.W), 0xFFFFFFFF, dtype=np.uint32)
        self.values = np.zeros((s.H, s.W), dtype=np.float32)
        self.counts = np.zeros((s.H, s.W), dtype=np.uint32)
        self.rays = np.zeros((s.H, s.W, 3), dtype=np.float32)
        self.after = []


def harness_render(s, form, k=500, passes=None, frac_bits=8):
    """the host build's frame and read-backs; k: VRC_OPT_COMPOSITE_DEPTH (0: the plain frame); passes: [(a, b)] of
    s.nodes, accumulating in one buffer"""
    out = Host(s)
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for j, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().cdepth_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(out.frame.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(frac_bits), C.c_int(1 if j == 0 else 0), C.c_int(k), C.byref(samples), C.c_void_p(each.ctypes.data),
            C.c_void_p(out.depths.ctypes.data), C.c_void_p(out.bits.ctypes.data), C.c_void_p(out.values.ctypes.data),
            C.c_void_p(out.counts.ctypes.data), C.c_void_p(out.rays.ctypes.data))
        assert rc == 0, "cdepth_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        out.samples += int(samples.value)
        out.each += each
        out.after.append((out.frame.copy(), out.depths.copy()))
    return out
