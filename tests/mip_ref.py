"""A float64 restatement of the maximum-intensity projection (include/vrc_hip.h, "A MIP frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py's reading of the reference's geometry (its helpers are imported, the
module is not edited); it shares nothing with libre_amd/csrc/vrc_core.h.

The sample set S of a ray is what ref64.render composites with an all-transparent transfer function: the same ray,
interval, node list order (a brick whose tNear lies beyond the interval ends the ray), restart per brick and
ceil(dist x samplesPerRay) samples per segment, and no early termination.  M is the largest sampled density, the pixel
one classification of M without opacity correction, premultiplied.

Float64 cannot say which way a float kernel decides a tie, so a pixel gets a finite CANDIDATE SET for M instead of
one value: the maximum over the samples that are certain, plus every larger value a doubtful sample could contribute.
Doubtful, by the windows of the parity contract (tests/scenes.py; orc.TIE_DELTA with drift and ref64.REL_WINDOW --
no new numbers):
  * point sampling: a sample within delta_k of a voxel face may read the voxel across it (every combination at an
    edge or corner); the smallest of its possible values is certain, the others are doubtful;
  * the single sample of a brick the ray grazes;
  * the last sample of a segment where dist is within the window of a whole number of steps: barely taken (doubtful)
    or barely not taken (the next one is doubtful).
A frame passes where some candidate's classification lies within scenes.E0 of the pixel on all four channels; pixels
with an empty S must hold the cleared value; pixels whose S is empty or not depending on a doubtful sample are
ambiguous (either outcome passes) and are counted.

`_mutate` is for tests/test_mip_cpu.py alone: deliberate misreadings, to show that the comparison has teeth.
"""
import numpy as np

import orc
import scenes
from ref64 import DRIFT, EPSILON, EXACT_TIE, REL_WINDOW, _Ctx, _mat, _nearest, _slab, _tf_fetch, _trilinear, _vec, node_ids

MUTATIONS = ("drop_last_sample", "first_brick_only")


class Result:
    """Per pixel (H x W): certain[bool] S surely not empty; maybe[bool] S not empty only if a doubtful sample is taken;
    m[float] the certain maximum (-inf without one); extra[y][x] list of doubtful values above it; counts the certain
    |S| and counts_hi the |S| with every doubtful sample taken (counts_lo: with none)."""

    def __init__(self, h, w):
        self.certain = np.zeros((h, w), dtype=bool)
        self.maybe = np.zeros((h, w), dtype=bool)
        self.m = np.full((h, w), -np.inf)
        self.extra = {}
        self.counts = np.zeros((h, w), dtype=np.int64)
        self.counts_lo = np.zeros((h, w), dtype=np.int64)
        self.counts_hi = np.zeros((h, w), dtype=np.int64)

    def candidates(self, y, x):
        out = [self.m[y, x]] if self.certain[y, x] else []
        out += sorted(v for v in self.extra.get((y, x), ()) if v > self.m[y, x])
        return out

    def ambiguous(self):
        """pixels with more than one acceptable outcome"""
        a = self.maybe & ~self.certain
        for (y, x), vals in self.extra.items():
            if any(v > self.m[y, x] for v in vals):
                a[y, x] = True
        return a

    def hit(self):
        return self.certain | self.maybe


def _classifier(s, frac_bits):
    cx = _Ctx()
    cx.mutate, cx.frac_bits = None, int(frac_bits)
    cx.tf = np.asarray(s.tf, dtype=np.float64).reshape(256, 4)
    r0, r1 = float(s.render.dataSourceRange[0]), float(s.render.dataSourceRange[1])
    cx.mult, cx.add = 1.0 / (r1 - r0), -r0 / (r1 - r0)
    return cx


def classify64(s, m, frac_bits=8):
    """The pixel of a maximum m: TF((m - r0) / (r1 - r0)), premultiplied; no opacity correction, no 255/256 clamp."""
    cx = _classifier(s, frac_bits)
    m = np.asarray(m, dtype=np.float64)
    t = _tf_fetch(cx, m * cx.mult + cx.add)
    out = t * t[..., 3:4]
    out[..., 3] = t[..., 3]
    return out


def _values(brick, c, k, vpw, filter_mode):
    """Per sample: the smallest value it can come out as, and the list of (mask, value) of the larger ones."""
    if filter_mode:
        cx = _Ctx()
        cx.mutate = None
        return _trilinear(cx, brick, c), []
    v, idx = _nearest(brick, c)
    v = v.astype(np.float64)
    dims = brick.shape[::-1]
    off = []
    for a in range(3):
        fr = c[..., a] - np.floor(c[..., a])
        delta = orc.TIE_DELTA + k * DRIFT * vpw[a]
        off.append(np.where(fr < delta, -1, 0) + np.where(fr > 1.0 - delta, 1, 0))
    lo, others = v.copy(), []
    if not ((off[0] != 0) | (off[1] != 0) | (off[2] != 0)).any():
        return lo, others
    for m in range(1, 8):
        use = [(m >> a) & 1 for a in range(3)]
        valid = np.ones(v.shape, dtype=bool)
        for a in range(3):
            if use[a]:
                valid &= off[a] != 0
        if not valid.any():
            continue
        q = [np.clip(idx[a] + use[a] * off[a], 0, dims[a] - 1) for a in range(3)]
        there = brick[q[2], q[1], q[0]].astype(np.float64)
        others.append((valid, there))
        lo = np.where(valid, np.minimum(lo, there), lo)
    others.append((np.ones(v.shape, dtype=bool), v))
    return lo, others


def render(s, filter_mode=0, prev=None, _mutate=None, trace=None):
    """One pass over s.nodes[:s.n_nodes]; prev: the Result of the passes before it (the running maximum).

    trace: a list that receives, per brick of the list that some ray meets and in list order, what every such ray takes
    from it (tests/skip_window.py predicts the sample count with skipping from that): a dict of `node` (the index in
    the list), `rays` (flat pixel indices) and, per ray, `tn` (the entry distance), `c_lo` / `c_hi` (the samples it
    surely takes / takes with every doubtful one) and the largest and smallest value among them as intervals --
    `max_lo` (over the certain samples at their smallest reading, -inf without one) <= `max_hi` (over every possible
    sample at its largest reading), `min_lo` <= `min_hi` likewise; `samples`: (smallest reading, largest reading, certain?, possible?), each rays x
    samples in march order (absent for a grazed brick's one doubtful sample).  Nothing else changes."""
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

    res = Result(s.H, s.W)
    if prev is not None:
        res.certain, res.maybe, res.m = prev.certain.copy(), prev.maybe.copy(), prev.m.copy()
        res.extra = {k: list(v) for k, v in prev.extra.items()}
        res.counts, res.counts_lo, res.counts_hi = prev.counts.copy(), prev.counts_lo.copy(), prev.counts_hi.copy()
    certain, maybe, m = res.certain.reshape(n), res.maybe.reshape(n), res.m.reshape(n)
    counts, c_lo, c_hi = res.counts.reshape(n), res.counts_lo.reshape(n), res.counts_hi.reshape(n)

    def doubt(pix, vals):
        for p_, v_ in zip(pix, vals):
            res.extra.setdefault((int(p_) // s.W, int(p_) % s.W), []).append(float(v_))

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

        # (a brick touched exactly where the ray leaves the interval -- an edge of the volume on a brick face -- is grazed
        # too: which side of the interval's end its tNear falls on is decided by the last bit, so the window applies)
        win = REL_WINDOW * np.maximum(1.0, np.abs(tn))
        graze = (~done & (np.abs(tf - tn) <= win) & (tf >= tn_g - win) & (tn <= tf_g + win) & (tf >= t_near_plane - win))
        hit = ~done & (tf - tn > EXACT_TIE * np.maximum(1.0, np.abs(tn)))
        ended = hit & (tn > tf_g)
        done |= ended
        hit &= ~ended & ~(tf < tn_g)
        tn = np.maximum(np.maximum(t_near_plane, tn), tn_g)
        tf = np.minimum(tf, tf_g)
        hit &= ~(tn > tf)
        if graze.any():
            # one sample or none: if the march below takes it, it is counted there as certain -- a difference of
            # nothing for the candidates (doubtful values below the certain maximum are dropped)
            g = np.nonzero(graze)[0]
            vlo, others = _values(brick, coords(origin + d[g] * tn[g, None]), 0.0, vpw, filter_mode)
            doubt(g, vlo)
            for mask, there in others:
                doubt(g[mask], there[mask])
            maybe[g] = True
            c_hi[g] += np.where(hit[g], 0, 1)
            if trace is not None and (~hit[g]).any():  # one sample or none, of any of its readings
                ghi, only = vlo.copy(), ~hit[g]
                for mask, there in others:
                    ghi = np.where(mask, np.maximum(ghi, there), ghi)
                zero = np.zeros(int(only.sum()), dtype=np.int64)
                trace.append(dict(node=i, rays=g[only], tn=tn[g][only], c_lo=zero, c_hi=zero + 1,
                                  max_lo=zero - np.inf, max_hi=ghi[only], min_lo=vlo[only], min_hi=zero + np.inf))
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
        vlo, others = _values(brick, coords(pos), kk[None, :], vpw, filter_mode)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)
        next_tie = (count > 0) & (dist - count * step > -end_eps)
        if _mutate == "drop_last_sample":
            count = count - 1
            last_tie[:] = False
            next_tie[:] = False
        kidx = np.arange(kk.size)[None, :]
        # a grazed brick that float64 calls hit: its sample(s) are doubtful all the same (noted above)
        n_sure = np.where(graze[p], 0, count - last_tie)
        sure = kidx < n_sure[:, None]
        seg_max = np.where(sure, vlo, -np.inf).max(axis=1)
        has = n_sure > 0
        m[p] = np.where(has, np.fmax(m[p], seg_max), m[p])  # (fmax: a NaN sample drops out)
        certain[p] |= has
        counts[p] += count
        c_lo[p] += n_sure
        c_hi[p] += count + next_tie
        if trace is not None:
            vhi = vlo.copy()
            for mask, there in others:
                vhi = np.where(mask, np.maximum(vhi, there), vhi)
            poss = kidx < (count + next_tie)[:, None]
            trace.append(dict(node=i, rays=p, tn=tn[p], c_lo=n_sure, c_hi=count + next_tie,
                              max_lo=np.where(sure, vlo, -np.inf).max(axis=1), max_hi=np.where(poss, vhi, -np.inf).max(axis=1),
                              min_lo=np.where(poss, vlo, np.inf).min(axis=1), min_hi=np.where(sure, vhi, np.inf).min(axis=1),
                              samples=(vlo, vhi, sure, poss)))
        # doubtful: the larger readings of samples near faces, the barely-taken last and barely-not-taken next sample
        for mask, there in others:
            sel = np.nonzero(mask & (kidx < count[:, None]))
            doubt(p[sel[0]], there[sel])
        for tie, at in ((last_tie, count - 1), (next_tie, count)):
            r = np.nonzero(tie)[0]
            if r.size:
                doubt(p[r], vlo[r, at[r]])
                for mask, there in others:
                    q = r[mask[r, at[r]]]
                    doubt(p[q], there[q, at[q]])
                maybe[p[r]] = True
    # doubtful values that cannot beat the certain maximum say nothing
    for key in list(res.extra):
        keep = sorted({v for v in res.extra[key] if not res.certain[key] or v > res.m[key]})
        if keep:
            res.extra[key] = keep
        else:
            del res.extra[key]
    return res


def render_passes(s, passes, **kw):
    import nongrid
    r = None
    for t in nongrid.passes_of(s, passes):
        r = render(t, prev=r, **kw)
    return r


def check_frame(s, res, frame, frac_bits=8, cleared=0.0):
    """The acceptance rule.  Returns (number of failing pixels, worst excess over E0, number of ambiguous pixels)."""
    frame = np.asarray(frame, dtype=np.float64)
    bad, worst = 0, 0.0
    base = classify64(s, np.where(res.certain, res.m, 0.0), frac_bits)
    err = np.abs(frame - base).max(axis=-1)
    ok = res.certain & (err <= scenes.E0)
    empty_ok = np.all(frame == cleared, axis=-1)
    ok |= ~res.certain & empty_ok  # S empty, or empty-or-not ambiguous: the cleared value passes
    for y, x in zip(*np.nonzero(~ok)):
        cands = res.candidates(y, x)
        best = np.inf
        if cands:
            best = float(np.abs(classify64(s, np.array(cands), frac_bits) - frame[y, x]).max(axis=-1).min())
        if not res.certain[y, x] and not res.maybe[y, x]:
            best = np.inf  # S is empty: only the cleared value passes, and it did not
        if best > scenes.E0:
            bad += 1
            worst = max(worst, best - scenes.E0 if np.isfinite(best) else 1.0)
    return bad, worst, int(res.ambiguous().sum())
