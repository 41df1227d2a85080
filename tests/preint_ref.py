"""A float64 restatement of a pre-integrated composite frame (include/vrc_hip.h, "A pre-integrated composite frame"), in
NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py (its helpers are imported, nothing there is edited); it shares nothing with
libre_amd/csrc/vrc_core.h.

table() is the contract's table by a quadrature of its own: every texel interval (and every partial one at the ends of a
value-indexed step) is split where TF_alpha crosses 255/256, every part is cut into 16 equal sub-pieces and each of those
integrated with a 32-point Gauss-Legendre rule (the logarithm's singularity lies outside every sub-piece by more than a
sixteenth of its length: the rule is exact to rounding there); an entry is the plain sum of its pieces, added up from
its own lower end.  No closed form, no difference of prefix sums: not the builder's method.

render() is ref64.render's march, statement for statement, with two changes:
  * what sample k of a brick visit adds is E(d_{k-1}, d_k) from the float64 table (E(d_0, d_0) for the visit's first
    sample): the value-indexed table read exactly for point samples of 8-bit voxels, the texel-indexed one read
    bilinearly, in float64, at the two clamped texel coordinates for everything else;
  * the tie budget follows ref64's parts, extended where pairing couples neighbours.  Part 1 (point samples within
    delta_k of a voxel face): the change of BOTH entries the sample enters when it reads the voxel across the face -- its
    own, E(d_{k-1}, d_k), and its successor's in the same visit, E(d_k, d_{k+1}).  Parts 2 and 3 (a sample whose
    membership of a visit is in doubt): its own entry, as in ref64.  In ref64's parts such a sample is the LAST of its
    visit or the only one (a grazed brick): it has no successor, and a predecessor's entry does not depend on it, so
    there is no neighbour whose entry changes between the paired and the self-paired form; the FIRST sample of a visit
    is never in doubt there.  Part 4 is ref64's.

The comparison is scenes.assert_parity(got, frame, budget=budget), with the constants of tests/scenes.py as they stand.

`mutate` gives deliberate misreadings of the contract, for tests/test_preint_cpu.py alone.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import mip_scenes
import orc
import scenes
import shade_ref
from ref64 import (DRIFT, EARLY_EXIT, EPSILON, EXACT_TIE, REL_WINDOW, Result, _Ctx, _classify, _mat, _nearest, _slab,
                   _trilinear, _vec, node_ids)

MUTATIONS = ("no_preintegration", "carried_across_visits", "front_only", "mean_of_classifications", "alpha_mean",
             "colour_unweighted", "correction_ignored")
_TABLE_MUTATIONS = ("alpha_mean", "colour_unweighted", "correction_ignored")
VALUE, TEXEL = 0, 1
ALPHA_MAX = 255.0 / 256.0

_SUB = 16
_GX, _GW = np.polynomial.legendre.leggauss(32)
_GX, _GW = 0.5 * (_GX + 1.0), 0.5 * _GW  # on [0, 1]


def _part(tf, i, p, q):
    """Integrals over t in [p, q] of the interval between texel centres i and i + 1, on which the integrand is smooth:
    [..., 11] = tau, tau rgb, a, a rgb, rgb."""
    t = p[..., None, None] + (q - p)[..., None, None] * ((np.arange(_SUB)[:, None] + _GX[None, :]) / _SUB)
    w = (q - p)[..., None, None] * (_GW[None, :] / _SUB)
    a = np.minimum(tf[i, 3][..., None, None] + (tf[i + 1, 3] - tf[i, 3])[..., None, None] * t, ALPHA_MAX)
    tau = -np.log1p(-a)
    out = np.empty(p.shape + (11,))
    out[..., 0] = (tau * w).sum(axis=(-1, -2))
    out[..., 4] = (a * w).sum(axis=(-1, -2))
    for ch in range(3):
        c = tf[i, ch][..., None, None] + (tf[i + 1, ch] - tf[i, ch])[..., None, None] * t
        out[..., 1 + ch] = (tau * c * w).sum(axis=(-1, -2))
        out[..., 5 + ch] = (a * c * w).sum(axis=(-1, -2))
        out[..., 8 + ch] = (c * w).sum(axis=(-1, -2))
    return out


def _span(tf, i, s, e):
    """[s, e] of texel interval i (arrays of one shape), split at the 255/256 crossing."""
    i = np.asarray(i, dtype=np.intp)
    s, e = np.asarray(s, dtype=np.float64), np.asarray(e, dtype=np.float64)
    a0, a1 = tf[i, 3], tf[i + 1, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (ALPHA_MAX - a0) / (a1 - a0)
    cut = np.where(np.isfinite(t) & (t > s) & (t < e), t, e)
    return _part(tf, i, s, cut) + _part(tf, i, cut, e)


def _outside(tf, i, length):
    a = min(float(tf[i, 3]), ALPHA_MAX)
    tau = -np.log1p(-a)
    c = tf[i, :3]
    unit = np.concatenate([[tau], tau * c, [a], a * c, c])
    return np.maximum(length, 0.0)[..., None] * unit


def value_coord(d, r0, r1):
    """x(d): the coordinate the plain classification uses"""
    return (np.asarray(d, dtype=np.float64) - r0) / (r1 - r0) * 256.0 - 0.5


_TABLES = {}


def table(tf, r0, r1, k, kind, frac_bits=8, mutate=None):
    """The contract's table in float64: [256, 256, 4].  kind VALUE: P[u][v] = E(x(u), x(v)), the diagonal the classified
    table's entries (frac_bits); kind TEXEL: T[i][j] = E(i, j), the diagonal the plain classification at the texel."""
    tf = np.asarray(tf, dtype=np.float64).reshape(256, 4)
    if mutate not in _TABLE_MUTATIONS:
        mutate = None
    key = (tf.tobytes(), float(r0), float(r1), float(k), int(kind), int(frac_bits), mutate)
    if key in _TABLES:
        return _TABLES[key]
    assert r1 > r0
    kk = 1.0 if mutate == "correction_ignored" else float(k)
    whole = _span(tf, np.arange(255), np.zeros(255), np.ones(255))        # [255, 11]
    between = np.zeros((256, 257, 11))                                    # between[a, b] = sum of whole[a:b], a <= b
    for a in range(255):
        between[a, a + 1:256] = np.cumsum(whole[a:], axis=0)
    x = np.arange(256, dtype=np.float64) if kind == TEXEL else value_coord(np.arange(256), float(r0), float(r1))
    cl = np.clip(x, 0.0, 255.0)
    it = np.minimum(np.floor(cl), 254).astype(np.intp)
    up = _span(tf, it, cl - it, np.ones(256))      # from the value to the end of its interval
    down = _span(tf, it, np.zeros(256), cl - it)   # from the start of its interval to the value
    lo, hi = np.minimum(x[:, None], x[None, :]), np.maximum(x[:, None], x[None, :])
    ilo, ihi = np.minimum(it[:, None], it[None, :]), np.maximum(it[:, None], it[None, :])
    first = np.where(x[:, None] <= x[None, :], np.arange(256)[:, None], np.arange(256)[None, :])
    last = np.where(x[:, None] <= x[None, :], np.arange(256)[None, :], np.arange(256)[:, None])
    total = up[first] + between[np.minimum(ilo + 1, 255), np.maximum(ihi, np.minimum(ilo + 1, 255))] + down[last]
    same = (ilo == ihi)
    sel = np.nonzero(same)
    assert sel[0].size < 20000, "a range this wide puts too many values into one texel interval for this quadrature"
    total[sel] = _span(tf, ilo[sel], np.clip(lo[sel], 0.0, 255.0) - ilo[sel], np.clip(hi[sel], 0.0, 255.0) - ilo[sel])
    total += _outside(tf, 0, np.minimum(hi, 0.0) - lo) + _outside(tf, 255, hi - np.maximum(lo, 255.0))
    width = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        taubar = total[..., 0] / width
        alpha = -np.expm1(-kk * taubar)
        colour = total[..., 1:4] / total[..., 0:1]
        if mutate == "alpha_mean":
            alpha = 1.0 - (1.0 - total[..., 4] / width) ** kk
            colour = total[..., 5:8] / total[..., 4:5]
        elif mutate == "colour_unweighted":
            colour = total[..., 8:11] / width[..., None]
    out = np.zeros((256, 256, 4))
    out[..., :3] = colour * alpha[..., None]
    out[..., 3] = alpha
    out[~(total[..., 0] > 0.0) | ~(width > 0.0)] = 0.0
    # the diagonal: the plain classification
    cx = _Ctx()
    cx.mutate, cx.tf, cx.corr, cx.alpha_max = None, tf, kk, ALPHA_MAX
    if kind == VALUE:
        cx.frac_bits, cx.mult, cx.add = int(frac_bits), 1.0 / (r1 - r0), -r0 / (r1 - r0)
        diag = _classify(cx, np.arange(256, dtype=np.float64))
    else:
        cx.frac_bits, cx.mult, cx.add = 0, 1.0 / 256.0, 0.5 / 256.0   # u 256 - 0.5 = i
        diag = _classify(cx, np.arange(256, dtype=np.float64))
    out[np.arange(256), np.arange(256)] = diag
    _TABLES[key] = out
    return out


def _read(tab, kind, before, value, r0, r1):
    """E(before, value) as the frame reads it: exactly (VALUE: stored bytes), or bilinearly at the clamped coordinates."""
    if kind == VALUE:
        return tab[before.astype(np.intp), value.astype(np.intp)]
    xf = np.clip(value_coord(before, r0, r1), 0.0, 255.0)
    xb = np.clip(value_coord(value, r0, r1), 0.0, 255.0)
    i0, j0 = np.floor(xf).astype(np.intp), np.floor(xb).astype(np.intp)
    i1, j1 = np.minimum(i0 + 1, 255), np.minimum(j0 + 1, 255)
    wf, wb = (xf - i0)[..., None], (xb - j0)[..., None]
    return ((1.0 - wb) * ((1.0 - wf) * tab[i0, j0] + wf * tab[i1, j0]) +
            wb * ((1.0 - wf) * tab[i0, j1] + wf * tab[i1, j1]))


def _entries(tab, kind, before, value, r0, r1, mutate):
    if mutate == "no_preintegration":
        return _read(tab, kind, value, value, r0, r1)
    if mutate == "front_only":
        return _read(tab, kind, before, before, r0, r1)
    if mutate == "mean_of_classifications":
        return 0.5 * (_read(tab, kind, before, before, r0, r1) + _read(tab, kind, value, value, r0, r1))
    return _read(tab, kind, before, value, r0, r1)


def _paired(val, first_before=None):
    """the value before every sample of a visit: the sample's own for the first"""
    before = np.concatenate([val[:, :1], val[:, :-1]], axis=1)
    if first_before is not None:
        before[:, 0] = np.where(np.isnan(first_before), val[:, 0], first_before)
    return before


def _face_ties(tab, kind, brick, c, idx, val, before, ent, k, vpw, r0, r1, mutate):
    """Part 1, per unit transmittance: for the point samples within delta_k of a voxel face, the largest channel
    difference of the sample's own entry plus that of its successor's when the sample reads the voxel across the face
    (edge, corner: every combination)."""
    dims = brick.shape[::-1]
    out = np.zeros(c.shape[:-1])
    off = []
    for a in range(3):
        fr = c[..., a] - np.floor(c[..., a])
        delta = orc.TIE_DELTA + k * DRIFT * vpw[a]
        off.append(np.where(fr < delta, -1, 0) + np.where(fr > 1.0 - delta, 1, 0))
    sel = np.nonzero((off[0] != 0) | (off[1] != 0) | (off[2] != 0))
    if sel[0].size == 0:
        return out
    o = [off[a][sel] for a in range(3)]
    i = [idx[a][sel] for a in range(3)]
    own_before, own, own_ent = before[sel], val[sel], ent[sel]
    has_next = sel[1] + 1 < val.shape[1]
    nxt = (sel[0], np.minimum(sel[1] + 1, val.shape[1] - 1))
    next_val, next_ent = val[nxt], ent[nxt]
    is_first = sel[1] == 0
    worst = np.zeros(sel[0].size)
    for m in range(1, 8):
        use = [(m >> a) & 1 for a in range(3)]
        valid = np.ones(sel[0].size, dtype=bool)
        for a in range(3):
            if use[a]:
                valid &= o[a] != 0
        if not valid.any():
            continue
        q = [np.clip(i[a] + use[a] * o[a], 0, dims[a] - 1) for a in range(3)]
        there = brick[q[2], q[1], q[0]].astype(np.float64)
        mine = _entries(tab, kind, np.where(is_first, there, own_before), there, r0, r1, mutate)
        change = np.abs(mine - own_ent).max(axis=-1)
        after = _entries(tab, kind, there, next_val, r0, r1, mutate)
        change = change + np.where(has_next, np.abs(after - next_ent).max(axis=-1), 0.0)
        worst = np.maximum(worst, np.where(valid, change, 0.0))
    out[sel] = worst
    return out


def kind_of(s, filter_mode):
    some_brick = next(iter(s.bricks.values()))
    return VALUE if (not filter_mode and some_brick.dtype.itemsize == 1) else TEXEL


def render(s, fb=None, budget=None, frac_bits=8, filter_mode=0, mutate=None):
    """One pass of the pre-integrated ray cast over s.nodes[:s.n_nodes] (ref64.render with the two changes above)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    assert s.render.samplesPerPixel == 1
    view, rd = s.view, s.render
    cx = _Ctx()
    cx.mutate, cx.frac_bits, cx.filter_mode = None, int(frac_bits), int(filter_mode)
    r0, r1 = float(rd.dataSourceRange[0]), float(rd.dataSourceRange[1])
    spr = float(rd.samplesPerRay)
    step = 1.0 / spr
    kind = kind_of(s, filter_mode)
    tab = table(s.tf, r0, r1, float(rd.maxSamplesPerRay) / spr, kind, frac_bits=frac_bits, mutate=mutate)

    # ---- rays (cuda/Renderer.cu:40-51, :106-122)
    ys, xs = np.arange(s.H), np.arange(s.W)
    h, w = len(ys), len(xs)
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

    done = ~alive
    shadow = np.zeros(n, dtype=bool)
    sh_a = np.zeros(n)
    ert_lo = np.full(n, -1.0)
    ert_eps = np.zeros(n)
    counts = np.zeros(n, dtype=np.int64)
    carried = np.full(n, np.nan)  # (mutate = "carried_across_visits" alone)
    ov = np.array([float(s.vi.overlap[a]) for a in range(3)])

    def values(brick, c):
        """the sample's value: the stored voxel (and its index), or the interpolated float"""
        if filter_mode:
            return _trilinear(cx, brick, c), None
        v, idx = _nearest(brick, c)
        return v.astype(np.float64), idx

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

        # budget, part 2: a brick the ray grazes gets one sample, or none: the self-paired entry
        graze = (~done & ~shadow & (np.abs(tf - tn) <= REL_WINDOW * np.maximum(1.0, np.abs(tn))) &
                 (tf >= tn_g) & (tn <= tf_g) & (tf >= t_near_plane))
        if graze.any():
            g = np.nonzero(graze)[0]
            v, _ = values(brick, coords(origin + d[g] * tn[g, None]))
            bud[g] += _entries(tab, kind, v, v, r0, r1, mutate).max(axis=-1) * (1.0 - col[g, 3])

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
        c = coords(pos)
        # ---- change 1: every sample paired with the one before it in this visit
        val, idx = values(brick, c)
        before = _paired(val, carried[p] if mutate == "carried_across_visits" else None)
        ent = _entries(tab, kind, before, val, r0, r1, mutate)
        heavy = ent.max(axis=-1)
        # ---- change 2: part 1 of the budget on both entries a sample enters
        ties = (np.zeros(val.shape) if idx is None else
                _face_ties(tab, kind, brick, c, idx, val, before, ent, kk[None, :], vpw, r0, r1, mutate))
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)   # barely taken
        next_tie = (count > 0) & (dist - count * step > -end_eps)          # barely not

        # ---- front to back, sample by sample (:208-226)
        c_col, c_bud = col[p], bud[p]
        c_done, c_shadow, c_sha = done[p], shadow[p], sh_a[p]
        c_lo, c_eps, c_n = ert_lo[p], ert_eps[p], counts[p]
        c_carried = carried[p]
        for k in range(kk.size):
            normal = ~c_done & ~c_shadow
            extra = normal & (count == k) & next_tie
            if extra.any():
                c_bud[extra] += heavy[extra, k] * (1.0 - c_col[extra, 3])
            act = ~c_done & (k < count)
            if not act.any():
                break
            normal &= act
            trans = 1.0 - c_col[:, 3]
            c_bud += np.where(normal, ties[:, k] * trans, 0.0)
            if k > 0:
                c_bud += np.where(normal & last_tie & (count == k + 1), heavy[:, k] * trans, 0.0)
            c_col += np.where(normal[:, None], ent[:, k, :] * trans[:, None], 0.0)   # :83-93, the step's entry
            c_n += normal
            c_carried = np.where(act, val[:, k], c_carried)
            follow = act & c_shadow
            c_sha = np.where(follow, c_sha + ent[:, k, 3] * (1.0 - c_sha), c_sha)
            acc = np.where(c_shadow, c_sha, c_col[:, 3])
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
        carried[p] = c_carried

    acc = np.where(shadow, sh_a, col[:, 3])
    bud += np.where(ert_lo >= 0.0, np.maximum(0.0, acc - ert_lo), 0.0)
    return Result(col.reshape(h, w, 4), int(counts.sum()), bud.reshape(h, w), counts.reshape(h, w))


# ---- the scenes of tests/test_preint_cpu.py, tests/test_preint.py and tests/test_preint_host.py, and their references ----
NAMES = ("axis", "spin", "inside", "clip", "nucleon", "peak")
PEAK = dict(voxels=(32, 32, 32), block=16, viewport=(43, 35), spr=24, spin=(0.35, 0.2))
PEAK_TEXEL = 120  # the spike: texels 120 and 121
_SCENES, _REFS = {}, {}


def peak_volume(n=32):
    """smooth data: 8-bit values falling linearly with the distance from the centre, 255 there and 0 in the corners"""
    g = (np.arange(n, dtype=np.float64) + 0.5) / n - 0.5
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z) / np.sqrt(0.75)
    return np.ascontiguousarray(np.clip(np.floor(255.0 * (1.0 - r) + 0.5), 0, 255).astype(np.uint8))


def peak_tf(texel=PEAK_TEXEL, alpha=0.9):
    """a transfer function whose only opacity is a spike two texels wide, on a colour ramp"""
    tf = mip_scenes.colour_ramp_tf().copy()
    tf[:, 3] = 0.0
    tf[texel:texel + 2, 3] = np.float32(alpha)
    return np.ascontiguousarray(tf)


def scene(name):
    """shade_ref's scenes by name (axis at its 43 x 35 viewport, spin with its colour ramp at a quarter of the opacity,
    nucleon at 44 x 36) and "peak": a radial ramp under a two-texel spike at 24 samples per ray, where consecutive
    samples of a ray are about 20 values apart and straddle the spike."""
    if name not in _SCENES:
        if name == "peak":
            s = orc.build_scene(dtype="u8", volume=peak_volume(PEAK["voxels"][0]), **PEAK)
            s.tf = peak_tf()
            _SCENES[name] = s
        else:
            _SCENES[name] = shade_ref.scene(name)
    return _SCENES[name]


def ref(name, filter_mode=0):
    """preint_ref's frame of a scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode)
    if key not in _REFS:
        _REFS[key] = render(scene(name), filter_mode=filter_mode)
    return _REFS[key]


def typed_ref(image, filter_mode):
    """of the uint16 scene q behind a typed image v = a + b q, b > 0: the range moves with the values, x(d) stays"""
    key = ("typed", image, filter_mode)
    if key not in _REFS:
        _REFS[key] = render(mip_scenes.typed(image)[0], filter_mode=filter_mode)
    return _REFS[key]


def check(s, got, r, what):
    """THE comparison: the frozen rule of tests/scenes.py with the reference's own budget.  Prints what it used."""
    orc._LAST_SCENE = s  # assert_parity takes its weak / strong decision from the scene under test
    d = np.abs(got.astype(np.float64) - r.frame).max(axis=-1)
    print("%s: max|d| %.3g mean|d| %.3g, mean budget %.3g, %.3f of the pixels over E0"
          % (what, float(d.max()), float(d.mean()), float(r.budget.mean()), float((d > scenes.E0).mean())))
    return scenes.assert_parity(got, r.frame, what + " against preint_ref", budget=r.budget)


# ---- the host build (tests/cpu_harness/preint_harness.cpp), built as shade_harness.cpp is -------------------------------
GRID, FIXED, TRILINEAR, UNIFORM = mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.TRILINEAR, mip_scenes.UNIFORM
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "preint_harness.cpp")
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
        _H = C.CDLL(build(os.path.join(HERE, "cpu_harness", "libpreint_harness.so"), ["-fPIC", "-shared"]))
    return _H


def harness_table(tf, r0, r1, k, kind, frac_bits=8):
    """the host builder's table, float32 [256, 256, 4]"""
    tf = np.ascontiguousarray(tf, dtype=np.float32)
    out = np.zeros((256, 256, 4), dtype=np.float32)
    rc = harness().preint_harness_table(C.c_void_p(tf.ctypes.data), C.c_float(r0), C.c_float(r1), C.c_float(k),
                                        C.c_int(frac_bits), C.c_int(kind), C.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


def harness_lut(tf, r0, r1, k, frac_bits=8):
    tf = np.ascontiguousarray(tf, dtype=np.float32)
    out = np.zeros((256, 4), dtype=np.float32)
    rc = harness().preint_harness_lut(C.c_void_p(tf.ctypes.data), C.c_float(r0), C.c_float(r1), C.c_float(k),
                                      C.c_int(frac_bits), C.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


class Host:
    def __init__(self, s):
        self.frame = np.zeros((s.H, s.W, 4), dtype=np.float32)
        self.samples = 0
        self.each = np.zeros((s.H, s.W), dtype=np.int64)


def harness_render(s, form, preint=1, passes=None, frac_bits=8):
    """the host build's frame; passes: [(a, b)] of s.nodes, accumulating in one buffer"""
    out = Host(s)
    each = np.zeros((s.H, s.W), dtype=np.uint32)
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().preint_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(out.frame.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.c_int(preint), C.byref(samples),
            C.c_void_p(each.ctypes.data))
        assert rc == 0, "preint_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        out.samples += int(samples.value)
        out.each += each
    return out
