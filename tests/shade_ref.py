"""A float64 restatement of a shaded composite frame (include/vrc_hip.h, "A shaded composite frame"), in NumPy.

TEST INFRASTRUCTURE.  Built on tests/ref64.py (its helpers are imported, nothing there is edited) and on the gradient of
tests/iso_ref.py; it shares nothing with libre_amd/csrc/vrc_core.h.

render() is ref64.render's march, statement for statement, with two changes:
  * the classified sample's rgb is multiplied by s = ambient + (1 - ambient) |G.dir| / |G| (1 where |G| is 0), G the
    central differences, indices clamped, of the brick's voxels around the voxel the POINT sampler addresses at the
    sample (the floor of the brick-local coordinate, under both filters), times the brick's voxels per world unit;
  * part 1 of the tie budget (samples within delta_k of a voxel face) compares the SHADED sample with the SHADED reading
    across the face: the neighbour voxel's value with the neighbour voxel's gradient.  Under the trilinear filter part 1
    now exists too: the value stays, the gradient is the neighbouring voxel's.
Parts 2-4 are ref64's: bounds by the largest channel of the unshaded sample, alpha included, and s <= 1.

The comparison is scenes.assert_parity(got, frame, budget=budget), with the constants of tests/scenes.py as they stand.

`mutate` gives deliberate misreadings of the shading, for tests/test_shade_cpu.py alone.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import mip_scenes
import orc
import scenes
from iso_ref import _gradient
from ref64 import (DRIFT, EARLY_EXIT, EPSILON, EXACT_TIE, REL_WINDOW, Result, _Ctx, _classify, _mat, _nearest, _sample, _slab,
                   _vec, node_ids)

AMBIENT = 0.25
MUTATIONS = ("no_shading", "ambient_ignored", "one_sided", "axes_swapped", "neighbour_x", "unscaled", "trilinear_floor_half")


def _shade(brick, idx, vpw, dirs, ambient, mutate=None):
    """s of the voxels idx = [x, y, z] (arrays of one shape) for rays of direction dirs (that shape + (3,))."""
    shape = idx[0].shape
    flat = [np.asarray(i).reshape(-1) for i in idx]
    if mutate == "no_shading":
        return np.ones(shape)
    if mutate == "neighbour_x":
        flat[0] = np.minimum(flat[0] + 1, brick.shape[2] - 1)
    g = _gradient(brick, flat, np.ones(3) if mutate == "unscaled" else vpw, None).reshape(shape + (3,))
    if mutate == "axes_swapped":
        g = g[..., [1, 0, 2]]
    ln = np.sqrt((g * g).sum(axis=-1))
    dot = (g * dirs).sum(axis=-1)
    dot = np.maximum(0.0, -dot) if mutate == "one_sided" else np.abs(dot)
    a = 0.0 if mutate == "ambient_ignored" else ambient
    with np.errstate(invalid="ignore", divide="ignore"):
        s = a + (1.0 - a) * dot / ln
    return np.where((ln > 0.0) & np.isfinite(ln), s, 1.0)


def _lit(cls, s):
    out = cls * s[..., None]
    out[..., 3] = cls[..., 3]
    return out


def _face_ties(cx, brick, c, idx, cls, lit, k, vpw, dirs, ambient):
    """ref64._face_ties on shaded readings: for the samples within delta_k of a voxel face, the largest channel
    difference between the shaded sample and the shaded reading across that face (edge, corner: every combination) --
    the neighbour voxel's classified value (point samples; a trilinear sample keeps its own) with the neighbour voxel's
    gradient."""
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
    own, own_cls = lit[sel], cls[sel]
    d = np.broadcast_to(dirs, c.shape)[sel]
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
        there = own_cls if cx.filter_mode else cx.table[brick[q[2], q[1], q[0]]]
        there = _lit(there, _shade(brick, q, vpw, d, ambient))
        worst = np.maximum(worst, np.where(valid, np.abs(there - own).max(axis=-1), 0.0))
    out[sel] = worst
    return out


def render(s, fb=None, budget=None, frac_bits=8, filter_mode=0, ambient=AMBIENT, mutate=None):
    """One pass of the shaded ray cast over s.nodes[:s.n_nodes] (ref64.render with the two changes above)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    assert s.render.samplesPerPixel == 1
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
    cx.table = _classify(cx, np.arange(256 if some_brick.dtype.itemsize == 1 else 65536, dtype=np.float64))

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

        # budget, part 2: a brick the ray grazes gets one sample, or none
        graze = (~done & ~shadow & (np.abs(tf - tn) <= REL_WINDOW * np.maximum(1.0, np.abs(tn))) &
                 (tf >= tn_g) & (tn <= tf_g) & (tf >= t_near_plane))
        if graze.any():
            g = np.nonzero(graze)[0]
            cls, _, _ = _sample(cx, brick, coords(origin + d[g] * tn[g, None]))
            bud[g] += cls.max(axis=-1) * (1.0 - col[g, 3])

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
        cls, idx, c = _sample(cx, brick, coords(pos))
        # ---- change 1: the headlight, from the voxel the point sampler addresses
        if idx is None:
            cc = c - 0.5 if mutate == "trilinear_floor_half" else c
            _, idx = _nearest(brick, cc)
        dirs = d[p][:, None, :]
        lit = _lit(cls, _shade(brick, idx, vpw, dirs, ambient, mutate))
        heavy = cls.max(axis=-1)
        # ---- change 2: part 1 of the budget on shaded readings, under both filters
        ties = _face_ties(cx, brick, c, idx, cls, lit, kk[None, :], vpw, dirs, ambient)
        end_eps = REL_WINDOW * np.maximum(1.0, np.abs(tf[p]))
        last_tie = (count > 1) & (dist - (count - 1) * step <= end_eps)   # barely taken
        next_tie = (count > 0) & (dist - count * step > -end_eps)          # barely not

        # ---- front to back, sample by sample (:208-226)
        c_col, c_bud = col[p], bud[p]
        c_done, c_shadow, c_sha = done[p], shadow[p], sh_a[p]
        c_lo, c_eps, c_n = ert_lo[p], ert_eps[p], counts[p]
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
            c_col += np.where(normal[:, None], lit[:, k, :] * trans[:, None], 0.0)   # :83-93, the colour lit
            c_n += normal
            follow = act & c_shadow
            c_sha = np.where(follow, c_sha + cls[:, k, 3] * (1.0 - c_sha), c_sha)
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

    acc = np.where(shadow, sh_a, col[:, 3])
    bud += np.where(ert_lo >= 0.0, np.maximum(0.0, acc - ert_lo), 0.0)
    return Result(col.reshape(h, w, 4), int(counts.sum()), bud.reshape(h, w), counts.reshape(h, w))


# ---- the scenes of tests/test_shade_cpu.py, tests/test_shade.py and tests/test_shade_host.py, and their references ------
NAMES = ("axis", "spin", "inside", "clip", "skip", "skip16")
AXIS_VIEWPORT = (43, 35)
_SCENES, _REFS = {}, {}


def scene(name):
    """mip_scenes' scenes by name, "nucleon" (the 41^3 fixture without overlap at a 44 x 36 viewport) and "aniso" (the
    same brick in a box half as high: voxels per world unit differ between the axes)."""
    if name not in _SCENES:
        if name == "nucleon":
            _SCENES[name] = scenes.nucleon_scene(viewport=(44, 36))
        elif name == "aniso":
            _SCENES[name] = _aniso_nucleon()
        elif name == "axis":
            # mip_scenes' axis view at a 43 x 35 viewport instead of 44 x 36: at the even one four rays run through
            # brick corners exactly, which ref64 reads as missing the brick (EXACT_TIE) and float32 as hitting it -- the
            # UNSHADED host build and the oracle (they agree bit for bit) differ from ref64 there by 5e-3 with a budget
            # of 0.  No ray of the odd viewport does (tests/test_shade_cpu.py holds the host build to the rule on it)
            _SCENES[name] = orc.build_scene(dtype="u8", alpha=0.8, **dict(mip_scenes.SCENES["axis"], viewport=AXIS_VIEWPORT))
        else:
            _SCENES[name] = mip_scenes.get(name)
            if name == "spin":
                # mip_scenes' colour ramp at a quarter of its opacity (alpha 0.05 ... 0.2 instead of 0.2 ... 0.8).  On
                # noise a flipped sample takes an unrelated gradient; with the full opacity the host build, float and
                # fixed stepping alike, stays inside the per-pixel rule but one pixel reaches 0.050 against the
                # frame-level cap of 0.03 (the grey ramp of alpha 0.8: 0.031).  With this one the largest is 0.013
                _SCENES[name].tf = spin_tf()
    return _SCENES[name]


def spin_tf():
    tf = mip_scenes.colour_ramp_tf().copy()
    tf[:, 3] *= np.float32(0.25)
    return np.ascontiguousarray(tf)


def _aniso_nucleon():
    """For the float64 reference alone (the teeth of the rule): the nucleon brick in a world box squeezed to half its
    height, so that a gradient not scaled by the voxels per world unit points elsewhere."""
    s = scenes.nucleon_scene(viewport=(44, 36))
    nid = s.ids[0]
    lo, hi = float(s.lod[nid].worldBoxMin[1]), float(s.lod[nid].worldBoxMax[1])
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    s.lod[nid].worldBoxMin[1], s.lod[nid].worldBoxMax[1] = mid - half, mid + half
    s.nodes[0].aabbMin[1] = s.lod[nid].worldBoxMin[1]
    s.nodes[0].aabbSize[1] = s.lod[nid].worldBoxMax[1] - s.lod[nid].worldBoxMin[1]
    s.view.aabbMin[1], s.view.aabbMax[1] = s.lod[nid].worldBoxMin[1], s.lod[nid].worldBoxMax[1]
    return s


def ref(name, filter_mode=0, ambient=AMBIENT):
    """shade_ref's frame of a scene, computed once and shared; callers leave it unchanged."""
    key = (name, filter_mode, ambient)
    if key not in _REFS:
        _REFS[key] = render(scene(name), filter_mode=filter_mode, ambient=ambient)
    return _REFS[key]


def typed_ref(image, filter_mode, ambient=AMBIENT):
    """of the uint16 scene q behind a typed image v = a + b q, b > 0: G scales by b, s does not change"""
    key = ("typed", image, filter_mode, ambient)
    if key not in _REFS:
        _REFS[key] = render(mip_scenes.typed(image)[0], filter_mode=filter_mode, ambient=ambient)
    return _REFS[key]


def check(s, got, r, what):
    """THE comparison: the frozen rule of tests/scenes.py with the reference's own budget.  Prints what it used."""
    orc._LAST_SCENE = s  # assert_parity takes its weak / strong decision from the scene under test
    d = np.abs(got.astype(np.float64) - r.frame).max(axis=-1)
    print("%s: max|d| %.3g mean|d| %.3g, mean budget %.3g, %.3f of the pixels over E0"
          % (what, float(d.max()), float(d.mean()), float(r.budget.mean()), float((d > scenes.E0).mean())))
    return scenes.assert_parity(got, r.frame, what + " against shade_ref", budget=r.budget)


# ---- the host build of the per-ray code (tests/cpu_harness/shade_harness.cpp), built as iso_harness.cpp is ---------------
GRID, FIXED, TRILINEAR, UNIFORM = mip_scenes.GRID, mip_scenes.FIXED, mip_scenes.TRILINEAR, mip_scenes.UNIFORM
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_harness", "shade_harness.cpp")
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
        _H = C.CDLL(build(os.path.join(HERE, "cpu_harness", "libshade_harness.so"), ["-fPIC", "-shared"]))
    return _H


class Host:
    """frame, samples, and per pixel: samples taken, those with and those without their gradient gathers; rays[H, W, 3]"""

    def __init__(self, s):
        self.frame = np.zeros((s.H, s.W, 4), dtype=np.float32)
        self.samples = 0
        self.each = np.zeros((s.H, s.W), dtype=np.int64)
        self.gathered = np.zeros((s.H, s.W), dtype=np.int64)
        self.skipped = np.zeros((s.H, s.W), dtype=np.int64)
        self.rays = np.zeros((s.H, s.W, 3), dtype=np.float32)


def harness_render(s, form, shading=1, ambient=AMBIENT, skip=1, passes=None, frac_bits=8):
    """the host build's frame; passes: [(a, b)] of s.nodes, accumulating in one buffer"""
    out = Host(s)
    each, wg, wo = [np.zeros((s.H, s.W), dtype=np.uint32) for _ in range(3)]
    mb = [s.vi.maximumBlockSize[a] for a in range(3)]
    for k, (a, b) in enumerate(passes or [(0, s.n_nodes)]):
        samples = C.c_uint64(0)
        nodes = C.cast(C.byref(s.nodes, a * C.sizeof(orc.NodeData)), C.POINTER(orc.NodeData))
        rc = harness().shade_harness_render(
            C.c_void_p(s.atlas.ctypes.data), C.c_uint32(s.atlas.dtype.itemsize), orc.u32x3(*s.atlas_dim),
            orc.u32x3(*s.slot_dim), orc.u32x3(*mb), C.c_void_p(out.frame.ctypes.data), C.c_uint32(s.W), C.c_uint32(s.H),
            C.c_void_p(s.planes.ctypes.data if len(s.planes) else None), C.c_uint32(len(s.planes)),
            C.c_void_p(s.tf.ctypes.data), C.byref(s.view), C.c_uint32(b - a), nodes, C.byref(s.render), C.c_int(form),
            C.c_int(frac_bits), C.c_int(1 if k == 0 else 0), C.c_int(shading), C.c_float(ambient), C.c_int(skip),
            C.byref(samples), C.c_void_p(each.ctypes.data), C.c_void_p(wg.ctypes.data), C.c_void_p(wo.ctypes.data),
            C.c_void_p(out.rays.ctypes.data))
        assert rc == 0, "shade_harness_render: %d" % rc
        assert int(each.sum()) == int(samples.value)
        out.samples += int(samples.value)
        out.each += each
        out.gathered += wg
        out.skipped += wo
    return out
