"""An independent float64 restatement of the reference's ray cast, in NumPy.

TEST INFRASTRUCTURE.  Every pixel the suite asserts on is compared with oracle/livre_oracle.c, and the oracle and the
kernels (libre_amd/csrc/vrc_core.h) come from one reading of renderers/cudaRaycaster/cuda/Renderer.cu:95-230.  This
module is a second reading, written from the reference's text alone, in exact-as-can-be arithmetic: everything is
float64, vectorised over the pixels of a frame and over the samples of a brick segment.  It shares no code with the
oracle or the host build: it calls neither integrator, and it does not look at the atlas.

What it takes from an orc.Scene is what the kernel ABI gets: s.view (eye, viewport, invProjMatrix, invViewMatrix,
global box, near plane), s.nodes[:s.n_nodes] in list order, s.render, s.tf, s.planes.  The voxels come from
s.bricks[nid], brick-local,

        c = overlap + (pos - boxMin) / boxSize * blockSize          (voxels, per axis; blockSize from s.lod[nid])

and NOT from s.atlas through textureMin / textureSize (Renderer.cu:203-214, CudaTextureObject.cpp:61-84): the result
is independent of slot order, atlas layout and orc_texture_object.  tests/test_ref64_cpu.py checks that the two
addressings name the same voxel.  A node of the list is matched to its NodeId by its world box.

The reference, as read here (paths under renderers/cudaRaycaster/):
  * pixel (x, y) WITHOUT a half-pixel offset -> NDC -> eye space (z = w = 1 in NDC) -> world; the ray leaves the eye
    through that point; zero direction components become 1e-10 (cuda/Renderer.cu:40-51, :111-122);
  * slab test against the global box: no hit, no pixel (:56-80, :124-130); every clip plane (n, d) cuts the interval:
    t = -(n.eye + d) / (n.dir), a lower bound where n.dir > 0, an upper bound otherwise -- the kept half space is
    n.p + d >= 0 (:132-149);
  * a pixel whose alpha already exceeds 0.999 is left alone; otherwise the march goes on from the pixel's colour, so
    passes accumulate (:151-157, :229);
  * tNearPlane = -nearPlane / z of the normalised eye-space position (:159-160);
  * per node, in list order (:172-193): no hit -> next; tNear beyond the far end of the interval -> the ray ENDS;
    tFar before its near end -> next; clamp [tNear, tFar] to near plane and interval; empty -> next;
  * the march restarts at the entry point of every brick (:195-201): pos_k = start + k x step, step = unit vector x
    1 / samplesPerRay (world units), for as long as dist - k / samplesPerRay > 0: ceil(dist x samplesPerRay) samples;
  * voxel = point sample, clamp addressing (cuda/TexturePool.cu:163-170); density x 1/(r1 - r0) - r0/(r1 - r0)
    (:162-164) -- also for the 16-bit voxels of this project's extension;
  * transfer function: 256 texels, linear filter, normalised coordinate, clamp (cuda/ColorMap.cu:40-45): per the CUDA
    programming guide's "linear filtering", x = 256 u - 0.5, i = floor(x), a = frac(x), (1 - a) T[i] + a T[i + 1]; `a`
    is exact (frac_bits = 0) or rounded to 1.8 fixed point, as the guide documents the hardware (frac_bits = 8);
  * composite (:83-93): alpha' = 1 - (1 - min(alpha, 255/256)) ^ (maxSamplesPerRay / samplesPerRay);
    rgb += rgb_tf x alpha' x (1 - A); A += alpha' x (1 - A); the ray ends when A > 0.999 (:218-226).

The trilinear filter (an extension) is taken from the words of include/vrc_hip.h (VRC_FILTER_TRILINEAR): voxel i has
its centre at i + 0.5 in the brick-local coordinate above, the eight voxels around the sample are weighted with
exact (float) weights, and the transfer function and the opacity correction are applied per sample to the
interpolated density.  The header did not say what happens to a tap outside the brick and its overlap border (only
possible with overlap 0): decided here as clamp addressing, the nearest voxel of the brick -- what the point sampler
does -- and the header now says so.

Not covered: the glRaycaster variant, samplesPerPixel > 1, and per-ray LOD.  Per-ray LOD is defined by the oracle
alone: there is no reference text to read independently.

Next to the frame the module returns the number of composited samples and its OWN tie budget B64[H, W], from its
own float64 geometry, by the definition at the head of tests/scenes.py with the contract's constants
(orc.TIE_DELTA, k x 2^-25, the 4e-6 relative windows, E0 and TIE_FACTOR for the early-exit window):
  1. samples within delta_k of a voxel face: the largest channel difference between the classified sample and the
     classified neighbour across the face(s), times the transmittance (point sampling only);
  2. the one sample of a brick the ray grazes (|tFar - tNear| <= 4e-6 max(1, |tNear|));
  3. the last sample of a segment, taken or not, where dist is within 4e-6 max(1, |tFar|) of a whole number of steps;
  4. the opacity gained between the first sample that leaves the ray within E0 + 2 B below 0.999 and the first that
     leaves it that far above.

`_mutate` is for tests/test_ref64_cpu.py alone: deliberate misreadings, to show that the comparison has teeth.
"""
import numpy as np

import orc
import scenes

EARLY_EXIT = 0.999   # cuda/Renderer.cu:34
EPSILON = 1e-10      # cuda/Renderer.cu:35
REL_WINDOW = 4e-6    # tests/scenes.py: grazed bricks, last samples
#: float64 is not exact either: where a comparison of the reference comes out closer than this (relative), the two sides
#: are taken as EQUAL, which is what they are in exact arithmetic whenever the rounding of this module could decide --
#: tFar > tNear is then false (a ray through a brick edge misses the brick) and dist / step is a whole number
EXACT_TIE = 1e-11
DRIFT = 2.0 ** -25   # tests/scenes.py: world units per step of the reference's pos += step

MUTATIONS = ("half_voxel_x", "pixel_centre", "exponent_spr_plus_1", "tf_no_half_texel", "alpha_clamp_1", "clip_sign",
             "floor_count", "trilinear_centre_i")


class Result:
    """frame[H, W, 4] float64, samples, budget[H, W] float64 (B64)."""

    def __init__(self, frame, samples, budget, counts=None):
        self.frame, self.samples, self.budget = frame, samples, budget
        self.counts = counts  # composited samples per pixel

    def __iter__(self):  # frame, samples, budget = render(...)
        return iter((self.frame, self.samples, self.budget))


def _vec(ct, n):
    return np.array([float(ct[i]) for i in range(n)], dtype=np.float64)


def _mat(ct):
    """float[16] column-major (vmmlib; cuda/math.cuh:1457-1465) -> 4 x 4 rows."""
    return _vec(ct, 16).reshape(4, 4).T


def node_ids(s):
    """NodeId of every entry of s.nodes[:s.n_nodes], matched by world box (list order is the caller's)."""
    by_box = {}
    for nid, node in s.lod.items():
        lo = [float(np.float32(node.worldBoxMin[a])) for a in range(3)]
        size = [float(np.float32(float(node.worldBoxMax[a]) - float(node.worldBoxMin[a]))) for a in range(3)]
        by_box[tuple(lo + size)] = nid
    out = []
    for i in range(s.n_nodes):
        nd = s.nodes[i]
        key = tuple([float(nd.aabbMin[a]) for a in range(3)] + [float(nd.aabbSize[a]) for a in range(3)])
        out.append(by_box[key])
    return out


def brick_coords(s, nid, rel):
    """Brick-local voxel coordinate (x, y, z) of the relative position rel in [0, 1]^3 of node nid's box."""
    node = s.lod[nid]
    ov = np.array([float(s.vi.overlap[a]) for a in range(3)])
    bs = np.array([float(node.blockSize[a]) for a in range(3)])
    return ov + rel * bs


class _Ctx:
    pass


def _tf_fetch(cx, u):
    x = u * 256.0 - (0.0 if cx.mutate == "tf_no_half_texel" else 0.5)
    fl = np.floor(x)
    a = x - fl
    if cx.frac_bits > 0:
        q = float(1 << cx.frac_bits)
        a = np.floor(a * q + 0.5) / q
    i0 = np.clip(fl, 0, 255).astype(np.intp)
    i1 = np.clip(fl + 1.0, 0, 255).astype(np.intp)
    return (1.0 - a)[..., None] * cx.tf[i0] + a[..., None] * cx.tf[i1]


def _classify(cx, density):
    """(rgb x alpha', alpha') of a sample of this density: what one composite step adds, per unit transmittance."""
    t = _tf_fetch(cx, density * cx.mult + cx.add)
    alpha = 1.0 - (1.0 - np.minimum(t[..., 3], cx.alpha_max)) ** cx.corr
    out = t * alpha[..., None]
    out[..., 3] = alpha
    return out


def _nearest(brick, c):
    dims = brick.shape[::-1]
    idx = [np.clip(np.floor(c[..., a]), 0, dims[a] - 1).astype(np.intp) for a in range(3)]
    return brick[idx[2], idx[1], idx[0]], idx


def _trilinear(cx, brick, c):
    dims = brick.shape[::-1]
    cc = c if cx.mutate == "trilinear_centre_i" else c - 0.5
    lo, hi, w = [], [], []
    for a in range(3):
        fl = np.floor(cc[..., a])
        w.append(cc[..., a] - fl)
        lo.append(np.clip(fl, 0, dims[a] - 1).astype(np.intp))
        hi.append(np.clip(fl + 1.0, 0, dims[a] - 1).astype(np.intp))
    b = brick.astype(np.float64)
    out = 0.0
    for kz, wz in ((lo[2], 1.0 - w[2]), (hi[2], w[2])):
        for ky, wy in ((lo[1], 1.0 - w[1]), (hi[1], w[1])):
            for kx, wx in ((lo[0], 1.0 - w[0]), (hi[0], w[0])):
                out = out + b[kz, ky, kx] * (wz * wy * wx)
    return out


def _sample(cx, brick, c):
    """Classified samples at the brick-local coordinates c[..., 3]; for the point sampler also the voxel index."""
    if cx.mutate == "half_voxel_x":
        c = c + np.array([0.5, 0.0, 0.0])
    if cx.filter_mode:
        return _classify(cx, _trilinear(cx, brick, c)), None, c
    v, idx = _nearest(brick, c)
    return cx.table[v], idx, c


def _face_ties(cx, brick, c, idx, cls, k, voxels_per_world):
    """Part 1 of the budget, per unit transmittance: for the samples within delta_k of a voxel face, the largest
    channel difference to the classified voxel across that face (edge, corner: every combination)."""
    dims = brick.shape[::-1]
    out = np.zeros(c.shape[:-1])
    off = []
    for a in range(3):
        fr = c[..., a] - np.floor(c[..., a])
        delta = orc.TIE_DELTA + k * DRIFT * voxels_per_world[a]
        off.append(np.where(fr < delta, -1, 0) + np.where(fr > 1.0 - delta, 1, 0))
    sel = np.nonzero((off[0] != 0) | (off[1] != 0) | (off[2] != 0))
    if sel[0].size == 0:
        return out
    o = [off[a][sel] for a in range(3)]
    i = [idx[a][sel] for a in range(3)]
    own = cls[sel]
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
        there = cx.table[brick[q[2], q[1], q[0]]]
        worst = np.maximum(worst, np.where(valid, np.abs(there - own).max(axis=-1), 0.0))
    out[sel] = worst
    return out


def _slab(origin, direction, lo, hi):
    """cuda/Renderer.cu:56-80: (tnear, tfar) of the slab test; a hit is tfar > tnear."""
    inv = 1.0 / direction
    t0 = inv * (lo - origin)
    t1 = inv * (hi - origin)
    return np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)


def render(s, fb=None, budget=None, frac_bits=8, filter_mode=0, stride=(1, 1), _mutate=None):
    """One pass of the cudaRaycaster ray cast over s.nodes[:s.n_nodes].  fb / budget: frame and B64 of the passes
    before this one (accumulating frames).  stride = (sy, sx): only every sy-th row and sx-th column of the
    viewport (the rays are the full viewport's); the arrays returned have that many rows and columns."""
    assert _mutate is None or _mutate in MUTATIONS, _mutate
    assert s.render.samplesPerPixel == 1
    view, rd = s.view, s.render
    cx = _Ctx()
    cx.mutate, cx.frac_bits, cx.filter_mode = _mutate, int(frac_bits), int(filter_mode)
    cx.tf = np.asarray(s.tf, dtype=np.float64).reshape(256, 4)
    r0, r1 = float(rd.dataSourceRange[0]), float(rd.dataSourceRange[1])
    cx.mult, cx.add = 1.0 / (r1 - r0), -r0 / (r1 - r0)
    spr = float(rd.samplesPerRay)
    cx.corr = float(rd.maxSamplesPerRay) / (spr + 1.0 if _mutate == "exponent_spr_plus_1" else spr)
    cx.alpha_max = 1.0 if _mutate == "alpha_clamp_1" else 255.0 / 256.0
    step = 1.0 / spr
    some_brick = next(iter(s.bricks.values()))
    if not filter_mode:
        cx.table = _classify(cx, np.arange(256 if some_brick.dtype.itemsize == 1 else 65536, dtype=np.float64))

    # ---- rays (cuda/Renderer.cu:40-51, :106-122)
    ys = np.arange(0, s.H, stride[0])
    xs = np.arange(0, s.W, stride[1])
    h, w = len(ys), len(xs)
    py, px = [g.reshape(-1).astype(np.float64) for g in np.meshgrid(ys, xs, indexing="ij")]
    if _mutate == "pixel_centre":
        px, py = px + 0.5, py + 0.5
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
        lower = (rn < 0.0) if _mutate == "clip_sign" else (rn > 0.0)
        tn_g = np.where(lower, np.maximum(tn_g, t), tn_g)
        tf_g = np.where(lower, tf_g, np.minimum(tf_g, t))
    alive &= ~(tn_g > tf_g)

    col = np.zeros((n, 4)) if fb is None else np.asarray(fb, dtype=np.float64).reshape(n, 4).copy()
    bud = np.zeros(n) if budget is None else np.asarray(budget, dtype=np.float64).reshape(n).copy()
    alive &= ~(col[:, 3] > EARLY_EXIT)  # :151-155

    done = ~alive                       # nothing more happens to the pixel, budget included
    shadow = np.zeros(n, dtype=bool)    # past its own exit, followed for part 4 of the budget only
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
        count = (np.floor(ratio) if _mutate == "floor_count" else np.ceil(ratio)).astype(np.int64)
        count = np.where(dist > 0.0, count, 0)
        if count.max() == 0:
            continue
        unit = diff / np.where(dist > 0.0, dist, 1.0)[:, None]
        kk = np.arange(int(count.max()) + 1, dtype=np.float64)   # one more: the sample that was barely not taken
        pos = start[:, None, :] + kk[None, :, None] * (unit * step)[:, None, :]
        cls, idx, c = _sample(cx, brick, coords(pos))
        heavy = cls.max(axis=-1)
        ties = None if filter_mode else _face_ties(cx, brick, c, idx, cls, kk[None, :], vpw)
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
            if ties is not None:
                c_bud += np.where(normal, ties[:, k] * trans, 0.0)
            if k > 0:
                c_bud += np.where(normal & last_tie & (count == k + 1), heavy[:, k] * trans, 0.0)
            c_col += np.where(normal[:, None], cls[:, k, :] * trans[:, None], 0.0)   # :83-93
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


def render_passes(s, passes, **kw):
    """The list rendered in passes [(a, b)] of its nodes into one buffer (CudaRaycastPipeline.cpp:149-185)."""
    import nongrid
    frame = budget = None
    counts = 0
    for t in nongrid.passes_of(s, passes):
        r = render(t, fb=frame, budget=budget, **kw)
        frame, budget, counts = r.frame, r.budget, counts + r.counts
    return Result(frame, int(counts.sum()), budget, counts)
