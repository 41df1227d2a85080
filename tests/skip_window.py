"""vrc_stats.samples of a MIP frame with VRC_OPT_MIP_SKIP on, predicted: a window [lo, hi] from tests/mip_ref.py and the
header's rule alone, for the scenes "skip" and "skip16" of tests/mip_scenes.py (tests/test_mip.py, test_fold.py assert the
GPU's count inside it; tests/test_slot_words_cpu.py checks that the window is honest -- narrow, and below the count
without skipping).  Point samples of the 8- and 16-bit atlases, the maximum and the minimum fold, both brick loops.

The rule (include/vrc_hip.h, "A MIP frame", "The folds of a MIP frame"): a ray marches the bricks it meets in the
loop's order -- the node list's for VRC_KERNEL_REFERENCE_ORDER, increasing entry distance for VRC_KERNEL_GRID_DDA --
and does not march a brick whose largest (smallest) stored voxel cannot raise (lower) the M it holds; a ray that holds
no sample yet marches.  The slot's word is the extremum NumPy finds in the brick as it is uploaded, overlap included
(the slot's padding repeats voxels of the brick and adds no value).  A uniform brick is folded from its word and counted
as if marched.

mip_ref.render(trace=...) gives, per ray and brick, the entry distance, the count and the extremum of the samples as
intervals: what float64 can say for certain, and what it cannot (a sample within the parity contract's window of a
voxel face, of the segment's end, a grazed brick).  The prediction carries the intervals through: a brick is skipped
for certain if even the weakest M the ray may hold settles it, marched for certain if not even the strongest does, and
counts towards hi but not lo in between.  Two bricks whose entry distances tie within the grid walk's tolerance may be
met in either order: every order of such a group is evaluated, and the ray contributes its smallest and largest."""
import itertools

import numpy as np

import mip_ref

REFORDER, DDA = "reforder", "dda"
MAX, MIN = "max", "min"
#: the grid walk hands the bricks around an edge or a corner over in a fixed order; they tie to within 2e-6 of t
#: (libre_amd/csrc/vrc_core.h, vrc_ray_grid_dda: tolE; VRC_ISO_WALK_MARGIN is twice that, and so is this)
TIE = 4e-6


class Window:
    """lo, hi: the frame's count with skipping; off_lo, off_hi: mip_ref's without; per ray (H x W): ray_lo, ray_hi;
    doubtful: rays with lo != hi; hit: rays with a sample."""


def _ray(visits):
    """visits: [(c_lo, c_hi, v_lo, v_hi, top)] in the order met, for the maximum (the minimum comes negated).  Returns
    the ray's (lo, hi)."""
    lo = hi = 0
    has_lo = has_hi = False
    m_lo = m_hi = -np.inf
    for c_lo, c_hi, v_lo, v_hi, top in visits:
        if c_hi == 0:
            continue
        may_skip = has_hi and m_hi >= top
        must_skip = has_lo and m_lo >= top
        lo += 0 if may_skip else c_lo
        hi += 0 if must_skip else c_hi
        if not must_skip:
            m_hi, has_hi = max(m_hi, v_hi), True
        if not may_skip and c_lo > 0:
            m_lo, has_lo = max(m_lo, v_lo), True
    return lo, hi


def _orders(visits, loop):
    """The orders in which the loop may meet a ray's bricks: [[index into visits]]."""
    if loop == REFORDER or len(visits) < 2:
        return [list(range(len(visits)))]
    tn = [v[0] for v in visits]
    idx = sorted(range(len(visits)), key=lambda k: (tn[k], k))
    groups, cur = [], [idx[0]]
    for k in idx[1:]:
        if tn[k] - tn[cur[-1]] <= TIE * max(1.0, abs(tn[k])):
            cur.append(k)
        else:
            groups.append(cur)
            cur = [k]
    groups.append(cur)
    if all(len(g) == 1 for g in groups):
        return [idx]
    out = []
    for combo in itertools.product(*[list(itertools.permutations(g)) for g in groups]):
        out.append([k for g in combo for k in g])
    return out


def window(s, fold, loop, bricks=None):
    """s: the scene as mip_ref reads it (8- or 16-bit bricks); bricks: what the pool holds if not s.bricks."""
    trace = []
    r = mip_ref.render(s, trace=trace)
    ids = mip_ref.node_ids(s)
    bricks = s.bricks if bricks is None else bricks
    sign = 1.0 if fold == MAX else -1.0
    top = [sign * float(bricks[nid].max() if fold == MAX else bricks[nid].min()) for nid in ids]
    per_ray = {}
    for t in trace:
        if fold == MAX:
            v_lo, v_hi = t["max_lo"], t["max_hi"]
        else:
            v_lo, v_hi = -t["min_hi"], -t["min_lo"]
        for k, ray in enumerate(t["rays"]):
            per_ray.setdefault(int(ray), []).append((float(t["tn"][k]), int(t["c_lo"][k]), int(t["c_hi"][k]),
                                                     float(v_lo[k]), float(v_hi[k]), top[t["node"]]))
    w = Window()
    w.ray_lo, w.ray_hi = np.zeros(s.H * s.W, dtype=np.int64), np.zeros(s.H * s.W, dtype=np.int64)
    w.tied = np.zeros(s.H * s.W, dtype=bool)
    for ray, visits in per_ray.items():
        orders = _orders(visits, loop)
        got = [_ray([visits[k][1:] for k in order]) for order in orders]
        w.ray_lo[ray], w.ray_hi[ray] = min(g[0] for g in got), max(g[1] for g in got)
        w.tied[ray] = len(orders) > 1
    w.ray_lo, w.ray_hi, w.tied = (a.reshape(s.H, s.W) for a in (w.ray_lo, w.ray_hi, w.tied))
    w.lo, w.hi = int(w.ray_lo.sum()), int(w.ray_hi.sum())
    w.off_lo, w.off_hi = int(r.counts_lo.sum()), int(r.counts_hi.sum())
    w.doubtful = (r.counts_lo != r.counts_hi) | w.tied | (w.ray_lo != w.ray_hi)
    w.hit = r.hit()
    w.ref = r
    return w


_WINDOWS = {}


def of(name, fold, loop):
    """The window of mip_scenes' scene `name` ("skip", "skip16"), once per process: under the minimum fold of the
    complemented scene tests/test_fold.py renders."""
    key = (name, fold, loop)
    if key not in _WINDOWS:
        import fold_ref
        import mip_scenes
        s = mip_scenes.get(name) if fold == MAX else fold_ref.complemented_scene(name)
        _WINDOWS[key] = window(s, fold, loop)
    return _WINDOWS[key]


def check(w, n, what):
    print("%s: samples with skipping %d, predicted %d .. %d (without: %d .. %d)" % (what, n, w.lo, w.hi, w.off_lo, w.off_hi))
    assert w.lo <= n <= w.hi, what


# ---- an isosurface frame ------------------------------------------------------------------------------------------------------
#: "it leaves a segment in front of the first group of samples whose t lies strictly above D" (include/vrc_hip.h): the
#: header does not say how long a group is; DESIGN.md does ("whole groups of 8 ... the same tails").  The prediction
#: uses it as an upper bound only: a ray that hits at sample j of a segment takes at most the 7 samples behind it.
ISO_GROUP = 8


def _iso_ray(visits, thr):
    """visits: [(tn, c_lo, c_hi, j_certain, j_possible, t_hit, top)] in the order met; j_certain / j_possible: the
    index of the segment's first sample that surely / possibly hits (None: there is none), t_hit: the largest t the
    certain hit can have.  D, the depth of the ray's first hit, is carried as an interval."""
    lo = hi = 0
    d_lo, d_hi = np.inf, np.inf  # D >= d_lo for certain (inf: the ray surely holds no hit); D <= d_hi for certain
    for tn, c_lo, c_hi, j_cert, j_poss, t_hit, top in visits:
        if c_hi == 0 or top < thr:
            continue  # the slot cannot reach the threshold: not marched
        tol = TIE * max(1.0, abs(tn))
        if tn > d_hi + tol:
            continue  # tNear lies strictly above the D the ray holds
        behind = tn > d_lo - tol  # ... or may lie above it
        if j_poss is None:  # no sample of this ray hits: marched to its end (or, entered behind D, not at all)
            lo += 0 if behind else c_lo
            hi += c_hi
            continue
        lo += 0 if behind else min(c_lo, j_poss + 1)  # every sample up to the first that may hit
        hi += c_hi if j_cert is None else min(c_hi, j_cert + ISO_GROUP)
        d_lo = min(d_lo, tn - tol)
        if j_cert is not None:
            d_hi = min(d_hi, t_hit)
    return lo, hi


def _first(mask):
    """Per row: the index of the first True, or -1."""
    return np.where(mask.any(axis=1), mask.argmax(axis=1), -1)


def iso_window(s, iso_value, loop, bricks=None):
    """An isosurface frame with skipping on (include/vrc_hip.h, "An isosurface frame", VRC_OPT_MIP_SKIP): no sample of
    a brick whose largest voxel lies below the threshold, none of a brick entered strictly behind D; a brick in which
    the ray hits is left in front of the first group of samples behind D."""
    trace = []
    r = mip_ref.render(s, trace=trace)
    ids = mip_ref.node_ids(s)
    bricks = s.bricks if bricks is None else bricks
    thr = float(np.ceil(iso_value))
    step = 1.0 / float(s.render.samplesPerRay)
    top = [float(bricks[nid].max()) for nid in ids]
    per_ray = {}
    for t in trace:
        n = len(t["rays"])
        if "samples" in t:
            vlo, vhi, sure, poss = t["samples"]
            j_cert, j_poss = _first(sure & (vlo >= thr)), _first(poss & (vhi >= thr))
        else:
            j_cert, j_poss = np.full(n, -1), np.where(t["max_hi"] >= thr, 0, -1)
        for k, ray in enumerate(t["rays"]):
            tn, jc, jp = float(t["tn"][k]), int(j_cert[k]), int(j_poss[k])
            per_ray.setdefault(int(ray), []).append((tn, int(t["c_lo"][k]), int(t["c_hi"][k]), None if jc < 0 else jc,
                                                     None if jp < 0 else jp, tn + (jc + 1) * step, top[t["node"]]))
    w = Window()
    w.ray_lo, w.ray_hi = np.zeros(s.H * s.W, dtype=np.int64), np.zeros(s.H * s.W, dtype=np.int64)
    w.tied = np.zeros(s.H * s.W, dtype=bool)
    for ray, visits in per_ray.items():
        orders = _orders(visits, loop)
        got = [_iso_ray([visits[k] for k in order], thr) for order in orders]
        w.ray_lo[ray], w.ray_hi[ray] = min(g[0] for g in got), max(g[1] for g in got)
        w.tied[ray] = len(orders) > 1
    w.ray_lo, w.ray_hi, w.tied = (a.reshape(s.H, s.W) for a in (w.ray_lo, w.ray_hi, w.tied))
    w.lo, w.hi = int(w.ray_lo.sum()), int(w.ray_hi.sum())
    w.off_lo, w.off_hi = int(r.counts_lo.sum()), int(r.counts_hi.sum())
    w.doubtful = (r.counts_lo != r.counts_hi) | w.tied
    w.hit = r.hit()
    w.ref = r
    return w


def iso_of(name, loop):
    """The window of iso_ref's scene `name` at iso_ref.ISO[name], once per process."""
    key = (name, "iso", loop)
    if key not in _WINDOWS:
        import iso_ref
        _WINDOWS[key] = iso_window(iso_ref.scene(name), iso_ref.ISO[name], loop)
    return _WINDOWS[key]
