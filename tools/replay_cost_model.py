"""A cost model of the uniform-only lean replay on the judged frame, on the CPU (numpy alone: no GPU, no library).

What it models.  The C2 view: eye (0, 0, 1.5) looking at the origin, frustum -/+0.05 at near 0.1, a unit cube of 8^3
bricks, step 1 / 1024, a square viewport in tiles of 8 x 8 pixels, one wave per tile.  A ray's visits are the stretches
between the brick planes it crosses inside the cube, each of n = ceil(length / step) samples; the lanes of a wave march
their k-th visits together.  The first visit comes from the table where n < 256 (VRC_OPT_FIRST_VISIT_TABLE) and costs
nothing here.  A wave pays for a visit
    group * max over its lanes of (n // group)   samples in whole groups, at `trip` instructions of loop control each,
    plus every remainder body (group / 2 ... 1)  that any of its lanes needs (a bit of n set in some lane),
at three vector instructions a sample (v_sub_f32 and two v_fmac_f32 in the grey form).  Loads, the per-visit set-up
and the prologue are not modelled: the model says where the march's own instructions go, not what the kernel costs.

usage: python tools/replay_cost_model.py [--spin X Y] [--viewport 1024] [--group 32] [--trip 8] [--free-group 8] [--free-trip 1]
prints one JSON line per camera (the default one and --spin, default 0.5235988 0.3490659): samples per frame, the
first visits' share of them, the share of lanes active on sample instructions, and steps, trips and march
instructions per wave for the tested march (--group, --trip) and the free body (--free-group, --free-trip) beside the
steps per wave of groups of 64, 32, 16 and 8."""
import argparse
import json

import numpy as np

BRICKS = 8
STEP = 1.0 / 1024.0
ROWS = 256  # rows of the first-visit table


def rays(viewport, spin):
    """Origin and unit directions in the volume's frame: the model view is Ry(y) Rx(x) behind the look-at, the eye stays
    1.5 in front of the origin (the oracle's orc_spin_model)."""
    x, y = spin
    cx, sx, cy, sy = np.cos(x), np.sin(x), np.cos(y), np.sin(y)
    rx = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]])
    ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
    rot = ry @ rx  # world -> eye
    c = (np.arange(viewport) + 0.5) / viewport * 0.1 - 0.05
    px, py = np.meshgrid(c, c)
    d = np.stack([px, py, np.full_like(px, -0.1)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origin = rot.T @ np.array([0.0, 0.0, 1.5])
    return origin, d @ rot  # (rot^T d, row-wise)


def visits(viewport, spin):
    """n[ray, k]: the samples of the ray's k-th visit, 0 behind its last one."""
    o, d = rays(viewport, spin)
    planes = np.arange(BRICKS + 1) / BRICKS - 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (planes[None, None, :] - o[None, :, None]) / d[:, :, None]  # ray, axis, plane
    t = np.where(np.isfinite(t), t, np.inf)
    lo, hi = np.minimum(t[..., 0], t[..., -1]), np.maximum(t[..., 0], t[..., -1])
    enter, leave = np.maximum(lo.max(axis=1), 0.0), hi.min(axis=1)
    hit = leave > enter
    cuts = np.sort(np.clip(t.reshape(len(d), -1), enter[:, None], np.maximum(leave, enter)[:, None]), axis=1)
    n = np.ceil(np.diff(cuts, axis=1) / STEP - 1e-6).astype(np.int64)
    n[~hit] = 0
    order = np.argsort(n == 0, axis=1, kind="stable")  # the visits to the front, in their order
    return np.take_along_axis(n, order, axis=1)


def waves(n, viewport):
    tiles = viewport // 8
    k = n.shape[1]
    return n.reshape(tiles, 8, tiles, 8, k).transpose(0, 2, 1, 3, 4).reshape(tiles * tiles, 64, k)


def march(w, group):
    """(steps, trips) per wave: what the waves pay for the visits of w (wave, lane, visit) in groups of `group`."""
    trips = (w // group).max(axis=1)
    steps = group * trips
    body = group // 2
    while body:
        steps = steps + body * ((w & body) != 0).any(axis=1)
        body //= 2
    return steps.sum(axis=1), trips.sum(axis=1)


def figures(viewport, spin, group, trip, free_group, free_trip):
    n = visits(viewport, spin)
    total = int(n.sum())
    w = waves(n, viewport)
    first = w[:, :, 0]
    marched = w.copy()
    marched[:, :, 0] = np.where(first < ROWS, 0, first)  # the table's share is not marched
    out = {"spin": list(spin), "viewport": viewport, "samples_per_frame": total,
           "first_visit_share": round(float(first.sum()) / total, 4),
           "visits_per_ray_hit": round(float((n > 0).sum()) / max(1, int((n[:, 0] > 0).sum())), 2)}
    by = {}
    for g in (64, 32, 16, 8):
        steps, _ = march(marched, g)
        by[str(g)] = round(float(steps.mean()), 1)
    out["steps_per_wave_by_group"] = by
    for name, g, t in (("tested", group, trip), ("free", free_group, free_trip)):
        steps, trips = march(marched, g)
        out[name] = {"group": g, "trip": t, "steps_per_wave": round(float(steps.mean()), 1),
                     "trips_per_wave": round(float(trips.mean()), 1),
                     "march_instructions_per_wave": round(float((3 * steps + t * trips).mean()), 1),
                     "lanes_active": round(float(marched.sum()) / (64.0 * float(steps.sum())), 4)}
    out["free_minus_tested"] = round(out["free"]["march_instructions_per_wave"] - out["tested"]["march_instructions_per_wave"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spin", type=float, nargs=2, default=(0.5235988, 0.3490659))
    ap.add_argument("--viewport", type=int, default=1024)
    ap.add_argument("--group", type=int, default=32, help="samples per group of the tested march")
    ap.add_argument("--trip", type=float, default=8.0, help="its loop-control instructions per trip")
    ap.add_argument("--free-group", type=int, default=8)
    ap.add_argument("--free-trip", type=float, default=1.0)
    a = ap.parse_args()
    for spin in ((0.0, 0.0), tuple(a.spin)):
        print(json.dumps(figures(a.viewport, spin, a.group, a.trip, a.free_group, a.free_trip)))


if __name__ == "__main__":
    main()
