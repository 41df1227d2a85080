"""The lean replay with its prefetches unconditional (vrc_core.h: vrc_lean_list_word, vrc_lean_slot_load) on the GPU.

vrc_k_raycast_replay<...,lean> reads the words of a ray's first two visits, and in every visit k the list word of
visit min(k + 2, K - 1) and the slot word of visit k + 1, whatever the ray's count says, none of them under a branch;
a visit that gathers takes its interval and ray inside its own branch.  Nothing of the result may change: every frame
here is replayed with VRC_OPT_WALK_CACHE at its default (or at 2 where the bricks gather) and compared, frame and
sample count, bit for bit, with the frame of a context that walks (VRC_OPT_WALK_CACHE = 0); no tolerance appears.
VRC_OPT_WALK_LEAN_USED = 1 is asserted on every replayed frame, and that it was replayed (mode 4).

Shapes, the smallest that reach each edge of the clamped reads: one brick (lists of K = 1 visit: both words in front
of the loop and every prefetch are the clamped one), two bricks along the view axis (K = 2: the second word is the
last, and k + 2 is always clamped), 64^3 in bricks of 32^3 at 64 x 64 (whole tiles; rays of one, two and three visits
in one wave, so counts below K) and at 60 x 52 (partial tiles: ray indices up to the end of the planes' last
whole tile, and a schedule with empty slots), two camera angles, the ramp at alpha 0.05 and at 1.0 (rays end inside a group of 32 and
inside a remainder; over mem:// bricks with the data range narrowed so that they do), row bands, and hash:// volumes
under VRC_OPT_WALK_CACHE = 2: one where every visit gathers and two where a uniform brick and a brick of noise share a
list, in either order, so that the loads a gather visit now makes inside its branch are exercised.  Helpers are those
of tests/test_walk_cache.py."""
import copy

import numpy as np
import pytest

import orc
from test_walk_cache import FRESH, _get, _gpu, _opt, always, frame, table
from test_walk_cache import vrc  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

SHAPES = {
    "one brick": dict(voxels=(32, 32, 32), block=32, viewport=(64, 64)),
    "two bricks along the view axis": dict(voxels=(32, 32, 64), block=32, viewport=(64, 64)),
    "64^3 in 32^3 bricks": dict(voxels=(64, 64, 64), block=32, viewport=(64, 64)),
    "64^3 in 32^3 bricks, partial tiles": dict(voxels=(64, 64, 64), block=32, viewport=(60, 52)),
}
SPINS = [(0.0, 0.0), (0.5, 0.35)]

_scenes = {}


def scene(shape, spin, volume="mem", data_range=None):
    key = (shape, spin, volume, data_range)
    if key not in _scenes:
        vol = banded_volume(volume) if volume.startswith("uniform") else volume
        _scenes[key] = orc.build_scene(spin=spin, spr=256, volume=vol, data_range=data_range, **SHAPES[shape])
    return copy.copy(_scenes[key])  # (tf and view are replaced, never written in place)


def same(got, want, what, counted):
    (fb, n), (wfb, wn) = got, want
    assert np.array_equal(fb, wfb), "%s: %d pixels differ" % (what, int((fb != wfb).any(axis=-1).sum()))
    assert n == wn and (n > 0) == counted, (what, n, wn)


def steady(vrc, g, ref, what, expect=FRESH, **kw):
    """Frames of g reading the modes of `expect`, each equal to the frame of ref (which walks); the replayed ones are
    lean, and the kernel's name says so.  Returns ref's frame."""
    want, m, _ = frame(vrc, ref, **kw)
    assert m == 0, what
    for i, e in enumerate(expect):
        got, m, _ = frame(vrc, g, **kw)
        assert m == e, "%s: frame %d read mode %d, expected %r" % (what, i, m, expect)
        lean = _get(vrc, g, vrc.OPT_WALK_LEAN_USED)
        name = g.L.vrc_last_kernel()
        assert lean == (1 if m == 4 else 0), (what, i, m, lean)
        assert (b"vrc_k_raycast_replay<" in name and name.endswith(b",lean>")) == (m == 4), (what, m, name)
        same(got, want, "%s frame %d (mode %d)" % (what, i, m), kw.get("count", True))
    assert expect[-1] == 4, what  # (every call ends on a replayed frame)
    return want


def all_tables(vrc, g, ref, what, opaque=None):
    """alpha 0.05 and 1.0, grey (the two-float instances) and coloured (the four-float ones), counted and uncounted,
    over one recording of the lists.  opaque: the render data of the frames at alpha 1.0 (below)."""
    expect = FRESH
    for alpha in (0.05, 1.0):
        if alpha == 1.0 and opaque is not None:
            g.s.render = ref.s.render = opaque
        for coloured in (False, True):
            g.s.tf = ref.s.tf = table(alpha, coloured)
            w = "%s alpha %g coloured %d" % (what, alpha, coloured)
            fb, _ = steady(vrc, g, ref, w, expect=expect)
            assert fb[..., 3].max() > 0.05, w  # rays that hit
            if alpha == 1.0:
                assert fb[..., 3].max() > 0.999, w  # early ray termination
            steady(vrc, g, ref, w + " uncounted", expect=(4,), count=False)
            expect = (4,)  # the transfer function changes nothing of the lists


@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_uniform_bricks_replay_the_walked_frame(vrc, shape, spin):
    s = scene(shape, spin)
    assert s.n_nodes == {"one brick": 1, "two bricks along the view axis": 2}.get(shape, 8)
    # the bricks of mem:// volumes this small hold 16 to 37 of 255, and the ramp at alpha 1.0 ends no ray over them:
    # the frames at alpha 1.0 map the data range 0 .. 40 onto the ramp instead (the lists do not depend on it), under
    # which the oracle's frame of each of these scenes passes 0.999 and takes a half to a quarter of the samples
    opaque = scene(shape, spin, data_range=(0.0, 40.0)).render
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)  # (g keeps the default, 1)
        all_tables(vrc, g, ref, "%s spin %r" % (shape, spin), opaque)
        # the planes hold 1 + 4 K words per ray of every whole tile
        W, H = SHAPES[shape]["viewport"]
        plane = ((W + 7) // 8) * ((H + 7) // 8) * 64 * 4
        used = _get(vrc, g, vrc.OPT_WALK_CACHE_BYTES)
        assert used % plane == 0 and (used // plane - 1) % 4 == 0, (used, plane)
        k = (used // plane - 1) // 4
        if shape == "one brick":
            assert k == 1
        elif shape == "two bricks along the view axis" and spin == (0.0, 0.0):
            assert k == 2
        else:
            assert k >= 2


def test_row_bands(vrc):
    s = scene("64^3 in 32^3 bricks", (0.5, 0.35))
    s.tf = table(0.3, False)
    rows = np.ascontiguousarray(list(range(3, 20)) + list(range(40, 57)), dtype=np.uint32)
    banded = copy.copy(s)
    banded.H = len(rows)
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        whole = steady(vrc, g, ref, "whole frame")
        for x in (g, ref):
            vrc.check(x.L, x.L.vrc_set_row_map(x.ctx, rows.ctypes.data, len(rows)))
            x.s = copy.copy(banded)
        part = steady(vrc, g, ref, "row bands")
        assert np.array_equal(part[0], whole[0][rows])


def banded_volume(which):
    """64^3 of noise with a slab across z, the axis the default camera looks along, that makes the four bricks of one
    z layer uniform (overlap included) and leaves the four of the other layer noise: a ray's list holds a visit that
    gathers and a uniform one, in the one order or the other."""
    vol = orc.hash_volume(64, 64, 64)
    if which == "uniform low z":
        vol[:36, :, :] = 90
    else:
        vol[28:, :, :] = 200
    return vol


@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("volume", ["hash", "uniform low z", "uniform high z"])
def test_gather_visits_take_their_loads_inside_their_branch(vrc, volume, spin):
    s = scene("64^3 in 32^3 bricks, partial tiles", spin, volume)
    uniform = sum(1 for b in s.bricks.values() if (b == b.flat[0]).all())
    assert uniform == (0 if volume == "hash" else 4), uniform
    with _gpu(s) as g, _gpu(s) as ref:
        _opt(vrc, ref, vrc.OPT_WALK_CACHE, 0)
        always(vrc, g)  # VRC_OPT_WALK_CACHE = 2: replay whatever the bricks hold
        all_tables(vrc, g, ref, "%s spin %r" % (volume, spin))
