"""The oracle and the host build of the kernel code (vrc_core.h) against tests/ref64.py, an independent float64
restatement of the reference's ray cast.  Everything else in the suite compares with the oracle; here the oracle itself
is the thing under test.  Every comparison is the frozen rule of tests/scenes.py, unchanged, with ref64's OWN tie budget:
scenes.assert_parity(frame, ref64 frame, budget=B64).

The cases (CASES, case()) are shared with tests/test_ref64_gpu.py.  With VRC_REF64_STATS=<file> every comparison is
appended to <file> as one JSON line (profiles/ref64_parity_errors.json is made from such a run)."""
import functools
import json
import os

import numpy as np
import pytest

import nongrid
import orc
import ref64
import scenes
from test_cpu_harness import NONGRID, U16_SCENES, _fuzz_scene, nongrid_scene

_STATS = os.environ.get("VRC_REF64_STATS")


# ---- smooth volumes: scenes on which the tie budget cannot be what makes a comparison pass -------------------------------
# A quantised sum of three slow sines: neighbouring voxels differ by at most one level, so ONE flipped sample changes a
# pixel by at most about alpha / 255 x 32 / 512 = 1.2e-5 with the thin ramp at 512 samples per ray, and the mean tie
# budget of a frame stays below E0 (asserted).  A half-voxel or one-voxel position error, a wrong exponent or a shifted
# table lookup is a systematic error of 10-100 x E0 on them.
def smooth_volume(n=64, mean=80.0, amp=2.0):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    v = mean + amp * (np.sin(2 * np.pi * x / 61.0 + 0.3) + np.sin(2 * np.pi * y / 47.0 + 1.1) +
                      np.sin(2 * np.pi * z / 53.0 + 2.0))
    return np.floor(v + 0.5).astype(np.uint8)


SMOOTH = {
    "smooth_a": dict(spin=(0.7, 0.4), viewport=(40, 40)),
    "smooth_b": dict(spin=(-1.9, -0.6), viewport=(36, 44)),
    "smooth_clip": dict(spin=(2.6, 0.9), viewport=(44, 36), planes=[[0.6, 0.0, 0.8, 0.3]]),
}


def smooth_scene(name, **over):
    kw = dict(SMOOTH[name], **over)
    return orc.build_scene(voxels=(64, 64, 64), block=16, volume=smooth_volume(), **kw)


def saturated_scene():
    """alpha = 1.0 and voxels that reach the top of the table, where the 255/256 clamp of composite acts
    (cuda/Renderer.cu:88): the noise volume with its upper values raised to 255."""
    vol = orc.hash_volume(64, 64, 64)
    vol[vol > 150] = 255
    return orc.build_scene(voxels=(64, 64, 64), block=16, viewport=(40, 40), volume=vol, spin=(0.3, -0.2), alpha=1.0)


# ---- the cases --------------------------------------------------------------------------------------------------------
#: name -> how ref64, the oracle, the host build and the GPU render it: passes of the node list, pixel stride
CASES = (sorted(scenes.SCENES) + ["nucleon"] + sorted(U16_SCENES) + ["c1", "two_pass"] + NONGRID + sorted(SMOOTH) +
         ["saturated"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, passes or None, (row stride, column stride))."""
    if name in scenes.SCENES:
        return scenes.get(name), None, (1, 1)
    if name == "nucleon":
        return scenes.nucleon_scene(), None, (1, 1)
    if name in U16_SCENES:
        return orc.build_scene(**U16_SCENES[name]), None, (1, 1)
    if name == "c1":
        # mem://#128,128,128,32, 512^2 viewport, 512 samples per ray; ref64 takes every 8th row and
        # column of that viewport (4096 of its rays)
        return orc.build_scene(voxels=(128, 128, 128), block=32, viewport=(512, 512)), None, (8, 8)
    if name == "two_pass":
        s = scenes.get("hash64_spin")
        return s, [(0, s.n_nodes // 2), (s.n_nodes // 2, s.n_nodes)], (1, 1)
    if name in NONGRID:
        return nongrid_scene(name), None, (1, 1)
    if name in SMOOTH:
        return smooth_scene(name), None, (1, 1)
    if name == "saturated":
        return saturated_scene(), None, (1, 1)
    raise KeyError(name)


_REF = {}


def ref(name, filter_mode=0, frac_bits=8):
    """ref64's frame of a case, computed once per process."""
    key = (name, filter_mode, frac_bits)
    if key not in _REF:
        s, passes, stride = case(name)
        if passes:
            _REF[key] = ref64.render_passes(s, passes, filter_mode=filter_mode, frac_bits=frac_bits)
        else:
            _REF[key] = ref64.render(s, filter_mode=filter_mode, frac_bits=frac_bits, stride=stride)
    return _REF[key]


def check(s, got, n_got, r, what, impl, stride=(1, 1), count=True):
    """THE comparison: the frozen rule with ref64's budget; the sample count within 1e-4 n + 8 (what
    test_scene_parity_both_kernels grants the reference-order kernel)."""
    got = got[::stride[0], ::stride[1]]
    orc._LAST_SCENE = s  # assert_parity takes its weak / strong decision from the scene under test
    if _STATS:
        d = np.abs(got.astype(np.float64) - r.frame).max(axis=-1)
        free = r.budget == 0.0
        rec = dict(scene=what, impl=impl, max_tie_free=float(d[free].max()) if free.any() else None, max=float(d.max()),
                   mean=float(d.mean()), budget_mean=float(r.budget.mean()),
                   budget_use=float(max(d.mean() - scenes.MEAN_E0, 0.0) / r.budget.mean()) if r.budget.mean() > 0 else 0.0,
                   samples_ref64=int(r.samples), samples=None if n_got is None else int(n_got))
        with open(_STATS, "a") as f:
            f.write(json.dumps(rec) + "\n")
    scenes.assert_parity(got, r.frame, "%s, %s against ref64" % (what, impl), budget=r.budget)
    if count and stride == (1, 1):
        assert abs(n_got - r.samples) <= 1e-4 * r.samples + 8, (what, impl, n_got, r.samples)


def oracle(s, passes=None, stride=(1, 1), **kw):
    if passes:
        return nongrid.oracle_passes(s, passes, threads=4, **kw)
    rows = None if stride[0] == 1 else (0, s.H, stride[0])
    return orc.oracle_render(s, threads=4, rows=rows, **kw)


def harness_kernels(s, filter_mode, grid=True):
    """Every kernel id of the host build that renders the scene with this filter (tests/orc.py: harness_render):
    1 / 2 reference order / grid walk, 3 / 4 with fixed-point stepping, 7 / 8 classified per sample, 5 / 6 trilinear
    gathers, 9 / 10 the tap-packed atlas, 11 / 12 its (grey, alpha) form.  Lists that are no grid: the odd ids."""
    u16 = s.atlas.dtype.itemsize == 2
    packed = min(s.vi.overlap[a] for a in range(3)) >= 1 and max(s.slot_dim) <= 248
    grey = (s.tf[:, 0] == s.tf[:, 1]).all() and (s.tf[:, 0] == s.tf[:, 2]).all()
    if filter_mode:
        ids = [5, 6] + ([9, 10] + ([11, 12] if grey else []) if packed else [])
    else:
        ids = ([] if u16 else [1, 2, 3, 4]) + [7, 8]
    return [k for k in ids if grid or k % 2 == 1]


def harness(s, kernel, passes=None, **kw):
    if not passes:
        return orc.harness_render(s, kernel=kernel, **kw)
    fb, total = None, 0
    for t in nongrid.passes_of(s, passes):
        fb, n, ok = orc.harness_render(t, kernel=kernel, fb=fb, **kw)
        total += n
    return fb, total, ok


def is_grid(s):
    return orc.harness_render(s, kernel=7)[2]


# ---- the two addressings name the same voxel ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(scenes.SCENES) + ["nucleon"] + sorted(U16_SCENES))
def test_brick_local_and_atlas_addressing_name_the_same_voxel(name):
    # ref64 reads s.bricks[nid] at overlap + rel x blockSize; the reference, the oracle and the kernels read the atlas at
    # (textureMin + rel x textureSize) x atlas size (cuda/Renderer.cu:210-214, CudaTextureObject.cpp:61-84).  At every
    # voxel centre of every brick the two must be the same voxel: this pins textureMin / textureSize, the slot order and
    # the atlas layout, which ref64 by design does not see.
    s, _, _ = case(name)
    dim = np.array(s.atlas_dim, dtype=np.float64)
    for i, nid in enumerate(ref64.node_ids(s)):
        nd = s.nodes[i]
        bs = [int(s.lod[nid].blockSize[a]) for a in range(3)]
        rel = np.stack(np.meshgrid(*[(np.arange(b) + 0.5) / b for b in bs], indexing="ij"), axis=-1).reshape(-1, 3)
        c = np.floor(ref64.brick_coords(s, nid, rel)).astype(int)
        local = s.bricks[nid][c[:, 2], c[:, 1], c[:, 0]]
        tmin = np.array([float(nd.textureMin[a]) for a in range(3)])
        tsize = np.array([float(nd.textureSize[a]) for a in range(3)])
        t = np.floor((tmin + rel * tsize) * dim).astype(int)
        assert (s.atlas[t[:, 2], t[:, 1], t[:, 0]] == local).all(), (name, i)


# ---- the oracle against ref64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_ref64(name):
    s, passes, stride = case(name)
    got, n_got = oracle(s, passes, stride)
    check(s, got, n_got, ref(name), name, "oracle", stride)


@pytest.mark.parametrize("name", sorted(scenes.SCENES) + ["nucleon"] + sorted(U16_SCENES) + NONGRID + sorted(SMOOTH))
def test_oracle_trilinear_matches_ref64(name):
    # the extension as the words of include/vrc_hip.h define it (tests/ref64.py), not as the oracle's code does
    s, passes, stride = case(name)
    got, n_got = oracle(s, passes, stride, filter_mode=1)
    check(s, got, n_got, ref(name, filter_mode=1), name + " trilinear", "oracle", stride)


@pytest.mark.parametrize("name", ["hash64_spin", "hash64_ert", "smooth_a", "nucleon"])
def test_oracle_exact_tf_weight_matches_ref64(name):
    # frac_bits = 0 against the exact lerp weight, frac_bits = 8 (every other test) against the 1.8 fixed-point one
    s, passes, stride = case(name)
    got, n_got = oracle(s, passes, stride, frac_bits=0)
    check(s, got, n_got, ref(name, frac_bits=0), name + " exact weight", "oracle", stride)


# ---- the host build of vrc_core.h against ref64, without going through the oracle ---------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_build_matches_ref64(name):
    s, passes, stride = case(name)
    grid = all(is_grid(t) for t in (nongrid.passes_of(s, passes) if passes else [s]))
    for f in (0, 1):
        if f and name in ("c1", "two_pass", "saturated"):
            continue
        for k in harness_kernels(s, f, grid):
            got, n_got, _ = harness(s, k, passes)
            check(s, got, n_got, ref(name, filter_mode=f), "%s%s" % (name, " trilinear" if f else ""), "host k%d" % k,
                  stride)
    if name in ("hash64_spin", "smooth_a"):
        got, n_got, _ = harness(s, 2, passes, frac_bits=0)
        check(s, got, n_got, ref(name, frac_bits=0), name + " exact weight", "host k2", stride)


# ---- random views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16 * scenes.FUZZ_SCALE))
def test_random_views_match_ref64(seed):
    # _fuzz_scene draws volumes, cameras inside and outside, clip planes, viewports and step sizes; its `mem` volumes
    # give neighbouring bricks different constants, overlap included -- which is why ref64 samples brick-locally
    rng = np.random.default_rng(64000 + seed)
    kw = _fuzz_scene(rng)
    s = orc.build_scene(**kw)
    what = "seed %d %r" % (seed, kw)
    r = ref64.render(s)
    got, n_got = orc.oracle_render(s, threads=4)
    check(s, got, n_got, r, what, "oracle")
    for k in (1, 2, 4):
        got, n_got, _ = orc.harness_render(s, kernel=k)
        check(s, got, n_got, r, what, "host k%d" % k)
    r = ref64.render(s, filter_mode=1)
    got, n_got = orc.oracle_render(s, threads=4, filter_mode=1)
    check(s, got, n_got, r, what + " trilinear", "oracle")
    got, n_got, _ = orc.harness_render(s, kernel=6)
    check(s, got, n_got, r, what + " trilinear", "host k6")


# ---- the smooth scenes are what they claim ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_scenes_leave_no_room_in_the_budget(name):
    s, _, _ = case(name)
    vol = smooth_volume().astype(int)
    for ax in range(3):
        assert np.abs(np.diff(vol, axis=ax)).max() <= 1
    assert s.render.samplesPerRay == 512 and float(s.tf[:, 3].max()) == np.float32(0.05)
    r = ref(name)
    assert r.budget.mean() < scenes.E0, r.budget.mean()
    assert r.frame[..., 3].max() > 0.05


# ---- the rule has teeth -------------------------------------------------------------------------------------------------
#: deliberate misreading of the reference -> the cases on each of which the comparison must throw it out (filter)
TEETH = {
    "half_voxel_x": (["smooth", "hash64_spin"], 0),
    "pixel_centre": (["smooth", "hash64_spin"], 0),
    "exponent_spr_plus_1": (["smooth", "hash64_spin"], 0),
    "tf_no_half_texel": (["smooth", "hash64_spin"], 0),
    "alpha_clamp_1": (["saturated"], 0),
    "clip_sign": (["hash_clip"], 0),
    "floor_count": (["smooth", "hash64_spin"], 0),
    "trilinear_centre_i": (["hash64_spin"], 1),
}


def test_the_mutation_list_is_complete():
    assert sorted(TEETH) == sorted(ref64.MUTATIONS)


def _rejected(name, mutation, f):
    s, passes, stride = case(name)
    got, _ = oracle(s, passes, stride, filter_mode=f)
    good = ref(name, filter_mode=f)
    check(s, got, None, good, name, "oracle", count=False)  # the control: unmutated, it passes
    bad = ref64.render(s, filter_mode=f, _mutate=mutation)
    assert np.abs(bad.frame - good.frame).max() > 0.0
    orc._LAST_SCENE = s
    try:
        scenes.assert_parity(got, bad.frame, name, budget=bad.budget)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutation", sorted(TEETH))
def test_parity_rule_rejects_a_misread_reference(mutation):
    # NEGATIVE CONTROL (as test_parity_rule_rejects_a_biased_kernel): each misreading is applied to ref64 alone; the
    # comparison with the oracle must then fail -- on the named scene, or on a smooth-volume scene AND on hash64_spin
    names, f = TEETH[mutation]
    for name in names:
        if name == "smooth":
            assert any(_rejected(n, mutation, f) for n in sorted(SMOOTH)), "%s passes on every smooth scene" % mutation
        else:
            assert _rejected(name, mutation, f), "%s passes on %s" % (mutation, name)
