"""A slice frame (include/vrc_hip.h, "A slice frame") without a GPU: the acceptance rule of tests/slice_ref.py against
its own answer and deliberate misreadings of it, the condition that keeps the rule honest for every scene the GPU tests
use, and the host build of the per-pixel code (tests/cpu_harness/slice_harness.cpp: vrc_pixel_slice as g++ compiles it)
held to the rule; the refusals and latches of vrc_plan_mode for the new mode; the samplers under the sanitizers as a
program of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mip_scenes
import slice_ref as sr
import voxel_types
from libre_amd import vrc

FORMS = [(0, "reforder"), (sr.GRID, "grid")]
FILTERS = [(0, "nearest"), (1, "trilinear")]


def _form(grid, filter_mode, uniform=False):
    return grid | (sr.TRILINEAR if filter_mode else 0) | (sr.UNIFORM if uniform else 0)


def _report(what, r, bad):
    print("%s: %d failing pixels; %d covered, %d with more than one candidate value (share %.4f)" % (
        what, bad, int(r.covered().sum()), int(r.multi().sum()), r.share()))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("name", sr.RULE_SCENES)
def test_the_rule_accepts_its_own_answer(name, filter_mode):
    r = sr.ref(name, filter_mode)
    v, c, d = r.own()
    assert int(c.sum()) > 100
    assert sr.check(r, v, c, d) == 0


@pytest.mark.parametrize("mutate", [m for m in sr.MUTATIONS if m != "later_pass_overwrites"])
@pytest.mark.parametrize("filter_mode", [0, 1], ids=["nearest", "trilinear"])
def test_the_rule_rejects_a_misreading(filter_mode, mutate):
    """"clip" has the clip planes `unclipped` drops; the others are as wrong in every scene."""
    r = sr.ref("clip", filter_mode)
    v, c, d = r.own(mutate)
    bad = sr.check(r, v, c, d)
    print("%s, filter %d: %d of %d covered pixels fail" % (mutate, filter_mode, bad, int(r.covered().sum())))
    assert bad > 0.2 * int(r.covered().sum())


@pytest.mark.parametrize("order", ["front first", "back first"])
def test_the_rule_rejects_a_later_pass_that_overwrites(order):
    s, pl = sr.scene("oblique"), sr.plane("oblique")
    r, h = sr.ref("oblique"), s.n_nodes // 2
    halves = [(0, h), (h, s.n_nodes)] if order == "front first" else [(h, s.n_nodes), (0, h)]
    refs = [sr.render(s, pl, 0, nodes=p) for p in halves]
    first, second = [q.own() for q in refs]
    assert int(first[1].sum()) > 50 and int(second[1].sum()) > 50
    # (a pixel on the face between the halves is sure of its sample in the whole list and in neither half: own() of a
    # half leaves it out, and that is all the merged answer may miss)
    between = r.sure & ~refs[0].sure & ~refs[1].sure
    assert sr.check(r, *sr.merge(first, second)) == int(between.sum()) <= 0.01 * int(r.sure.sum())
    bad = sr.check(r, *second)  # what the later pass made of every pixel, sampled before or not
    assert bad >= int(first[1].sum()) - int((first[1] & second[1]).sum())


# ---- the cap: a condition of the scenes, asserted for every one the GPU tests use -------------------------------------
def _all_refs():
    for name in sr.RULE_SCENES + ("mem", "zindex"):
        for fm in (0, 1):
            yield name, sr.ref(name, fm)
    for fm in (0, 1):
        yield "nucleon", sr.nucleon_ref(fm)
        yield "lod", sr.render(sr.lod_scene(), sr.plane("oblique"), fm)
        for image in mip_scenes.TYPED_IMAGES:
            yield image, sr.typed_ref(image, fm)
    yield "allnan_brick", sr.nan_ref()


def test_every_scene_stays_under_the_cap():
    for name, r in _all_refs():
        cov = r.covered()
        assert int(cov.sum()) > 100, name
        print("%s filter %d: share %.4f, least |cos| %.3f" % (name, r.filter_mode, r.share(), float(r.cos[cov].min())))
        assert r.share() <= sr.MULTI_CAP, name
        assert float(r.cos[cov].min()) >= sr.MIN_COS, name
    # the exempt scenes are what they say they are
    assert not sr.ref("behind").covered().any() and not sr.ref("outside").covered().any()
    face = sr.ref("face")
    both = sum(1 for c in face.cands.values() if len({q[2] for q in c}) > 1)
    assert both == int(face.covered().sum()) > 100  # every covered pixel lies on the face of two bricks
    assert face.sure.sum() == face.covered().sum()   # ... and none may go unsampled


# ---- 2., 3. the host build passes the rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode,fname", FILTERS, ids=[f[1] for f in FILTERS])
@pytest.mark.parametrize("grid,gname", FORMS, ids=[f[1] for f in FORMS])
@pytest.mark.parametrize("name", sr.RULE_SCENES + ("behind", "outside", "face", "mem"))
def test_the_host_build_passes_the_rule(name, grid, gname, filter_mode, fname):
    s, r = sr.scene(name), sr.ref(name, filter_mode)
    fb, n, v, c, d = sr.harness_render(s, _form(grid, filter_mode), sr.plane(name))
    bad = sr.check(r, v, c, d, fb)
    _report("%s %s %s" % (name, gname, fname), r, bad)
    assert bad == 0
    assert n == int(c.sum())
    if name in ("behind", "outside"):
        assert n == 0 and not fb.any() and np.isposinf(d).all()
    if name == "face":
        assert (c[r.covered()] == 1).all()


@pytest.mark.parametrize("filter_mode,fname", FILTERS, ids=[f[1] for f in FILTERS])
def test_the_host_build_on_a_brick_without_overlap_and_a_cut_of_mixed_sizes(filter_mode, fname):
    s, r = sr.nucleon_scene(), sr.nucleon_ref(filter_mode)
    for grid, gname in FORMS:
        fb, n, v, c, d = sr.harness_render(s, _form(grid, filter_mode), sr.NUCLEON_PLANE)
        assert sr.check(r, v, c, d, fb) == 0 and n == int(c.sum()) > 100, gname
    s = sr.lod_scene()
    r = sr.render(s, sr.plane("oblique"), filter_mode)
    fb, n, v, c, d = sr.harness_render(s, _form(0, filter_mode), sr.plane("oblique"))
    bad = sr.check(r, v, c, d, fb)
    _report("lod cut %s" % fname, r, bad)
    assert bad == 0 and n > 100


@pytest.mark.parametrize("filter_mode,fname", FILTERS, ids=[f[1] for f in FILTERS])
@pytest.mark.parametrize("image", mip_scenes.TYPED_IMAGES)
def test_the_host_build_on_the_typed_images(image, filter_mode, fname):
    """uint16 voxels q behind every image v = a + b q: the host build renders q (16-bit voxels), and for the float image
    the float atlas itself, whose values are carried back to q."""
    q, t, _ = mip_scenes.typed(image)
    r = sr.typed_ref(image, filter_mode)
    for grid, gname in FORMS:
        fb, n, v, c, d = sr.harness_render(q, _form(grid, filter_mode), sr.TYPED_PLANE)
        assert sr.check(r, v, c, d, fb) == 0 and n > 100, gname
        if image == "float":
            im = voxel_types.IMAGES[image]
            fb, n, v, c, d = sr.harness_render(t, _form(grid, filter_mode), sr.TYPED_PLANE)
            vq = (v.astype(np.float64) - im.a) / im.b
            assert sr.check(r, vq, c, d, fb) == 0 and n > 100, gname


# ---- 4. uniform bricks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,gname", FORMS, ids=[f[1] for f in FORMS])
@pytest.mark.parametrize("name", ["mem", "oblique"])
def test_uniform_bricks_change_nothing(name, grid, gname):
    s = sr.scene(name)
    if name == "mem":
        assert mip_scenes.uniform_and_mixed(s)[0] == len(s.bricks)
    off = sr.harness_render(s, _form(grid, 0), sr.plane(name))
    on = sr.harness_render(s, _form(grid, 0, uniform=True), sr.plane(name))
    assert off[1] == on[1] > 100
    for a, b in zip(off, on):
        assert np.array_equal(a, b)


# ---- 5. two passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_mode,fname", FILTERS, ids=[f[1] for f in FILTERS])
@pytest.mark.parametrize("grid,gname", FORMS, ids=[f[1] for f in FORMS])
def test_two_passes_in_both_orders(grid, gname, filter_mode, fname):
    s, pl, r = sr.scene("oblique"), sr.plane("oblique"), sr.ref("oblique", filter_mode)
    h = s.n_nodes // 2
    one = sr.harness_render(s, _form(0, filter_mode), pl)
    single = r.single_node()
    assert int(single.sum()) > 100
    for passes in ([(0, h), (h, s.n_nodes)], [(h, s.n_nodes), (0, h)]):
        fb, n, v, c, d = sr.harness_render(s, _form(grid, filter_mode), pl, passes=passes)
        assert sr.check(r, v, c, d, fb) == 0
        assert n == int(c.sum()) == one[1]
        for a, b in zip((fb, v, c, d), (one[0], one[2], one[3], one[4])):
            assert np.array_equal(a[single], b[single])


# ---- 6. known answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,gname", FORMS, ids=[f[1] for f in FORMS])
def test_known_answers(grid, gname):
    s = sr.scene("zindex")  # the voxel is its z index: the axial slice through layer k reads k
    fb, n, v, c, d = sr.harness_render(s, _form(grid, 0), sr.plane("zindex"))
    assert n > 100 and (v[c == 1] == sr.AXIAL_LAYER).all()
    fb, n, v, c, d = sr.harness_render(s, _form(grid, 1), sr.plane("zindex"))
    assert n > 100 and np.abs(v[c == 1] - sr.AXIAL_LAYER).max() <= 1e-3  # the centre of the layer: a linear ramp along z
    s, r = sr.scene("mem"), sr.ref("mem")  # mem://: V is the brick's constant
    fb, n, v, c, d = sr.harness_render(s, _form(grid, 0), sr.plane("mem"))
    consts = {int(b.flat[0]) for b in s.bricks.values()}
    assert n > 100 and set(np.unique(v[c == 1]).astype(int)) <= consts
    assert sr.check(r, v, c, d, fb) == 0


def test_edge_on():
    """A plane that contains the central ray -- n.dir is 0 there and the eye lies in the plane -- and one just beside it,
    which the rays around the centre graze: no rule but sanity."""
    s = sr.scene("edge-on")
    lo, hi = min(int(b.min()) for b in s.bricks.values()), max(int(b.max()) for b in s.bricks.values())
    for pl in (sr.plane("edge-on"), sr.plane_through((0.03, 0.0, 0.0), (1.0, 0.0, 0.0))):
        for grid, _ in FORMS:
            for fm in (0, 1):
                fb, n, v, c, d = sr.harness_render(s, _form(grid, fm), pl)
                assert np.isfinite(fb).all()
                assert np.array_equal(c == 1, np.isfinite(d)) and set(np.unique(c)) <= {0, 1}
                assert not fb[c == 0].any()
                assert ((v[c == 1] >= lo) & (v[c == 1] <= hi)).all()
    assert n > 0  # the plane beside the centre is sampled somewhere


# ---- 7. the plan -----------------------------------------------------------------------------------------------------------
def _plan():
    here, _, _ = sr.harness_paths()
    src = os.path.join(here, "cpu_harness", "slice_plan_harness.cpp")
    out = os.path.join(here, "cpu_harness", "libslice_plan_harness.so")
    deps = [src, os.path.join(sr.orc.ROOT, "libre_amd", "csrc", "vrc_plan.h"), os.path.join(sr.orc.ROOT, "include", "vrc_hip.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", tmp, src])
        os.replace(tmp, out)
    return C.CDLL(out)


def _mode(projection=vrc.PROJECTION_SLICE, kernel=vrc.KERNEL_AUTO, variant=0, filter_mode=0, shading=0, cdepth=0, preint=0,
          mip_depth=0, ray_lod=0, latch_projection=-1, latched=None, plane=(0.0, 0.0, 1.0, 0.0), elem=1):
    H = _plan()
    opts = (C.c_int64 * 8)(projection, kernel, variant, filter_mode, shading, cdepth, preint, mip_depth)
    f4 = lambda p: None if p is None else (C.c_float * 4)(*p)
    out, msg = (C.c_int32 * 8)(), C.create_string_buffer(512)
    code = H.slice_plan_mode(opts, ray_lod, C.c_int64(latch_projection), f4(latched), f4(plane), elem, out, msg, 512)
    names = ("slice", "mip", "shade", "cdepth", "preint", "classify", "linear", "plain")
    return code, msg.value.decode(), dict(zip(names, [bool(v) for v in out]))


def test_plan_mode_serves_refuses_and_latches_a_slice_frame():
    code, msg, m = _mode(filter_mode=1, shading=1, cdepth=500, preint=1, mip_depth=1)
    assert code == vrc.VRC_OK and msg == ""
    # the options of the other frames are not read: none of their modes is set, and the frame is no plain composite
    assert m == dict(slice=True, mip=False, shade=False, cdepth=False, preint=False, classify=True, linear=True, plain=False)
    assert _mode(elem=1)[2]["classify"] and not _mode(elem=1)[2]["linear"]
    code, msg, _ = _mode(plane=None)
    assert code == vrc.VRC_EINVAL and "vrc_set_slice" in msg
    for kw, word in ((dict(kernel=vrc.KERNEL_LDS), "VRC_OPT_KERNEL"), (dict(kernel=vrc.KERNEL_PACKED, filter_mode=1), "VRC_OPT_KERNEL"),
                     (dict(ray_lod=1), "vrc_set_ray_lod"), (dict(variant=vrc.VARIANT_GLRAYCASTER), "VRC_OPT_VARIANT")):
        code, msg, _ = _mode(**kw)
        assert code == vrc.VRC_EINVAL and word in msg and "SLICE" in msg, (kw, msg)
    # the latches: the projection, and the plane of the frame's first slice pass
    same = (0.0, 0.0, 1.0, 0.0)
    assert _mode(latch_projection=vrc.PROJECTION_SLICE, latched=same)[0] == vrc.VRC_OK
    for other in ((0.0, 0.0, 1.0, 0.125), (0.0, 1.0, 0.0, 0.0)):
        code, msg, _ = _mode(latch_projection=vrc.PROJECTION_SLICE, latched=other)
        assert code == vrc.VRC_EINVAL and "vrc_set_slice" in msg and "vrc_pre_render" in msg
    code, msg, _ = _mode(latch_projection=vrc.PROJECTION_MIP)
    assert code == vrc.VRC_EINVAL and "VRC_OPT_PROJECTION" in msg
    code, msg, _ = _mode(projection=vrc.PROJECTION_COMPOSITE, latch_projection=vrc.PROJECTION_SLICE, latched=same)
    assert code == vrc.VRC_EINVAL and "VRC_OPT_PROJECTION" in msg
    # another projection is decided as before, whatever the plane
    for projection in (vrc.PROJECTION_COMPOSITE, vrc.PROJECTION_MIP):
        a, b = _mode(projection=projection, plane=None), _mode(projection=projection, latched=(1.0, 0.0, 0.0, 0.0))
        assert a == b and a[0] == vrc.VRC_OK and not a[2]["slice"]


def test_the_untouched_plan_harness_still_builds_and_passes():
    import test_render_plan_cpu as t
    t.test_the_copied_text_has_the_literals_the_issue_counted()
    t.test_mode_and_form_decide_what_the_text_they_replaced_decided()


# ---- 8. the samplers under the sanitizers, as a program of their own ----------------------------------------------------
def test_the_samplers_as_a_stand_alone_program_under_the_sanitizers():
    here, src, deps = sr.harness_paths()
    exe = os.path.join(here, "cpu_harness", "slice_san")
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        tmp = "%s.%d.tmp" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                               "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSLICE_HARNESS_MAIN", "-o", tmp, src])
        os.replace(tmp, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert "pixels sampled" in r.stdout


# ---- the bindings, as far as they go without a GPU ------------------------------------------------------------------------
def test_null_arguments_and_the_weak_binding_of_the_plugin():
    """vrc_set_slice and lvh_app_set_slice name a NULL context / app; the plugin binds vrc_set_slice weakly, so that it
    still links against a device stand-in without the symbol (tests/host_san/vrc_stub.cpp), and setSlice says so there."""
    from libre_amd import driver
    L = vrc.load_library()
    plane = (C.c_float * 4)(0.0, 0.0, 1.0, 0.0)
    assert L.vrc_set_slice(None, plane) == vrc.VRC_EINVAL and b"vrc_set_slice" in L.vrc_last_error()
    D = driver.load_library()
    assert D.lvh_app_set_slice(None, plane) != 0 and b"NULL argument" in D.lvh_last_error()
    root = sr.orc.ROOT
    src = open(os.path.join(root, "libre_amd", "host", "src", "hip_plugin.cpp")).read()
    assert "#pragma weak vrc_set_slice" in src
    assert "vrc_set_slice == nullptr" in src and "the device layer has no slice projection" in src
    assert "vrc_set_slice" not in open(os.path.join(root, "tests", "host_san", "vrc_stub.cpp")).read()
