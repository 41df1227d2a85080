"""The gfx950 kernels, through the C ABI, against tests/ref64.py -- the independent float64 restatement of the
reference's ray cast -- and not against the oracle: the same cases as tests/test_ref64_cpu.py, the same frozen rule
scenes.assert_parity(frame, ref64 frame, budget=B64), every kernel form that can render the case.  ref64's frame of a
case is computed once per process and reused across kernel forms (test_ref64_cpu.ref)."""
import numpy as np
import pytest

import nongrid
import orc
import ref64
import scenes
from test_cpu_harness import _fuzz_scene
from test_ref64_cpu import CASES, case, check, is_grid, ref
from test_uniform_bricks_cpu import assert_split, mixed_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vrc():
    from libre_amd import vrc as v
    v.load_library()  # fails loudly when the HIP extension is missing
    return v


def _gpu(s):
    from gpu_run import GpuScene
    return GpuScene(s)


def _opt(vrc, g, option, value):
    vrc.check(g.L, g.L.vrc_set_option(g.ctx, option, value))


def every_form(vrc, g, s, what, r_near, r_lin, r_exact=None, passes=None, stride=(1, 1), grid=True):
    """Every kernel form that renders the scene, each against ref64.  The sample count is held to ref64's for the grid
    walk (the reference's samples, one for one)."""
    staged = min(s.vi.overlap[a] for a in range(3)) >= 1 and max(s.slot_dim) <= 248
    kernels = [vrc.KERNEL_REFERENCE_ORDER] + ([vrc.KERNEL_GRID_DDA] if grid else [])
    names = {vrc.KERNEL_REFERENCE_ORDER: "reference order", vrc.KERNEL_GRID_DDA: "grid walk", vrc.KERNEL_LDS: "LDS",
             vrc.KERNEL_PACKED: "packed"}
    for kernel in kernels:
        for stepping in (1, 0):
            for grey in (1, 0):
                _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                got, n_got, st = g.render(kernel=kernel, stepping=stepping, passes=passes)
                assert st.kernel_variant == kernel
                check(s, got, n_got, r_near, what, "gpu %s, stepping %d, grey %d" % (names[kernel], stepping, grey), stride,
                      count=kernel == vrc.KERNEL_GRID_DDA)
    _opt(vrc, g, vrc.OPT_GREY_TABLE, 1)
    if r_exact is not None:  # VRC_OPT_TF_FRAC_BITS = 0 against the exact lerp weight
        got, n_got, _ = g.render(kernel=kernels[-1], frac_bits=0, passes=passes)
        check(s, got, n_got, r_exact, what + " exact weight", "gpu %s" % names[kernels[-1]], stride,
              count=kernels[-1] == vrc.KERNEL_GRID_DDA)
    if r_lin is None:
        return
    lin = list(kernels)
    if staged and grid:
        lin += [vrc.KERNEL_LDS, vrc.KERNEL_PACKED]
        if s.atlas.dtype.itemsize == 1:  # the staged form also point-samples 8-bit bricks
            got, n_got, st = g.render(kernel=vrc.KERNEL_LDS, passes=passes)
            assert st.kernel_variant == vrc.KERNEL_LDS
            check(s, got, n_got, r_near, what, "gpu LDS", stride, count=False)
    elif staged:
        lin += [vrc.KERNEL_PACKED]
    for kernel in lin:
        got, n_got, st = g.render(kernel=kernel, filter_mode=vrc.FILTER_TRILINEAR, passes=passes)
        assert st.kernel_variant == kernel
        check(s, got, n_got, r_lin, what + " trilinear", "gpu %s" % names[kernel], stride,
              count=kernel == vrc.KERNEL_GRID_DDA)


@pytest.mark.parametrize("name", CASES)
def test_every_kernel_form_matches_ref64(vrc, name):
    s, passes, stride = case(name)
    grid = all(is_grid(t) for t in (nongrid.passes_of(s, passes) if passes else [s]))
    trilinear = name not in ("c1", "two_pass", "saturated")
    exact = name in ("hash64_spin", "hash64_ert", "smooth_a", "nucleon")
    with _gpu(s) as g:
        every_form(vrc, g, s, name, ref(name), ref(name, filter_mode=1) if trilinear else None,
                   ref(name, frac_bits=0) if exact else None, passes, stride, grid)


@pytest.mark.parametrize("which", ["mem64_spin", "mixed"])
def test_uniform_bricks_on_and_off_match_ref64(vrc, which):
    # VRC_OPT_UNIFORM_BRICKS marches a brick of one value from one table entry; on and off, against ref64
    if which == "mixed":
        s = mixed_scene()
        assert_split(s)
        r = ref64.render(s)
    else:
        s, r = case(which)[0], ref(which)
    with _gpu(s) as g:
        for on in (1, 0):
            _opt(vrc, g, vrc.OPT_UNIFORM_BRICKS, on)
            for kernel in (vrc.KERNEL_GRID_DDA, vrc.KERNEL_REFERENCE_ORDER):
                for grey in (1, 0):
                    _opt(vrc, g, vrc.OPT_GREY_TABLE, grey)
                    got, n_got, _ = g.render(kernel=kernel)
                    check(s, got, n_got, r, which, "gpu kernel %d, uniform bricks %d, grey %d" % (kernel, on, grey),
                          count=kernel == vrc.KERNEL_GRID_DDA)


@pytest.mark.parametrize("seed", range(16 * scenes.FUZZ_SCALE))
def test_random_views_match_ref64(vrc, seed):
    # the seeds of tests/test_ref64_cpu.py::test_random_views_match_ref64
    rng = np.random.default_rng(64000 + seed)
    kw = _fuzz_scene(rng)
    s = orc.build_scene(**kw)
    what = "seed %d %r" % (seed, kw)
    with _gpu(s) as g:
        every_form(vrc, g, s, what, ref64.render(s), ref64.render(s, filter_mode=1))
