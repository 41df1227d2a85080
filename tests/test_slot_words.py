"""The three words a brick upload leaves per slot -- largest voxel, smallest voxel, uniformity -- read back on the GPU
through the public contract alone: the exact sample counts of the probes of tests/slot_words.py, which says what is
compared with what and why a count pins a word.  Every upload kernel (vrc_k_repack_u8x8, _generic, _padded), every voxel
type, host and device sources, the places a fold can miss (first and last voxel, the overlap border, every byte lane, the
grid-stride tail), float edges, recycled slots and concurrent uploads.  tests/test_slot_words_cpu.py checks the scenes
and the expected counts without a GPU."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # before the library under test loads its HIP runtime: both then share one

import slot_words as sw
from gpu_run import GpuScene
from libre_amd import vrc

pytestmark = pytest.mark.gpu

KERNELS = {"reforder": vrc.KERNEL_REFERENCE_ORDER, "dda": vrc.KERNEL_GRID_DDA}
FOLDS = {"min": vrc.MIP_FOLD_MIN, "max": vrc.MIP_FOLD_MAX}


class Pool(GpuScene):
    """A typed pool of n_slots slots for bricks of geometry g; bricks are uploaded one by one and a frame renders the
    nodes it is given from the slots they landed in."""

    def __init__(self, g, tname, n_slots, device=0):
        self.L = L = vrc.load_library()
        self.g, self.tname, self.s = g, tname, None
        self.ctx, self.pool = C.c_void_p(), C.c_void_p()
        vrc.check(L, L.vrc_ctx_create(device, C.byref(self.ctx)))
        vt, dt = sw.TYPES[tname]
        self.voxel_bytes = np.dtype(dt).itemsize
        try:
            mb = vrc.u32x3(*[g.vi.maximumBlockSize[a] for a in range(3)])
            vrc.check(L, L.vrc_pool_create_typed(self.ctx, vt, mb, sw.pool_bytes(g, n_slots) * self.voxel_bytes,
                                                 C.byref(self.pool)))
            info = self.info()
            self.atlas_dim = info["atlas_dim"]
            self.slot_dim = [info["atlas_dim"][a] // info["slots"][a] for a in range(3)]
            assert self.slot_dim == list(g.slot_dim) and info["free"] >= n_slots
            assert info["slot_bytes"] == self.slot_dim[0] * self.slot_dim[1] * self.slot_dim[2] * self.voxel_bytes
        except Exception:
            self.close()
            raise

    def upload(self, brick, how="host", kernel=None):
        """Returns the slot.  how: "host", "device" (a torch buffer) or "unaligned" (the same, one byte further);
        kernel: the repack kernel the case is meant to take, asserted from vrc_pool_info's slot."""
        L = self.L
        brick = np.ascontiguousarray(brick)
        assert brick.dtype == sw.TYPES[self.tname][1]
        size = [brick.shape[2], brick.shape[1], brick.shape[0]]
        if kernel is not None:
            assert sw.upload_kernel(self.voxel_bytes, size, self.slot_dim, how != "unaligned") == kernel
        slot = vrc.f32x3()
        if how == "host":
            vrc.check(L, L.vrc_pool_copy_to_slot(self.pool, brick.ctypes.data, vrc.u32x3(*size), slot))
        else:
            off = 1 if how == "unaligned" else 0
            buf = torch.empty(brick.nbytes + 8, dtype=torch.uint8, device="cuda:0")
            assert buf.data_ptr() % 8 == 0
            buf[off:off + brick.nbytes].copy_(torch.from_numpy(brick.reshape(-1).view(np.uint8)))
            torch.cuda.synchronize()
            # (returns when the repack has run: the buffer may go afterwards)
            vrc.check(L, L.vrc_pool_copy_to_slot_device(self.pool, C.c_void_p(buf.data_ptr() + off), vrc.u32x3(*size), slot))
        return tuple(slot)

    def release(self, slot):
        vrc.check(self.L, self.L.vrc_pool_release_slot(self.pool, vrc.f32x3(*slot)))

    def scene(self, bricks, slots, g=None):
        """bricks, slots: {node id: ...}; the nodes in the geometry's front-to-back order"""
        g = g or self.g
        ids = [nid for nid in g.ids if nid in bricks]
        return sw.gpu_scene(g, ids, bricks, self.tname, slots, self.atlas_dim)

    def _opt(self, option, value):
        vrc.check(self.L, self.L.vrc_set_option(self.ctx, option, value))

    def iso(self, s, iso_value, skip, kernel, filter_mode=0):
        self.s = s
        vrc.set_isosurface(self.L, self.ctx, iso_value, 0.25)
        self._opt(vrc.OPT_PROJECTION, vrc.PROJECTION_ISO)
        self._opt(vrc.OPT_MIP_SKIP, skip)
        fb, n, st = self.render(kernel=kernel, filter_mode=filter_mode)
        assert st.kernel_variant == kernel and b"vrc_k_raycast_mip" in self.L.vrc_last_kernel()
        return fb, n

    def mip(self, s, fold, skip, kernel, depth=0, uniform=1, filter_mode=0):
        self.s = s
        self._opt(vrc.OPT_PROJECTION, vrc.PROJECTION_MIP)
        self._opt(vrc.OPT_MIP_FOLD, fold)
        self._opt(vrc.OPT_MIP_DEPTH, depth)
        self._opt(vrc.OPT_MIP_SKIP, skip)
        self._opt(vrc.OPT_UNIFORM_BRICKS, uniform)
        fb, n, st = self.render(kernel=kernel, filter_mode=filter_mode)
        assert st.kernel_variant == kernel and b"vrc_k_raycast_mip" in self.L.vrc_last_kernel()
        return fb, n


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def probe_a(p, s, checks, total, what, filter_mode=0):
    """checks: [(iso_value, marched?)].  With skipping on the count is |S| (mip_ref's) where the slot's maximum reaches
    the isovalue and 0 where it does not; with skipping off it is |S| and the frame is the same, bit for bit."""
    for kname, kernel in KERNELS.items():
        for iso_value, marched in checks:
            on, n_on = p.iso(s, iso_value, 1, kernel, filter_mode)
            off, n_off = p.iso(s, iso_value, 0, kernel, filter_mode)
            where = "%s, %s, iso_value %r" % (what, kname, iso_value)
            print("%s: samples %d with skipping, %d without; mip_ref %d" % (where, n_on, n_off, total))
            assert n_off == total, where
            assert n_on == (total if marched else 0), where
            assert _same(on, off), where
            assert (off == 0).all(), where + ": a sample read the planted voxel"


def probe_b(p, s, fold, marched, what, depth=(0,), filter_mode=0):
    """The front brick's samples, and the back brick's only if it is marched (slot_words.expected_two); with skipping off
    every sample, and the same frame."""
    g = p.g
    total, want = sw.expected_two(g, True), sw.expected_two(g, marched)
    for kname, kernel in KERNELS.items():
        for d in depth:
            on, n_on = p.mip(s, fold, 1, kernel, depth=d, filter_mode=filter_mode)
            off, n_off = p.mip(s, fold, 0, kernel, depth=d, filter_mode=filter_mode)
            where = "%s, %s, depth %d" % (what, kname, d)
            print("%s: samples %d with skipping (expected %d), %d without (mip_ref %d)" % (where, n_on, want, n_off, total))
            assert n_off == total, where
            assert n_on == want, where
            assert _same(on, off), where


# ---- probe A: the maximum, per upload path, voxel type and place ----------------------------------------------------------
#: path -> (geometry, how the brick is uploaded, the kernel 8-bit voxels take, the kernel the other types take)
PATHS = {
    "whole": ("whole", "host", "u8x8", "generic"),
    "padded": ("padded", "host", "padded", "padded"),
    "ragged": ("ragged", "host", "padded", "padded"),
    "device": ("whole", "device", "u8x8", "generic"),
    "unaligned": ("whole", "unaligned", "generic", None),  # 8-bit voxels through the generic kernel
}
A_CASES = [(t, path) for path in PATHS for t in sorted(sw.TYPES) if PATHS[path][3] is not None or t in ("uint8", "int8")]


@pytest.mark.parametrize("tname,path", A_CASES, ids=["%s-%s" % c for c in A_CASES])
def test_the_maximum_word_is_the_planted_voxel(tname, path):
    gname, how, k8, kn = PATHS[path]
    g = sw.geometry(gname)
    nid = g.ids[0]
    shape = g.shape[nid]
    eight = np.dtype(sw.TYPES[tname][1]).itemsize == 1
    assert shape[::-1] == (18, 11, 7) or path != "ragged"
    base = sw.max_noise(tname, shape)
    values = sw.maxima(tname)
    cases = []
    for pname, pos in sw.positions(shape, eight).items():
        for v in (values[:1] if pname.startswith("lane") else values):
            cases.append((pname, v, sw.with_voxel(base, pos, v)))
    total = int(g.ref.counts.sum())
    with Pool(g, tname, len(cases)) as p:
        slots = [p.upload(b, how, k8 if eight else kn) for _, _, b in cases]
        assert len(set(slots)) == len(cases)
        for (pname, v, brick), slot in zip(cases, slots):
            s = p.scene({nid: brick}, {nid: slot})
            probe_a(p, s, [(sw.iso_of(tname, v), True), (sw.next_above(tname, v), False)], total,
                    "%s %s at %s, maximum %r" % (tname, path, pname, v))


def test_the_last_voxel_of_a_136_cubed_brick():
    """2.5 M voxels against the 2048 * 4 * 256 threads of the upload's grid: the last voxel is folded on a second trip."""
    g = sw.geometry("big")
    nid = g.ids[0]
    shape = g.shape[nid]
    pos = sw.positions(shape, False)["last"]
    base = sw.max_noise("uint16", shape)
    total = int(g.ref.counts.sum())
    with Pool(g, "uint16", 2) as p:
        for v in (65535, 4000):
            brick = sw.with_voxel(base, pos, v)
            slot = p.upload(brick, "host", "generic")
            probe_a(p, p.scene({nid: brick}, {nid: slot}), [(float(v), True), (float(v + 1), False)], total,
                    "136^3 uint16, maximum %d at the last voxel" % v)


@pytest.mark.parametrize("path", ["whole", "padded", "device"])
def test_float_edges_of_the_maximum_word(path):
    """A negative maximum, the two zeros, a denormal, +-FLT_MAX, NaN everywhere but one voxel, NaN everywhere.  Values
    are compared as numbers, as the contract's ">= in float32" does: -0.0 and +0.0 are one isovalue and one maximum."""
    gname, how, _, kn = PATHS[path]
    g = sw.geometry(gname)
    nid = g.ids[0]
    pos = sw.positions(g.shape[nid], False)["last"]
    edges = sw.float_edges_a(g.shape[nid], pos)
    total = int(g.ref.counts.sum())
    with Pool(g, "float32", len(edges)) as p:
        for name, (brick, checks) in edges.items():
            slot = p.upload(brick, how, kn)
            probe_a(p, p.scene({nid: brick}, {nid: slot}), checks, total, "float32 %s %s" % (path, name))


# ---- probe B: the minimum, and the maximum again, under the folds -----------------------------------------------------------
B_PATHS = {"whole": ("two_whole", "host"), "padded": ("two_padded", "host"), "device": ("two_whole", "device")}


@pytest.mark.parametrize("fold", sorted(FOLDS))
@pytest.mark.parametrize("path", sorted(B_PATHS))
@pytest.mark.parametrize("tname", sorted(sw.TYPES))
def test_the_fold_skips_the_back_brick_exactly_when_its_extremum_cannot_beat_the_front(tname, path, fold):
    gname, how = B_PATHS[path]
    g = sw.geometry(gname)
    front, back = g.ids
    eight = np.dtype(sw.TYPES[tname][1]).itemsize == 1
    dt = sw.TYPES[tname][1]
    noise = sw.back_noise(tname, g.shape[back], FOLDS[fold])
    cases = []
    for ci, (a, ext, marched) in enumerate(sw.fold_cases(tname, FOLDS[fold])):
        for pname, pos in sw.positions(g.shape[back], eight and ci == 0).items():  # (the byte lanes: once per fold)
            cases.append((ci, a, ext, marched, pname, sw.with_voxel(noise, pos, ext)))
    with Pool(g, tname, 2 * len(cases)) as p:
        for ci, a, ext, marched, pname, brick in cases:
            bricks = {front: np.full(g.shape[front], a, dtype=dt), back: brick}
            slots = {nid: p.upload(b, how) for nid, b in bricks.items()}
            # depth tracking on for the first marched and the first skipped case: the back brick's tNear lies above the
            # D the front brick left, so the decision is the same
            depth = (0, 1) if pname == "first" and ci < 2 else (0,)
            probe_b(p, p.scene(bricks, slots), FOLDS[fold], marched,
                    "%s %s %s: front %r, back's extremum %r at %s" % (tname, path, fold, a, ext, pname), depth)


@pytest.mark.parametrize("path", ["whole", "padded"])
def test_float_edges_under_the_maximum_fold(path):
    gname, how = B_PATHS[path]
    g = sw.geometry(gname)
    front, back = g.ids
    pos = sw.positions(g.shape[back], False)["last"]
    edges = sw.float_edges_b(g.shape[back], pos)
    with Pool(g, "float32", 2 * len(edges)) as p:
        for name, (a, brick, marched) in edges.items():
            bricks = {front: np.full(g.shape[front], a, dtype=np.float32), back: brick}
            slots = {nid: p.upload(b, how) for nid, b in bricks.items()}
            probe_b(p, p.scene(bricks, slots), vrc.MIP_FOLD_MAX, marched, "float32 %s %s" % (path, name), (0, 1))


# ---- trilinear samples: one integer case per probe ----------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["uint8", "uint16"])
def test_trilinear_samples_keep_the_margin(tname):
    """A trilinear sample may exceed the slot's maximum by the interpolation's rounding, so M (the isovalue) has to reach
    max + |max| * 1e-6: an isovalue of vmax + 1 is skipped and vmax is marched, as for point samples, but under the
    folds a back brick whose extremum EQUALS the front's value is marched -- the margin -- and one a whole level short
    of it is skipped.  (The sample positions are the point samples': the same counts.)"""
    g = sw.geometry("whole")
    nid = g.ids[0]
    brick = sw.with_voxel(sw.max_noise(tname, g.shape[nid]), sw.positions(g.shape[nid], False)["first"], 200)
    with Pool(g, tname, 1) as p:
        slot = p.upload(brick)
        probe_a(p, p.scene({nid: brick}, {nid: slot}), [(200.0, True), (201.0, False)], int(g.ref.counts.sum()),
                "%s trilinear" % tname, filter_mode=1)
    g = sw.geometry("two_whole")
    front, back = g.ids
    dt = sw.TYPES[tname][1]
    pos = sw.positions(g.shape[back], False)["first"]
    with Pool(g, tname, 12) as p:
        for fold, cases in (("max", [(101, True), (100, True), (99, False)]), ("min", [(99, True), (100, True), (101, False)])):
            noise = sw.back_noise(tname, g.shape[back], FOLDS[fold])
            for ext, marched in cases:
                bricks = {front: np.full(g.shape[front], 100, dtype=dt), back: sw.with_voxel(noise, pos, ext)}
                slots = {k: p.upload(b) for k, b in bricks.items()}
                probe_b(p, p.scene(bricks, slots), FOLDS[fold], marched,
                        "%s trilinear %s: front 100, back's extremum %d" % (tname, fold, ext), filter_mode=1)


# ---- recycled slots ---------------------------------------------------------------------------------------------------------
def _histograms_and_packed_atlas(p, s):
    """Both share the upload's section of the stream from here on: every later upload bins its brick and packs it."""
    ov = vrc.u32x3(*[p.g.vi.overlap[a] for a in range(3)])
    vrc.check(p.L, p.L.vrc_pool_enable_histograms(p.pool, 256, ov))
    p.s = s
    p._opt(vrc.OPT_PROJECTION, vrc.PROJECTION_COMPOSITE)
    _, _, st = p.render(kernel=vrc.KERNEL_PACKED, filter_mode=vrc.FILTER_TRILINEAR)
    assert st.kernel_variant == vrc.KERNEL_PACKED


#: (type, the second brick's path, histograms and packed atlas on?) -- a float pool has neither
RECYCLE = [(t, second, False) for t in ("uint8", "uint16", "float32") for second in ("whole", "padded")] + [
    ("uint8", "whole", True), ("uint8", "padded", True), ("uint16", "padded", True)]


@pytest.mark.parametrize("tname,second,extras", RECYCLE,
                         ids=["%s-%s%s" % (t, s, "-histograms_and_packed" if e else "") for t, s, e in RECYCLE])
def test_a_recycled_slot_forgets_the_larger_maximum(tname, second, extras):
    """A brick with maximum 200, released; into the same slot a brick with maximum 50, once filling the slot and once
    smaller than the first: the word is 50's."""
    g1, g2 = sw.geometry("whole"), sw.geometry(second)
    nid = g1.ids[0]
    kernel = {"whole": "u8x8" if tname == "uint8" else "generic", "padded": "padded"}
    lo = sw._limits(tname)
    band = (0, 40) if lo else (-0.9, -0.6)
    first = sw.with_voxel(sw.noise(tname, g1.shape[nid], band[0], band[1], 21), sw.positions(g1.shape[nid], False)["face"], 200)
    then = sw.with_voxel(sw.noise(tname, g2.shape[nid], band[0], band[1], 22), sw.positions(g2.shape[nid], False)["last"], 50)
    with Pool(g1, tname, 1) as p:
        slot = p.upload(first, "host", kernel["whole"])
        s1 = p.scene({nid: first}, {nid: slot})
        if extras:
            _histograms_and_packed_atlas(p, s1)
        probe_a(p, s1, [(200.0, True), (sw.next_above(tname, 200), False)], int(g1.ref.counts.sum()), "%s first" % tname)
        p.release(slot)
        again = p.upload(then, "host", kernel[second])
        assert again == slot
        probe_a(p, p.scene({nid: then}, {nid: again}, g2), [(50.0, True), (sw.next_above(tname, 50), False)],
                int(g2.ref.counts.sum()), "%s %s over a larger maximum" % (tname, second))


@pytest.mark.parametrize("second", ["two_whole", "two_padded"])
@pytest.mark.parametrize("tname", ["uint8", "uint16", "float32"])
def test_a_recycled_slot_forgets_the_smaller_minimum(tname, second):
    """The mirror under VRC_MIP_FOLD_MIN: the back brick's minimum was 20, below the front's 100; the brick that
    replaces it has minimum 100 and is skipped."""
    g1, g2 = sw.geometry("two_whole"), sw.geometry(second)
    front, back = g1.ids
    dt = sw.TYPES[tname][1]
    band = (150, 250) if sw._limits(tname) else (150.0, 250.0)
    first = sw.with_voxel(sw.noise(tname, g1.shape[back], band[0], band[1], 23), sw.positions(g1.shape[back], False)["last"], 20)
    then = sw.with_voxel(sw.noise(tname, g2.shape[back], band[0], band[1], 24), sw.positions(g2.shape[back], False)["first"], 100)
    with Pool(g1, tname, 2) as p:
        bricks = {front: np.full(g1.shape[front], 100, dtype=dt), back: first}
        slots = {nid: p.upload(b) for nid, b in bricks.items()}
        probe_b(p, p.scene(bricks, slots), vrc.MIP_FOLD_MIN, True, "%s first" % tname)
        p.release(slots[back])
        p.release(slots[front])
        # (the pool hands out the slot released last: the front brick returns to its own slot, the back brick to its)
        bricks = {front: np.full(g2.shape[front], 100, dtype=dt), back: then}
        again = {front: p.upload(bricks[front]), back: p.upload(bricks[back])}
        assert again == slots
        p.g = g2
        probe_b(p, p.scene(bricks, again, g2), vrc.MIP_FOLD_MIN, False, "%s %s over a smaller minimum" % (tname, second))


def test_the_uniformity_word_of_16_bit_bricks_follows_the_slot():
    """A uniform uint16 brick replaced by noise and the reverse, through MIP point samples (which read the word): every
    frame and count is a fresh pool's."""
    g = sw.geometry("whole")
    nid = g.ids[0]
    uni = np.full(g.shape[nid], 300, dtype=np.uint16)
    mix = sw.noise("uint16", g.shape[nid], 0, 65535, 31)
    total = int(g.ref.counts.sum())
    fresh = {}
    for name, brick in (("uniform", uni), ("noise", mix)):
        with Pool(g, "uint16", 1) as p:
            slot = p.upload(brick, "host", "generic")
            fresh[name] = p.mip(p.scene({nid: brick}, {nid: slot}), vrc.MIP_FOLD_MAX, 1, vrc.KERNEL_GRID_DDA)
            assert fresh[name][1] == total
    assert not _same(fresh["uniform"][0], fresh["noise"][0])
    with Pool(g, "uint16", 1) as p:
        slot = p.upload(uni, "host", "generic")
        for name, brick in (("noise", mix), ("uniform", uni), ("noise", mix)):
            p.release(slot)
            assert p.upload(brick, "host", "generic") == slot
            for uniform in (1, 0):
                fb, n = p.mip(p.scene({nid: brick}, {nid: slot}), vrc.MIP_FOLD_MAX, 1, vrc.KERNEL_GRID_DDA, uniform=uniform)
                assert _same(fb, fresh[name][0]) and n == fresh[name][1], (name, uniform)


# ---- concurrent uploads -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["uint8", "uint16", "float32"])
def test_concurrent_uploads_leave_every_slot_its_own_maximum(tname):
    """Three threads upload bricks with distinct maxima into one pool (the reference calls copyToSlot from three
    threads): afterwards every slot answers for its own brick."""
    g = sw.geometry("whole")
    nid = g.ids[0]
    shape = g.shape[nid]
    spots = list(sw.positions(shape, False).values())
    base = sw.max_noise(tname, shape)
    lo = sw._limits(tname)
    maxima = [(lo[0] + 50 + 7 * k) if lo else float(np.float32(-0.5 + 0.03 * k)) for k in range(12)]
    bricks = [sw.with_voxel(base, spots[k % len(spots)], v) for k, v in enumerate(maxima)]
    total = int(g.ref.counts.sum())
    with Pool(g, tname, len(bricks)) as p:
        got, errors = {}, []

        def work(ks):
            try:
                for k in ks:
                    got[k] = p.upload(bricks[k])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(range(i, len(bricks), 3),)) for i in range(3)]
        [t.start() for t in threads]
        [t.join() for t in threads]
        assert not errors and len(set(got.values())) == len(bricks)
        for k, v in enumerate(maxima):
            probe_a(p, p.scene({nid: bricks[k]}, {nid: got[k]}), [(sw.iso_of(tname, v), True), (sw.next_above(tname, v), False)],
                    total, "%s brick %d of 12, maximum %r" % (tname, k, v))
