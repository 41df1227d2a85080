"""Node lists that are NOT a brick grid: the inputs on which every kernel form leaves the grid walk for the
reference-order loop (vrc_pixel_reference_order; on the device with the ballot tile culling of
vrc_kernels.hip).  vrc_tables.h's gridOk takes a list only if its bricks tile one regular grid, one brick per
cell; these lists fail that test by construction:

  * overlapping lists -- some coarse bricks together with bricks of a finer level inside them.  This is the shape
    of an asynchronous frame whose missing bricks are stood in for by a cached ancestor
    (RenderingSetGeneratorFilter.ipp:39-95), and of the resident hierarchy of per-ray LOD;
  * ragged lists -- the reference's UVF fixture, whose two levels are bricked in 28^3 blocks that do not
    divide the volume (75x75x138 voxels: bricks of 28 and 19 voxels a side).

Every builder returns an orc scene (tests/orc.py) whose node list is in the oracle's front-to-back order, so
the oracle, the CPU harness and the device all composite the same list in the same order."""
import os

import numpy as np

import orc

UVF = "uvf://" + os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_reduced.uvf")


def children(nid):
    """The eight NodeIds one level below `nid` (a cube of 2^level x the root blocks)."""
    level, x, y, z, t = orc.unpack(nid)
    return [orc.pack(level + 1, 2 * x + i, 2 * y + j, 2 * z + k, t) for i in (0, 1) for j in (0, 1) for k in (0, 1)]


def descendants(nid, level):
    """Every NodeId of `level` inside `nid`."""
    out = [nid]
    while orc.unpack(out[0])[0] < level:
        out = [c for n in out for c in children(n)]
    return out


def ancestors_plus_leaves(vi, parents, child_keep=None):
    """`parents` (NodeIds above the leaf level) plus leaves.  child_keep=None: ALL leaves, also those inside a
    parent (every ray through a parent meets its volume twice).  child_keep=rng: of the leaves inside each parent
    only a random, non-empty, incomplete subset; every leaf outside the parents."""
    leaves = orc.leaf_ids(vi)
    leaf_level = vi.depth - 1
    inside = {p: set(descendants(p, leaf_level)) for p in parents}
    ids = list(parents)
    covered = set().union(*inside.values()) if inside else set()
    ids += [i for i in leaves if i not in covered]
    for p in parents:
        under = sorted(inside[p])
        if child_keep is None:
            ids += under
        else:
            k = int(child_keep.integers(1, len(under)))
            ids += [under[j] for j in sorted(child_keep.choice(len(under), size=k, replace=False))]
    return ids


def root_plus_children(vi):
    """The root brick and the eight bricks of level 1."""
    root = orc.pack(0, 0, 0, 0)
    return [root] + children(root)


def is_overlapping(s):
    """True if two bricks of the scene's list overlap in space (so the list cannot be one brick grid)."""
    boxes = [(np.array(nd.aabbMin[:]), np.array(nd.aabbMin[:]) + np.array(nd.aabbSize[:])) for nd in s.nodes]
    for i in range(len(boxes)):
        for j in range(i + 1, len(boxes)):
            lo = np.maximum(boxes[i][0], boxes[j][0])
            hi = np.minimum(boxes[i][1], boxes[j][1])
            if (hi - lo > 1e-6).all():
                return True
    return False


# name: (kwargs of orc.build_scene without ids, how to pick the ids).  64^3 voxels in 16^3 bricks: depth 3, level 1
# is 2^3 bricks of 32^3 voxels' extent, level 2 the 64 leaves.
OVERLAPPING = {
    # three level-1 parents + all 64 leaves (the async ancestor fill-in at its most overlapped)
    "hash_parents_all_leaves": (dict(volume="hash", spin=(0.5, 0.35), viewport=(48, 40)), ("parents", (0, 3, 6))),
    "hash_parents_all_leaves_u16": (dict(volume="hash", spin=(-0.7, 0.25), viewport=(40, 48), dtype="u16"),
                                    ("parents", (1, 4, 7))),
    # two parents + some of each parent's children (the children a cache has, the parent for the rest)
    "hash_parents_some_children": (dict(volume="hash", spin=(2.3, -0.4), viewport=(44, 44), alpha=0.3),
                                   ("some", (2, 5))),
    "mem_parents_some_children_u16": (dict(volume="mem", spin=(0.2, 0.9), viewport=(37, 29), dtype="u16",
                                           data_range=(0.0, 300.0)), ("some", (0, 7))),
    "mem_parents_all_leaves": (dict(volume="mem", spin=(1.2, -0.3), viewport=(41, 33)), ("parents", (2, 3, 5))),
    # the root and its eight children (a coarse frame under a finer one)
    "mem_root_children": (dict(volume="mem", spin=(0.3, -0.2), viewport=(40, 40)), ("root", None)),
    "hash_root_children_u16": (dict(volume="hash", spin=(0.9, 0.5), viewport=(36, 44), dtype="u16",
                                    alpha=0.3), ("root", None)),
}


def overlapping_scene(name, **over):
    """orc scene of OVERLAPPING[name] (64^3 voxels, 16^3 bricks); keyword arguments override the scene's."""
    kw, (how, which) = OVERLAPPING[name]
    kw = dict(dict(voxels=(64, 64, 64), block=16), **kw)
    kw.update(over)
    vi = orc.mem_volume_info(*kw["voxels"], kw["block"])
    level1 = descendants(orc.pack(0, 0, 0, 0), 1)
    if how == "parents":
        ids = ancestors_plus_leaves(vi, [level1[i] for i in which])
    elif how == "some":
        ids = ancestors_plus_leaves(vi, [level1[i] for i in which], child_keep=np.random.default_rng(len(name)))
    else:
        ids = root_plus_children(vi)
    s = orc.build_scene(ids=ids, **kw)
    assert is_overlapping(s), name
    return s


def baseline_root_and_leaves(spin=(0.5236, 0.349), **kw):
    """BASELINE's slot shape: 256^3 noise in bricks of 128 (slots of 136^3), the root and its eight leaves, a 256^2
    frame."""
    vi = orc.mem_volume_info(256, 256, 256, 128)
    s = orc.build_scene(voxels=(256, 256, 256), block=128, viewport=(256, 256), volume="hash", spin=spin,
                        ids=root_plus_children(vi), **kw)
    assert s.slot_dim == [136, 136, 136] and s.n_nodes == 9 and is_overlapping(s)
    return s


def uvf_ids(drv, levels):
    """Every valid NodeId of the UVF fixture on the given levels (level 0: 12 bricks, level 1: 45)."""
    info = drv.datasource_info(UVF)
    ids = []
    for level in levels:
        for x in range(info["root_blocks"][0] << level):
            for y in range(info["root_blocks"][1] << level):
                for z in range(info["root_blocks"][2] << level):
                    nid = orc.pack(level, x, y, z, 0)
                    if drv.datasource_node(UVF, nid)["valid"]:
                        ids.append(nid)
    return ids


#: the UVF cases: name -> (levels or "culled", scene kwargs of orc.scene_from_datasource)
RAGGED = {
    "uvf_leaves": ((1,), dict(viewport=(56, 48), spin=(0.6, 0.3), alpha=0.3)),
    "uvf_both_levels": ((0, 1), dict(viewport=(48, 40), spin=(-1.1, 0.4), alpha=0.3)),
    "uvf_culled": ("culled", dict(viewport=(48, 48), spin=(2.0, -0.3), alpha=0.3, eye=(0.05, -0.08, 0.45))),
}


def uvf_scene(drv, name, **over):
    """orc scene of RAGGED[name].  "uvf_culled": the leaves the host's visible-set selection keeps for a camera close
    to the volume (frustum culled: fewer than the 45 leaves)."""
    levels, kw = RAGGED[name]
    kw = dict(kw, **over)
    if levels == "culled":
        info = drv.datasource_info(UVF)
        mv = list(orc.default_mv(kw["spin"], kw["eye"]))
        ids = drv.select_visibles(UVF, mv, list(orc.default_proj()), kw["viewport"][1], 1.0, info["depth"] - 1,
                                  info["depth"] - 1)
        assert 0 < len(ids) < 45, len(ids)
    else:
        ids = uvf_ids(drv, levels)
    return orc.scene_from_datasource(drv, UVF, ids, kw.pop("viewport"), **kw)


def random_overlapping_ids(vi, rng):
    """1-3 random bricks of a random level above the leaves, plus all leaves or (half the draws) only some of
    the leaves inside each of them."""
    level = int(rng.integers(0, vi.depth - 1))
    dims = [vi.rootBlocks[a] << level for a in range(3)]
    cells = [orc.pack(level, x, y, z) for x in range(dims[0]) for y in range(dims[1]) for z in range(dims[2])]
    k = int(rng.integers(1, min(3, len(cells)) + 1))
    parents = [cells[i] for i in sorted(rng.choice(len(cells), size=k, replace=False))]
    return ancestors_plus_leaves(vi, parents, child_keep=rng if rng.random() < 0.5 else None)


def fuzz_scene(rng, **over):
    """The randomized views of tests/test_cpu_harness.py (_fuzz_scene: volume, camera, eye inside, clip planes,
    samples per ray) over a random overlapping list; volumes of a single level are bricked finer until the tree has
    two.  Returns (orc scene, the build_scene kwargs)."""
    from test_cpu_harness import _fuzz_scene
    kw = _fuzz_scene(rng)
    kw.update(over)
    vi = orc.mem_volume_info(*kw["voxels"], kw["block"])
    if vi.depth < 2:
        kw["block"] = 16
        vi = orc.mem_volume_info(*kw["voxels"], kw["block"])
    assert vi.depth >= 2, kw
    ids = random_overlapping_ids(vi, rng)
    s = orc.build_scene(ids=ids, **kw)
    assert is_overlapping(s), kw
    return s, kw


def passes_of(s, passes):
    """The scene split into passes [(a, b)] of its node list (what the plugin does when the atlas is smaller than the
    frame): one scene per pass, same atlas, view and settings, nodes a..b-1."""
    import copy
    import ctypes as C
    out = []
    for a, b in passes:
        t = copy.copy(s)
        t.nodes = (orc.NodeData * (b - a))()
        C.memmove(t.nodes, C.byref(s.nodes, a * C.sizeof(orc.NodeData)), (b - a) * C.sizeof(orc.NodeData))
        t.n_nodes = b - a
        out.append(t)
    return out


def oracle_passes(s, passes, **kw):
    """The oracle's frame of the list rendered in these passes, accumulating in one pixel buffer.  Not always the
    single pass's frame: the reference's node loop ends a ray at the first brick of the list that starts beyond the
    far end of its clip-plane interval (cuda/Renderer.cu:183-184), and every pass starts that loop anew."""
    fb = None
    n = 0
    for t in passes_of(s, passes):
        fb, k = orc.oracle_render(t, fb=fb, **kw)
        n += k
    orc._LAST_SCENE = s
    return fb, n


def non_grid_passes(s, passes):
    """Merge neighbouring passes until none of them is a brick grid by itself (the harness's table builder decides, as
    vrc_render's does): a grid-aligned pass of mixed brick sizes would be walked along the rays by the trilinear forms,
    not in the list order the oracle composites in."""
    out = list(passes)
    k = 0
    while k < len(out):
        (a, b), = [out[k]]
        if len(out) > 1 and orc.harness_render(passes_of(s, [(a, b)])[0], kernel=7)[2]:
            if k + 1 < len(out):
                out[k:k + 2] = [(a, out[k + 1][1])]
            else:
                out[k - 1:k + 1] = [(out[k - 1][0], b)]
                k -= 1
            continue
        k += 1
    return out
