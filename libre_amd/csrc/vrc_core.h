/*
 * vrc_core.h -- per-ray arithmetic of the raycaster, shared by the gfx950 kernels
 * (vrc_kernels.hip) and by a host-compiled unit harness (tests/cpu_harness.cpp, g++,
 * used only to exercise this logic under sanitizers where no GPU exists; it is never
 * loaded by the product).
 *
 * What the arithmetic must reproduce is the reference kernel
 * renderers/cudaRaycaster/cuda/Renderer.cu:95-230 (cited per function).  How it is
 * organised is new: a brick-grid DDA instead of the O(nodes) loop, a per-frame 256-entry
 * "classified sample" table instead of a per-sample TF fetch + pow, and an atlas stored as
 * 8x8x8-voxel micro-blocks.
 */
#ifndef VRC_CORE_H
#define VRC_CORE_H

/* ---- one guard for every compile-time switch of the kernels (round 3) ------------------------------------------
 * The product is built with NONE of them on the command line (__graft_entry__.build()).  Timing ablations that
 * render wrong pixels on purpose (VRC_ABLATE_NO_FETCH, VRC_PACKED_ABLATE), statistics and timeline builds, the biased
 * negative control of the parity tests and every tuning value live behind VRC_DEV_BUILD: a stray -DVRC_... without
 * it does not compile, and a library built with it says so (vrc_abi_version() < 0, vrc_is_dev_build() = 1;
 * bench.py refuses it).  tools/build_variants.sh and the test harnesses pass -DVRC_DEV_BUILD. */
#if !defined( VRC_DEV_BUILD ) && ( \
    defined( VRC_ABLATE_NO_FETCH ) || \
    defined( VRC_WG_TIMELINE ) || \
    defined( VRC_UNIFORM_GROUP ) || \
    defined( VRC_LEAN_GROUP ) || defined( VRC_LEAN_FREE_GROUP ) || \
    defined( VRC_TEST_BIAS_ENTRY ) || \
    defined( VRC_LDS_STATS ) || defined( VRC_LDS_STATS2 ) || \
    defined( VRC_LDS_TIMING ) || \
    defined( VRC_LDS_PASSES ) || defined( VRC_LDS_ROWS ) || defined( VRC_LDS_OCC ) || defined( VRC_LDS_STAGE_N ) || \
    defined( VRC_LDS_ROWS16 ) || defined( VRC_LDS_OCC16 ) || defined( VRC_LDS_STAGE_N16 ) || \
    defined( VRC_LDS_KMAX ) || \
    defined( VRC_LDS_MAX_DZ ) || \
    defined( VRC_LDS_LBATCH ) || \
    defined( VRC_LDS_GBATCH ) || \
    defined( VRC_LDS_G ) || defined( VRC_LDS_GF ) || \
    defined( VRC_LDS_WAVES ) || \
    defined( VRC_LDS_REFILL ) || defined( VRC_LDS_SOON ) || \
    defined( VRC_GROUP ) || \
    defined( VRC_GREY_GROUP ) || \
    defined( VRC_GREY_MAX_WAVES ) || defined( VRC_REPLAY_GREY_MAX_WAVES ) || \
    defined( VRC_REPLAY_UNIFORM_MAX_WAVES ) || defined( VRC_REPLAY_UNIFORM_WG_WAVES ) || \
    defined( VRC_LGROUP ) || \
    defined( VRC_PGROUP ) || defined( VRC_PGROUP16 ) || defined( VRC_PACKED_WAVES ) || defined( VRC_PACKED_ABLATE ) || \
    defined( VRC_SPLIT_GROUP ) || \
    defined( VRC_SMALL_GROUP ) || \
    defined( VRC_SMALL_LAUNCH_TILES ) || \
    defined( VRC_TILE_W ) || defined( VRC_SUPER_UNITS ) || \
    defined( VRC_WAVES_PER_WG ) || \
    defined( VRC_MIN_WAVES ) || \
    defined( VRC_RL_WAVES ) || \
    defined( VRC_RL_MIN_BLOCKS ) )
#error "developer switches of the raycast kernels need -DVRC_DEV_BUILD (the product is built without any of them)"
#endif

#include <stdint.h>
#include <type_traits>

#if defined( __HIPCC__ )
#define VRC_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#include <string.h>
#define VRC_HD inline
#endif

/* Ray and brick-segment set-up is evaluated without FMA contraction, operation for operation
 * as the oracle does: the first sample of every brick segment lies exactly on a brick face
 * (= a voxel face), so one ulp in rayStart decides which of two voxels it reads.  The
 * per-sample loop keeps contraction (it is the hot path). */
#if defined( __clang__ )
#pragma clang fp contract( off ) /* file scope: everything below unless re-enabled */
#define VRC_STRICT_FP _Pragma( "clang fp contract(off)" )
#define VRC_FAST_FP _Pragma( "clang fp contract(fast)" )
#else
#define VRC_STRICT_FP
#define VRC_FAST_FP
#endif

#define VRC_VARIANT_CUDA 0u
#define VRC_VARIANT_GL 1u
#define VRC_EARLY_EXIT 0.999f     /* Renderer.cu:34 */
#define VRC_EPSILON 0.0000000001f /* Renderer.cu:35 */

/* per-ray LOD: levels of the brick hierarchy; entries of one classified table */
#define VRC_MAX_LOD_LEVELS 8
#define VRC_LUT_ENTRIES 257u

/* atlas micro-block: 8x8x8 voxels, x fastest inside the block */
#define VRC_MB 8u
#define VRC_MB_SHIFT 3u
#define VRC_MB_VOXELS 512u

struct vrc_f3
{
    float x, y, z;
};
struct vrc_f4
{
    float x, y, z, w;
};
/* (grey, alpha): a colour or a classified-table entry whose red, green and blue are one number (VRC_MODE_GREY) */
struct vrc_f2
{
    float x, w;
};

/* Kernel-side copy of vrc_node_data plus what the sampler needs per brick. 64 bytes. */
struct vrc_dev_node
{
    float aabbMin[3];
    float aabbSize[3];
    float voxPerWorld[3]; /* texSize*atlasDim/aabbSize: atlas voxels per world unit */
    float localOrigin[3]; /* atlas-voxel coordinate of aabbMin, relative to the slot origin */
    uint32_t slotBase;    /* element offset of the brick's slot in the atlas buffer, low 32 bits */
    uint32_t level;       /* per-ray LOD: 0 = the finest voxel size in the node list, +1 per doubling */
    uint32_t slotBaseHi;  /* high 32 bits: non-zero only in atlases of more than 2^32 voxels (BIG kernels) */
    uint32_t slotInfoIndex; /* linear ordinal of the slot + 1 into vrc_frame::slotInfo; 0 = none (general march) */
};

/* Per-slot uniformity word (vrc_frame::slotInfo), written by the brick upload together with the voxels it describes:
 * low 16 bits = the brick's first voxel, KNOWN = some upload wrote the word, MIXED = a voxel of that upload differs
 * from the first.  0 = nothing known.  A brick is marched from one table entry only when its word is KNOWN and not
 * MIXED: every voxel the upload wrote -- overlap included, i.e. every voxel a sample of that brick can reach -- is
 * the value. */
#define VRC_SLOT_VALUE_MASK 0xFFFFu
#define VRC_SLOT_KNOWN 0x10000u
#define VRC_SLOT_MIXED 0x20000u
VRC_HD bool vrc_slot_holds_one_value( uint32_t word ) { return ( word & ( VRC_SLOT_KNOWN | VRC_SLOT_MIXED ) ) == VRC_SLOT_KNOWN; }

/* Frame constants, derived on the host exactly as Renderer.cu:159-170 does per thread. */
struct vrc_frame
{
    float eye[3];
    float vpX, vpY, vpW, vpH;      /* glViewport as floats */
    float pixelOffX, pixelOffY;    /* sort-first tile offset added to the buffer-local pixel */
    float invProj[16];
    float invView[16];
    float aabbMin[3], aabbMax[3];
    float nearPlane;
    float stepSize;
    uint32_t width, height;        /* pixel buffer */
    uint32_t nPlanes;
    float planes[6][4];
    uint32_t nodeCount;
    /* atlas */
    uint32_t sbx, sby;             /* micro-blocks per slot row / column (slotDim/8) */
    uint32_t slotDim[3];           /* padded slot size in voxels */
    /* brick grid for the DDA kernel */
    float gridMin[3];
    float cellSize[3];
    float invCellSize[3];
    int32_t gridDim[3];
    /* sort-first row bands: frame row of every row of the pixel buffer (NULL = identity).  The
     * buffer then holds height rows picked from a frame of vpH rows (vrc_set_row_map). */
    const uint32_t* rowMap;
    /* one uniformity word per atlas slot (VRC_SLOT_*), indexed by vrc_dev_node::slotInfoIndex - 1; NULL = every brick
     * takes the general march (VRC_OPT_UNIFORM_BRICKS = 0, the CPU harness) */
    const uint32_t* slotInfo;
    /* maximum-intensity projection (VRC_MODE_MIP*): one word per atlas slot holding the largest value the slot's last
     * upload stored (vrc_slot_max_*; same index, stream and fences as slotInfo), NULL = no brick is skipped
     * (VRC_OPT_MIP_SKIP = 0); the context's running maximum per pixel of the pixel buffer (VRC_MIP_EMPTY: no sample
     * yet); and whether this is the frame's first MIP pass, which does not read mipMax */
    const uint32_t* slotMax;
    uint32_t* mipMax;
    uint32_t mipFirst;
    /* 0: cudaRaycaster semantics (cuda/Renderer.cu); 1: the GLSL twin's
     * (glRaycaster/shaders/fragRaycast.glsl), see vrc_brick_segment */
    uint32_t variant;
    /* glRaycaster variant only: nSamplesPerPixel of fragRaycast.glsl:121-129, :212-214 (>= 1).  More than one:
     * every brick is marched by that many jittered rays per pixel and the pixel becomes their average, brick by
     * brick (vrc_pixel_gl_supersampled); the CUDA kernel ignores RenderData.samplesPerPixel (quirk Q3) */
    uint32_t samplesPerPixel;
    /* 1: first march into a pixel buffer that vrc_pre_render declared cleared but did not touch:
     * every pixel starts from 0 and is stored, hit or miss (the clear of
     * cuda/PixelBufferObject.cu:80 folded into the march: one pass over the frame less) */
    uint32_t clearFirst;
    /* per-ray LOD (vrc_pixel_ray_lod): number of levels in the node list,
     * finestVoxelWorldSize / (screenSpaceError * worldSpacePerPixel), and one brick grid per
     * level anchored at gridMin (gridDim / cellSize are level 0's): cells per axis, 1 / cell size,
     * offset of the level's cell -> node table in the table buffer; lodMax = max corner of all
     * bricks; lodEps = 1 % of the finest voxel */
    uint32_t lodLevels;
    float lodBase;
    float lodEps;
    float lodMax[3];
    float lodInvCell[VRC_MAX_LOD_LEVELS][3];
    int32_t lodDim[VRC_MAX_LOD_LEVELS][3];
    uint32_t lodTable[VRC_MAX_LOD_LEVELS];
    /* the other folds of a MIP frame (VRC_OPT_MIP_FOLD; at the end: no field above moves).  slotMin: one word per atlas
     * slot holding the smallest value the slot's last upload stored, as a complemented key (vrc_slot_min_*; a part of
     * slotInfo's allocation, same index, stream and fences), NULL = the minimum fold skips no brick.  meanSum /
     * meanCount: the mean fold's running state per pixel of the pixel buffer, the context's as mipMax is -- the sum of
     * the samples so far (point samples of the 8- and 16-bit atlases: an unsigned 64-bit integer of stored values;
     * everything else: the bits of a double) and their number; a first pass (mipFirst) does not read them */
    const uint32_t* slotMin;
    unsigned long long* meanSum;
    uint32_t* meanCount;
    /* the depth of the projected sample (VRC_OPT_MIP_DEPTH, the depth-tracking instances of the maximum and the minimum;
     * at the end: no field above moves).  mipDepth: the context's running D per pixel of the pixel buffer beside mipMax --
     * the smallest t_j = seg.tNear + (float)j * stepSize over the samples that equal M, +infinity where none does -- owned,
     * invalidated and not read by a first pass as mipMax is; NULL in every other frame.  mipCue: the strength of the
     * depth cue in [0, 1] (VRC_OPT_MIP_DEPTH_CUE / 1000), 0 = the pixel is the classification of M as it is */
    float* mipDepth;
    float mipCue;
    /* the ray cache (VRC_OPT_RAY_CACHE; at the end: no field above moves).  What vrc_setup_ray returns depends on the
     * camera, the viewport, the global box and the clip planes alone, so a view that stands still -- the passes of a
     * multi-pass frame, frames re-rendered while bricks stream in, transfer-function edits, a time series -- need not
     * compute it again.  rayCache: VRC_RAY_CACHE_PLANES planes of rayCachePlane words each, the context's; a plane holds
     * one component of vrc_ray for every pixel, indexed tile * 64 + lane in the kernel's own tile and lane order (whole
     * tiles: a wave's load of one component is one run of 256 bytes).  rayMode: VRC_RAY_COMPUTE (0: the ray is computed,
     * nothing else is read), VRC_RAY_STORE (computed and stored), VRC_RAY_LOAD (loaded: the bits that were stored).
     * Read by vrc_pixel_grid_dda only -- the tile-scheduled grid walk of every vrc_k_raycast instance; the
     * reference-order loop, the LDS-staged, per-ray-LOD and MIP kernels, the depth split and ray compaction compute
     * their rays whatever these say (the host leaves rayMode 0 for them) */
    float* rayCache;
    uint32_t rayCachePlane;
    uint32_t rayMode;
    /* an isosurface frame (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO, the VRC_FOLD_FIRST instances; at the end: no field
     * above moves).  The passes of the frame meet in mipMax (the bits of V, VRC_MIP_EMPTY = no hit), mipDepth (D) and
     * isoGrad: the context's running G, three floats per pixel of the pixel buffer, 0 where there is no hit -- owned,
     * invalidated and not read by a first pass as mipDepth is; NULL in every other frame.  isoThreshold: what a stored
     * voxel of an 8- or 16-bit atlas is compared against (vrc_iso_int_threshold); isoStored: what a float voxel and
     * every trilinear sample is (vrc_iso_float_threshold); isoClassify: the isovalue as the classifier takes a density
     * (the offset-binary shift added); isoAmbient: the ambient share of the shading in [0, 1] */
    float* isoGrad;
    uint32_t isoThreshold;
    float isoStored;
    float isoClassify;
    float isoAmbient;
    /* the walk cache (VRC_OPT_WALK_CACHE; at the end: no field above moves).  Which bricks a ray visits, and the interval
     * of each, depend on the ray, the brick grid, the node table and the frame constants vrc_brick_interval and
     * vrc_ray_grid_dda read -- not on the transfer function, the voxels or early termination -- so a view that stands
     * still over a resident brick set need not walk the grid again.  walkCache: 1 + 4 * walkK planes of walkPlane words
     * each, the context's, indexed tile * 64 + lane as rayCache is: plane 0 holds the ray's number of visits (0: the ray
     * misses, meets no brick, or the lane lies outside the frame), planes 1 + 4 k ... 4 + 4 k the k-th visit in the order
     * the walk makes them -- the index into the node table, the bits of vrc_segment_dist (all the uniform march reads
     * of a segment), tNear and tFar of the interval (what every other march completes, vrc_segment_complete).  Written
     * by the record form of the walk (VRC_MODE_WALK_RECORD, vrc_pixel_walk_record; walkK = 0: nothing is stored, the
     * pass only counts) and read by vrc_pixel_walk_replay; no other kernel looks at these */
    uint32_t* walkCache;
    uint32_t walkPlane;
    uint32_t walkK;
    /* the lean form of the lists (at the end: no field above moves).  walkLean != 0: a visit's second plane holds, where
     * the other form holds the bits of dist, the word vrc_walk_lean_word packs -- the visit's exact step count and its
     * node's slotInfoIndex, what the uniform march would otherwise fetch and compute again in every frame -- and the
     * replay is vrc_pixel_walk_replay_lean.  In the count pass (walkK = 0) it asks whether every visit can be packed.
     * walkSlots: the words of slotInfo, what an index read from a list is clamped by.  The host sets both
     * (vrc_render); a frame that leaves them 0 records and replays the other form.  VRC_WALK_LEAN_UNIFORM (a replayed
     * frame only): the same lists, and the host knows that none of their visits gathers -- the replay is the uniform-only
     * instance (vrc_pixel_walk_replay_lean< ..., true >) */
#define VRC_WALK_LEAN_UNIFORM 2u
    uint32_t walkLean;
    uint32_t walkSlots;
    /* a shaded composite frame (VRC_OPT_SHADING, the vrc_k_raycast_shade instances; at the end: no field above moves):
     * the ambient share of the headlight in [0, 1] (VRC_OPT_SHADING_AMBIENT / 1000).  No other kernel reads it */
    float shadeAmbient;
    /* the depth of a composite frame (VRC_OPT_COMPOSITE_DEPTH, the vrc_k_raycast_cdepth instances; at the end: no field
     * above moves): the opacity threshold, (float)value / 1000.0f.  The passes of the frame meet in mipMax (the bits of V,
     * VRC_MIP_EMPTY = not crossed) and mipDepth (D), owned, invalidated and not read by a first pass (mipFirst) as an
     * isosurface frame's are.  No other kernel reads it */
    float cdepthTau;
    /* a pre-integrated composite frame (VRC_OPT_PREINTEGRATION, the vrc_k_raycast_preint instances; at the end: no field
     * above moves): the 256 x 256 table of the frame, value-indexed (point samples of 8-bit voxels) or texel-indexed
     * (vrc_preint_entry).  No other kernel reads it */
    const vrc_f4* preintTable;
    /* how a replayed frame's pixels leave the march (VRC_OPT_STORE_THROUGH, vrc_store_pixel; at the end: no field above
     * moves).  1: every pixel store of the replay is a 16-byte write-through store through a buffer resource of
     * width * height * 16 bytes, which the host has checked fits 32 bits (vrc_plan_store_through); 0: the plain store.
     * The same bytes either way.  Set behind everything that compares frames; no other kernel reads it */
    uint32_t storeThrough;
    /* the first-visit table of a replayed lean frame (VRC_OPT_FIRST_VISIT_TABLE, vrc_first_visit_row; at the end: no
     * field above moves).  VRC_FIRST_VISIT_ENTRIES rows of VRC_FIRST_VISIT_ROWS colours in the form the frame marches
     * (vrc_lean_colour: two floats under a grey table, else four), built from the classified table the frame stages;
     * NULL: every first visit is marched (vrc_plan_first_visit).  Set behind everything that compares frames; read by
     * the uncounted lean instances of vrc_k_raycast_replay alone */
    const void* firstVisit;
    /* the free body of the lean march (VRC_OPT_LEAN_FREE_MARCH, vrc_march_uniform_free; at the end: no field above
     * moves).  1: a uniform visit of a replayed lean frame that cannot reach VRC_EARLY_EXIT -- by a per-lane test of its
     * start alpha, entry and count -- runs its composites without the exit test; 0: every lane takes the tested march.
     * The same bytes either way (vrc_plan_lean_free_march).  Set behind everything that compares frames; read by the
     * uncounted lean instances of vrc_k_raycast_replay alone */
    uint32_t leanFree;
    /* the resolved visit words of a uniform-only replay (VRC_OPT_WALK_RESOLVED, vrc_walk_resolved_word; at the end: no
     * field above moves).  walkK planes of walkPlane words, visit v of ray i at [v * walkPlane + i]: the list word's
     * step count, the value of the brick's slot word and whether the visit is marched at all -- what the slot words
     * say of these lists for as long as the pool takes no upload and slotInfo is the same array (vrc_render keeps the
     * planes to that).  NULL: the replay reads the list word and the slot word of every visit (vrc_plan_walk_resolved).
     * The same bytes either way.  Set behind everything that compares frames; read by the uncounted uniform-only
     * instances of vrc_k_raycast_replay alone */
    const uint32_t* walkResolved;
    /* a slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE, the vrc_k_raycast_slice instances; at the end: no field
     * above moves): vrc_set_slice's plane (nx, ny, nz, d), n.x + d = 0.  The passes of the frame meet in mipMax (the bits
     * of V, VRC_MIP_EMPTY = not sampled) and mipDepth (D = t_p), owned, invalidated and not read by a first pass (mipFirst)
     * as a composite-depth frame's are.  All zero in every other frame; no other kernel reads it */
    float slicePlane[4];
};
#define VRC_RAY_COMPUTE 0u
#define VRC_RAY_STORE 1u
#define VRC_RAY_LOAD 2u
/* planes of vrc_frame::rayCache: dir, invDir, tNearGlobal, tFarGlobal, tNearPlane, hit (a word: 0 or 1); origin is the eye */
#define VRC_RAY_CACHE_PLANES 10u

/* Atlas memory layout.  The logical atlas is the reference's 3-D array of slots
 * (cuda/TexturePool.cu:128-150); physically every slot is one contiguous run of
 * slotDim.x*slotDim.y*slotDim.z elements, and inside a slot voxels are grouped in 8x8x8
 * micro-blocks (x fastest inside a block, blocks x-fastest inside the slot).  A brick is
 * therefore one contiguous 2.4 MiB range (TLB-friendly) and the 64 fetches of a wave step
 * land in a few 64-byte segments. */
struct vrc_layout
{
    uint32_t slots[3];   /* slot grid */
    uint32_t slotDim[3]; /* padded slot size in voxels, multiples of 8 */
};

/* ---- slot-local layout: element offset = LX(x) + LY(y) + LZ(z), one part per axis ---------------
 * 8x8x8 micro-blocks, blocks x-fastest inside the slot; inside a block the 64 x-rows of 8 voxels lie in the order y & 3, z & 3, y >> 2, z >> 2, so that a 128-byte line -- what an L2 fetches
 * from HBM -- is a block of 8 x 4 x 4 voxels and the lines a tile touches per step are the same for views along every
 * axis (round 4; rounds 1-3 had the rows in the order y, z -- lines of 8 x 8 x 2 -- and ran views along x and y
 * 17 % / 7 % slower than along z: profiles/r4_byte_atlas_line_shapes.txt).  Rows y and y + 1 (y even) stay neighbours.
 * The layouts measured against it and retired: DESIGN_HISTORY.md and profiles/r4_byte_atlas_line_shapes.txt. */
/* in-block offset of row y / slice z (bits 0-2 of u count) */
VRC_HD uint32_t vrc_mb_y( uint32_t u ) { return ( ( u & 3u ) << 3 ) | ( ( u & 4u ) << 5 ); }
VRC_HD uint32_t vrc_mb_z( uint32_t u ) { return ( ( u & 3u ) << 5 ) | ( ( u & 4u ) << 6 ); }
/* the same as corrections of the plain order: vrc_mb_y( u ) = 8 (u & 7) + VRC_MB_FIX_Y( u ),
 * vrc_mb_z( u ) = 64 (u & 7) - VRC_MB_FIX_Z( u ) -- what the arithmetic address paths add to 8 y + 64 z */
#define VRC_MB_FIX_Y( u ) ( 96u * ( ( ( u ) >> 2 ) & 1u ) )
#define VRC_MB_FIX_Z( u ) ( 32u * ( ( u ) & 3u ) )
struct vrc_lay
{
    uint32_t a, b, c; /* what a step to the next micro-block adds along x, y, z beyond the plain 1, 8, 64 per voxel */
};
VRC_HD vrc_lay vrc_make_lay( uint32_t sbx, uint32_t sby )
{
    vrc_lay l;
    l.a = 504u; l.b = sbx * VRC_MB_VOXELS - 64u; l.c = sbx * sby * VRC_MB_VOXELS - 512u;
    return l;
}
VRC_HD uint32_t vrc_lay_x( const vrc_lay& l, uint32_t u )
{
    return u + l.a * ( u >> 3 );
}
VRC_HD uint32_t vrc_lay_y( const vrc_lay& l, uint32_t u )
{
    return 8u * u + l.b * ( u >> 3 ) + VRC_MB_FIX_Y( u );
}
VRC_HD uint32_t vrc_lay_z( const vrc_lay& l, uint32_t u )
{
    return 64u * u + l.c * ( u >> 3 ) - VRC_MB_FIX_Z( u );
}
/* physical elements of one slot */
VRC_HD uint64_t vrc_slot_elems( uint32_t sdx, uint32_t sdy, uint32_t sdz )
{
    return (uint64_t)sdx * sdy * sdz;
}

/* element offset of voxel (x,y,z), local to a slot of sbx x sby x * micro-blocks */
VRC_HD uint32_t vrc_slot_local_index( uint32_t x, uint32_t y, uint32_t z, uint32_t sbx, uint32_t sby )
{
    const uint32_t blk = ( ( z >> VRC_MB_SHIFT ) * sby + ( y >> VRC_MB_SHIFT ) ) * sbx +
                         ( x >> VRC_MB_SHIFT );
    const uint32_t inner = vrc_mb_z( z ) | vrc_mb_y( y ) | ( x & 7u );
    return blk * VRC_MB_VOXELS + inner;
}

/* element offset of slot (i,j,k): 64 bits, an atlas may hold more than 2^32 voxels (it is sized
 * for the GPU's memory, not for a 32-bit index; the reference truncates, quirk Q12) */
VRC_HD uint64_t vrc_slot_base( const vrc_layout& l, uint32_t i, uint32_t j, uint32_t k )
{
    const uint64_t slotVoxels = vrc_slot_elems( l.slotDim[0], l.slotDim[1], l.slotDim[2] );
    return ( ( (uint64_t)k * l.slots[1] + j ) * l.slots[0] + i ) * slotVoxels;
}

/* physical element index of logical atlas voxel (x,y,z) */
VRC_HD uint64_t vrc_atlas_index( const vrc_layout& l, uint32_t x, uint32_t y, uint32_t z )
{
    const uint32_t i = x / l.slotDim[0], j = y / l.slotDim[1], k = z / l.slotDim[2];
    return vrc_slot_base( l, i, j, k ) +
           vrc_slot_local_index( x - i * l.slotDim[0], y - j * l.slotDim[1], z - k * l.slotDim[2],
                                 l.slotDim[0] >> VRC_MB_SHIFT, l.slotDim[1] >> VRC_MB_SHIFT );
}

/* ------------------------------------------------------------------------------------------
 * Classified-sample table entry for u8 density d: what Renderer.cu:215-218 computes from a
 * sample of that density: tf = tex1D(tfTex, d*mult+add) (cuda/ColorMap.cu:40-45: 256 texels,
 * linear, normalized, clamp; the lerp weight is kept in fracBits fractional bits, 8 on CUDA
 * hardware, 0 = exact float); alpha' = 1 - pow(1 - min(tf.a, 255/256), alphaCorrection)
 * (Renderer.cu:88-89); entry = (tf.rgb*alpha', alpha').  A pure function of d within a frame.
 * ---------------------------------------------------------------------------------------- */
struct vrc_lut_params
{
    float rangeMin, rangeMax; /* RenderData.dataSourceRange, Renderer.cu:162-164 */
    float alphaCorrection;    /* maxSamplesPerRay / samplesPerRay, Renderer.cu:167-168 */
    int fracBits;
};

VRC_HD vrc_f4 vrc_lut_entry( const float* tf, uint32_t d, vrc_lut_params p )
{
#if defined( __clang__ )
#pragma clang fp contract( off )
#endif
    const float multiplyer = 1.0f / ( p.rangeMax - p.rangeMin );
    const float addedValue = -p.rangeMin / ( p.rangeMax - p.rangeMin );
    const float u = (float)d * multiplyer + addedValue;
    const float xB = u * 256.0f - 0.5f;
    const float fl = floorf( xB );
    float a = xB - fl;
    if( p.fracBits > 0 )
    {
        const float q = (float)( 1 << p.fracBits );
        a = floorf( a * q + 0.5f ) / q;
    }
    int i0 = (int)fl, i1 = (int)fl + 1;
    i0 = i0 < 0 ? 0 : ( i0 > 255 ? 255 : i0 );
    i1 = i1 < 0 ? 0 : ( i1 > 255 ? 255 : i1 );
    float c[4];
    for( int k = 0; k < 4; ++k )
        c[k] = ( 1.0f - a ) * tf[i0 * 4 + k] + a * tf[i1 * 4 + k];
    const float corr = 1.0f - fminf( c[3], 1.0f - 1.0f / 256.0f );
    const float alpha = 1.0f - powf( corr, p.alphaCorrection );
    vrc_f4 e;
    e.x = c[0] * alpha;
    e.y = c[1] * alpha;
    e.z = c[2] * alpha;
    e.w = alpha;
    return e;
}

/* cuda/math.cuh:1457-1464 (column-major 4x4 times vec4) */
VRC_HD vrc_f4 vrc_mul44( const float* m, vrc_f4 v )
{
    VRC_STRICT_FP
    vrc_f4 r;
    r.x = m[0] * v.x + m[4] * v.y + m[8] * v.z + m[12] * v.w;
    r.y = m[1] * v.x + m[5] * v.y + m[9] * v.z + m[13] * v.w;
    r.z = m[2] * v.x + m[6] * v.y + m[10] * v.z + m[14] * v.w;
    r.w = m[3] * v.x + m[7] * v.y + m[11] * v.z + m[15] * v.w;
    return r;
}

VRC_HD float vrc_dot( vrc_f3 a, vrc_f3 b )
{
    VRC_STRICT_FP
    return a.x * b.x + a.y * b.y + a.z * b.z;
}

/* cuda/math.cuh:1310-1314 */
VRC_HD vrc_f3 vrc_normalize( vrc_f3 v )
{
    VRC_STRICT_FP
    const float invLen = 1.0f / sqrtf( vrc_dot( v, v ) );
    vrc_f3 r = { v.x * invLen, v.y * invLen, v.z * invLen };
    return r;
}

/* Renderer.cu:56-80; invR is hoisted (the reference recomputes the same value per call) */
VRC_HD bool vrc_intersect_box( vrc_f3 origin, vrc_f3 invR, vrc_f3 boxMin, vrc_f3 boxMax,
                               float* tnear, float* tfar )
{
    VRC_STRICT_FP
    const float tbx = invR.x * ( boxMin.x - origin.x ), ttx = invR.x * ( boxMax.x - origin.x );
    const float tby = invR.y * ( boxMin.y - origin.y ), tty = invR.y * ( boxMax.y - origin.y );
    const float tbz = invR.z * ( boxMin.z - origin.z ), ttz = invR.z * ( boxMax.z - origin.z );
    const float tminx = fminf( ttx, tbx ), tmaxx = fmaxf( ttx, tbx );
    const float tminy = fminf( tty, tby ), tmaxy = fmaxf( tty, tby );
    const float tminz = fminf( ttz, tbz ), tmaxz = fmaxf( ttz, tbz );
    const float largestTmin = fmaxf( fmaxf( tminx, tminy ), tminz );
    const float smallestTmax = fminf( fminf( tmaxx, tmaxy ), tmaxz );
    *tnear = largestTmin;
    *tfar = smallestTmax;
    return smallestTmax > largestTmin;
}

struct vrc_ray
{
    vrc_f3 origin, dir, invDir;
    float tNearGlobal, tFarGlobal, tNearPlane;
    bool hit;
};

/* Renderer.cu:106-149 + :159-160: pixel -> world ray, global box, clip planes, near plane */
/* wx, wy: window-space position the ray is cast through (gl_FragCoord of the GLSL twin; its jittered
 * sub-pixel positions, fragRaycast.glsl:123-127) */
VRC_HD vrc_ray vrc_setup_ray_at( const vrc_frame& f, float wx, float wy )
{
    VRC_STRICT_FP
    vrc_ray r;
    /* Renderer.cu:40-51 */
    const float nx = 2.0f * ( wx - f.vpX - ( f.vpW / 2.0f ) ) / f.vpW;
    const float ny = 2.0f * ( wy - f.vpY - ( f.vpH / 2.0f ) ) / f.vpH;
    const vrc_f4 ndc = { nx, ny, 1.0f, 1.0f };
    const vrc_f4 e = vrc_mul44( f.invProj, ndc );
    const vrc_f4 eyeSpace = { e.x / e.w, e.y / e.w, e.z / e.w, e.w / e.w };
    const vrc_f4 world = vrc_mul44( f.invView, eyeSpace );
    r.origin.x = f.eye[0];
    r.origin.y = f.eye[1];
    r.origin.z = f.eye[2];
    const vrc_f3 d0 = { world.x - r.origin.x, world.y - r.origin.y, world.z - r.origin.z };
    r.dir = vrc_normalize( d0 );
    if( r.dir.x == 0.0f ) r.dir.x = VRC_EPSILON;
    if( r.dir.y == 0.0f ) r.dir.y = VRC_EPSILON;
    if( r.dir.z == 0.0f ) r.dir.z = VRC_EPSILON;
    r.invDir.x = 1.0f / r.dir.x;
    r.invDir.y = 1.0f / r.dir.y;
    r.invDir.z = 1.0f / r.dir.z;

    const vrc_f3 gmin = { f.aabbMin[0], f.aabbMin[1], f.aabbMin[2] };
    const vrc_f3 gmax = { f.aabbMax[0], f.aabbMax[1], f.aabbMax[2] };
    r.hit = vrc_intersect_box( r.origin, r.invDir, gmin, gmax, &r.tNearGlobal, &r.tFarGlobal );
    if( f.variant == VRC_VARIANT_GL ) /* fragRaycast.glsl:101: t0 <= t1 */
        r.hit = r.tNearGlobal <= r.tFarGlobal;

    /* Renderer.cu:132-146; the GLSL twin clips per brick instead (fragRaycast.glsl:162-174) */
    for( uint32_t i = 0; i < ( f.variant == VRC_VARIANT_GL ? 0u : f.nPlanes ); ++i )
    {
        const vrc_f3 n = { f.planes[i][0], f.planes[i][1], f.planes[i][2] };
        float rn = vrc_dot( r.dir, n );
        if( rn == 0.0f )
            rn = VRC_EPSILON;
        const float t = -( vrc_dot( n, r.origin ) + f.planes[i][3] ) / rn;
        if( rn > 0.0f )
            r.tNearGlobal = fmaxf( r.tNearGlobal, t );
        else
            r.tFarGlobal = fminf( r.tFarGlobal, t );
    }
    if( r.tNearGlobal > r.tFarGlobal )
        r.hit = false;

    /* Renderer.cu:159-160 */
    const vrc_f3 e3 = { eyeSpace.x, eyeSpace.y, eyeSpace.z };
    const vrc_f3 ne = vrc_normalize( e3 );
    r.tNearPlane = -f.nearPlane / ne.z;
    return r;
}

VRC_HD vrc_ray vrc_setup_ray( const vrc_frame& f, uint32_t px, uint32_t py )
{
    VRC_STRICT_FP
    return vrc_setup_ray_at( f, (float)px + f.pixelOffX, (float)py + f.pixelOffY );
}

/* rand() of fragRaycast.glsl:59-62: fract(sin(dot(co, vec2(12.9898, 78.233))) * 43758.5453).  What a GL
 * implementation's sin() returns for arguments of 1e4..1e6 is implementation-defined to more bits than the
 * factor 43758 leaves, so no two GPUs jitter alike; THIS build defines it with the sine evaluated in double
 * (libm and the device library agree to the float), the rest in float without contraction -- the oracle's
 * gl_rand, bit for bit. */
VRC_HD float vrc_gl_rand( float x, float y )
{
    VRC_STRICT_FP
    const float d = x * 12.9898f + y * 78.233f;
    const float sn = (float)sin( (double)d );
    const float v = sn * 43758.5453f;
    return v - floorf( v );
}

/* One brick segment of one ray, Renderer.cu:179-201: returns false if the brick is skipped.
 * stop: set when the reference would leave the node loop (tNear > tFarGlobal). */
struct vrc_segment
{
    vrc_f3 pos;   /* rayStart */
    vrc_f3 step;  /* normalize(stop-start)*stepSize */
    float dist;
    float tNear;  /* ray parameter of rayStart */
};

/* The segment in two parts.  The interval part is everything of Renderer.cu:179-194 -- the slab test, the global
 * interval, the near plane, and for the GLSL twin the lattice snap and the per-brick clip planes -- up to the final
 * tNear / tFar, `stop` and the early returns.  The completion part (Renderer.cu:195-201) makes pos, step, dist and
 * tNear of it.  vrc_brick_segment is the two in a row, statement for statement what it was as one function.  A march
 * that needs less completes less: the uniform march reads dist alone (vrc_segment_dist: the same expressions in the
 * same order, so the same bits) and leaves the division and the three products of `step` to the marches that step
 * (vrc_march_brick on an interval, below). */
struct vrc_interval
{
    float tNear, tFar;
};

VRC_HD bool vrc_brick_interval( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node& n,
                                float stepSize, vrc_interval* iv, bool* stop )
{
    VRC_STRICT_FP
    const vrc_f3 boxMin = { n.aabbMin[0], n.aabbMin[1], n.aabbMin[2] };
    const vrc_f3 boxMax = { boxMin.x + n.aabbSize[0], boxMin.y + n.aabbSize[1],
                            boxMin.z + n.aabbSize[2] };
    float tNear = 0.0f, tFar = 0.0f;
    *stop = false;
    if( f.variant == VRC_VARIANT_GL )
    {
        /* fragRaycast.glsl:142-177: hit test t0 <= t1; tnear raised to the near plane only;
         * first sample snapped to the lattice tnearGlobal + k*stepSize; clip planes move this
         * brick's interval, after the snap */
        (void)vrc_intersect_box( r.origin, r.invDir, boxMin, boxMax, &tNear, &tFar );
        if( !( tNear <= tFar ) )
            return false;
        if( tNear < r.tNearPlane )
            tNear = r.tNearPlane;
        const float a = tNear - r.tNearGlobal;
        const float residu = a - stepSize * floorf( a / stepSize );
        if( residu > 0.0f )
            tNear += stepSize - residu;
        if( tNear > tFar )
            return false;
        for( uint32_t i = 0; i < f.nPlanes; ++i )
        {
            const vrc_f3 pn = { f.planes[i][0], f.planes[i][1], f.planes[i][2] };
            float rn = vrc_dot( r.dir, pn );
            if( rn == 0.0f )
                rn = VRC_EPSILON;
            const float t = -( vrc_dot( pn, r.origin ) + f.planes[i][3] ) / rn;
            if( rn > 0.0f )
                tNear = fmaxf( tNear, t );
            else
                tFar = fminf( tFar, t );
        }
        if( tNear > tFar )
            return false;
    }
    else
    {
        if( !vrc_intersect_box( r.origin, r.invDir, boxMin, boxMax, &tNear, &tFar ) )
            return false;
        if( tNear > r.tFarGlobal )
        {
            *stop = true;
            return false;
        }
        if( tFar < r.tNearGlobal )
            return false;
        tNear = fmaxf( fmaxf( r.tNearPlane, tNear ), r.tNearGlobal );
        tFar = fminf( tFar, r.tFarGlobal );
        if( tNear > tFar )
            return false;
    }
    iv->tNear = tNear;
    iv->tFar = tFar;
    return true;
}

/* dist of the completed segment, and nothing else of it */
VRC_HD float vrc_segment_dist( const vrc_ray& r, const vrc_interval& iv )
{
    VRC_STRICT_FP
    const float tNear = iv.tNear, tFar = iv.tFar;
    const vrc_f3 rayStart = { r.origin.x + r.dir.x * tNear, r.origin.y + r.dir.y * tNear,
                              r.origin.z + r.dir.z * tNear };
    const vrc_f3 rayStop = { r.origin.x + r.dir.x * tFar, r.origin.y + r.dir.y * tFar,
                             r.origin.z + r.dir.z * tFar };
    const vrc_f3 diff = { rayStop.x - rayStart.x, rayStop.y - rayStart.y,
                          rayStop.z - rayStart.z };
    const float d2 = vrc_dot( diff, diff );
    return sqrtf( d2 );
}

VRC_HD void vrc_segment_complete( const vrc_ray& r, const vrc_interval& iv, float stepSize, vrc_segment* s )
{
    VRC_STRICT_FP
    const float tNear = iv.tNear, tFar = iv.tFar;
    const vrc_f3 rayStart = { r.origin.x + r.dir.x * tNear, r.origin.y + r.dir.y * tNear,
                              r.origin.z + r.dir.z * tNear };
    const vrc_f3 rayStop = { r.origin.x + r.dir.x * tFar, r.origin.y + r.dir.y * tFar,
                             r.origin.z + r.dir.z * tFar };
    const vrc_f3 diff = { rayStop.x - rayStart.x, rayStop.y - rayStart.y,
                          rayStop.z - rayStart.z };
    const float d2 = vrc_dot( diff, diff );
    const float invLen = 1.0f / sqrtf( d2 );
    s->pos = rayStart;
#if defined( VRC_DEV_BUILD ) && defined( VRC_TEST_BIAS_ENTRY )
    /* NEGATIVE CONTROL of the parity rule (tests/test_cpu_harness.py::test_parity_rule_rejects_a_biased_kernel; never in
     * the product: __graft_entry__.build() does not define VRC_DEV_BUILD): every brick segment starts 2e-7 world units
     * early, so its first sample -- the reference puts it exactly on the brick face, cuda/Renderer.cu:195-196 -- always
     * reads the voxel on the near side of the face.  Every such flip is inside the oracle's tie zone; the rule must
     * still reject a kernel that takes all of them. */
    s->pos.x -= r.dir.x * 2e-7f;
    s->pos.y -= r.dir.y * 2e-7f;
    s->pos.z -= r.dir.z * 2e-7f;
#endif
    s->step.x = diff.x * invLen * stepSize;
    s->step.y = diff.y * invLen * stepSize;
    s->step.z = diff.z * invLen * stepSize;
    s->dist = sqrtf( d2 );
    s->tNear = tNear;
}

VRC_HD bool vrc_brick_segment( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node& n,
                               float stepSize, vrc_segment* s, bool* stop )
{
    vrc_interval iv;
    if( !vrc_brick_interval( f, r, n, stepSize, &iv, stop ) )
        return false;
    vrc_segment_complete( r, iv, stepSize, s );
    return true;
}

/* Where a march takes its segment from: one that is complete already, or the interval it is completed from at the
 * place it is used (vrc_march_brick).  full(): the segment; distOnly(): dist and tNear of it, the rest zero -- all the
 * uniform march reads */
struct vrc_segment_ready
{
    const vrc_segment& s;
    VRC_HD const vrc_segment& full() const { return s; }
    VRC_HD const vrc_segment& distOnly() const { return s; }
};
struct vrc_segment_from_interval
{
    const vrc_ray& r;
    const vrc_interval& iv;
    float stepSize;
    VRC_HD vrc_segment full() const
    {
        vrc_segment s;
        vrc_segment_complete( r, iv, stepSize, &s );
        return s;
    }
    VRC_HD vrc_segment distOnly() const
    {
        const vrc_f3 zero = { 0.0f, 0.0f, 0.0f };
        vrc_segment s = { zero, zero, vrc_segment_dist( r, iv ), iv.tNear };
        return s;
    }
};

/* 24-bit multiply (v_mul_u32_u24 / v_mad_u32_u24 on gfx950: full rate, where a 32-bit
 * multiply is quarter rate). */
VRC_HD uint32_t vrc_mul24( uint32_t a, uint32_t b )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __umul24( a, b );
#else
    return ( a & 0xFFFFFFu ) * ( b & 0xFFFFFFu );
#endif
}

/* Per-brick sampler constants, hoisted out of the march loop. */
struct vrc_sampler
{
    float minx, miny, minz;   /* aabbMin */
    float kx, ky, kz;         /* atlas voxels per world unit */
    float ox, oy, oz;         /* slot-local voxel coordinate of aabbMin (= overlap) */
    float hix, hiy, hiz;      /* slotDim - 1 (clamped sampler only) */
    uint32_t slotBase;        /* element offset of the slot */
    uint32_t cyy, czz;        /* micro-block stride in y / z minus the in-block stride * 8 */
};

VRC_HD vrc_sampler vrc_make_sampler( const vrc_dev_node& n, const vrc_frame& f )
{
    vrc_sampler s;
    s.minx = n.aabbMin[0]; s.miny = n.aabbMin[1]; s.minz = n.aabbMin[2];
    s.kx = n.voxPerWorld[0]; s.ky = n.voxPerWorld[1]; s.kz = n.voxPerWorld[2];
    s.ox = n.localOrigin[0]; s.oy = n.localOrigin[1]; s.oz = n.localOrigin[2];
    s.hix = (float)( f.slotDim[0] - 1u );
    s.hiy = (float)( f.slotDim[1] - 1u );
    s.hiz = (float)( f.slotDim[2] - 1u );
    s.slotBase = n.slotBase;
    s.cyy = f.sbx * VRC_MB_VOXELS - 64u;
    s.czz = f.sbx * f.sby * VRC_MB_VOXELS - 512u;
    return s;
}

/* brick-local voxel of a world position (nearest, Renderer.cu:210-214 + point sampling of
 * cuda/TexturePool.cu:163-170), as the physical element index in the atlas.
 * Evaluated brick-locally so the float grid is finer than the reference's normalized
 * atlas coordinate; voxel choice can differ only for samples within ~1e-4 voxel of a
 * voxel face ("nearest-voxel flips").  Coordinates are >= 0 here, so the
 * float->int truncation is the floor of the point-sampling rule. */
/* element offset of slot-local voxel (ux,uy,uz) */
VRC_HD uint32_t vrc_voxel_address( const vrc_sampler& s, uint32_t ux, uint32_t uy, uint32_t uz )
{
    /* element = slotBase + sum over axes of (c >> 3) * blockStride + (c & 7) * inStride with
     * inStride = 1, 8, 64 and blockStride = 512, 512*sbx, 512*sbx*sby.  Since
     * (c & 7) * s = c * s - (c >> 3) * 8 * s this is
     *   slotBase + x + 8 y + 64 z + qx * 504 + qy * (512 sbx - 64) + qz * (512 sbx sby - 512):
     * three shifts, three 24-bit multiply-adds (full rate; operands < 2^24: slot-local block
     * counts <= 512, slot < 16 Mi elements, checked at pool creation), two shift-adds, one add --
     * plus the row order's corrections (VRC_MB_FIX_Y / _Z: the rows of a block lie y & 3, z & 3, y >> 2, z >> 2). */
#if defined( __HIP_DEVICE_COMPILE__ )
    /* spelled out: hipcc otherwise emits multiply + 3-input add pairs (eleven instructions).
     * v_mad_u32_u24 takes one scalar operand (the stride). */
    uint32_t e, t;
    asm( "v_mad_u32_u24 %0, %1, %2, %3" : "=v"( e ) : "v"( ux >> VRC_MB_SHIFT ), "s"( 504u ), "v"( ux ) );
    asm( "v_mad_u32_u24 %0, %1, %2, %3" : "=v"( t ) : "v"( uy >> VRC_MB_SHIFT ), "s"( s.cyy ), "v"( e ) );
    asm( "v_mad_u32_u24 %0, %1, %2, %3" : "=v"( e ) : "v"( uz >> VRC_MB_SHIFT ), "s"( s.czz ), "v"( t ) );
    asm( "v_lshl_add_u32 %0, %1, 3, %2" : "=v"( t ) : "v"( uy ), "v"( e ) );
    asm( "v_lshl_add_u32 %0, %1, 6, %2" : "=v"( e ) : "v"( uz ), "v"( t ) );
    return e + s.slotBase + VRC_MB_FIX_Y( uy ) - VRC_MB_FIX_Z( uz );
#else
    uint32_t e = vrc_mul24( ux >> VRC_MB_SHIFT, 504u ) + ux;
    e = vrc_mul24( uy >> VRC_MB_SHIFT, s.cyy ) + e;
    e = vrc_mul24( uz >> VRC_MB_SHIFT, s.czz ) + e;
    e = ( uy << 3 ) + e;
    e = ( uz << 6 ) + e;
    return e + s.slotBase + VRC_MB_FIX_Y( uy ) - VRC_MB_FIX_Z( uz );
#endif
}

/* Atlas element indices of the next N samples of a segment, advancing pos by N steps.
 * Per sample: brick-local voxel of the world position (nearest, Renderer.cu:210-214 + point
 * sampling of cuda/TexturePool.cu:163-170): l = (pos - aabbMin) * voxelsPerWorld + localOrigin,
 * voxel = trunc(l) (l >= 0, so truncation is the floor of the point-sampling rule), evaluated
 * brick-locally so the float grid is finer than the reference's normalized atlas coordinate;
 * the voxel can differ only for samples within ~1e-4 voxel of a voxel face (DESIGN.md,
 * "nearest-voxel flips").  pos advances by sequential additions of step, as in the reference.
 * Scalar f32 instructions on purpose: on gfx950 a v_pk_add/fma_f32 costs ~2.9x a scalar
 * v_add_f32 (profiles/r1_ubench_valu_issue_costs.txt), so packing two lanes' worth of data
 * into one instruction loses; the file is also built with -fno-slp-vectorize. */
template < bool CLAMP, int N >
VRC_HD void vrc_group_indices( const vrc_sampler& s, vrc_f3& pos, const vrc_f3& step, uint32_t* idx )
{
    VRC_FAST_FP
#pragma unroll
    for( int k = 0; k < N; ++k )
    {
        float lx = ( pos.x - s.minx ) * s.kx + s.ox;
        float ly = ( pos.y - s.miny ) * s.ky + s.oy;
        float lz = ( pos.z - s.minz ) * s.kz + s.oz;
        if( CLAMP )
        {
            lx = fminf( fmaxf( lx, 0.0f ), s.hix );
            ly = fminf( fmaxf( ly, 0.0f ), s.hiy );
            lz = fminf( fmaxf( lz, 0.0f ), s.hiz );
        }
        idx[k] = vrc_voxel_address( s, (uint32_t)(int)lx, (uint32_t)(int)ly, (uint32_t)(int)lz );
        pos.x += step.x;
        pos.y += step.y;
        pos.z += step.z;
    }
}

/* Fixed-point alternative to the float position chain above (VRC_OPT_STEPPING = 1).
 * The slot-local voxel coordinate of the segment's first sample is computed exactly as above
 * (same float expression, so the sample on the brick face picks the same voxel), converted to
 * 8.24 fixed point (exact: l < 256 has at most 24 fraction bits below 2^8), and every further
 * sample adds the per-step voxel increment round(step * voxelsPerWorld * 2^24): one integer
 * add per axis instead of add + subtract + multiply-add + convert.  It is a more accurate
 * evaluation of start + n*step than the reference's float accumulation (error <= n * 2^-25
 * voxel against ~n * 6e-5), but not the same rounding path, so a sample within ~1e-4 voxel
 * of a voxel face may read the neighbouring voxel ("nearest-voxel flips").
 * Not used with the clamped sampler (coordinates must stay in [0, 256)). */
struct vrc_fixpos
{
    uint32_t x, y, z;    /* 8.24 slot-local voxel coordinates */
    uint32_t dx, dy, dz; /* per-step increments (two's complement) */
};

VRC_HD vrc_fixpos vrc_fixpos_init( const vrc_sampler& s, const vrc_f3& pos, const vrc_f3& step )
{
    /* (round 4, VERDICT r3 item 4: evaluated without contraction like the rest of the set-up -- VRC_STRICT_FP -- the
     * tie bias of the C2 noise rows stays 0.212 to the third digit and the kernel time where it was: the bias comes from
     * the truncation below, which at a face entered from above is the near side, not from the multiply-add) */
    VRC_FAST_FP
    vrc_fixpos p;
    const float lx = ( pos.x - s.minx ) * s.kx + s.ox;
    const float ly = ( pos.y - s.miny ) * s.ky + s.oy;
    const float lz = ( pos.z - s.minz ) * s.kz + s.oz;
    p.x = (uint32_t)( lx * 16777216.0f );
    p.y = (uint32_t)( ly * 16777216.0f );
    p.z = (uint32_t)( lz * 16777216.0f );
    p.dx = (uint32_t)(int32_t)rintf( step.x * s.kx * 16777216.0f );
    p.dy = (uint32_t)(int32_t)rintf( step.y * s.ky * 16777216.0f );
    p.dz = (uint32_t)(int32_t)rintf( step.z * s.kz * 16777216.0f );
    return p;
}

#if defined( __HIPCC__ )
/* Per-axis address parts of vrc_voxel_address as three 256-entry tables in LDS (filled by the
 * raycast kernel): TX[u] = u + 504 (u>>3), TY[u] = 8u + cyy (u>>3) + FIX_Y(u), TZ[u] = 64u + czz (u>>3) - FIX_Z(u).
 * Replaces 3 shifts + 3 24-bit multiply-adds + 2 shift-adds (the slow VALU classes) by 3 masks
 * + 3 LDS reads + one 3-input add per sample (measured 4 % faster on C2 than the arithmetic form, which the host
 * build keeps). */
__shared__ uint32_t vrc_addr_tab[3 * 256];
#endif

template < int N >
VRC_HD void vrc_group_indices_fixed( const vrc_sampler& s, vrc_fixpos& p, uint32_t* idx )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    uint32_t tx[N], ty[N], tz[N];
#pragma unroll
    for( int k = 0; k < N; ++k )
    {
        const char* const t = reinterpret_cast< const char* >( vrc_addr_tab );
        tx[k] = *reinterpret_cast< const uint32_t* >( t + ( ( p.x >> 22 ) & 0x3FCu ) );
        ty[k] = *reinterpret_cast< const uint32_t* >( t + 1024 + ( ( p.y >> 22 ) & 0x3FCu ) );
        tz[k] = *reinterpret_cast< const uint32_t* >( t + 2048 + ( ( p.z >> 22 ) & 0x3FCu ) );
        p.x += p.dx;
        p.y += p.dy;
        p.z += p.dz;
        /* keep the three additions per step: left alone, hipcc rewrites the chain as p + k * d with a
         * v_mul_lo_u32 or a shift-add per step and axis (the slow integer classes, profiles/r1_ubench_valu_issue_costs.txt)
         * to shorten a dependency that the other waves hide anyway */
        asm( "" : "+v"( p.x ), "+v"( p.y ), "+v"( p.z ) );
    }
#pragma unroll
    for( int k = 0; k < N; ++k )
        idx[k] = tx[k] + ty[k] + tz[k] + s.slotBase;
#else
#pragma unroll
    for( int k = 0; k < N; ++k )
    {
        idx[k] = vrc_voxel_address( s, p.x >> 24, p.y >> 24, p.z >> 24 );
        p.x += p.dx;
        p.y += p.dy;
        p.z += p.dz;
    }
#endif
}

/* Renderer.cu:83-93 with the classified table: e = (rgb*alpha', alpha') for the density.
 * frozen: the ray already crossed the early-exit threshold; the weight is forced to 0 so the
 * step is an exact no-op (x + e*0 == x) without making the table address depend on it. */
VRC_HD void vrc_composite( vrc_f4& c, const vrc_f4& e, bool frozen = false )
{
    VRC_FAST_FP
    float t = 1.0f - c.w;
    t = frozen ? 0.0f : t;
    c.x = c.x + e.x * t;
    c.y = c.y + e.y * t;
    c.z = c.z + e.z * t;
    c.w = c.w + e.w * t;
}
/* the same blend for a grey table: red, green and blue of the four-float form are the same three operations on the
 * same numbers, so doing them once gives the same bits */
VRC_HD void vrc_composite( vrc_f2& c, const vrc_f2& e, bool frozen = false )
{
    VRC_FAST_FP
    float t = 1.0f - c.w;
    t = frozen ? 0.0f : t;
    c.x = c.x + e.x * t;
    c.w = c.w + e.w * t;
}

/* ------------------------------------------------------------------------------------------
 * March one brick segment (Renderer.cu:206-223).
 *
 * The kernel is VALU-issue bound on MI355X (a wave64 VALU instruction costs ~4 cycles of its
 * SIMD; measured: removing every memory access changes the frame time by < 15 %), so the
 * march is organised to spend as few vector instructions per sample as possible:
 *   - samples are taken in groups of VRC_GROUP: indices, then VRC_GROUP byte gathers issued
 *     back to back, then VRC_GROUP table reads, then the blends;
 *   - FAST groups: while more than VRC_GROUP steps remain on the segment every sample of the
 *     group is one the reference loop reaches, so there is no per-sample bounds test, no
 *     index select and no table-index select;
 *   - early ray termination is tested once per group (alpha never decreases); only when the
 *     threshold was crossed inside the group is the group replayed sample by sample from the
 *     saved colour, which reproduces the reference's exit after the crossing sample exactly;
 *   - the TAIL (at most VRC_GROUP + 1 remaining steps) runs the general branch-free form: a
 *     sample the reference would not reach fetches element 0 and blends table entry 256,
 *     which is all zeros -- an exact no-op.
 * The composited sample sequence is the reference's, sample for sample, in both paths.
 * lut has 257 entries; lut[256] = 0.
 * Returns true when the early-ray-termination threshold was crossed (Renderer.cu:219-226).
 * ---------------------------------------------------------------------------------------- */
#ifndef VRC_GROUP
#define VRC_GROUP 8
#endif

struct vrc_classifier;
VRC_HD vrc_f4 vrc_classify( const vrc_f4* tfp, float d, const vrc_classifier& k );
VRC_HD vrc_f2 vrc_classify( const vrc_f2* tfp, float d, const vrc_classifier& k );

/* table entry of a fetched voxel: lut[d] -- or, PERSAMPLE (volumes the 257-entry table cannot index: 16-bit
 * voxels), the transfer function and the opacity correction evaluated on the value (vrc_classify; lut is then the
 * padded transfer function and the entries are four floats) */
/* D: what a fetched voxel is held as between the gather and the table: uint32_t for the integer atlases, float for the
 * float atlas (32-bit and float volumes, include/vrc_hip.h: vrc_pool_create_typed), which is always PERSAMPLE */
template < typename ATLAS_T >
struct vrc_density
{
    typedef uint32_t type;
};
template <>
struct vrc_density< float >
{
    typedef float type;
};
template < bool PERSAMPLE, typename E, typename D >
VRC_HD E vrc_entry( const E* lut, D d, const vrc_classifier* cls )
{
    if constexpr( PERSAMPLE )
        return vrc_classify( lut, (float)d, *cls );
    else
        return lut[d];
}

/* ------------------------------------------------------------------------------------------
 * The uniform march counted in integers (the form vrc_march_segment_as< ..., UNIFORM > takes when it is exact).
 *
 * The reference steps a segment with `travel -= stepSize` while `travel > 0` (Renderer.cu:206-223).  When stepSize
 * is a power of two 2^j and travel < 2^24 * stepSize, every one of those subtractions is exact as long as
 * travel >= stepSize: travel is a multiple of its own ulp 2^k, and travel < 2^(j+24) gives k <= j, so stepSize is a
 * multiple of 2^k as well and the smaller difference is representable.  The last subtraction (0 < travel <
 * stepSize) only has to come out negative, which rounding cannot change.  The loop therefore takes exactly
 * n = ceil( travel / stepSize ) trips, and q = travel * (1 / stepSize) is exact too (a change of exponent; should it
 * underflow, q is below one and n = 1 either way).  With n in hand, "travel > 0" is "nLeft > 0", and a group of G
 * samples is all the reference's when nLeft >= G -- no float chain, no guard of one spare step.
 * stepSize is 1 / samplesPerRay (vrc_fill_frame), times 2^level under per-ray LOD: sample counts of 256, 512, 1024,
 * 2048 qualify, 300 or 1000 do not and keep the float chain.
 * ---------------------------------------------------------------------------------------- */
VRC_HD uint32_t vrc_float_bits( float v )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __float_as_uint( v );
#else
    uint32_t u;
    __builtin_memcpy( &u, &v, 4 );
    return u;
#endif
}
VRC_HD float vrc_bits_float( uint32_t u )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __uint_as_float( u );
#else
    float v;
    __builtin_memcpy( &v, &u, 4 );
    return v;
#endif
}

/* What a brick upload does to a voxel on its way into the atlas (include/vrc_hip.h: vrc_pool_create_typed), and
 * vrc_pool_read_region undoes where it can.  T is the unsigned integer of the voxel's size; the 32-bit forms return
 * the bits of the float the atlas holds.
 *   FLIP  signed 8/16-bit: offset binary, v ^ sign bit = v + 128 / + 32768 as an unsigned number (its own inverse);
 *   U32F / I32F  32-bit integers: converted to float32, round to nearest even (the conversion the GLSL reference
 *         applies to every usampler3D / isampler3D texel, fragRaycast.glsl:197-203, done once). */
#define VRC_XF_NONE 0
#define VRC_XF_FLIP 1
#define VRC_XF_U32F 2
#define VRC_XF_I32F 3
template < int XF, typename T >
VRC_HD T vrc_voxel_xform( T v )
{
    if constexpr( XF == VRC_XF_FLIP )
        return (T)( v ^ (T)( (T)1 << ( 8u * sizeof( T ) - 1u ) ) );
    else if constexpr( XF == VRC_XF_U32F )
        return (T)vrc_float_bits( (float)(uint32_t)v );
    else if constexpr( XF == VRC_XF_I32F )
        return (T)vrc_float_bits( (float)(int32_t)v );
    else
        return v;
}

/* travel > 0.  Whether the count is exact, and the count: the trips of `for( ; travel > 0; travel -= stepSize )` */
VRC_HD bool vrc_exact_step_count( float travel, float stepSize, uint32_t* n )
{
    const uint32_t sb = vrc_float_bits( stepSize );
    const uint32_t e = sb >> 23; /* (a negative step has bit 8 set here and fails the range test) */
    /* exponent 254 is left out: its reciprocal is not a normal number */
    const bool pow2 = ( sb & 0x7FFFFFu ) == 0u && e >= 1u && e <= 253u;
    const float inv = vrc_bits_float( ( 254u - ( pow2 ? e : 127u ) ) << 23 );
    const float q = travel * inv;
    const bool ok = pow2 && q < 16777216.0f;
    const float qs = ok ? q : 0.0f;
    uint32_t c = (uint32_t)qs; /* truncation; qs is an integer already from 2^23 on */
    c += (float)c < qs ? 1u : 0u;
    *n = c == 0u ? 1u : c;
    return ok;
}

#if defined( VRC_UNIFORM_FORM_HOOK ) && !defined( __HIPCC__ )
/* host test builds only (tests/cpu_harness/intsteps_harness.cpp): 1 = never take the counted form; and how many
 * segments took the [0] float chain, [1] counted form */
extern int vrc_uniform_form_hook;
extern uint64_t vrc_uniform_form_taken[2];
#endif

/* Groups of the counted form.  Nothing is fetched, so the group is not sized by gather latency or by the registers
 * of GROUP indices (the gather path's 14 and its tails of 4, vrc_march_segment_as): a group costs its samples plus
 * the copy of `saved`, one exit test and the count's subtract and compare.  What is left below a whole group is marched
 * sample by sample with the reference's exit test after each -- a lane runs exactly its own samples, no predicated
 * slots -- and that same loop is the replay of a group the threshold was crossed in.  Two loops and no per-size
 * bodies on purpose: this code is inlined into every table-form kernel, next to a gather march that fills the
 * register budget of its occupancy (a first version with unrolled bodies of 8, 4, 2 and 1 samples after the groups
 * of 16 made the four-float gather kernels spill).
 * Measured on C2 (profiles/r7_int_steps.txt; the float chain: 0.1119 ms): groups of 8 / 16 / 32: 0.0988 / 0.0942 /
 * 0.0996 ms; groups of 16, then of 4, then single samples: 0.0964 ms. */
#ifndef VRC_UNIFORM_GROUP
#define VRC_UNIFORM_GROUP 16
#endif

/* Whole groups of G while nLeft >= G: all G samples are the reference's, the early-exit test comes once at the end
 * (alpha never decreases).  Crossed inside a group: the colour goes back to the group's start and nLeft becomes G --
 * the caller's sample-by-sample loop replays it and stops after the crossing sample, as the reference does. */
template < bool COUNT, int G, typename E >
VRC_HD bool vrc_uniform_groups( E& color, const E ue, uint32_t& nLeft, uint32_t& nSamples )
{
    while( nLeft >= (uint32_t)G )
    {
        const E saved = color;
#pragma unroll
        for( int k = 0; k < G; ++k )
            vrc_composite( color, ue );
        if( color.w > VRC_EARLY_EXIT )
        {
            color = saved;
            nLeft = (uint32_t)G;
            return true;
        }
        nLeft -= (uint32_t)G;
        if( COUNT )
            nSamples += (uint32_t)G;
    }
    return false;
}

template < bool COUNT, typename E >
VRC_HD bool vrc_march_uniform_counted( E& color, const E ue, uint32_t nLeft, uint32_t& nSamples )
{
    /* (crossed or not, the loop below runs what is left: the remainder, or the group to replay) */
    (void)vrc_uniform_groups< COUNT, VRC_UNIFORM_GROUP, E >( color, ue, nLeft, nSamples );
    for( ; nLeft > 0u; --nLeft )
    {
        vrc_composite( color, ue );
        if( COUNT )
            nSamples += 1u;
        if( color.w > VRC_EARLY_EXIT )
            return true;
    }
    return false;
}

/* The uniform march of the lean replay (vrc_pixel_walk_replay_lean): n samples of one entry, n < 4096 known from the
 * list.  Whole groups as above, of VRC_LEAN_GROUP samples: with the remainder in bodies a larger group no longer pays
 * in single samples, and on C2 groups of 32 beat 16 by 4 % and 64 by 3 % of the kernel, an opaque table and a rotated
 * view included.  What is left below a group is a saved colour, bodies of 16, 8, 4, 2 and 1 samples by the bits of the
 * number left, and one test; where that test fires -- the threshold was crossed somewhere in the remainder -- the
 * colour goes back and the single-sample loop replays it and stops after the crossing sample: the reference's exit, as
 * for a whole group.  The same composites in the same order and the same count as vrc_march_uniform_counted.  The
 * bodies are confined to the lean instances, which is why they can be here and not there (see above).  Two other forms
 * of the remainder -- that single-sample loop alone, and the samples left in one loop without a test -- were measured
 * and lost: profiles/r11_lean_visit.txt */
#ifndef VRC_LEAN_GROUP
#define VRC_LEAN_GROUP 32 /* samples per whole group of the lean march: a power of two */
#endif
/* The free body of the lean march (VRC_OPT_LEAN_FREE_MARCH, vrc_frame::leanFree): a visit that cannot reach the
 * threshold needs neither the exit test nor what serves it -- the saved colour, the count's reset -- and a trip of its
 * group loop is the composites and one subtract whose borrow is the loop's condition.
 * The bound.  A composite adds e.w * t to alpha, t = 1 - w_k rounded.  With 0 <= w_k <= 1 and 0 <= e.w that is at
 * least 0 and at most e.w, so alpha never falls and, in real arithmetic, w_n <= w_0 + n * e.w.  Every composite rounds
 * twice at values of at most 1, the test below twice more: under n * 2^-24, below 2.5e-4 for n < 4096 (the list
 * word's 12 bits).  So a visit with 0 <= w_0, 0 <= e.w and w_0 + n * e.w <= 0.99 stays below 0.99 + 2.5e-4, and
 * 0.99 leaves VRC_EARLY_EXIT (0.999) a margin of 0.009, 36 times that rounding: every w_k of it is in [0, 0.9903],
 * the tested march never sees its test fire and never goes back, and n plain composites are its sequence bit for
 * bit.  (e.w <= 1 need not be asked: with n >= 1 the sum says so, with n = 0 nothing is composited.)  The comparisons
 * are written so that a NaN on either side fails them; a negative entry or start fails the first two.
 * Whole groups of VRC_LEAN_FREE_GROUP on a count of groups, then bodies by the bits of n down to four, then the last
 * zero to three samples one by one.  Groups of 8: the tested march takes 32 because its trip costs eight instructions
 * beside the composites, and pays for that with lanes that march up to 31 samples in bodies while their neighbours run
 * a group; at one instruction a trip the small group wins (tools/replay_cost_model.py).  Measured on C2
 * (profiles/r19_lean_free_march.txt; the tested march: 0.0360 ms): groups of 4 / 8 / 16 / 32 with this remainder
 * 0.0348 / 0.0331 / 0.0332 / 0.0342 ms.  The remainder decides as much as the group: with bodies of 2 and 1 the
 * compiler forms selects that always compute three samples, and groups of 8 / 16 / 32 over them take 0.0369 / 0.0374 /
 * 0.0351 ms -- two of them slower than the tested march; a body of 2 and a branch for the last sample, 0.0360 */
#ifndef VRC_LEAN_FREE_GROUP
#define VRC_LEAN_FREE_GROUP 8 /* samples per whole group of the free body: a power of two */
#endif
#if defined( VRC_LEAN_FREE_HOOK ) && !defined( __HIPCC__ )
/* host test builds only (tests/cpu_harness/lean_free_harness.cpp): how many marches took [0] the tested, [1] the free body */
extern uint64_t vrc_lean_free_taken[2];
#endif
template < typename E >
VRC_HD bool vrc_lean_free_visit( const E& color, const E& ue, uint32_t n )
{
    return 0.0f <= color.w && 0.0f <= ue.w && color.w + (float)n * ue.w <= 0.99f;
}
template < typename E >
VRC_HD void vrc_march_uniform_free( E& color, const E ue, const uint32_t n )
{
    static_assert( VRC_LEAN_FREE_GROUP >= 4 && ( VRC_LEAN_FREE_GROUP & ( VRC_LEAN_FREE_GROUP - 1 ) ) == 0,
                   "the bodies below are the bits of a count below the group, the loop behind them its last two" );
    uint32_t groups = n / (uint32_t)VRC_LEAN_FREE_GROUP;
    /* (the decrement and the loop's condition in one: the subtract's borrow) */
    while( !__builtin_sub_overflow( groups, 1u, &groups ) )
    {
#pragma unroll
        for( int k = 0; k < VRC_LEAN_FREE_GROUP; ++k )
            vrc_composite( color, ue );
    }
#pragma unroll
    for( int body = VRC_LEAN_FREE_GROUP / 2; body > 2; body >>= 1 )
        if( n & (uint32_t)body )
        {
#pragma unroll
            for( int k = 0; k < body; ++k )
                vrc_composite( color, ue );
        }
    /* what is left below four, sample by sample on the same kind of trip (kept a loop: unrolled it becomes selects) */
    uint32_t left = n & 3u;
#pragma unroll 1
    while( !__builtin_sub_overflow( left, 1u, &left ) )
        vrc_composite( color, ue );
}

/* freeMarch: the frame's word (vrc_frame::leanFree != 0, the same in every lane); read by the uncounted instances */
template < bool COUNT, typename E >
VRC_HD bool vrc_march_uniform_lean( E& color, const E ue, uint32_t nLeft, uint32_t& nSamples, const bool freeMarch = false )
{
    static_assert( VRC_LEAN_GROUP >= 2 && ( VRC_LEAN_GROUP & ( VRC_LEAN_GROUP - 1 ) ) == 0,
                   "the bodies below are the bits of a count below the group" );
    if constexpr( !COUNT )
    {
        if( freeMarch && vrc_lean_free_visit( color, ue, nLeft ) )
        {
#if defined( VRC_LEAN_FREE_HOOK ) && !defined( __HIPCC__ )
            ++vrc_lean_free_taken[1];
#endif
            vrc_march_uniform_free< E >( color, ue, nLeft );
            return false;
        }
#if defined( VRC_LEAN_FREE_HOOK ) && !defined( __HIPCC__ )
        ++vrc_lean_free_taken[0];
#endif
    }
    const bool crossed = vrc_uniform_groups< COUNT, VRC_LEAN_GROUP, E >( color, ue, nLeft, nSamples );
    if( !crossed )
    {
        const E saved = color;
#pragma unroll
        for( int body = VRC_LEAN_GROUP / 2; body > 0; body >>= 1 )
            if( nLeft & (uint32_t)body )
            {
#pragma unroll
                for( int k = 0; k < body; ++k )
                    vrc_composite( color, ue );
            }
        if( !( color.w > VRC_EARLY_EXIT ) )
        {
            if( COUNT )
                nSamples += nLeft;
            return false;
        }
        color = saved;
    }
    for( ; nLeft > 0u; --nLeft )
    {
        vrc_composite( color, ue );
        if( COUNT )
            nSamples += 1u;
        if( color.w > VRC_EARLY_EXIT )
            return true;
    }
    return false;
}

/* The first-visit table of the lean replay (VRC_OPT_FIRST_VISIT_TABLE, vrc_frame::firstVisit).  A ray's first visit
 * starts from the cleared colour, so where it is a uniform brick its result depends on the brick's classified entry e
 * and the step count n of the list word alone, not on the ray: T[e][j], e in 0 .. 255, j in 0 .. ROWS - 1, is the
 * colour after min( j, cross_e ) composites of entry e from `start`, cross_e the first sample after which
 * w > VRC_EARLY_EXIT.  A row is the single-sample loop -- vrc_composite, then the exit test -- frozen after the
 * crossing: the sequence vrc_march_uniform_lean reproduces by construction (its groups and bodies go back to a saved
 * colour and replay sample by sample where the threshold was crossed), so T[e][n] is that march's colour from `start`
 * bit for bit, and its return value is T[e][n].w > VRC_EARLY_EXIT (alpha never decreases, and the row is frozen).
 * The colour is in the march's own form E (vrc_lean_colour).  Layout [e][j]: the lanes of a wave share e and differ a
 * little in j.  ROWS = 256: C2's first visits take at most 151 steps, a view rotated by 30 and 20 degrees stays below
 * 128 sqrt(3) = 222; 512 KiB in the grey form, 1 MiB in the four-float form.  `start` is an argument, not a literal: a
 * compiler that knows it is zero may fold the first composite, and fma( -0, 1, +0 ) is +0 where the product alone is -0 */
#ifndef VRC_FIRST_VISIT_ROWS
#define VRC_FIRST_VISIT_ROWS 256u
#endif
#define VRC_FIRST_VISIT_ENTRIES 256u
template < typename E >
VRC_HD void vrc_first_visit_row( E* row, const E ue, E color )
{
    bool frozen = false;
    for( uint32_t j = 0u; j < VRC_FIRST_VISIT_ROWS; ++j )
    {
        row[j] = color;
        if( !frozen )
        {
            vrc_composite( color, ue );
            frozen = color.w > VRC_EARLY_EXIT;
        }
    }
}

/* The second plane of a lean list's visit (vrc_frame::walkLean): n << 20 | slotInfoIndex, n = the samples of the
 * uniform march over `dist` -- what vrc_exact_step_count returns, 0 where the march takes none -- and the node's own
 * slotInfoIndex (0: none, else ordinal + 1).  false: the visit cannot be packed -- the count is not exact, or does not
 * fit 12 bits, or the index does not fit 20 -- and the view keeps the other form */
#define VRC_WALK_LEAN_INDEX_BITS 20u
#define VRC_WALK_LEAN_MAX_STEPS 4096u /* n below this */
VRC_HD bool vrc_walk_lean_word( float dist, float stepSize, uint32_t slotInfoIndex, uint32_t* word )
{
    uint32_t n = 0u;
    bool ok = true;
    if( dist > 0.0f )
        ok = vrc_exact_step_count( dist, stepSize, &n );
    ok = ok && n < VRC_WALK_LEAN_MAX_STEPS && slotInfoIndex < ( 1u << VRC_WALK_LEAN_INDEX_BITS );
    *word = ( n << VRC_WALK_LEAN_INDEX_BITS ) | ( slotInfoIndex & ( ( 1u << VRC_WALK_LEAN_INDEX_BITS ) - 1u ) );
    return ok;
}

/* UNIFORM: every voxel a sample of this brick can reach holds one value (the slot's uniformity word,
 * vrc_march_brick) and `ue` is its table entry.  The control structure is the general form's, statement for
 * statement -- groups under the same guard, the sequential travel chain, the early-exit test with its replay, the
 * tail with its per-sample test, the counter -- so the composited sequence and the count are the general form's by
 * construction; only the position stepping, the addresses, the gathers and the table reads are compiled out. */
template < bool CLAMP, bool COUNT, bool FIXED, typename ATLAS_T, int GROUP, typename E, bool PERSAMPLE = false,
           bool UNIFORM = false >
VRC_HD bool vrc_march_segment_as( const vrc_frame& f, const vrc_dev_node& n, vrc_segment s,
                                  const ATLAS_T* __restrict__ atlas, const E* lut,
                                  E& color, uint32_t& nSamples, float levelStep,
                                  const vrc_classifier* cls = nullptr, const E ue = E{} )
{
    static_assert( !( UNIFORM && PERSAMPLE ), "the uniform march takes its entry from the classified table" );
    typedef typename vrc_density< ATLAS_T >::type D;
    static_assert( PERSAMPLE || sizeof( D ) == sizeof( uint32_t ), "a table is indexed by an integer voxel" );
    /* levelStep: step of a coarser brick under per-ray LOD (vrc_pixel_ray_lod); 0 = the frame's */
    const float stepSize = levelStep > 0.0f ? levelStep : f.stepSize;
    const vrc_sampler sm = vrc_make_sampler( n, f ); /* (unused, and compiled out, when UNIFORM) */
    float travel = s.dist;
    vrc_f3 pos = s.pos;
    bool done = false;
    if( !( travel > 0.0f ) )
        return false;
    if constexpr( UNIFORM )
    {
        /* counted in integers where that is the float chain's count exactly (vrc_exact_step_count); taken, like the
         * uniform form itself, by the whole wave or not at all, so that a wave runs one loop and not two */
        uint32_t nLeft;
        bool counted = vrc_exact_step_count( travel, stepSize, &nLeft );
#if defined( __HIP_DEVICE_COMPILE__ )
        counted = __builtin_amdgcn_ballot_w64( !counted ) == 0ull;
#elif defined( VRC_UNIFORM_FORM_HOOK )
        counted = counted && vrc_uniform_form_hook != 1;
        ++vrc_uniform_form_taken[counted ? 1 : 0];
#endif
        if( counted )
            return vrc_march_uniform_counted< COUNT, E >( color, ue, nLeft, nSamples );
    }
    vrc_fixpos fp = { 0, 0, 0, 0, 0, 0 };
    if( FIXED && !UNIFORM )
        fp = vrc_fixpos_init( sm, pos, s.step );

    /* all GROUP samples of a group are reached by the reference loop if more than
     * GROUP steps remain (the sequentially rounded travel differs from the exact one by
     * far less than one step) */
    const float guard = stepSize * (float)( GROUP + 1 );
    while( travel > guard )
    {
        uint32_t idx[GROUP];
        if constexpr( UNIFORM )
            (void)idx;
        else if( FIXED )
            vrc_group_indices_fixed< GROUP >( sm, fp, idx );
        else
            vrc_group_indices< CLAMP, GROUP >( sm, pos, s.step, idx );
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            travel -= stepSize; /* same sequential subtraction as the reference */
        E e[GROUP];
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
        {
            if constexpr( UNIFORM )
                e[k] = ue;
            else
#if defined( VRC_ABLATE_NO_FETCH ) /* timing experiment only */
                e[k] = lut[64u + ( idx[k] >> 31 )];
#else
                e[k] = vrc_entry< PERSAMPLE, E >( lut, (D)atlas[idx[k]], cls );
#endif
        }
        const E saved = color;
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            vrc_composite( color, e[k] );
        if( COUNT )
            nSamples += GROUP;
        if( color.w > VRC_EARLY_EXIT )
        {
            /* crossed inside this group: replay it with the reference's per-sample exit */
            color = saved;
            if( COUNT )
                nSamples -= GROUP;
#pragma unroll
            for( int k = 0; k < GROUP; ++k )
            {
                vrc_composite( color, e[k], done );
                if( COUNT )
                    nSamples += done ? 0u : 1u;
                done = done || ( color.w > VRC_EARLY_EXIT );
            }
            return true;
        }
    }

    /* tail: general form, in smaller groups (fewer slots wasted on steps no lane takes) */
    /* measured on C2 (groups of 8): tail groups of 8 / 4 / 2 / 1: 0.500 / 0.491 / 0.484 / 0.502 ms relative:
     * fewer gather slots spent on steps no lane takes, until the dependent round trips of a short group
     * cost more than the slots did */
    /* (whole groups of GROUP / 2 between the full groups and this tail were tried for GROUP = 14: the second unrolled
     * body costs the registers of a fifth wave -- spills, 0.488 -> 0.539 ms) */
    /* groups of 14: tails of 2 / 3 / 4 / 5 / 7: 0.492 / 0.489 / 0.479 / 0.485 / 0.485 ms (C2), 0.622 / 0.615 / 0.587 / 0.580 /
     * 0.582 ms (noise, 30/20 degrees) */
    constexpr int TAILG = GROUP >= 8 ? ( GROUP + 2 ) / 4 : ( GROUP >= 2 ? GROUP / 2 : 1 );
    while( travel > 0.0f && !done )
    {
        uint32_t idx[TAILG], cnt = 0;
        D d[TAILG];
        if constexpr( UNIFORM )
        {
#pragma unroll
            for( int k = 0; k < TAILG; ++k )
                idx[k] = 0u;
        }
        else if( FIXED )
            vrc_group_indices_fixed< TAILG >( sm, fp, idx );
        else
            vrc_group_indices< CLAMP, TAILG >( sm, pos, s.step, idx );
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            const bool v = travel > 0.0f;
            cnt += v ? 1u : 0u;
            idx[k] = v ? idx[k] : 0u;
            travel -= stepSize;
        }
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
            d[k] = UNIFORM ? (D)0 : (D)atlas[idx[k]];
        E e[TAILG];
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            if constexpr( UNIFORM )
            {
                /* a step the reference does not take blends table entry 256: all zeros */
                const E z = {};
                e[k] = (uint32_t)k < cnt ? ue : z;
            }
            else if constexpr( PERSAMPLE )
            {
                /* a step the reference does not take blends nothing */
                const E z = {};
                e[k] = (uint32_t)k < cnt ? vrc_entry< true, E >( lut, d[k], cls ) : z;
            }
            else
                e[k] = lut[(uint32_t)k < cnt ? d[k] : 256u];
        }
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            const bool active = ( (uint32_t)k < cnt ) && !done;
            vrc_composite( color, e[k], done );
            if( COUNT )
                nSamples += active ? 1u : 0u;
            done = done || ( color.w > VRC_EARLY_EXIT );
        }
    }
    return done;
}

template < bool CLAMP, bool COUNT, bool FIXED, typename ATLAS_T, int GROUP = VRC_GROUP, bool GREY = false >
VRC_HD bool vrc_march_segment( const vrc_frame& f, const vrc_dev_node& n, vrc_segment s,
                               const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                               vrc_f4& color, uint32_t& nSamples, float levelStep = 0.0f )
{
    if constexpr( GREY )
    {
        /* lut holds two-float entries (the kernel fills it that way); the colour came in grey (a cleared pixel)
         * and leaves grey */
        vrc_f2 c = { color.x, color.w };
        const bool done = vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, GROUP, vrc_f2 >(
            f, n, s, atlas, reinterpret_cast< const vrc_f2* >( lut ), c, nSamples, levelStep );
        color.x = color.y = color.z = c.x;
        color.w = c.w;
        return done;
    }
    else
        return vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, GROUP, vrc_f4 >( f, n, s, atlas, lut, color,
                                                                                  nSamples, levelStep );
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION: trilinear volume filter (VRC_OPT_FILTER = 1).  Not in the reference, whose 3-D
 * sampler is point-sampled (cuda/TexturePool.cu:167); named by the build's north star.  The
 * integrator is the reference's, statement for statement, with the fetch replaced by a
 * trilinear one (texel centres at i + 0.5, exact float weights, clamp addressing) -- the
 * oracle's fetch_trilinear.  The density is then continuous, so the transfer function is
 * evaluated per sample (post-classification, Renderer.cu:215-218) instead of through the
 * 257-entry classified table:
 *   tf = tex1D(tfTex, d*mult+add), alpha' = 1 - pow(1 - min(tf.a, 255/256), alphaCorrection).
 * tfp is the transfer function padded by one entry on both sides (tfp[j] = tf[clamp(j-1)],
 * 258 entries) so the two lerp operands need no index clamps.
 * ---------------------------------------------------------------------------------------- */
#define VRC_TFP_ENTRIES 258u

struct vrc_classifier
{
    float mult, add;       /* u*256 - 0.5 = d*mult + add */
    float alphaCorrection;
    float q, invq;         /* TF lerp weight quantisation (2^fracBits), q = 0: exact */
};

VRC_HD vrc_classifier vrc_make_classifier( vrc_lut_params p )
{
    vrc_classifier k;
    const float multiplyer = 1.0f / ( p.rangeMax - p.rangeMin );
    const float addedValue = -p.rangeMin / ( p.rangeMax - p.rangeMin );
    k.mult = multiplyer * 256.0f;
    k.add = addedValue * 256.0f - 0.5f;
    k.alphaCorrection = p.alphaCorrection;
    k.q = p.fracBits > 0 ? (float)( 1 << p.fracBits ) : 0.0f;
    k.invq = p.fracBits > 0 ? 1.0f / (float)( 1 << p.fracBits ) : 0.0f;
    return k;
}

/* (VRC_HOST_FUSED_LERP: a host build that is to give the device's bits -- tests/slice_ref.py: harness( fused ) -- takes
 * the device's form; with a compiler that honours VRC_FAST_FP and a target that has the instruction) */
#if defined( __HIP_DEVICE_COMPILE__ ) || defined( VRC_HOST_FUSED_LERP )
#define VRC_LERP2( B, X, A, Y ) __builtin_fmaf( ( A ), ( Y ), ( B ) * ( X ) )
#else
#define VRC_LERP2( B, X, A, Y ) ( ( B ) * ( X ) + ( A ) * ( Y ) )
#endif
VRC_HD vrc_f4 vrc_classify( const vrc_f4* tfp, float d, const vrc_classifier& k )
{
    VRC_FAST_FP
    float xB = d * k.mult + k.add;
    xB = fminf( fmaxf( xB, -1.0f ), 255.99998f );
    const float fl = floorf( xB );
    float a = xB - fl;
    if( k.q > 0.0f )
        a = floorf( a * k.q + 0.5f ) * k.invq;
    const int j = (int)fl + 1;
    const vrc_f4 t0 = tfp[j], t1 = tfp[j + 1];
    const float b = 1.0f - a;
    /* on the device the interpolation is spelled as one product and one fused multiply-add: which of the two
     * products hipcc fuses otherwise depends on the code around it, and the grey form (below) has to produce the
     * same bits as this one */
    const float cw = VRC_LERP2( b, t0.w, a, t1.w );
    const float corr = 1.0f - fminf( cw, 1.0f - 1.0f / 256.0f );
#if defined( __HIP_DEVICE_COMPILE__ )
    const float alpha = 1.0f - __builtin_amdgcn_exp2f( k.alphaCorrection * __builtin_amdgcn_logf( corr ) );
#else
    const float alpha = 1.0f - powf( corr, k.alphaCorrection );
#endif
    vrc_f4 e;
    e.x = VRC_LERP2( b, t0.x, a, t1.x ) * alpha;
    e.y = VRC_LERP2( b, t0.y, a, t1.y ) * alpha;
    e.z = VRC_LERP2( b, t0.z, a, t1.z ) * alpha;
    e.w = alpha;
    return e;
}

/* the same for a grey transfer function kept as (grey, alpha) pairs: the colour channels of vrc_classify are one
 * expression evaluated three times on equal numbers */
VRC_HD vrc_f2 vrc_classify( const vrc_f2* tfp, float d, const vrc_classifier& k )
{
    VRC_FAST_FP
    float xB = d * k.mult + k.add;
    xB = fminf( fmaxf( xB, -1.0f ), 255.99998f );
    const float fl = floorf( xB );
    float a = xB - fl;
    if( k.q > 0.0f )
        a = floorf( a * k.q + 0.5f ) * k.invq;
    const int j = (int)fl + 1;
    const vrc_f2 t0 = tfp[j], t1 = tfp[j + 1];
    const float b = 1.0f - a;
    const float cw = VRC_LERP2( b, t0.w, a, t1.w );
    const float corr = 1.0f - fminf( cw, 1.0f - 1.0f / 256.0f );
#if defined( __HIP_DEVICE_COMPILE__ )
    const float alpha = 1.0f - __builtin_amdgcn_exp2f( k.alphaCorrection * __builtin_amdgcn_logf( corr ) );
#else
    const float alpha = 1.0f - powf( corr, k.alphaCorrection );
#endif
    vrc_f2 e;
    e.x = VRC_LERP2( b, t0.x, a, t1.x ) * alpha;
    e.w = alpha;
    return e;
}

/* the eight taps of one sample: per-axis address parts (micro-blocked slot layout, see
 * vrc_voxel_address) of floor(c) and floor(c)+1, and the weights */
struct vrc_taps
{
    uint32_t ax[2], ay[2], az[2];
    float wx, wy, wz;
};

template < bool CLAMP >
VRC_HD vrc_taps vrc_trilinear_taps( const vrc_sampler& s, float lx, float ly, float lz )
{
    vrc_taps t;
    /* texel centres at i + 0.5 */
    float cx = lx - 0.5f, cy = ly - 0.5f, cz = lz - 0.5f;
    const float fx = floorf( cx ), fy = floorf( cy ), fz = floorf( cz );
    t.wx = cx - fx;
    t.wy = cy - fy;
    t.wz = cz - fz;
    int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
    if( CLAMP )
    {
        const int hx = (int)s.hix, hy = (int)s.hiy, hz = (int)s.hiz;
        x0 = x0 < 0 ? 0 : ( x0 > hx ? hx : x0 );
        x1 = x1 < 0 ? 0 : ( x1 > hx ? hx : x1 );
        y0 = y0 < 0 ? 0 : ( y0 > hy ? hy : y0 );
        y1 = y1 < 0 ? 0 : ( y1 > hy ? hy : y1 );
        z0 = z0 < 0 ? 0 : ( z0 > hz ? hz : z0 );
        z1 = z1 < 0 ? 0 : ( z1 > hz ? hz : z1 );
    }
    const uint32_t ux[2] = { (uint32_t)x0, (uint32_t)x1 }, uy[2] = { (uint32_t)y0, (uint32_t)y1 },
                   uz[2] = { (uint32_t)z0, (uint32_t)z1 };
#pragma unroll
    for( int i = 0; i < 2; ++i )
    {
        t.ax[i] = vrc_mul24( ux[i] >> VRC_MB_SHIFT, 504u ) + ux[i];
        t.ay[i] = vrc_mul24( uy[i] >> VRC_MB_SHIFT, s.cyy ) + ( uy[i] << 3 ) + VRC_MB_FIX_Y( uy[i] );
        t.az[i] = vrc_mul24( uz[i] >> VRC_MB_SHIFT, s.czz ) + ( uz[i] << 6 ) - VRC_MB_FIX_Z( uz[i] ) + s.slotBase;
    }
    return t;
}

VRC_HD float vrc_trilerp( const float v[8], float wx, float wy, float wz )
{
    VRC_FAST_FP
    /* the oracle's order: x, then y, then z; a*(1-w) + b*w */
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
    const float c00 = v[0] * ux + v[1] * wx;
    const float c10 = v[2] * ux + v[3] * wx;
    const float c01 = v[4] * ux + v[5] * wx;
    const float c11 = v[6] * ux + v[7] * wx;
    const float c0 = c00 * uy + c10 * wy;
    const float c1 = c01 * uy + c11 * wy;
    return c0 * uz + c1 * wz;
}

/* one voxel by its element index.  On the device the index goes through an empty asm and the pointer is typed as
 * global memory: the load then takes the scalar base + 32-bit lane offset form where the base is wave-uniform and
 * the voxels are bytes; written as atlas[valid ? e : 0u] the compiler widened a select of 64-bit values and spent a
 * 64-bit vector addition per gather (eight per trilinear sample). */
template < typename ATLAS_T >
VRC_HD ATLAS_T vrc_gather( const ATLAS_T* __restrict__ atlas, uint32_t e )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    typedef __attribute__( ( address_space( 1 ) ) ) const ATLAS_T g_t;
    asm( "" : "+v"( e ) );
    return ( (g_t*)atlas )[e];
#else
    return atlas[e];
#endif
}

/* gather form of the trilinear march: eight byte gathers per sample, groups of
 * VRC_LGROUP samples, general branch-free form throughout (a sample the reference loop would
 * not reach reads element 0 and is blended with weight 0).  Sample positions follow the
 * reference's float accumulation.  The LDS-staged kernel (vrc_kernels.hip) is the fast
 * path for overlap >= 1; this form also serves the clamped sampler. */
#ifndef VRC_LGROUP
#define VRC_LGROUP 4
#endif

template < bool CLAMP, bool COUNT, bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_march_segment_linear( const vrc_frame& f, const vrc_dev_node& n, vrc_segment s,
                                      const ATLAS_T* __restrict__ atlas, const vrc_f4* tfp,
                                      const vrc_classifier& cls, vrc_f4& color,
                                      uint32_t& nSamples, float levelStep = 0.0f )
{
    const float stepSize = levelStep > 0.0f ? levelStep : f.stepSize;
    const vrc_sampler sm = vrc_make_sampler( n, f );
    float travel = s.dist;
    vrc_f3 pos = s.pos;
    bool done = false;
    while( travel > 0.0f && !done )
    {
        bool valid[VRC_LGROUP];
        float d[VRC_LGROUP];
        if( TRILINEAR )
        {
            vrc_taps t[VRC_LGROUP];
#pragma unroll
            for( int k = 0; k < VRC_LGROUP; ++k )
            {
                VRC_FAST_FP
                valid[k] = travel > 0.0f;
                const float lx = ( pos.x - sm.minx ) * sm.kx + sm.ox;
                const float ly = ( pos.y - sm.miny ) * sm.ky + sm.oy;
                const float lz = ( pos.z - sm.minz ) * sm.kz + sm.oz;
                t[k] = vrc_trilinear_taps< CLAMP >( sm, lx, ly, lz );
                pos.x += s.step.x;
                pos.y += s.step.y;
                pos.z += s.step.z;
                travel -= stepSize;
            }
            float v[VRC_LGROUP][8];
#pragma unroll
            for( int k = 0; k < VRC_LGROUP; ++k )
#pragma unroll
                for( int c = 0; c < 8; ++c )
                {
                    const uint32_t e = t[k].ax[c & 1] + t[k].ay[( c >> 1 ) & 1] + t[k].az[c >> 2];
                    v[k][c] = (float)vrc_gather( atlas, valid[k] ? e : 0u );
                }
#pragma unroll
            for( int k = 0; k < VRC_LGROUP; ++k )
                d[k] = vrc_trilerp( v[k], t[k].wx, t[k].wy, t[k].wz );
        }
        else
        {
            /* point sampling of a volume the classified table cannot index (16-bit voxels) */
            uint32_t idx[VRC_LGROUP];
#pragma unroll
            for( int k = 0; k < VRC_LGROUP; ++k )
            {
                valid[k] = travel > 0.0f;
                travel -= stepSize;
            }
            vrc_group_indices< CLAMP, VRC_LGROUP >( sm, pos, s.step, idx );
#pragma unroll
            for( int k = 0; k < VRC_LGROUP; ++k )
                d[k] = (float)vrc_gather( atlas, valid[k] ? idx[k] : 0u );
        }
#pragma unroll
        for( int k = 0; k < VRC_LGROUP; ++k )
        {
            const vrc_f4 e = vrc_classify( tfp, d[k], cls );
            const bool active = valid[k] && !done;
            vrc_composite( color, e, !active );
            if( COUNT )
                nSamples += active ? 1u : 0u;
            done = done || ( active && color.w > VRC_EARLY_EXIT );
        }
    }
    return done;
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION, tap-packed form of the trilinear filter (round 4).  The filter the north star names is one sampler
 * enum in the reference (cuda/TexturePool.cu:163-170, cudaFilterModePoint -> Linear) and free in its hardware; here
 * the eight taps were eight byte gathers (above) or a staged box in LDS (vrc_kernels_lds.hip), both bound by the
 * instructions and cache look-ups around the sample while HBM idles.  This form spends memory instead: next to the
 * byte atlas the pool keeps a second atlas of 16-bit texels, each a voxel and its neighbour along z,
 *     t(x,y,z) = v[x,y,z] | v[x,y,z+1] << 8      (16-bit voxels: 32-bit texels, << 16, the gathers 8 bytes each),
 * in which t(x,y,z) and t(x+1,y,z) are ALWAYS neighbours in memory: the texels lie in blocks of 8x8x8 whose x-rows
 * carry a ninth texel, a copy of the next block's first (9/8 x 2 = 2.25 times the bytes of the byte atlas; written by
 * vrc_k_pack_slots when a brick is uploaded; the slot's overlap >= 1 supplies the +1 neighbours).  The eight taps of
 * a sample are then TWO 4-byte gathers -- global_load_dword at 2-byte-aligned addresses that never leave an 18-byte
 * row: t(x0, y0, z0) | t(x0+1, y0, z0) << 16 and the same at y0 + 1 -- eight byte -> float conversions straight out
 * of the two registers and the seven interpolations: no box, no staging, no walk batching, the same work for every
 * view direction.  The 64 rows of a block lie in Morton order of (y, z), so a 128-byte line holds 9 x 2 x 2 ... 9 x 4
 * x 2 texels and what a tile touches per step is about the same along every axis.
 * (Measured and dropped, profiles/r4_packed_kernel_experiments.txt: 32-bit texels of the 2x2 neighbourhood in (x, y)
 * or (y, z) -- one 8-byte gather, twice the line fills --, rows of 8 with the pair across a block fetched by masked
 * second gathers, and four other row orders.)
 *
 * Sample positions, weights, interpolation and classification are the staged kernel's, operation for operation
 * (8.24 fixed-point positions from vrc_fixpos_init minus half a voxel, 24-bit weights used unscaled, x then y then
 * z, the transfer function through CUDA's 1.8 fixed-point weight out of one float -> integer conversion), so the
 * two forms composite the same numbers.
 * ---------------------------------------------------------------------------------------- */
/* slot-local element order of the packed atlas: offset = PX(x) + PY(y) + PZ(z), blocks x-fastest inside the slot */
/* bytes per texel: twice the voxel's -- 2 (8-bit voxels: TB = 2 below) or 4 (16-bit voxels: t = v[z] | v[z+1] << 16,
 * 4.5 bytes per voxel next to the atlas's 2; the pairs of rows y and y + 1 are then two 8-byte gathers) */
#define VRC_PK_TEXEL( voxelBytes ) ( 2u * ( voxelBytes ) )
#define VRC_PK_ROW 9u
#define VRC_PK_BLOCK ( VRC_PK_ROW * 64u ) /* 576 texels */
/* row number of (y & 7, z & 7) inside a block: the bits of y and z interleaved */
VRC_HD uint32_t vrc_pk_ry( uint32_t u ) { return ( u & 1u ) | ( ( ( u >> 1 ) & 1u ) << 2 ) | ( ( ( u >> 2 ) & 1u ) << 4 ); }
VRC_HD uint32_t vrc_pk_rz( uint32_t u ) { return vrc_pk_ry( u ) << 1; }
VRC_HD uint32_t vrc_pk_x( uint32_t u ) { return ( u & 7u ) + VRC_PK_BLOCK * ( u >> 3 ); }
VRC_HD uint32_t vrc_pk_y( uint32_t u, uint32_t sbx ) { return VRC_PK_ROW * vrc_pk_ry( u ) + VRC_PK_BLOCK * sbx * ( u >> 3 ); }
VRC_HD uint32_t vrc_pk_z( uint32_t u, uint32_t sbx, uint32_t sby ) { return VRC_PK_ROW * vrc_pk_rz( u ) + VRC_PK_BLOCK * sbx * sby * ( u >> 3 ); }
VRC_HD uint32_t vrc_packed_local_index( uint32_t x, uint32_t y, uint32_t z, uint32_t sbx, uint32_t sby )
{
    return vrc_pk_x( x ) + vrc_pk_y( y, sbx ) + vrc_pk_z( z, sbx, sby );
}
/* slot-local voxel of packed element `in` of a block (the pack kernel's decode); ix == 8: the copy's column */
VRC_HD void vrc_packed_decode( uint32_t in, uint32_t& ix, uint32_t& iy, uint32_t& iz )
{
    const uint32_t r = in / VRC_PK_ROW;
    ix = in % VRC_PK_ROW;
    iy = ( r & 1u ) | ( ( ( r >> 2 ) & 1u ) << 1 ) | ( ( ( r >> 4 ) & 1u ) << 2 );
    iz = ( ( r >> 1 ) & 1u ) | ( ( ( r >> 3 ) & 1u ) << 1 ) | ( ( ( r >> 5 ) & 1u ) << 2 );
}
/* texels of a packed slot / element offset of the packed slot that belongs to the byte slot at element slotBase
 * (byte slots are whole blocks of 512) */
VRC_HD uint64_t vrc_packed_elems( uint64_t byteElems ) { return byteElems / VRC_MB_VOXELS * VRC_PK_BLOCK; }

/* texel of a voxel and its neighbour along z; T = uint16_t (8-bit voxels) or uint32_t (16-bit voxels) */
template < typename T >
VRC_HD T vrc_pack_taps( uint32_t vz0, uint32_t vz1 ) { return (T)( vz0 | ( vz1 << ( 4u * sizeof( T ) ) ) ); }

/* classifier of a trilinear sample that arrives scaled by 2^72 (three unscaled 24-bit weights): the oracle's
 * orc_tf_fetch + composite (cuda/ColorMap.cu:40-45, cuda/Renderer.cu:83-93) with the transfer-function texel pair
 * and CUDA's 1.8 fixed-point lerp weight taken out of ONE float -> integer conversion: tq = xB * 256 + 256.5 with
 * xB = u * 256 - 0.5 the texel coordinate; texel pair (tq >> 8, + 1) of the padded table, weight (tq & 255) / 256
 * rounded to nearest as the hardware does.  VRC_OPT_TF_FRAC_BITS = 8 only. */
struct vrc_cls8
{
    float mult, add, kexp;
};
VRC_HD vrc_cls8 vrc_make_cls8( const vrc_classifier& c )
{
    vrc_cls8 k;
    k.mult = c.mult * 256.0f * 0x1p-72f;
    k.add = c.add * 256.0f + 256.5f;
    k.kexp = c.alphaCorrection;
    return k;
}
/* entries of the classifier's table: per texel j of the padded transfer function tfp (VRC_TFP_ENTRIES entries)
 * (colour_j, 1 - alpha_j) / 256 -- the weights are used as integers 0..256 -- one texel more than tfp has: a
 * sample at the upper clamp reads the pair (257, 258) with weights (256, 0).  Grey transfer function: texels j and
 * j + 1 side by side, (g_j, 1 - a_j, g_j+1, 1 - a_j+1) / 256, one 16-byte read per sample. */
#define VRC_CLS8_ENTRIES ( VRC_TFP_ENTRIES + 1u )
VRC_HD vrc_f4 vrc_cls8_entry( const vrc_f4* tfp, uint32_t i, bool grey )
{
    const float sc = 1.0f / 256.0f;
    const vrc_f4 e0 = tfp[i < VRC_TFP_ENTRIES - 1u ? i : VRC_TFP_ENTRIES - 1u];
    const vrc_f4 e1 = tfp[i + 1u < VRC_TFP_ENTRIES - 1u ? i + 1u : VRC_TFP_ENTRIES - 1u];
    vrc_f4 t;
    if( grey )
    {
        t.x = e0.x * sc; t.y = ( 1.0f - e0.w ) * sc; t.z = e1.x * sc; t.w = ( 1.0f - e1.w ) * sc;
    }
    else
    {
        t.x = e0.x * sc; t.y = e0.y * sc; t.z = e0.z * sc; t.w = ( 1.0f - e0.w ) * sc;
    }
    return t;
}
VRC_HD float vrc_alpha8( float corr, float kexp )
{
    /* 1 - min(a, 255/256) = max(1 - a, 1/256) (Renderer.cu:88); pow as exp2(k log2 x) on the device */
    corr = fmaxf( corr, 1.0f / 256.0f );
#if defined( __HIP_DEVICE_COMPILE__ )
    return 1.0f - __builtin_amdgcn_exp2f( kexp * __builtin_amdgcn_logf( corr ) );
#else
    return 1.0f - powf( corr, kexp );
#endif
}
VRC_HD uint32_t vrc_cls8_texel( float d, const vrc_cls8& k )
{
    float tq = __builtin_fmaf( d, k.mult, k.add );
#if defined( __HIP_DEVICE_COMPILE__ )
    tq = __builtin_amdgcn_fmed3f( tq, 0.5f, 65792.25f );
#else
    tq = fminf( fmaxf( tq, 0.5f ), 65792.25f );
#endif
    return (uint32_t)tq;
}
VRC_HD vrc_f2 vrc_classify8( const vrc_f2*, const vrc_f4* tab, float d, const vrc_cls8& k )
{
    const uint32_t u = vrc_cls8_texel( d, k );
    const float a = (float)( u & 255u ), b = 256.0f - a;
    const vrc_f4 t = *reinterpret_cast< const vrc_f4* >( reinterpret_cast< const char* >( tab ) + ( ( u >> 4 ) & 0xFFFF0u ) );
    const float alpha = vrc_alpha8( __builtin_fmaf( a, t.w, b * t.y ), k.kexp );
    vrc_f2 e;
    e.x = __builtin_fmaf( a, t.z, b * t.x ) * alpha;
    e.w = alpha;
    return e;
}
VRC_HD vrc_f4 vrc_classify8( const vrc_f4*, const vrc_f4* tab, float d, const vrc_cls8& k )
{
    const uint32_t u = vrc_cls8_texel( d, k );
    const float a = (float)( u & 255u ), b = 256.0f - a;
    const vrc_f4* const p = reinterpret_cast< const vrc_f4* >( reinterpret_cast< const char* >( tab ) + ( ( u >> 4 ) & 0xFFFF0u ) );
    const vrc_f4 t0 = p[0], t1 = p[1];
    const float alpha = vrc_alpha8( __builtin_fmaf( a, t1.w, b * t0.w ), k.kexp );
    vrc_f4 e;
    e.x = __builtin_fmaf( a, t1.x, b * t0.x ) * alpha;
    e.y = __builtin_fmaf( a, t1.y, b * t0.y ) * alpha;
    e.z = __builtin_fmaf( a, t1.z, b * t0.z ) * alpha;
    e.w = alpha;
    return e;
}

/* the taps of a sample as they come out of the two gathers (TB = bytes per texel).  TB = 2: t0 = t(x0,y0,z0) |
 * t(x0+1,y0,z0) << 16, t1 the same at y0 + 1 (a texel's low byte is z0, its high byte z0 + 1).  TB = 4: one texel per
 * word, a = row y0, b = row y0 + 1, 0 / 1 = x0 / x0 + 1 (low half z0, high half z0 + 1). */
template < int TB >
struct vrc_pk_taps;
template <>
struct vrc_pk_taps< 2 >
{
    uint32_t t0, t1;
};
template <>
struct vrc_pk_taps< 4 >
{
    uint32_t a0, a1, b0, b1;
};

/* the interpolated density of a sample, times 2^72; weights = the 24 fraction bits of the sample's 8.24 coordinates,
 * NOT scaled by 2^-24 -- W and 2^24 - W are exact, so every product and sum is 2^24 (2^48, 2^72) times the one with
 * scaled weights, bit for bit; vrc_cls8.mult carries the 2^-72.  The oracle's order: x, then y, then z;
 * a * (1 - w) + b * w. */
VRC_HD float vrc_trilerp_packed( const vrc_pk_taps< 2 >& t, uint32_t fx, uint32_t fy, uint32_t fz )
{
    const uint32_t T0 = t.t0, T1 = t.t1;
    const float wx = (float)( fx & 0xFFFFFFu ), wy = (float)( fy & 0xFFFFFFu ), wz = (float)( fz & 0xFFFFFFu );
    const float ux = 16777216.0f - wx, uy = 16777216.0f - wy, uz = 16777216.0f - wz;
    const float c00 = __builtin_fmaf( (float)( ( T0 >> 16 ) & 255u ), wx, (float)( T0 & 255u ) * ux );  /* y0 z0 */
    const float c01 = __builtin_fmaf( (float)( T0 >> 24 ), wx, (float)( ( T0 >> 8 ) & 255u ) * ux );    /* y0 z1 */
    const float c10 = __builtin_fmaf( (float)( ( T1 >> 16 ) & 255u ), wx, (float)( T1 & 255u ) * ux );  /* y1 z0 */
    const float c11 = __builtin_fmaf( (float)( T1 >> 24 ), wx, (float)( ( T1 >> 8 ) & 255u ) * ux );    /* y1 z1 */
    const float c0 = __builtin_fmaf( c10, wy, c00 * uy );
    const float c1 = __builtin_fmaf( c11, wy, c01 * uy );
    return __builtin_fmaf( c1, wz, c0 * uz );
}
VRC_HD float vrc_trilerp_packed( const vrc_pk_taps< 4 >& t, uint32_t fx, uint32_t fy, uint32_t fz )
{
    const float wx = (float)( fx & 0xFFFFFFu ), wy = (float)( fy & 0xFFFFFFu ), wz = (float)( fz & 0xFFFFFFu );
    const float ux = 16777216.0f - wx, uy = 16777216.0f - wy, uz = 16777216.0f - wz;
    const float c00 = __builtin_fmaf( (float)( t.a1 & 0xFFFFu ), wx, (float)( t.a0 & 0xFFFFu ) * ux ); /* y0 z0 */
    const float c01 = __builtin_fmaf( (float)( t.a1 >> 16 ), wx, (float)( t.a0 >> 16 ) * ux );         /* y0 z1 */
    const float c10 = __builtin_fmaf( (float)( t.b1 & 0xFFFFu ), wx, (float)( t.b0 & 0xFFFFu ) * ux ); /* y1 z0 */
    const float c11 = __builtin_fmaf( (float)( t.b1 >> 16 ), wx, (float)( t.b0 >> 16 ) * ux );         /* y1 z1 */
    const float c0 = __builtin_fmaf( c10, wy, c00 * uy );
    const float c1 = __builtin_fmaf( c11, wy, c01 * uy );
    return __builtin_fmaf( c1, wz, c0 * uz );
}

/* the two gathers of a sample at byte offsets of the lane's packed slot.  TB = 2: 4-byte loads at 2-byte-aligned
 * addresses; TB = 4: 8-byte loads at 4-byte-aligned addresses (multi-dword loads need dword alignment only).  On the
 * device the pointer is typed as global memory, so the compiler emits global_load_dword / _dwordx2. */
VRC_HD vrc_pk_taps< 2 > vrc_packed_load( const vrc_pk_taps< 2 >*, const uint8_t* slot, uint32_t byteOffset, uint32_t byteOffsetY1 )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    typedef uint32_t u32_a2 __attribute__( ( aligned( 2 ) ) );
    typedef __attribute__( ( address_space( 1 ) ) ) const u32_a2 g_t;
    return vrc_pk_taps< 2 >{ *reinterpret_cast< g_t* >( (uintptr_t)( slot + byteOffset ) ),
                          *reinterpret_cast< g_t* >( (uintptr_t)( slot + byteOffsetY1 ) ) };
#else
    vrc_pk_taps< 2 > t;
    memcpy( &t.t0, slot + byteOffset, 4 );
    memcpy( &t.t1, slot + byteOffsetY1, 4 );
    return t;
#endif
}
VRC_HD vrc_pk_taps< 4 > vrc_packed_load( const vrc_pk_taps< 4 >*, const uint8_t* slot, uint32_t byteOffset, uint32_t byteOffsetY1 )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    typedef uint32_t u32x2_a4 __attribute__( ( ext_vector_type( 2 ), aligned( 4 ) ) );
    typedef __attribute__( ( address_space( 1 ) ) ) const u32x2_a4 g_t;
    const u32x2_a4 a = *reinterpret_cast< g_t* >( (uintptr_t)( slot + byteOffset ) );
    const u32x2_a4 b = *reinterpret_cast< g_t* >( (uintptr_t)( slot + byteOffsetY1 ) );
    return vrc_pk_taps< 4 >{ a.x, a.y, b.x, b.y };
#else
    vrc_pk_taps< 4 > t;
    memcpy( &t.a0, slot + byteOffset, 8 );
    memcpy( &t.b0, slot + byteOffsetY1, 8 );
    return t;
#endif
}
/* (timing experiments only) */
VRC_HD vrc_pk_taps< 2 > vrc_pk_taps_fake( const vrc_pk_taps< 2 >*, uint32_t off ) { return vrc_pk_taps< 2 >{ off * 0x01010101u, off * 0x00010101u }; }
VRC_HD vrc_pk_taps< 4 > vrc_pk_taps_fake( const vrc_pk_taps< 4 >*, uint32_t off ) { return vrc_pk_taps< 4 >{ off * 0x01010101u, off * 0x00010101u, off, ~off }; }
VRC_HD uint32_t vrc_pk_taps_mix( const vrc_pk_taps< 2 >& t ) { return t.t0 ^ t.t1; }
VRC_HD uint32_t vrc_pk_taps_mix( const vrc_pk_taps< 4 >& t ) { return t.a0 ^ t.a1 ^ t.b0 ^ t.b1; }

/* byte offsets (slot-local + bias) of the texel pairs of the next N samples; p advances by N steps.  Device: the per-axis
 * parts from the tables in LDS (filled by the kernel with TB * vrc_pk_x / y / z). */
template < int N, int TB >
VRC_HD void vrc_packed_offsets( const vrc_sampler& s, vrc_fixpos& p, uint32_t bias, uint32_t* off, uint32_t* offY1 )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    (void)s;
#pragma unroll
    for( int k = 0; k < N; ++k )
    {
        const char* const t = reinterpret_cast< const char* >( vrc_addr_tab );
        const uint32_t tx = *reinterpret_cast< const uint32_t* >( t + ( ( p.x >> 22 ) & 0x3FCu ) );
        const uint32_t* const py = reinterpret_cast< const uint32_t* >( t + 1024 + ( ( p.y >> 22 ) & 0x3FCu ) );
        const uint32_t tz = *reinterpret_cast< const uint32_t* >( t + 2048 + ( ( p.z >> 22 ) & 0x3FCu ) );
        const uint32_t xz = tx + tz + bias; /* (one v_add3_u32) */
        off[k] = xz + py[0];
        offY1[k] = xz + py[1]; /* (y = 255 reads the z table's first entry: no sample with a weight has it) */
        p.x += p.dx;
        p.y += p.dy;
        p.z += p.dz;
        asm( "" : "+v"( p.x ), "+v"( p.y ), "+v"( p.z ) ); /* keep the additions (vrc_group_indices_fixed) */
    }
#else
    const uint32_t sbx = ( s.cyy + 64u ) / VRC_MB_VOXELS, sby = ( s.czz + 512u ) / ( sbx * VRC_MB_VOXELS );
#pragma unroll
    for( int k = 0; k < N; ++k )
    {
        off[k] = bias + (uint32_t)TB * vrc_packed_local_index( p.x >> 24, p.y >> 24, p.z >> 24, sbx, sby );
        offY1[k] = bias + (uint32_t)TB * vrc_packed_local_index( p.x >> 24, ( ( p.y >> 24 ) + 1u ) & 255u, p.z >> 24, sbx, sby );
        p.x += p.dx;
        p.y += p.dy;
        p.z += p.dz;
    }
#endif
}

#ifndef VRC_PGROUP
#define VRC_PGROUP 12 /* (4 ... 24 measured: the fetches in flight per wave decide; 12 at three waves per SIMD) */
#endif
#ifndef VRC_PGROUP16
#define VRC_PGROUP16 12 /* 16-bit voxels: four registers of taps per sample in flight (6 / 8 / 12 measured: 2.03 / 1.92 / 1.80 ms on C2) */
#endif

/* March one brick segment through the packed atlas (Renderer.cu:206-223 with the trilinear fetch).  Organised as
 * vrc_march_segment_as: whole groups without per-sample tests while more than GROUP steps remain, the early-exit
 * test once per group with an exact replay, a general tail.  tab: vrc_cls8_entry table.  E: vrc_f4, or vrc_f2
 * for a grey transfer function (vrc_raycast_args.greyTable). */
template < bool COUNT, int GROUP, typename E, bool WIDE, int TB >
VRC_HD bool vrc_march_segment_packed( const vrc_frame& f, const vrc_dev_node& n, vrc_segment s,
                                      const void* __restrict__ packed, const vrc_f4* tab, const vrc_cls8& kc,
                                      E& color, uint32_t& nSamples, float levelStep )
{
    const float stepSize = levelStep > 0.0f ? levelStep : f.stepSize;
    float travel = s.dist;
    if( !( travel > 0.0f ) )
        return false;
    const vrc_sampler sm = vrc_make_sampler( n, f );
    /* the lane's packed slot.  A packed atlas of at most 4 GiB: the atlas pointer (uniform: a scalar base) + a 32-bit
     * byte offset per lane, the slot's offset folded into it.  WIDE (a larger one): a 64-bit pointer per lane. */
    const uint64_t slotBytes = vrc_packed_elems( WIDE ? ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase : (uint64_t)n.slotBase ) * (uint32_t)TB;
    const uint8_t* const slot = reinterpret_cast< const uint8_t* >( packed ) + ( WIDE ? slotBytes : 0u );
    const uint32_t bias = WIDE ? 0u : (uint32_t)slotBytes;
    vrc_fixpos fp = vrc_fixpos_init( sm, s.pos, s.step );
    /* texel centres at i + 0.5: the integer part of (coordinate - 0.5) is the lower tap, its fraction the weight */
    fp.x -= 1u << 23;
    fp.y -= 1u << 23;
    fp.z -= 1u << 23;
    bool done = false;
    const float guard = stepSize * (float)( GROUP + 1 );
    while( travel > guard )
    {
        uint32_t off[GROUP], offY1[GROUP];
        vrc_pk_taps< TB > t[GROUP];
        vrc_fixpos q = fp; /* the group's first sample: the weights are taken again from here after the loads */
        vrc_packed_offsets< GROUP, TB >( sm, fp, bias, off, offY1 );
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
        {
#if defined( VRC_PACKED_ABLATE ) && VRC_PACKED_ABLATE == 1 /* timing experiment only: no fetch */
            t[k] = vrc_pk_taps_fake( (const vrc_pk_taps< TB >*)nullptr, off[k] );
#else
            t[k] = vrc_packed_load( (const vrc_pk_taps< TB >*)nullptr, slot, off[k], offY1[k] );
#endif
        }
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            travel -= stepSize; /* same sequential subtraction as the reference */
        E e[GROUP];
#if defined( VRC_PACKED_ABLATE ) && VRC_PACKED_ABLATE == 2 /* timing experiment only: fetches, next to no arithmetic */
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
        {
            e[k] = E{};
            e[k].w = (float)( vrc_pk_taps_mix( t[k] ) >> 31 ) * 1e-9f;
        }
#else
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
        {
            e[k] = vrc_classify8( (const E*)nullptr, tab, vrc_trilerp_packed( t[k], q.x, q.y, q.z ), kc );
            q.x += q.dx;
            q.y += q.dy;
            q.z += q.dz;
        }
#endif
        const E saved = color;
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            vrc_composite( color, e[k] );
        if( COUNT )
            nSamples += GROUP;
        if( color.w > VRC_EARLY_EXIT )
        {
            /* crossed inside this group: replay it with the reference's per-sample exit */
            color = saved;
            if( COUNT )
                nSamples -= GROUP;
#pragma unroll
            for( int k = 0; k < GROUP; ++k )
            {
                vrc_composite( color, e[k], done );
                if( COUNT )
                    nSamples += done ? 0u : 1u;
                done = done || ( color.w > VRC_EARLY_EXIT );
            }
            return true;
        }
    }
    constexpr int TAILG = GROUP >= 4 ? GROUP / 2 : 1;
    while( travel > 0.0f && !done )
    {
        uint32_t off[TAILG], offY1[TAILG], cnt = 0;
        vrc_pk_taps< TB > t[TAILG];
        vrc_fixpos q = fp;
        vrc_packed_offsets< TAILG, TB >( sm, fp, bias, off, offY1 );
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            const bool v = travel > 0.0f;
            cnt += v ? 1u : 0u;
            /* a step the reference does not take reads the slot's first texels and blends nothing */
            off[k] = v ? off[k] : bias;
            offY1[k] = v ? offY1[k] : bias;
            t[k] = vrc_packed_load( (const vrc_pk_taps< TB >*)nullptr, slot, off[k], offY1[k] );
            travel -= stepSize;
        }
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            const E z = {};
            const E c = vrc_classify8( (const E*)nullptr, tab, vrc_trilerp_packed( t[k], q.x, q.y, q.z ), kc );
            const bool active = ( (uint32_t)k < cnt ) && !done;
            vrc_composite( color, (uint32_t)k < cnt ? c : z, done );
            if( COUNT )
                nSamples += active ? 1u : 0u;
            done = done || ( color.w > VRC_EARLY_EXIT );
            q.x += q.dx;
            q.y += q.dy;
            q.z += q.dz;
        }
    }
    return done;
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION: maximum-intensity projection (VRC_OPT_PROJECTION = VRC_PROJECTION_MIP; include/vrc_hip.h has the
 * definition of a MIP frame).  The sample set of a ray is the composite march's with an all-transparent transfer
 * function -- same ray, same bricks in the same order, same segments, positions and counts, no early termination -- and
 * the pixel is ONE classification of the largest sampled density, after the march.  A brick segment is walked by
 * vrc_projection_walk_point or vrc_projection_walk_trilinear, once for every projection (maximum, minimum, mean, first
 * crossing, with and without depth): they keep the control structure of vrc_march_segment_as /
 * vrc_march_segment_linear (whole groups under the same guard, the sequential travel chain, the same tails), so
 * positions and counts are theirs by construction.  What a projection makes of a group of samples is its fold; the
 * maximum's is folded into one register (integer voxels: two samples per instruction, v_max3_u32).  A brick visit
 * is the projection's own skip / uniform-brick preamble (lane-wise) and then vrc_projection_march.
 *
 * M is held as uint32_t for point samples of the integer atlases (the stored, offset-binary value: the shift is
 * monotone) and as float for the float atlas and every trilinear sample; a float M starts at -infinity and is folded
 * with a comparison that keeps M over a sample that is not a number, so NaN samples drop out.
 * ---------------------------------------------------------------------------------------- */
#define VRC_MODE_MIP 7           /* point samples */
#define VRC_MODE_MIP_TRILINEAR 8 /* trilinear samples by gathers */
#define VRC_MIP_EMPTY 0xFFFFFFFFu /* vrc_frame::mipMax: the pixel's rays have taken no sample (no integer voxel, and a NaN no float M can be) */

/* The fold of a MIP frame (VRC_OPT_MIP_FOLD) rides in the march mode, above the four bits that say how samples are taken:
 * the brick walks hand MODE through untouched.  Fold 0 -- the maximum -- leaves VRC_MODE_MIP and VRC_MODE_MIP_TRILINEAR
 * the numbers, and their instances the code, they were before there was a choice.
 *   minimum  the mirror of the maximum: identity (all ones / +infinity), comparison, skipping by the slot's smallest
 *            stored value (vrc_frame::slotMin).
 *   mean     the same march with an accumulate per sample: (sum, count) instead of M, see vrc_mean_state. */
#define VRC_FOLD_MAX 0
#define VRC_FOLD_MIN 1
#define VRC_FOLD_MEAN 2
#define VRC_FOLD_FIRST 3 /* the first sample at or above a threshold: an isosurface frame (below, "the first-crossing fold") */
#define VRC_MODE_WITH_FOLD( mode, fold ) ( ( mode ) + 16 * ( fold ) )
VRC_HD constexpr int vrc_mode_base( int mode ) { return mode & 15; }
VRC_HD constexpr int vrc_mode_fold( int mode ) { return ( mode >> 4 ) & 3; }
/* Depth tracking (VRC_OPT_MIP_DEPTH) rides above the fold: VRC_MODE_WITH_FOLD( mode, fold + VRC_FOLD_DEPTH ), for the
 * maximum and the minimum.  Without it a mode is the number, and its instances the code, they were before. */
#define VRC_FOLD_DEPTH 4
VRC_HD constexpr bool vrc_mode_depth( int mode ) { return ( ( mode >> 6 ) & 1 ) != 0; }
VRC_HD constexpr bool vrc_mode_is_mip( int mode )
{
    return vrc_mode_base( mode ) == VRC_MODE_MIP || vrc_mode_base( mode ) == VRC_MODE_MIP_TRILINEAR;
}

VRC_HD uint32_t vrc_mip_max( uint32_t a, uint32_t b ) { return a > b ? a : b; }
/* a: the maximum so far, never NaN (it starts at -infinity); b: a sample.  NOT fmaxf: a point sample of the float atlas
 * reaches this as the voxel's bits, and the maximum of a number and a SIGNALLING NaN is a NaN by IEEE 754-2008 maxNum --
 * v_max_f32 / v_max3_f32 in IEEE mode and glibc's fmaxf alike -- which would throw away the maximum so far.  The
 * comparison is false for every NaN and keeps a. */
VRC_HD float vrc_mip_max( float a, float b ) { return b > a ? b : a; }
template < typename D >
VRC_HD D vrc_mip_max3( D m, D a, D b ) { return vrc_mip_max( vrc_mip_max( m, a ), b ); }
VRC_HD uint32_t vrc_mip_bits( uint32_t m ) { return m; }
VRC_HD uint32_t vrc_mip_bits( float m ) { return vrc_float_bits( m ); }
VRC_HD void vrc_mip_from_bits( uint32_t b, uint32_t& m ) { m = b; }
VRC_HD void vrc_mip_from_bits( uint32_t b, float& m ) { m = vrc_bits_float( b ); }
/* the value that changes no maximum: what M starts from, and what a step the march does not take contributes */
VRC_HD void vrc_mip_identity( uint32_t& m ) { m = 0u; }
VRC_HD void vrc_mip_identity( float& m ) { m = vrc_bits_float( 0xFF800000u ); }

/* the same four for the minimum.  a: the minimum so far, never NaN (it starts at +infinity); the comparison form for the
 * reason vrc_mip_max( float ) gives: v_min_f32 and fminf make a NaN of a number and a signalling NaN too */
VRC_HD uint32_t vrc_mip_min( uint32_t a, uint32_t b ) { return a < b ? a : b; }
VRC_HD float vrc_mip_min( float a, float b ) { return b < a ? b : a; }
template < int FOLD, typename D >
VRC_HD D vrc_mip_fold( D m, D a )
{
    if constexpr( FOLD == VRC_FOLD_MIN )
        return vrc_mip_min( m, a );
    else
        return vrc_mip_max( m, a );
}
template < int FOLD, typename D >
VRC_HD D vrc_mip_fold3( D m, D a, D b )
{
    if constexpr( FOLD == VRC_FOLD_MIN )
        return vrc_mip_min( vrc_mip_min( m, a ), b ); /* integer voxels: v_min3_u32 */
    else
        return vrc_mip_max3( m, a, b );
}
/* (all ones is no voxel of an 8- or 16-bit atlas; a pixel's word holds it only as VRC_MIP_EMPTY, which means the same) */
template < int FOLD >
VRC_HD void vrc_mip_fold_identity( uint32_t& m )
{
    m = FOLD == VRC_FOLD_MIN ? 0xFFFFFFFFu : 0u;
}
template < int FOLD >
VRC_HD void vrc_mip_fold_identity( float& m )
{
    m = vrc_bits_float( FOLD == VRC_FOLD_MIN ? 0x7F800000u : 0xFF800000u );
}

/* vrc_frame::slotMax words.  0 = nothing known (the slot is never skipped).  Integer atlases: largest stored value + 1.
 * Float atlas: the largest voxel that is not NaN (-infinity if all are) as a key that orders like the floats do when
 * compared as unsigned integers -- what the upload's atomicMax needs; no float maps to 0. */
VRC_HD uint32_t vrc_slot_max_key( float v )
{
    const uint32_t b = vrc_float_bits( v );
    return ( b & 0x80000000u ) ? ~b : ( b | 0x80000000u );
}
VRC_HD float vrc_slot_max_float( uint32_t key )
{
    return vrc_bits_float( ( key & 0x80000000u ) ? ( key & 0x7FFFFFFFu ) : ~key );
}
/* can no sample of the slot raise M?  A point sample is a voxel of the slot: M >= the slot's maximum settles it.  A
 * trilinear sample is a convex combination of voxels of the slot (clamped taps stay inside it) evaluated in float:
 * three interpolations of a (1 - w) + b w, each at most (1 + 2.5 * 2^-24) times the larger operand's magnitude above
 * it, so below max + |max| * 1e-6; M has to reach that bound.  With operands of mixed sign a term can be far larger in
 * magnitude than |max|, and its rounding error with it -- but such a term is negative (no operand exceeds max, the
 * weights lie in [0, 1]) and lowers the result by 2^23 times its error: a result near max has terms of max's magnitude
 * or less, which is the case the bound is for.  (A bound that is not a number -- an all-NaN slot -- skips nothing.) */
template < bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_raise( uint32_t word, uint32_t m )
{
    static_assert( !TRILINEAR, "a trilinear M is a float" );
    return m >= word - 1u;
}
template < bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_raise( uint32_t word, float m )
{
    float top;
    if constexpr( sizeof( ATLAS_T ) == 4 )
        top = vrc_slot_max_float( word );
    else
        top = (float)( word - 1u );
    if constexpr( TRILINEAR )
    {
        VRC_STRICT_FP
        top = top + fabsf( top ) * 1e-6f;
    }
    return m >= top;
}

/* vrc_frame::slotMin words: the mirror, folded by the upload with the same atomicMax.  0 = nothing known.  Integer
 * atlases: the complement of the smallest stored value (never 0: a voxel has 16 bits at most).  Float atlas:
 * vrc_slot_max_key of the NEGATED voxel, NaN left out, the key of -infinity -- a minimum of +infinity -- for a brick
 * whose voxels are all NaN. */
VRC_HD uint32_t vrc_slot_min_key( uint32_t stored ) { return ~stored; }
VRC_HD uint32_t vrc_slot_min_key( float v ) { return vrc_slot_max_key( -v ); }
VRC_HD uint32_t vrc_slot_min_value( uint32_t word ) { return ~word; }
VRC_HD float vrc_slot_min_float( uint32_t word ) { return -vrc_slot_max_float( word ); }
/* can no sample of the slot lower M?  vrc_mip_cannot_raise read in a mirror.  Trilinear samples: the interpolation is
 * made of a (1 - w) + b w, products and sums that round to nearest, and rounding to nearest is an odd function, so
 * trilerp( -v ) = -trilerp( v ) bit for bit: the minimum of the samples of v is minus the maximum of the samples of -v,
 * whose voxels lie below -min.  The bound proven for the maximum therefore reads: no sample lies below
 * min - |min| * 1e-6, and M has to reach that. */
template < bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_lower( uint32_t word, uint32_t m )
{
    static_assert( !TRILINEAR, "a trilinear M is a float" );
    return m <= vrc_slot_min_value( word );
}
template < bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_lower( uint32_t word, float m )
{
    float bottom;
    if constexpr( sizeof( ATLAS_T ) == 4 )
        bottom = vrc_slot_min_float( word );
    else
        bottom = (float)vrc_slot_min_value( word );
    if constexpr( TRILINEAR )
    {
        VRC_STRICT_FP
        bottom = bottom - fabsf( bottom ) * 1e-6f;
    }
    return m <= bottom;
}

/* Depth tracking: can no sample of the slot even EQUAL M?  The two tests above with the comparison made strict.  A brick
 * that cannot beat M but can equal it holds the ray's depth if it lies nearer, and has to be marched then.  Trilinear
 * samples: the margin bounds them from above (below), and a sample can sit on the bound itself (a slot of zeros), so
 * only an M strictly beyond the bound rules a tie out. */
template < int FOLD, bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_reach( uint32_t word, uint32_t m )
{
    static_assert( !TRILINEAR, "a trilinear M is a float" );
    if constexpr( FOLD == VRC_FOLD_MIN )
        return m < vrc_slot_min_value( word );
    else
        return m >= word; /* word = the largest stored value + 1 */
}
template < int FOLD, bool TRILINEAR, typename ATLAS_T >
VRC_HD bool vrc_mip_cannot_reach( uint32_t word, float m )
{
    float bound;
    if constexpr( FOLD == VRC_FOLD_MIN )
    {
        if constexpr( sizeof( ATLAS_T ) == 4 )
            bound = vrc_slot_min_float( word );
        else
            bound = (float)vrc_slot_min_value( word );
        if constexpr( TRILINEAR )
        {
            VRC_STRICT_FP
            bound = bound - fabsf( bound ) * 1e-6f;
        }
        return m < bound;
    }
    else
    {
        if constexpr( sizeof( ATLAS_T ) == 4 )
            bound = vrc_slot_max_float( word );
        else
            bound = (float)( word - 1u );
        if constexpr( TRILINEAR )
        {
            VRC_STRICT_FP
            bound = bound + fabsf( bound ) * 1e-6f;
        }
        return m > bound;
    }
}

/* The depth of a ray beside its M: D = the smallest t_j = seg.tNear + (float)j * stepSize (the product and the sum each
 * rounded) over the samples that equal M, j the sample's index in its segment; +infinity while no sample equals M.  (M, D)
 * is folded lexicographically: a strictly better M replaces both, an equal M replaces D only by a smaller t.
 *   tNear  the segment's;  index: samples of the segment taken so far
 *   tie    M has not changed in this segment and an equal sample of it could still lie nearer than D (seg.tNear < D).
 *          Once the segment set D, or an equal sample came out no nearer, every later sample of it lies farther.
 * The marches fold a group as they did and look for the index only in a group that changed M or may hold such a tie. */
struct vrc_mip_depth
{
    float d;
    float tNear;
    uint32_t index;
    bool tie;
};
VRC_HD float vrc_mip_sample_t( float tNear, uint32_t j, float stepSize )
{
    VRC_STRICT_FP
    const float along = (float)j * stepSize;
    return tNear + along;
}
/* after a group of N samples d[] (taken[k]: sample k belongs to S) was folded into m, which was m0 before */
template < int N, typename D >
VRC_HD void vrc_mip_depth_group( vrc_mip_depth& z, D m0, D m, const D* d, const bool* taken, float stepSize )
{
    const bool changed = m != m0;
    if( changed || z.tie )
    {
        int first = -1;
#pragma unroll
        for( int k = N - 1; k >= 0; --k )
            first = ( taken[k] && d[k] == m ) ? k : first;
        if( first >= 0 )
        {
            const float t = vrc_mip_sample_t( z.tNear, z.index + (uint32_t)first, stepSize );
            if( changed || t < z.d )
                z.d = t;
            z.tie = false;
        }
    }
    z.index += (uint32_t)N;
}

/* trips of the reference's `for( ; travel > 0; travel -= stepSize )` (travel > 0): in integers where that is exact
 * (vrc_exact_step_count), else by the float chain itself */
VRC_HD uint32_t vrc_step_count( float travel, float stepSize )
{
    uint32_t n;
    if( vrc_exact_step_count( travel, stepSize, &n ) )
        return n;
    n = 0u;
    for( ; travel > 0.0f; travel -= stepSize )
        ++n;
    return n;
}

/* ---- the two walks of a brick segment: every projection takes its samples from these --------------------------------------
 * vrc_projection_walk_point is vrc_march_segment_as without table, blend and exit; vrc_projection_walk_trilinear is
 * vrc_march_segment_linear without classification, blend and exit.  What is made of the samples is the walk's FOLD
 * (vrc_extremum_fold, vrc_mean_fold, vrc_first_crossing_fold).  Per group of N samples a walk adds the samples the
 * reference takes to nSamples and calls
 *   fold.template group< N >( d, taken, elem )
 *     d[k]      the value of sample k: the stored voxel of a point sample (vrc_density< ATLAS_T >::type), the interpolated
 *               float of a trilinear one;
 *     taken[k]  the reference takes step k.  All true in a whole group; a step of a tail that the reference does not
 *               take reads element 0, and the fold leaves its d[k] out;
 *     elem( k ) the atlas element sample k is read from, for the fold that keeps where it hit;
 *   which returns true to leave the segment in front of the next group (the first-crossing fold of a ray that skips;
 *   every other fold returns false). */
template < bool CLAMP, bool FIXED, typename ATLAS_T, int GROUP, typename FOLD >
VRC_HD void vrc_projection_walk_point( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s, float travel,
                                       const ATLAS_T* __restrict__ atlas, FOLD& fold, uint32_t& nSamples )
{
    typedef typename vrc_density< ATLAS_T >::type D;
    const float stepSize = f.stepSize;
    const vrc_sampler sm = vrc_make_sampler( n, f );
    vrc_f3 pos = s.pos;
    if( !( travel > 0.0f ) )
        return;
    vrc_fixpos fp = { 0, 0, 0, 0, 0, 0 };
    if( FIXED )
        fp = vrc_fixpos_init( sm, pos, s.step );
    const float guard = stepSize * (float)( GROUP + 1 );
    while( travel > guard )
    {
        uint32_t idx[GROUP];
        if( FIXED )
            vrc_group_indices_fixed< GROUP >( sm, fp, idx );
        else
            vrc_group_indices< CLAMP, GROUP >( sm, pos, s.step, idx );
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            travel -= stepSize; /* same sequential subtraction as the reference */
        D d[GROUP];
        bool taken[GROUP];
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
        {
            d[k] = (D)vrc_gather( atlas, idx[k] );
            taken[k] = true;
        }
        nSamples += GROUP;
        if( fold.template group< GROUP >( d, taken, [&]( int k ) { return idx[k]; } ) )
            travel = 0.0f;
    }
    constexpr int TAILG = GROUP >= 8 ? ( GROUP + 2 ) / 4 : ( GROUP >= 2 ? GROUP / 2 : 1 );
    while( travel > 0.0f )
    {
        uint32_t idx[TAILG], cnt = 0;
        D d[TAILG];
        bool taken[TAILG];
        if( FIXED )
            vrc_group_indices_fixed< TAILG >( sm, fp, idx );
        else
            vrc_group_indices< CLAMP, TAILG >( sm, pos, s.step, idx );
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            taken[k] = travel > 0.0f;
            cnt += taken[k] ? 1u : 0u;
            idx[k] = taken[k] ? idx[k] : 0u; /* a step the reference does not take reads element 0 and contributes nothing */
            travel -= stepSize;
        }
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
            d[k] = (D)vrc_gather( atlas, idx[k] );
        nSamples += cnt;
        if( fold.template group< TAILG >( d, taken, [&]( int k ) { return idx[k]; } ) )
            travel = 0.0f;
    }
}

/* vrc_trilerp with its fused multiply-adds written out, for the maximum and the minimum, with and without depth tracking
 * (the SPELT walk): a frame has to come out with the same M, bit for bit, with depth tracking on and off, and under
 * contract(fast) the compiler is free to fuse either product of a (1 - w) + b w -- which one it takes depends on the
 * code around the expression (it keeps as a product the one with more uses; moving the fold behind the walk changed it
 * for the 8- and 16-bit atlases, profiles/r21_projection_walk.txt).  Read off the gfx950 code of the instances without
 * depth tracking as they were while they left the choice to the compiler, all of them:
 *   8- and 16-bit atlases  the first product is fused, fma( a, 1 - w, b * w ), at all three levels of every sample;
 *   the float atlas        the same, but for the first interpolation along x (c00) of the first sample of a group,
 *                          which comes out as fma( b, w, a * (1 - w) ) -- firstOfFloatGroup.
 * tests/test_depth.py holds the two kinds of instance to each other on the GPU, every atlas type, both folds, the grid
 * walk and the reference-order loop, with and without the clamped sampler.  The host build contracts nothing, either
 * way. */
VRC_HD float vrc_trilerp_fused_as_plain( const float v[8], float wx, float wy, float wz, bool firstOfFloatGroup )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    VRC_STRICT_FP
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
    const float c00 = firstOfFloatGroup ? __builtin_fmaf( v[1], wx, v[0] * ux ) : __builtin_fmaf( v[0], ux, v[1] * wx );
    const float c10 = __builtin_fmaf( v[2], ux, v[3] * wx );
    const float c01 = __builtin_fmaf( v[4], ux, v[5] * wx );
    const float c11 = __builtin_fmaf( v[6], ux, v[7] * wx );
    const float c0 = __builtin_fmaf( c00, uy, c10 * wy );
    const float c1 = __builtin_fmaf( c01, uy, c11 * wy );
    return __builtin_fmaf( c0, uz, c1 * wz );
#else
    (void)firstOfFloatGroup;
    return vrc_trilerp( v, wx, wy, wz );
#endif
}

/* the trilinear walk: masked groups of VRC_LGROUP.  SPELT: interpolate by vrc_trilerp_fused_as_plain */
template < bool CLAMP, bool SPELT, typename ATLAS_T, typename FOLD >
VRC_HD void vrc_projection_walk_trilinear( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s, float travel,
                                           const ATLAS_T* __restrict__ atlas, FOLD& fold, uint32_t& nSamples )
{
    const float stepSize = f.stepSize;
    const vrc_sampler sm = vrc_make_sampler( n, f );
    vrc_f3 pos = s.pos;
    while( travel > 0.0f )
    {
        bool valid[VRC_LGROUP];
        vrc_taps t[VRC_LGROUP];
#pragma unroll
        for( int k = 0; k < VRC_LGROUP; ++k )
        {
            VRC_FAST_FP
            valid[k] = travel > 0.0f;
            const float lx = ( pos.x - sm.minx ) * sm.kx + sm.ox;
            const float ly = ( pos.y - sm.miny ) * sm.ky + sm.oy;
            const float lz = ( pos.z - sm.minz ) * sm.kz + sm.oz;
            t[k] = vrc_trilinear_taps< CLAMP >( sm, lx, ly, lz );
            pos.x += s.step.x;
            pos.y += s.step.y;
            pos.z += s.step.z;
            travel -= stepSize;
        }
        float v[VRC_LGROUP][8];
#pragma unroll
        for( int k = 0; k < VRC_LGROUP; ++k )
#pragma unroll
            for( int c = 0; c < 8; ++c )
            {
                const uint32_t e = t[k].ax[c & 1] + t[k].ay[( c >> 1 ) & 1] + t[k].az[c >> 2];
                v[k][c] = (float)vrc_gather( atlas, valid[k] ? e : 0u );
            }
        float d[VRC_LGROUP];
#pragma unroll
        for( int k = 0; k < VRC_LGROUP; ++k )
        {
            if constexpr( SPELT )
                d[k] = vrc_trilerp_fused_as_plain( v[k], t[k].wx, t[k].wy, t[k].wz, k == 0 && sizeof( ATLAS_T ) == 4 );
            else
                d[k] = vrc_trilerp( v[k], t[k].wx, t[k].wy, t[k].wz );
            nSamples += valid[k] ? 1u : 0u;
        }
        /* The element a sample stands for (a hit's gradient is centred on it) is the voxel the point sampler addresses at
         * its position, the floor of the slot-local coordinate l: of the two taps of an axis (floor( l - 0.5 ) and the next,
         * clamped as the sampler clamps) it is the second exactly when the weight is >= 0.5 (l - 0.5 and the weight are
         * exact for l >= 0.5; below, both taps are 0). */
        if( fold.template group< VRC_LGROUP >( d, valid, [&]( int k ) {
                return t[k].ax[t[k].wx >= 0.5f ? 1 : 0] + t[k].ay[t[k].wy >= 0.5f ? 1 : 0] + t[k].az[t[k].wz >= 0.5f ? 1 : 0];
            } ) )
            travel = 0.0f;
    }
}

/* The end of a brick visit, whatever the fold: the lanes with `march` set walk segment s, the others stand by without
 * travel, and a wave none of whose lanes is left to march does not set the walk up.  BIG: the atlas holds more than 2^32
 * voxels; offsets inside a slot stay 32-bit and the slot's 64-bit base moves into the lane's atlas pointer
 * (vrc_march_brick), so the elements a fold is handed are slot-local */
template < bool CLAMP, bool FIXED, bool TRILINEAR, bool SPELT, typename ATLAS_T, int GROUP, bool BIG, typename FOLD >
VRC_HD void vrc_projection_march( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s, bool march,
                                  const ATLAS_T* __restrict__ atlas, FOLD& fold, uint32_t& nSamples )
{
    bool any = march;
#if defined( __HIP_DEVICE_COMPILE__ )
    any = __builtin_amdgcn_ballot_w64( march ) != 0ull;
#endif
    if( !any )
        return;
    const float travel = march ? s.dist : 0.0f;
    vrc_dev_node local = n;
    const ATLAS_T* slot = atlas;
    if( BIG )
    {
        local.slotBase = 0u;
        slot = atlas + ( ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase );
    }
    if constexpr( TRILINEAR )
        vrc_projection_walk_trilinear< CLAMP, SPELT, ATLAS_T >( f, local, s, travel, slot, fold, nSamples );
    else
        vrc_projection_walk_point< CLAMP, FIXED, ATLAS_T, GROUP >( f, local, s, travel, slot, fold, nSamples );
}

/* the maximum or the minimum of a ray, m, with its depth z where DEPTH (vrc_mip_depth_group).  Integer voxels: two
 * samples per instruction, v_max3_u32 / v_min3_u32.  A step that is not taken contributes the fold's identity */
template < int FOLD, bool DEPTH, typename D >
struct vrc_extremum_fold
{
    D& m;
    vrc_mip_depth& z;
    const float stepSize;

    template < int N, typename ELEM >
    VRC_HD bool group( const D* d, const bool* taken, const ELEM& ) const
    {
        D none, e[N];
        vrc_mip_fold_identity< FOLD >( none );
#pragma unroll
        for( int k = 0; k < N; ++k )
            e[k] = taken[k] ? d[k] : none;
        const D m0 = m;
#pragma unroll
        for( int k = 0; k + 1 < N; k += 2 )
            m = vrc_mip_fold3< FOLD >( m, e[k], e[k + 1] );
        if( N & 1 )
            m = vrc_mip_fold< FOLD >( m, e[N - 1] );
        if constexpr( DEPTH )
            vrc_mip_depth_group< N >( z, m0, m, e, taken, stepSize );
        return false;
    }
};

/* ---- the mean fold (VRC_FOLD_MEAN) ------------------------------------------------------------------------------------
 * The two walks above with an accumulate where the maximum was (vrc_mean_fold).  The sum of a ray is
 *   an unsigned 64-bit integer  for point samples of the 8- and 16-bit atlases: the stored values add exactly.  A group
 *     is summed in 32 bits, two samples per three-operand add (v_add3_u32; a group of 16-bit voxels stays far below
 *     2^32), and carried into the 64 once;
 *   a double  for the float atlas and every trilinear sample: one add per sample (full rate on this hardware), each
 *     float sample exact in it.  NaN and infinities go through the adds by IEEE rules.
 * A step the tail does not take contributes 0 and no count.  The ray's sample count is its nSamples. */
template < typename ACC >
VRC_HD uint32_t vrc_mean_bits_lo( ACC sum )
{
    unsigned long long b;
    memcpy( &b, &sum, 8 );
    return (uint32_t)b;
}
template < typename ACC >
VRC_HD uint32_t vrc_mean_bits_hi( ACC sum )
{
    unsigned long long b;
    memcpy( &b, &sum, 8 );
    return (uint32_t)( b >> 32 );
}
template < typename ACC >
VRC_HD ACC vrc_mean_from_bits( uint32_t lo, uint32_t hi )
{
    const unsigned long long b = ( (unsigned long long)hi << 32 ) | lo;
    ACC sum;
    memcpy( &sum, &b, 8 );
    return sum;
}

template < typename ACC >
struct vrc_mean_fold
{
    ACC& sum;

    template < int N, typename D, typename ELEM >
    VRC_HD bool group( const D* d, const bool* taken, const ELEM& ) const
    {
        if constexpr( std::is_integral< ACC >::value )
        {
            uint32_t e[N], g = 0u;
#pragma unroll
            for( int k = 0; k < N; ++k )
                e[k] = taken[k] ? d[k] : 0u;
#pragma unroll
            for( int k = 0; k + 1 < N; k += 2 )
                g = g + e[k] + e[k + 1];
            if( N & 1 )
                g += e[N - 1];
            sum += (ACC)g;
        }
        else
        {
#pragma unroll
            for( int k = 0; k < N; ++k )
                if( taken[k] )
                    sum += (ACC)d[k];
        }
        return false;
    }
};

/* the mean of a pixel's state, less the shift of an offset-binary atlas: the quotient in double, rounded to float once */
template < bool INTEGER >
VRC_HD float vrc_mean_value( uint32_t lo, uint32_t hi, uint32_t count, double shift )
{
    double sum;
    if constexpr( INTEGER )
        sum = (double)vrc_mean_from_bits< unsigned long long >( lo, hi );
    else
        sum = vrc_mean_from_bits< double >( lo, hi );
    return (float)( sum / (double)count - shift );
}

/* What vrc_get_projection_values returns for one pixel of the state a MIP frame's passes left: M in the volume's own
 * units and the pixel's count (the mean's samples; 1 or 0 for a maximum or minimum that exists or not).  floatState: M
 * is a float / the sum a double (the float atlas, trilinear samples), else integers; shift: what an offset-binary atlas
 * added to every voxel (exact in float, as an integer M is; a float M of such an atlas is a trilinear sample). */
VRC_HD void vrc_projection_value( uint32_t fold, bool floatState, float shift, uint32_t mipBits, unsigned long long meanSum,
                                  uint32_t meanCount, float& value, uint32_t& count )
{
    value = 0.0f;
    count = 0u;
    if( fold == VRC_FOLD_MEAN )
    {
        count = meanCount;
        if( count != 0u )
            value = floatState ? vrc_mean_value< false >( (uint32_t)meanSum, (uint32_t)( meanSum >> 32 ), count, (double)shift )
                               : vrc_mean_value< true >( (uint32_t)meanSum, (uint32_t)( meanSum >> 32 ), count, (double)shift );
    }
    else if( mipBits != VRC_MIP_EMPTY )
    {
        count = 1u;
        value = floatState ? (float)( (double)vrc_bits_float( mipBits ) - (double)shift ) : (float)mipBits - shift;
    }
}

/* One brick of one ray, mean fold.  The state: x, y = the low and high word of the sum, w = 0.  There is nothing to skip
 * by; uniform bricks (point samples of the 8- and 16-bit atlases) add value x step count, which is what the march
 * would have summed, exactly. */
template < bool CLAMP, bool FIXED, bool TRILINEAR, typename ATLAS_T, int GROUP, bool BIG >
VRC_HD void vrc_mean_brick( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s,
                            const ATLAS_T* __restrict__ atlas, vrc_f4& state, uint32_t& nSamples )
{
    constexpr bool INTEGER = !TRILINEAR && sizeof( ATLAS_T ) <= 2;
    typedef typename std::conditional< INTEGER, unsigned long long, double >::type ACC;
    ACC sum = vrc_mean_from_bits< ACC >( vrc_float_bits( state.x ), vrc_float_bits( state.y ) );
    bool march = s.dist > 0.0f;
    if constexpr( INTEGER )
    {
        if( march && n.slotInfoIndex != 0u && f.slotInfo != nullptr )
        {
            const uint32_t word = f.slotInfo[n.slotInfoIndex - 1u];
            if( vrc_slot_holds_one_value( word ) )
            {
                const uint32_t steps = vrc_step_count( s.dist, f.stepSize );
                sum += (ACC)( word & VRC_SLOT_VALUE_MASK ) * (ACC)steps;
                nSamples += steps;
                march = false;
            }
        }
    }
    /* (false: the interpolation is vrc_trilerp, fused as the compiler chooses, as it always was for this fold) */
    vrc_mean_fold< ACC > fold = { sum };
    vrc_projection_march< CLAMP, FIXED, TRILINEAR, false, ATLAS_T, GROUP, BIG >( f, n, s, march, atlas, fold, nSamples );
    state.x = vrc_bits_float( vrc_mean_bits_lo( sum ) );
    state.y = vrc_bits_float( vrc_mean_bits_hi( sum ) );
}

/* ---- the first-crossing fold (VRC_FOLD_FIRST): an isosurface frame ------------------------------------------------------
 * include/vrc_hip.h has the definition ("An isosurface frame").  The sample set is the MIP frame's, taken by the same
 * two walks (vrc_first_crossing_fold), and what is kept per ray is the hitting sample of the
 * smallest t_j (vrc_mip_sample_t): its value V, its depth D, and where it was read, for the gradient that is gathered once
 * after the march.  A sample hits when it is >= the frame's threshold: an integer comparison of the stored voxel for point
 * samples of the 8- and 16-bit atlases, a float comparison (false for a NaN) for everything else.
 *
 * t_j does not fall as j grows (the product (float)j * stepSize and the sum are each rounded, and rounding is monotone),
 * but two neighbours can share a t where stepSize is below an ulp of tNear, and of two hits with one t the larger V
 * stands.  So a ray that skips (VRC_OPT_MIP_SKIP) leaves a segment only in front of a group whose first t lies strictly
 * above the D it holds: no sample from there on can change (D, V).  Without skipping the same test only saves the search
 * of the group.  Either way every sample that is taken is computed by the same code: one kernel instance, and the
 * frame, V, D and G are the same bits with skipping on and off. */
VRC_HD uint32_t vrc_iso_int_threshold( float iso, float shift, uint32_t typeMax )
{
    /* the ceiling of iso + shift (exact in double), clamped to the type -- and one above it where no voxel can hit */
    const double s = (double)iso + (double)shift;
    if( !( s > 0.0 ) )
        return 0u;
    if( s > (double)typeMax )
        return typeMax + 1u;
    const uint32_t fl = (uint32_t)s;
    return (double)fl < s ? fl + 1u : fl;
}
/* The threshold of a float sample in stored units: the smallest float d that vrc_get_projection_values would report as
 * a value >= iso, i.e. (float)( (double)d - shift ) >= iso.  That report does not fall as d grows, so the hits are the
 * floats from one d on: found by bisection over the floats in their order (vrc_slot_max_key).  iso is not NaN. */
VRC_HD float vrc_iso_float_threshold( float iso, float shift )
{
    if( shift == 0.0f )
        return iso;
    uint32_t lo = vrc_slot_max_key( vrc_bits_float( 0xFF800000u ) ), hi = vrc_slot_max_key( vrc_bits_float( 0x7F800000u ) );
    while( lo < hi ) /* (+infinity always reports >= iso) */
    {
        const uint32_t mid = lo + ( hi - lo ) / 2u;
        const float d = vrc_slot_max_float( mid );
        if( (float)( (double)d - (double)shift ) >= iso )
            hi = mid;
        else
            lo = mid + 1u;
    }
    return vrc_slot_max_float( lo );
}
template < typename D >
VRC_HD D vrc_iso_threshold( const vrc_frame& f );
template <>
VRC_HD uint32_t vrc_iso_threshold< uint32_t >( const vrc_frame& f ) { return f.isoThreshold; }
template <>
VRC_HD float vrc_iso_threshold< float >( const vrc_frame& f ) { return f.isoStored; }

/* a ray inside one brick segment.  v, d: (V, D) so far; where: the atlas element the sample that set them was read
 * from, valid once lowered; tGroup: t of the next group's first sample */
template < typename D >
struct vrc_iso_march
{
    D v;
    float d;
    uint32_t where;
    bool lowered;
    float tNear;
    uint32_t index;
    float tGroup;
};
/* after a group of N samples d[] (taken[k]: sample k belongs to S), gmax their maximum with NaN left out; elem( k ): the
 * element sample k's gradient is centred on.  Returns true when nothing behind this group can change the ray. */
template < int N, typename D, typename ELEM >
VRC_HD bool vrc_iso_group( vrc_iso_march< D >& z, D thr, D gmax, const D* d, const bool* taken, float stepSize, ELEM elem )
{
    if( gmax >= thr && !( z.tGroup > z.d ) )
    {
#pragma unroll
        for( int k = 0; k < N; ++k )
            if( taken[k] && d[k] >= thr )
            {
                const float t = vrc_mip_sample_t( z.tNear, z.index + (uint32_t)k, stepSize );
                if( t < z.d || ( t == z.d && d[k] > z.v ) )
                {
                    z.d = t;
                    z.v = d[k];
                    z.where = elem( k );
                    z.lowered = true;
                }
            }
    }
    z.index += (uint32_t)N;
    z.tGroup = vrc_mip_sample_t( z.tNear, z.index, stepSize );
    return z.tGroup > z.d;
}

/* the first crossing of a ray, z, with the search in place of the maximum: per group the largest sample, NaN left out,
 * then vrc_iso_group.  skip: leave the segment once nothing behind the group can change the ray */
template < typename D >
struct vrc_first_crossing_fold
{
    vrc_iso_march< D >& z;
    const D thr;
    const bool skip;
    const float stepSize;

    template < int N, typename ELEM >
    VRC_HD bool group( const D* d, const bool* taken, const ELEM& elem ) const
    {
        D gmax;
        vrc_mip_identity( gmax );
#pragma unroll
        for( int k = 0; k < N; ++k )
            gmax = vrc_mip_max( gmax, taken[k] ? d[k] : gmax );
        return vrc_iso_group< N >( z, thr, gmax, d, taken, stepSize, elem ) && skip;
    }
};

/* What the uniform-brick shortcut counts for a segment it does not march: the samples vrc_projection_walk_point would
 * have taken under vrc_first_crossing_fold -- all of them without skipping, and with it the groups up to the one in front
 * of which the ray leaves.  It MIRRORS that walk's travel chain (guard, whole groups, TAILG, masked tail) and
 * vrc_iso_group's leave test by hand: a change to either is a change here.  Kept apart because the walk cannot run
 * without its addresses and gathers, and the host and the device have to count the same.  d: the ray's D after the
 * segment's first sample (a uniform segment changes it there or nowhere). */
template < int GROUP >
VRC_HD uint32_t vrc_iso_uniform_count( float travel, float stepSize, float tNear, float d, bool skip )
{
    if( !skip || !( d < vrc_bits_float( 0x7F800000u ) ) )
        return vrc_step_count( travel, stepSize );
    uint32_t n = 0u, index = 0u;
    const float guard = stepSize * (float)( GROUP + 1 );
    while( travel > guard )
    {
        for( int k = 0; k < GROUP; ++k )
            travel -= stepSize;
        n += GROUP;
        index += GROUP;
        if( vrc_mip_sample_t( tNear, index, stepSize ) > d )
            return n;
    }
    constexpr int TAILG = GROUP >= 8 ? ( GROUP + 2 ) / 4 : ( GROUP >= 2 ? GROUP / 2 : 1 );
    while( travel > 0.0f )
    {
        for( int k = 0; k < TAILG; ++k )
        {
            n += travel > 0.0f ? 1u : 0u;
            travel -= stepSize;
        }
        index += TAILG;
        if( vrc_mip_sample_t( tNear, index, stepSize ) > d )
            return n;
    }
    return n;
}

/* vrc_pixel_mip's state word of a hit in a uniform brick: there is nothing to gather, the gradient is 0 */
#define VRC_ISO_WHERE_UNIFORM 0xFFFFFFFFu
/* how far above D a brick's tNear has to lie for the grid walk to end the ray there.  The walk meets bricks by
 * increasing tNear -- but for the bricks around an edge or a corner, which it hands over in a fixed order and which tie
 * to within 2e-6 of t (vrc_ray_grid_dda: tolE); twice that */
#define VRC_ISO_WALK_MARGIN 4e-6f

/* One brick of one ray, first-crossing fold.  The state: x = the bits of V, z = D (+infinity: no hit yet), and, once
 * this pass has set them, y = 1 + the slot-local element the hit was read from (VRC_ISO_WHERE_UNIFORM: a uniform brick;
 * 0: this pass has not) and w = the bits of the node's index.
 *   skipping (vrc_frame::slotMax, NULL = off)  a lane takes no sample of a brick whose tNear lies strictly above its D,
 *     or whose slot cannot reach the threshold (vrc_mip_cannot_reach), and leaves a segment as described above;
 *   uniform bricks  a slot known to hold one value hits at the segment's first sample or not at all.
 * Returns true when the grid walk can end the ray. */
template < bool CLAMP, bool FIXED, bool TRILINEAR, typename ATLAS_T, int GROUP, bool BIG >
VRC_HD bool vrc_iso_brick( const vrc_frame& f, const vrc_dev_node& n, uint32_t nodeIndex, const vrc_segment& s,
                           const ATLAS_T* __restrict__ atlas, vrc_f4& state, uint32_t& nSamples )
{
    typedef typename vrc_density< ATLAS_T >::type P;
    typedef typename std::conditional< TRILINEAR, float, P >::type D;
    const D thr = vrc_iso_threshold< D >( f );
    const bool skip = f.slotMax != nullptr;
    vrc_iso_march< D > z;
    vrc_mip_from_bits( vrc_float_bits( state.x ), z.v );
    z.d = state.z;
    z.where = 0u;
    z.lowered = false;
    z.tNear = s.tNear;
    z.index = 0u;
    z.tGroup = s.tNear;
    bool march = s.dist > 0.0f;
    bool beyond = false;
    bool uniformHit = false;
    if( skip && march )
    {
        if( s.tNear > z.d )
        {
            VRC_STRICT_FP
            march = false;
            const float margin = fabsf( z.d ) * VRC_ISO_WALK_MARGIN;
            beyond = s.tNear > z.d + margin;
        }
        else if( n.slotInfoIndex != 0u )
        {
            const uint32_t word = f.slotMax[n.slotInfoIndex - 1u];
            if( word != 0u && vrc_mip_cannot_reach< VRC_FOLD_MAX, TRILINEAR, ATLAS_T >( word, thr ) )
                march = false;
        }
    }
    if constexpr( !TRILINEAR && sizeof( ATLAS_T ) <= 2 )
    {
        if( march && n.slotInfoIndex != 0u && f.slotInfo != nullptr )
        {
            const uint32_t word = f.slotInfo[n.slotInfoIndex - 1u];
            if( vrc_slot_holds_one_value( word ) )
            {
                const D value = (D)( word & VRC_SLOT_VALUE_MASK );
                if( value >= thr && ( s.tNear < z.d || ( s.tNear == z.d && value > z.v ) ) )
                {
                    z.d = s.tNear; /* (the segment's first sample: t_0 = tNear) */
                    z.v = value;
                    z.lowered = true;
                    uniformHit = true;
                }
                nSamples += vrc_iso_uniform_count< GROUP >( s.dist, f.stepSize, s.tNear, z.d, skip );
                march = false;
            }
        }
    }
    /* (false: vrc_trilerp, as vrc_mean_brick) */
    vrc_first_crossing_fold< D > fold = { z, thr, skip, f.stepSize };
    vrc_projection_march< CLAMP, FIXED, TRILINEAR, false, ATLAS_T, GROUP, BIG >( f, n, s, march, atlas, fold, nSamples );
    if( z.lowered )
    {
        /* (z.where of a marched hit: slot-local already where BIG) */
        const uint32_t base = BIG ? 0u : n.slotBase;
        state.x = vrc_bits_float( vrc_mip_bits( z.v ) );
        state.y = vrc_bits_float( uniformHit ? VRC_ISO_WHERE_UNIFORM : z.where - base + 1u );
        state.z = z.d;
        state.w = vrc_bits_float( nodeIndex );
    }
    return beyond;
}

/* slot-local voxel of a slot-local element offset: vrc_slot_local_index read backwards */
VRC_HD void vrc_slot_local_voxel( uint32_t e, uint32_t sbx, uint32_t sby, uint32_t& x, uint32_t& y, uint32_t& z )
{
    const uint32_t blk = e / VRC_MB_VOXELS, in = e % VRC_MB_VOXELS;
    const uint32_t bx = blk % sbx, by = ( blk / sbx ) % sby, bz = blk / ( sbx * sby );
    x = ( bx << VRC_MB_SHIFT ) | ( in & 7u );
    y = ( by << VRC_MB_SHIFT ) | ( ( in >> 3 ) & 3u ) | ( ( in >> 5 ) & 4u );
    z = ( bz << VRC_MB_SHIFT ) | ( ( in >> 5 ) & 3u ) | ( ( in >> 6 ) & 4u );
}

/* The addressing and the difference of a gradient, shared by the gradient of an isosurface hit (below) and the gradient of
 * every sample of a shaded composite frame (vrc_shade_policy): a voxel coordinate clamped to the slot, its two neighbours
 * along an axis clamped the same way, and the difference of the two stored voxels.  Whatever coordinate goes into
 * vrc_gradient_clamp, what comes out lies in [0, dim), and so do the two neighbours of such a coordinate: a gather at
 * them stays inside the slot. */
VRC_HD uint32_t vrc_gradient_clamp( uint32_t c, uint32_t dim ) { return c < dim ? c : dim - 1u; }
VRC_HD void vrc_gradient_neighbours( uint32_t c, uint32_t dim, uint32_t& lo, uint32_t& hi )
{
    lo = c > 0u ? c - 1u : 0u;
    hi = c + 1u < dim ? c + 1u : dim - 1u;
}
template < typename ATLAS_T >
VRC_HD float vrc_gradient_diff( ATLAS_T vHi, ATLAS_T vLo )
{
    VRC_STRICT_FP
    if constexpr( sizeof( ATLAS_T ) == 4 )
        return (float)vHi - (float)vLo;
    else
        return (float)( (int32_t)vHi - (int32_t)vLo );
}

/* The gradient of a hit: central differences of stored voxels around slot-local element `where` of node n, indices
 * clamped to the slot, times the node's voxels per world unit -- six gathers, once per ray and pass.  Integer voxels
 * are differenced in integers (exact; an offset-binary shift cancels), float voxels in float. */
template < typename ATLAS_T, bool BIG >
VRC_HD void vrc_iso_gradient( const vrc_frame& f, const vrc_dev_node& n, const ATLAS_T* __restrict__ atlas, uint32_t where,
                              float g[3] )
{
    VRC_STRICT_FP
    const uint32_t sbx = f.sbx, sby = f.sby;
    uint32_t c[3];
    vrc_slot_local_voxel( where, sbx, sby, c[0], c[1], c[2] );
    const ATLAS_T* slot = atlas;
    uint32_t base = n.slotBase;
    if( BIG )
    {
        base = 0u;
        slot = atlas + ( ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase );
    }
#pragma unroll
    for( int a = 0; a < 3; ++a ) /* (a coordinate read back from a sample's own address lies inside the slot) */
        c[a] = vrc_gradient_clamp( c[a], f.slotDim[a] );
#pragma unroll
    for( int a = 0; a < 3; ++a )
    {
        uint32_t lo[3] = { c[0], c[1], c[2] }, hi[3] = { c[0], c[1], c[2] };
        vrc_gradient_neighbours( c[a], f.slotDim[a], lo[a], hi[a] );
        const ATLAS_T vHi = vrc_gather( slot, base + vrc_slot_local_index( hi[0], hi[1], hi[2], sbx, sby ) );
        const ATLAS_T vLo = vrc_gather( slot, base + vrc_slot_local_index( lo[0], lo[1], lo[2], sbx, sby ) );
        g[a] = vrc_gradient_diff< ATLAS_T >( vHi, vLo ) * n.voxPerWorld[a];
    }
}

/* the headlight of an isosurface pixel: s = ambient + (1 - ambient) * |G.dir| / |G|, two-sided; 1 where |G| is 0 or not
 * finite.  Float, in this order, nothing contracted. */
VRC_HD float vrc_iso_shade( const float g[3], const vrc_f3& dir, float ambient )
{
    VRC_STRICT_FP
    const float xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
    const float len = sqrtf( ( xx + yy ) + zz );
    if( !( len > 0.0f ) || !( len < vrc_bits_float( 0x7F800000u ) ) )
        return 1.0f;
    const float dx = g[0] * dir.x, dy = g[1] * dir.y, dz = g[2] * dir.z;
    const float dot = fabsf( ( dx + dy ) + dz );
    const float diffuse = ( ( 1.0f - ambient ) * dot ) / len;
    return ambient + diffuse;
}

/* One brick of one ray.  The ray's state travels in the colour the brick walks hand on: x = the bits of M, y != 0 once
 * a sample was taken, w = 0 (no walk ever sees an opaque pixel).
 *   skipping (vrc_frame::slotMax)  a lane whose M no sample of the slot can raise takes none of them;
 *   uniform bricks (vrc_frame::slotInfo; point samples of the 8- and 16-bit atlases)  a lane in a slot known to hold
 *     one value takes max(M, value) and the segment's step count, without addressing or gathers (a trilinear sample
 *     of equal voxels is the value only up to rounding: those are fetched);
 *   a wave none of whose lanes is left to march does not set the march up. */
template < bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, int GROUP, bool BIG >
VRC_HD bool vrc_mip_brick( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s,
                           const ATLAS_T* __restrict__ atlas, vrc_f4& state, uint32_t& nSamples, uint32_t nodeIndex = 0u )
{
    constexpr bool TRILINEAR = vrc_mode_base( MODE ) == VRC_MODE_MIP_TRILINEAR;
    constexpr int FOLD = vrc_mode_fold( MODE );
    constexpr bool DEPTH = vrc_mode_depth( MODE );
    if constexpr( FOLD == VRC_FOLD_MEAN )
    {
        static_assert( !DEPTH, "the mean has no position" );
        vrc_mean_brick< CLAMP, FIXED, TRILINEAR, ATLAS_T, GROUP, BIG >( f, n, s, atlas, state, nSamples );
        return false;
    }
    else if constexpr( FOLD == VRC_FOLD_FIRST )
    {
        /* (nodeIndex: what only this fold keeps; true: the grid walk can end the ray) */
        static_assert( !DEPTH, "the first crossing keeps its depth by itself" );
        return vrc_iso_brick< CLAMP, FIXED, TRILINEAR, ATLAS_T, GROUP, BIG >( f, n, nodeIndex, s, atlas, state, nSamples );
    }
    else
    {
    typedef typename vrc_density< ATLAS_T >::type P;
    typedef typename std::conditional< TRILINEAR, float, P >::type D;
    D m;
    vrc_mip_from_bits( vrc_float_bits( state.x ), m );
    bool has = state.y != 0.0f;
    bool march = s.dist > 0.0f;
    /* depth tracking: z of the state = D; could an equal sample of this brick lie nearer? */
    vrc_mip_depth z = { state.z, s.tNear, 0u, DEPTH && s.tNear < state.z };
    if( march && n.slotInfoIndex != 0u )
    {
        if constexpr( FOLD == VRC_FOLD_MIN )
        {
            if( f.slotMin != nullptr && has )
            {
                const uint32_t word = f.slotMin[n.slotInfoIndex - 1u];
                if constexpr( DEPTH )
                {
                    /* skipped: no sample can equal M, or none can beat it and none lies nearer than D */
                    if( word != 0u && vrc_mip_cannot_lower< TRILINEAR, ATLAS_T >( word, m ) &&
                        ( !z.tie || vrc_mip_cannot_reach< FOLD, TRILINEAR, ATLAS_T >( word, m ) ) )
                        march = false;
                }
                else
                if( word != 0u && vrc_mip_cannot_lower< TRILINEAR, ATLAS_T >( word, m ) )
                    march = false;
            }
        }
        else if( f.slotMax != nullptr && has )
        {
            const uint32_t word = f.slotMax[n.slotInfoIndex - 1u];
            if constexpr( DEPTH )
            {
                if( word != 0u && vrc_mip_cannot_raise< TRILINEAR, ATLAS_T >( word, m ) &&
                    ( !z.tie || vrc_mip_cannot_reach< FOLD, TRILINEAR, ATLAS_T >( word, m ) ) )
                    march = false;
            }
            else
            if( word != 0u && vrc_mip_cannot_raise< TRILINEAR, ATLAS_T >( word, m ) )
                march = false;
        }
        if constexpr( !TRILINEAR && sizeof( ATLAS_T ) <= 2 )
        {
            if( march && f.slotInfo != nullptr )
            {
                const uint32_t word = f.slotInfo[n.slotInfoIndex - 1u];
                if( vrc_slot_holds_one_value( word ) )
                {
                    if constexpr( DEPTH )
                    {
                        /* (value, seg.tNear): the segment's first sample, j = 0, is the nearest of its equal ones */
                        const D m0 = m;
                        m = vrc_mip_fold< FOLD >( m, (D)( word & VRC_SLOT_VALUE_MASK ) );
                        if( m != m0 || ( z.tie && m == (D)( word & VRC_SLOT_VALUE_MASK ) ) )
                            z.d = s.tNear;
                    }
                    else
                    m = vrc_mip_fold< FOLD >( m, (D)( word & VRC_SLOT_VALUE_MASK ) );
                    has = true;
                    nSamples += vrc_step_count( s.dist, f.stepSize );
                    march = false;
                }
            }
        }
    }
    /* (every maximum and minimum spells the interpolation out, with depth and without: vrc_trilerp_fused_as_plain) */
    vrc_extremum_fold< FOLD, DEPTH, D > fold = { m, z, f.stepSize };
    vrc_projection_march< CLAMP, FIXED, TRILINEAR, true, ATLAS_T, GROUP, BIG >( f, n, s, march, atlas, fold, nSamples );
    has = has || march;
    state.x = vrc_bits_float( vrc_mip_bits( m ) );
    state.y = has ? 1.0f : 0.0f;
    if constexpr( DEPTH )
        state.z = z.d;
    return false;
    }
}

/* the pixel of a maximum M: TF((M - r0) / (r1 - r0)) as vrc_classify fetches it (256 texels, linear, the weight in
 * VRC_OPT_TF_FRAC_BITS bits), no opacity correction and no 255/256 clamp -- no step length is involved --, stored
 * premultiplied as the frame buffer's convention is */
VRC_HD vrc_f4 vrc_classify_mip( const vrc_f4* tfp, float d, const vrc_classifier& k )
{
    VRC_FAST_FP
    float xB = d * k.mult + k.add;
    xB = fminf( fmaxf( xB, -1.0f ), 255.99998f );
    const float fl = floorf( xB );
    float a = xB - fl;
    if( k.q > 0.0f )
        a = floorf( a * k.q + 0.5f ) * k.invq;
    const int j = (int)fl + 1;
    const vrc_f4 t0 = tfp[j], t1 = tfp[j + 1];
    const float b = 1.0f - a;
    const float alpha = VRC_LERP2( b, t0.w, a, t1.w );
    vrc_f4 e;
    e.x = VRC_LERP2( b, t0.x, a, t1.x ) * alpha;
    e.y = VRC_LERP2( b, t0.y, a, t1.y ) * alpha;
    e.z = VRC_LERP2( b, t0.z, a, t1.z ) * alpha;
    e.w = alpha;
    return e;
}

/* ------------------------------------------------------------------------------------------
 * The grouped march of the composite EXTENSIONS below (shaded, depth-tracking, pre-integrated): one front that takes a
 * group's samples, one segment loop around it, one wrapper around a brick visit.  What a mode makes of the values is its
 * policy (vrc_shade_policy, vrc_cdepth_policy, vrc_preint_policy).
 *
 * Sample positions, addresses and gathers are those of the unshaded march of the same sampler, expression for expression
 * (vrc_group_indices_fixed, vrc_group_indices, vrc_march_segment_linear), in the control structure of
 * vrc_march_segment_as: whole groups while more than a group of steps remains, one test per group with the exact replay
 * from the saved colour, a masked tail.
 * ---------------------------------------------------------------------------------------- */
/* per-axis parts of a slot-local element offset (vrc_voxel_address = x part + y part + z part + slotBase): the LDS
 * tables where the kernel filled them (fixed-point stepping: coordinates below 256), the arithmetic form elsewhere */
template < bool FIXED >
VRC_HD uint32_t vrc_shade_part( const vrc_sampler& s, int axis, uint32_t u )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    if constexpr( FIXED )
        return vrc_addr_tab[256u * (uint32_t)axis + ( u & 255u )];
#endif
    if( axis == 0 )
        return vrc_mul24( u >> VRC_MB_SHIFT, 504u ) + u;
    if( axis == 1 )
        return vrc_mul24( u >> VRC_MB_SHIFT, s.cyy ) + ( u << 3 ) + VRC_MB_FIX_Y( u );
    return vrc_mul24( u >> VRC_MB_SHIFT, s.czz ) + ( u << 6 ) - VRC_MB_FIX_Z( u );
}

/* the value of a sample: the stored voxel of a point sample, the interpolated float of a trilinear one */
template < bool TRILINEAR, typename ATLAS_T >
struct vrc_group_value
{
    typedef typename vrc_density< ATLAS_T >::type type;
};
template < typename ATLAS_T >
struct vrc_group_value< true, ATLAS_T >
{
    typedef float type;
};

/* The front of a group: the next N samples of a segment, pos / fp advanced past them: every address, then every gather,
 * then use( k, value of sample k ) for k = 0 ... N - 1 (the value: vrc_group_value< TRILINEAR, ATLAS_T >::type; handed
 * over one by one, the interpolation of a trilinear sample right before what the mode does with it, as the unshaded
 * marches order the two).  VOXEL: ux/uy/uz[k] is the voxel the POINT sampler addresses at sample k, under both filters.
 * MASKED: only the first cnt are the reference's; the others read element 0 */
template < bool CLAMP, bool FIXED, bool TRILINEAR, typename ATLAS_T, int N, bool MASKED, bool VOXEL, typename USE >
VRC_HD void vrc_group_values( const vrc_sampler& sm, vrc_f3& pos, const vrc_f3& step, vrc_fixpos& fp,
                              const ATLAS_T* __restrict__ atlas, uint32_t cnt, const USE& use,
                              [[maybe_unused]] uint32_t* ux = nullptr, [[maybe_unused]] uint32_t* uy = nullptr,
                              [[maybe_unused]] uint32_t* uz = nullptr )
{
    static_assert( !( TRILINEAR && FIXED ), "the trilinear gather march steps in float" );
    static_assert( !( CLAMP && FIXED ), "the clamped sampler steps in float" );
    if constexpr( TRILINEAR )
    {
        vrc_taps t[N];
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
            VRC_FAST_FP
            const float lx = ( pos.x - sm.minx ) * sm.kx + sm.ox;
            const float ly = ( pos.y - sm.miny ) * sm.ky + sm.oy;
            const float lz = ( pos.z - sm.minz ) * sm.kz + sm.oz;
            t[k] = vrc_trilinear_taps< CLAMP >( sm, lx, ly, lz );
            if constexpr( VOXEL )
            {
                float qx = lx, qy = ly, qz = lz;
                if( CLAMP )
                {
                    qx = fminf( fmaxf( qx, 0.0f ), sm.hix );
                    qy = fminf( fmaxf( qy, 0.0f ), sm.hiy );
                    qz = fminf( fmaxf( qz, 0.0f ), sm.hiz );
                }
                ux[k] = (uint32_t)(int)qx;
                uy[k] = (uint32_t)(int)qy;
                uz[k] = (uint32_t)(int)qz;
            }
            pos.x += step.x;
            pos.y += step.y;
            pos.z += step.z;
        }
        float v[N][8];
#pragma unroll
        for( int k = 0; k < N; ++k )
#pragma unroll
            for( int c = 0; c < 8; ++c )
            {
                const uint32_t a = t[k].ax[c & 1] + t[k].ay[( c >> 1 ) & 1] + t[k].az[c >> 2];
                v[k][c] = (float)vrc_gather( atlas, ( !MASKED || (uint32_t)k < cnt ) ? a : 0u );
            }
#pragma unroll
        for( int k = 0; k < N; ++k )
            use( k, vrc_trilerp( v[k], t[k].wx, t[k].wy, t[k].wz ) );
    }
    else
    {
        uint32_t idx[N];
        if constexpr( !VOXEL && FIXED )
            vrc_group_indices_fixed< N >( sm, fp, idx );
        else if constexpr( !VOXEL )
            vrc_group_indices< CLAMP, N >( sm, pos, step, idx );
        else if constexpr( FIXED )
        {
            /* (vrc_group_indices_fixed with the voxel kept) */
#pragma unroll
            for( int k = 0; k < N; ++k )
            {
                ux[k] = fp.x >> 24;
                uy[k] = fp.y >> 24;
                uz[k] = fp.z >> 24;
                fp.x += fp.dx;
                fp.y += fp.dy;
                fp.z += fp.dz;
#if defined( __HIP_DEVICE_COMPILE__ )
                asm( "" : "+v"( fp.x ), "+v"( fp.y ), "+v"( fp.z ) ); /* (vrc_group_indices_fixed: keep the three additions) */
#endif
            }
#pragma unroll
            for( int k = 0; k < N; ++k )
                idx[k] = vrc_shade_part< true >( sm, 0, ux[k] ) + vrc_shade_part< true >( sm, 1, uy[k] ) +
                         vrc_shade_part< true >( sm, 2, uz[k] ) + sm.slotBase;
        }
        else
        {
            /* (vrc_group_indices with the voxel kept) */
            VRC_FAST_FP
#pragma unroll
            for( int k = 0; k < N; ++k )
            {
                float lx = ( pos.x - sm.minx ) * sm.kx + sm.ox;
                float ly = ( pos.y - sm.miny ) * sm.ky + sm.oy;
                float lz = ( pos.z - sm.minz ) * sm.kz + sm.oz;
                if( CLAMP )
                {
                    lx = fminf( fmaxf( lx, 0.0f ), sm.hix );
                    ly = fminf( fmaxf( ly, 0.0f ), sm.hiy );
                    lz = fminf( fmaxf( lz, 0.0f ), sm.hiz );
                }
                ux[k] = (uint32_t)(int)lx;
                uy[k] = (uint32_t)(int)ly;
                uz[k] = (uint32_t)(int)lz;
                idx[k] = vrc_voxel_address( sm, ux[k], uy[k], uz[k] );
                pos.x += step.x;
                pos.y += step.y;
                pos.z += step.z;
            }
        }
        typename vrc_density< ATLAS_T >::type d[N];
#pragma unroll
        for( int k = 0; k < N; ++k )
            d[k] = (typename vrc_density< ATLAS_T >::type)vrc_gather( atlas, ( !MASKED || (uint32_t)k < cnt ) ? idx[k] : 0u );
#pragma unroll
        for( int k = 0; k < N; ++k )
            use( k, d[k] );
    }
}

/* what value d adds as the plain composite classifies it: vrc_classify (PERSAMPLE), else the classified table.  A
 * sample that is not taken (a no-op slot of a masked group) comes out as zeros, an exact no-op in the blend */
template < bool PERSAMPLE, typename V >
VRC_HD vrc_f4 vrc_group_classify( const vrc_f4* lut, const vrc_classifier& cls, bool taken, V d )
{
    if constexpr( PERSAMPLE )
    {
        const vrc_f4 z = { 0.f, 0.f, 0.f, 0.f };
        const vrc_f4 c = vrc_classify( lut, (float)d, cls );
        return taken ? c : z;
    }
    else
        return lut[taken ? d : 256u]; /* (entry 256: all zeros) */
}

/* One segment, marched in groups of GROUP.  POLICY p is the mode:
 *   p.template group< N, MASKED >( sm, pos, step, fp, atlas, cnt, e )   e[k] = what sample k adds (the front, then its own)
 *   POLICY::NOTES    false: nothing more.  true: the mode keeps something per ray beside the colour, and
 *   p.wants( color )            is its term of the per-group test: the group just blended has to be replayed
 *   p.note( color, j, k )       follows the blend of sample k of the group, sample j of the segment, where that sample
 *                               was composited (not frozen)
 * Every whole group holds only samples the reference loop reaches (vrc_march_segment_as); the group in which the test
 * fires is replayed from the saved colour with the reference's per-sample exit.  Where the ray goes on after a replay
 * (NOTES only), no weight was forced to 0 and the colour is the group's again, bit for bit */
template < bool COUNT, bool FIXED, int GROUP, typename ATLAS_T, typename POLICY >
VRC_HD bool vrc_group_segment( const vrc_frame& f, const vrc_dev_node& n, vrc_segment s, const ATLAS_T* __restrict__ atlas,
                               POLICY& p, vrc_f4& color, uint32_t& nSamples )
{
    const float stepSize = f.stepSize;
    const vrc_sampler sm = vrc_make_sampler( n, f );
    float travel = s.dist;
    vrc_f3 pos = s.pos;
    bool done = false;
    if( !( travel > 0.0f ) )
        return false;
    vrc_fixpos fp = { 0, 0, 0, 0, 0, 0 };
    if( FIXED )
        fp = vrc_fixpos_init( sm, pos, s.step );
    [[maybe_unused]] uint32_t first = 0u; /* the index, in its segment, of the first sample of the group in flight */
    const float guard = stepSize * (float)( GROUP + 1 );
    while( travel > guard )
    {
        vrc_f4 e[GROUP];
        p.template group< GROUP, false >( sm, pos, s.step, fp, atlas, (uint32_t)GROUP, e );
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            travel -= stepSize; /* same sequential subtraction as the reference */
        const vrc_f4 saved = color;
#pragma unroll
        for( int k = 0; k < GROUP; ++k )
            vrc_composite( color, e[k] );
        if( COUNT )
            nSamples += GROUP;
        const bool leave = color.w > VRC_EARLY_EXIT;
        bool replay = leave;
        if constexpr( POLICY::NOTES )
            replay = leave || p.wants( color );
        if( replay )
        {
            color = saved;
            if( COUNT )
                nSamples -= GROUP;
#pragma unroll
            for( int k = 0; k < GROUP; ++k )
            {
                vrc_composite( color, e[k], done );
                if( COUNT )
                    nSamples += done ? 0u : 1u;
                if constexpr( POLICY::NOTES )
                    if( !done )
                        p.note( color, first + (uint32_t)k, k );
                done = done || ( color.w > VRC_EARLY_EXIT );
            }
            if constexpr( !POLICY::NOTES )
                return true;
            else if( leave )
                return true;
        }
        if constexpr( POLICY::NOTES )
            first += (uint32_t)GROUP;
    }
    constexpr int TAILG = GROUP >= 4 ? GROUP / 2 : 1;
    while( travel > 0.0f && !done )
    {
        uint32_t cnt = 0;
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            cnt += travel > 0.0f ? 1u : 0u;
            travel -= stepSize;
        }
        vrc_f4 e[TAILG];
        p.template group< TAILG, true >( sm, pos, s.step, fp, atlas, cnt, e );
#pragma unroll
        for( int k = 0; k < TAILG; ++k )
        {
            const bool active = ( (uint32_t)k < cnt ) && !done;
            vrc_composite( color, e[k], done );
            if( COUNT )
                nSamples += active ? 1u : 0u;
            if constexpr( POLICY::NOTES )
                if( active )
                    p.note( color, first + (uint32_t)k, k );
            done = done || ( color.w > VRC_EARLY_EXIT );
        }
        if constexpr( POLICY::NOTES )
            first += (uint32_t)TAILG;
    }
    return done;
}

/* Is the brick one whose upload found one value in every voxel (the slot's word, written by the repack kernel on the
 * stream and under the fences of the voxels themselves; 0 where the frame has no words) -- for every lane of the wave?
 * Taken by the whole wave or not at all: a lane in a uniform brick of a wave that also holds other bricks gathers its
 * constant voxels like the rest, the same samples either way */
VRC_HD bool vrc_slot_uniform_wave( const vrc_frame& f, const vrc_dev_node& n, uint32_t& word )
{
    word = 0u;
    if( f.slotInfo != nullptr && n.slotInfoIndex != 0u )
        word = f.slotInfo[n.slotInfoIndex - 1u];
    bool general = !vrc_slot_holds_one_value( word );
#if defined( __HIP_DEVICE_COMPILE__ )
    general = __builtin_amdgcn_ballot_w64( general ) != 0ull;
#endif
    return !general;
}

/* One brick of one ray, around a mode's marches.  BIG: the atlas holds more than 2^32 voxels; offsets inside a slot stay
 * 32-bit and the slot's 64-bit base moves into the lane's pointer.  UNIFORM: the mode has a march for a slot known to
 * hold one value, uniform( n, s, atlas, value ) on the distance-only segment; otherwise, and for every other slot,
 * general( n, s, atlas ) on the full one */
template < bool BIG, bool UNIFORM, typename ATLAS_T, typename SRC, typename MARCH_UNIFORM, typename MARCH >
VRC_HD bool vrc_brick_visit( const vrc_frame& f, const vrc_dev_node& n, const SRC& src, const ATLAS_T* __restrict__ atlas,
                             const MARCH_UNIFORM& uniform, const MARCH& general )
{
    if constexpr( BIG )
    {
        vrc_dev_node local = n;
        local.slotBase = 0u;
        const ATLAS_T* slot = atlas + ( ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase );
        return vrc_brick_visit< false, UNIFORM >( f, local, src, slot, uniform, general );
    }
    else
    {
        if constexpr( UNIFORM )
        {
            uint32_t word;
            if( vrc_slot_uniform_wave( f, n, word ) )
            {
                const vrc_segment& s = src.distOnly();
                return uniform( n, s, atlas, word & 0xFFu );
            }
        }
        const vrc_segment& s = src.full();
        return general( n, s, atlas );
    }
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION: a shaded composite frame (VRC_OPT_SHADING = 1; include/vrc_hip.h, "A shaded composite frame").
 *
 * The composite frame with one change: the colour a sample adds is multiplied by the headlight term of the isosurface
 * frame, s = ambient + (1 - ambient) |G.dir| / |G| (vrc_iso_shade), G the central differences of the stored voxels around
 * the voxel the POINT sampler addresses at the sample's position (under both filters; vrc_gradient_* above: the
 * isosurface gradient's clamping and differencing), times the node's voxels per world unit.  The opacity is not
 * touched, so the samples, their order, early ray termination and the alpha channel are the unshaded frame's; with
 * ambient = 1, and wherever G is 0, so is the whole pixel.
 *
 * Sample positions, addresses, gathers and classification are those of the unshaded march of the same sampler
 * (vrc_group_values, vrc_group_classify), in the shared segment loop (vrc_group_segment) with the early-exit test alone.
 * Per group: centre addresses and gathers, classification, a ballot of
 * alpha' > 0, the six neighbour gathers of every sample that has one -- skipped by the lanes whose sample is transparent
 * (its e is 0 whatever s is) and by the wave when no lane needs them --, the differences, s, the blends.  A neighbour's
 * address is the centre's with one per-axis part swapped (the LDS tables under fixed-point stepping).
 * Groups of VRC_SHADE_GROUP = 4: 24 neighbour voxels in flight beside four classified samples; 8 x 6 do not fit the
 * registers of four waves per SIMD (DESIGN.md has the table of the instances).
 * ---------------------------------------------------------------------------------------- */
#define VRC_MODE_SHADE 10           /* point samples: the classified table for 8-bit voxels, vrc_classify otherwise */
#define VRC_MODE_SHADE_TRILINEAR 11 /* trilinear samples by gathers */
VRC_HD constexpr bool vrc_mode_is_shade( int mode ) { return mode == VRC_MODE_SHADE || mode == VRC_MODE_SHADE_TRILINEAR; }
#define VRC_SHADE_GROUP 4
#if defined( VRC_SHADE_SKIP_HOOK ) && !defined( __HIPCC__ )
/* host test builds only (tests/cpu_harness/shade_harness.cpp): 0 = gather the gradient of transparent samples too; and
 * how many samples were taken with / without their gradient */
static int vrc_shade_skip_hook = 1;
static unsigned long long vrc_shade_gradients[2];
#endif

/* the shaded mode of vrc_group_segment.  dir: the ray's unit direction */
template < bool CLAMP, bool FIXED, bool TRILINEAR, bool PERSAMPLE, typename ATLAS_T >
struct vrc_shade_policy
{
    static constexpr bool NOTES = false;
    const vrc_frame& f;
    const vrc_f4* lut;
    const vrc_classifier& cls;
    const vrc_f3& dir;

    /* e[k] = (rgb alpha' s, alpha') of sample k */
    template < int N, bool MASKED >
    VRC_HD void group( const vrc_sampler& sm, vrc_f3& pos, const vrc_f3& step, vrc_fixpos& fp,
                       const ATLAS_T* __restrict__ atlas, uint32_t cnt, vrc_f4* e ) const
    {
        /* 1. the sample itself: addresses, gathers, classification */
        uint32_t ux[N], uy[N], uz[N];
        typedef typename vrc_group_value< TRILINEAR, ATLAS_T >::type V;
        vrc_group_values< CLAMP, FIXED, TRILINEAR, ATLAS_T, N, MASKED, true >(
            sm, pos, step, fp, atlas, cnt,
            [&]( int k, V d ) { e[k] = vrc_group_classify< PERSAMPLE >( lut, cls, !MASKED || (uint32_t)k < cnt, d ); }, ux, uy, uz );
        /* 2. which samples need their gradient: a transparent one adds (0, 0) whatever s is */
        bool need[N], any = false;
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
            const bool taken = !MASKED || (uint32_t)k < cnt;
            need[k] = taken && e[k].w > 0.0f;
#if defined( VRC_SHADE_SKIP_HOOK ) && !defined( __HIPCC__ )
            if( vrc_shade_skip_hook == 0 )
                need[k] = taken;
            if( taken )
                ++vrc_shade_gradients[need[k] ? 1 : 0];
#endif
            any = any || need[k];
        }
#if defined( __HIP_DEVICE_COMPILE__ )
        any = __builtin_amdgcn_ballot_w64( any ) != 0ull;
#endif
        if( !any )
            return;
        /* 3. the six neighbours, back to back.  Every coordinate goes through vrc_gradient_clamp and
         * vrc_gradient_neighbours: all of them lie inside the slot, whatever the sampler made of the position */
        ATLAS_T vLo[N][3], vHi[N][3];
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
#pragma unroll
            for( int a = 0; a < 3; ++a )
                vLo[k][a] = vHi[k][a] = (ATLAS_T)0;
            if( need[k] )
            {
                const uint32_t c[3] = { vrc_gradient_clamp( ux[k], f.slotDim[0] ), vrc_gradient_clamp( uy[k], f.slotDim[1] ),
                                        vrc_gradient_clamp( uz[k], f.slotDim[2] ) };
                const uint32_t part[3] = { vrc_shade_part< FIXED >( sm, 0, c[0] ), vrc_shade_part< FIXED >( sm, 1, c[1] ),
                                           vrc_shade_part< FIXED >( sm, 2, c[2] ) };
#pragma unroll
                for( int a = 0; a < 3; ++a )
                {
                    uint32_t lo, hi;
                    vrc_gradient_neighbours( c[a], f.slotDim[a], lo, hi );
                    const uint32_t rest = part[( a + 1 ) % 3] + part[( a + 2 ) % 3] + sm.slotBase;
                    vHi[k][a] = vrc_gather( atlas, vrc_shade_part< FIXED >( sm, a, hi ) + rest );
                    vLo[k][a] = vrc_gather( atlas, vrc_shade_part< FIXED >( sm, a, lo ) + rest );
                }
            }
        }
        /* 4. differences, s, the shaded colour */
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
            VRC_STRICT_FP
            if( need[k] )
            {
                const float g[3] = { vrc_gradient_diff< ATLAS_T >( vHi[k][0], vLo[k][0] ) * sm.kx,
                                     vrc_gradient_diff< ATLAS_T >( vHi[k][1], vLo[k][1] ) * sm.ky,
                                     vrc_gradient_diff< ATLAS_T >( vHi[k][2], vLo[k][2] ) * sm.kz };
                const float sh = vrc_iso_shade( g, dir, f.shadeAmbient );
                e[k].x = e[k].x * sh;
                e[k].y = e[k].y * sh;
                e[k].z = e[k].z * sh;
            }
        }
    }
};

/* ------------------------------------------------------------------------------------------
 * EXTENSION: the depth of a composite frame (VRC_OPT_COMPOSITE_DEPTH; include/vrc_hip.h, "The depth of a composite
 * frame").
 *
 * The composite frame, untouched, and beside it per ray the first sample -- in the order the march composites them --
 * after which the ray's float32 alpha is >= tau: D = t_j = tNear + (float)j * stepSize of that sample
 * (vrc_mip_sample_t), V its value as a MIP frame keeps a sample's (the stored voxel of an 8- or 16-bit atlas as an
 * integer, the bits of the float voxel or of the interpolated float otherwise; vrc_projection_value reads it back).
 *
 * Sample positions, addresses, gathers and classification are those of the unshaded march of the same sampler
 * (vrc_group_values, vrc_group_classify), in the shared segment loop (vrc_group_segment) with a term of its own in the
 * per-group test and a note per replayed sample (vrc_cdepth_policy).  The test is the early exit's OR
 * "alpha >= tau and the ray has not crossed": alpha never decreases, so a group after which alpha is below tau holds no
 * crossing sample, and the group in which the test fires is replayed sample by sample -- once per ray for the crossing,
 * once for the early exit, in one loop.  The replay of a group that did not end the ray composites the same samples in
 * the same order with a weight that is never forced to 0: the colour it leaves is the group's, bit for bit, so frame
 * and count are the unshaded frame's whatever tau is.  The densities of the group in flight are kept beside its
 * classified samples (one register a sample) instead of fetching the crossing sample again.
 * Groups of VRC_CDEPTH_GROUP = 8 point samples through the classified table, VRC_CDEPTH_GROUP_CLASSIFIED = 6 under the
 * clamped sampler and for point samples classified one by one, and VRC_CDEPTH_GROUP_TRILINEAR = 4 trilinear ones: the largest at which no instance uses
 * scratch (DESIGN.md has the table of the instances).
 * ---------------------------------------------------------------------------------------- */
#define VRC_MODE_CDEPTH 12           /* point samples: the classified table for 8-bit voxels, vrc_classify otherwise */
#define VRC_MODE_CDEPTH_TRILINEAR 13 /* trilinear samples by gathers */
VRC_HD constexpr bool vrc_mode_is_cdepth( int mode ) { return mode == VRC_MODE_CDEPTH || mode == VRC_MODE_CDEPTH_TRILINEAR; }
#define VRC_CDEPTH_GROUP 8            /* point samples through the classified table (8-bit voxels) */
#define VRC_CDEPTH_GROUP_CLASSIFIED 6 /* ... under the clamped sampler, and point samples classified one by one (16-bit
                                       * and float voxels) */
#define VRC_CDEPTH_GROUP_TRILINEAR 4

/* what a ray keeps beside its colour: has it crossed (in this pass or, by the pixel's D, in one before), and the pair */
struct vrc_cdepth_state
{
    float d;    /* +infinity until the ray crosses */
    uint32_t v; /* VRC_MIP_EMPTY until then */
    bool crossed;
};
VRC_HD uint32_t vrc_cdepth_bits( uint32_t v ) { return v; }
VRC_HD uint32_t vrc_cdepth_bits( float v ) { return vrc_float_bits( v ); }

/* after sample j of the segment was composited (not frozen): the crossing, once per ray */
VRC_HD void vrc_cdepth_note( vrc_cdepth_state& z, const vrc_f4& color, float tau, float tNear, uint32_t j, float stepSize,
                             uint32_t v )
{
    if( !z.crossed && color.w >= tau )
    {
        z.crossed = true;
        z.d = vrc_mip_sample_t( tNear, j, stepSize );
        z.v = v;
    }
}

/* the depth-tracking mode of vrc_group_segment, for one segment (tNear: its first sample's t).  GROUP: the largest group
 * it is asked for */
template < bool CLAMP, bool FIXED, bool TRILINEAR, bool PERSAMPLE, typename ATLAS_T, int GROUP >
struct vrc_cdepth_policy
{
    static constexpr bool NOTES = true;
    const vrc_f4* lut;
    const vrc_classifier& cls;
    vrc_cdepth_state& z;
    float tau, tNear, stepSize;
    uint32_t vb[GROUP]; /* the values of the group in flight */

    /* e[k] = (rgb alpha', alpha') of sample k */
    template < int N, bool MASKED >
    VRC_HD void group( const vrc_sampler& sm, vrc_f3& pos, const vrc_f3& step, vrc_fixpos& fp,
                       const ATLAS_T* __restrict__ atlas, uint32_t cnt, vrc_f4* e )
    {
        static_assert( N <= GROUP, "vb holds the group" );
        typedef typename vrc_group_value< TRILINEAR, ATLAS_T >::type V;
        vrc_group_values< CLAMP, FIXED, TRILINEAR, ATLAS_T, N, MASKED, false >( sm, pos, step, fp, atlas, cnt, [&]( int k, V d ) {
            e[k] = vrc_group_classify< PERSAMPLE >( lut, cls, !MASKED || (uint32_t)k < cnt, d );
            vb[k] = vrc_cdepth_bits( d );
        } );
    }
    VRC_HD bool wants( const vrc_f4& color ) const { return !z.crossed && color.w >= tau; }
    VRC_HD void note( const vrc_f4& color, uint32_t j, int k ) { vrc_cdepth_note( z, color, tau, tNear, j, stepSize, vb[k] ); }
};

/* A slot known to hold one value (vrc_march_segment_as, UNIFORM): the same composites of its one table entry in the same
 * order and the same count -- counted in integers where that is the float chain's count exactly, taken by the whole wave
 * or not at all, else the float chain sample by sample -- with the crossing found as vrc_group_segment finds it */
template < bool COUNT >
VRC_HD bool vrc_cdepth_uniform( const vrc_frame& f, const vrc_segment& s, const vrc_f4 ue, uint32_t value, vrc_f4& color,
                                uint32_t& nSamples, vrc_cdepth_state& z )
{
    const float stepSize = f.stepSize;
    const float tau = f.cdepthTau;
    float travel = s.dist;
    if( !( travel > 0.0f ) )
        return false;
    uint32_t first = 0u;
    uint32_t nLeft;
    bool counted = vrc_exact_step_count( travel, stepSize, &nLeft );
#if defined( __HIP_DEVICE_COMPILE__ )
    counted = __builtin_amdgcn_ballot_w64( !counted ) == 0ull;
#endif
    if( !counted )
    {
        for( ; travel > 0.0f; travel -= stepSize, ++first )
        {
            vrc_composite( color, ue );
            if( COUNT )
                nSamples += 1u;
            vrc_cdepth_note( z, color, tau, s.tNear, first, stepSize, value );
            if( color.w > VRC_EARLY_EXIT )
                return true;
        }
        return false;
    }
    while( nLeft >= (uint32_t)VRC_UNIFORM_GROUP )
    {
        const vrc_f4 saved = color;
#pragma unroll
        for( int k = 0; k < VRC_UNIFORM_GROUP; ++k )
            vrc_composite( color, ue );
        if( color.w > VRC_EARLY_EXIT || ( !z.crossed && color.w >= tau ) )
        {
            color = saved;
#pragma unroll 1 /* (unrolled with its sixteen exits this loop took over 300 registers of scratch) */
            for( uint32_t k = 0; k < (uint32_t)VRC_UNIFORM_GROUP; ++k )
            {
                vrc_composite( color, ue );
                if( COUNT )
                    nSamples += 1u;
                vrc_cdepth_note( z, color, tau, s.tNear, first + k, stepSize, value );
                if( color.w > VRC_EARLY_EXIT )
                    return true;
            }
        }
        else if( COUNT )
            nSamples += (uint32_t)VRC_UNIFORM_GROUP;
        nLeft -= (uint32_t)VRC_UNIFORM_GROUP;
        first += (uint32_t)VRC_UNIFORM_GROUP;
    }
    for( ; nLeft > 0u; --nLeft, ++first )
    {
        vrc_composite( color, ue );
        if( COUNT )
            nSamples += 1u;
        vrc_cdepth_note( z, color, tau, s.tNear, first, stepSize, value );
        if( color.w > VRC_EARLY_EXIT )
            return true;
    }
    return false;
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION: a pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1; include/vrc_hip.h, "A pre-integrated
 * composite frame").
 *
 * The composite frame with one change: what a sample contributes is looked up by the values at both ends of its step,
 * E(d_{j-1}, d_j), in a 256 x 256 table pre-integrated from the transfer function; sample 0 of every brick visit is paired
 * with itself.  Positions, addresses, gathers, the order of the blends and early ray termination are the plain march's.
 *
 * 1. The table (vrc_preint_*; float64, the same body on the host and in vrc_k_build_preint).  TF(x) is the 256 texels read
 *    by exact linear interpolation at clamp(x, 0, 255); u(x) = 1 - min(TF_a(x), 255/256); tau = -ln u.  Between two texel
 *    centres u is linear but for the point where TF_a crosses 255/256, behind which it is 1/256: vrc_preint_span splits
 *    there.  On a piece with u and the colour linear, int tau and int tau c have closed forms (vrc_preint_piece); where u
 *    moves by less than a fifth of its smaller end these cancel, and an 8-point Gauss rule, there exact to rounding (the
 *    logarithm's singularity is more than ten half-lengths away), takes their place.  An entry is the partial span at
 *    either end plus a difference of per-texel prefix sums (256 x 4 doubles, built once per launch and block), or one
 *    partial span where both ends share a texel interval: nothing small is ever the difference of two large numbers
 *    but the prefix difference, whose error of 255 ln 256 x 2^-52 is far inside the 1e-6 the contract allows.
 * 2. The march (vrc_preint_policy): the shared front and segment loop (vrc_group_values, vrc_group_segment) with the
 *    early-exit test alone; per group the gathers, then the table reads, then the blends, and one carried value per lane: the last
 *    value of the group before (the visit's first sample: its own).  A no-op slot of the tail reads entry (0, 0) of the
 *    table, comes out as zeros and leaves the carried value alone.
 * ---------------------------------------------------------------------------------------- */
#define VRC_MODE_PREINT 14           /* point samples */
#define VRC_MODE_PREINT_TRILINEAR 15 /* trilinear samples by gathers */
VRC_HD constexpr bool vrc_mode_is_preint( int mode ) { return mode == VRC_MODE_PREINT || mode == VRC_MODE_PREINT_TRILINEAR; }
#define VRC_PREINT_GROUP 8       /* the value-indexed table: 8 voxels, then 8 table entries in flight */
#define VRC_PREINT_GROUP_TEXEL 4 /* the texel-indexed table: 4 voxels or 32 taps, then 16 table entries in flight (8 x 4
                                  * entries beside the walk's state do not fit the registers of four waves per SIMD) */
#define VRC_PREINT_DIM 256u
#define VRC_PREINT_ENTRIES ( VRC_PREINT_DIM * VRC_PREINT_DIM )
#define VRC_PREINT_VALUE 0 /* kinds of table: indexed by two stored bytes ... */
#define VRC_PREINT_TEXEL 1 /* ... or read bilinearly at two texel coordinates */

struct vrc_preint_sum
{
    double i, r, g, b; /* int tau, int tau red, int tau green, int tau blue */
};

/* one piece of length len on which u runs linearly from ua to ub and the colour from ca to cb */
VRC_HD void vrc_preint_piece( double len, double ua, double ub, const double* ca, const double* cb, vrc_preint_sum& acc )
{
    if( !( len > 0.0 ) )
        return;
    const double m = ub - ua;
    const double lo = ua < ub ? ua : ub;
    double i0, i1; /* int_0^1 -ln u dw and int_0^1 -ln u w dw, u = ua + m w */
    if( fabs( m ) >= 0.2 * lo )
    {
        const double la = log( ua ), lb = log( ub );
        const double h0 = ( ub * lb - ub ) - ( ua * la - ua );
        const double h1 = ( 0.5 * ub * ub * lb - 0.25 * ub * ub ) - ( 0.5 * ua * ua * la - 0.25 * ua * ua );
        i0 = -h0 / m;
        i1 = -( h1 - ua * h0 ) / ( m * m );
    }
    else
    {
        const double gx[4] = { 0.019855071751231912, 0.10166676129318664, 0.2372337950418355, 0.4082826787521751 };
        const double gw[4] = { 0.050614268145188344, 0.11119051722668717, 0.15685332293894352, 0.18134189168918088 };
        i0 = i1 = 0.0;
        for( int q = 0; q < 4; ++q )
        {
            const double w0 = gx[q], w1 = 1.0 - gx[q];
            const double t0 = -log( ua + m * w0 ), t1 = -log( ua + m * w1 );
            i0 += gw[q] * ( t0 + t1 );
            i1 += gw[q] * ( t0 * w0 + t1 * w1 );
        }
    }
    acc.i += len * i0;
    acc.r += len * ( ca[0] * i0 + ( cb[0] - ca[0] ) * i1 );
    acc.g += len * ( ca[1] * i0 + ( cb[1] - ca[1] ) * i1 );
    acc.b += len * ( ca[2] * i0 + ( cb[2] - ca[2] ) * i1 );
}

/* [s, e] of the interval between texel centres i and i + 1 (0 <= s <= e <= 1), split where TF_a crosses 255/256 */
VRC_HD void vrc_preint_span( const float* tf, uint32_t i, double s, double e, vrc_preint_sum& acc )
{
    if( !( e > s ) )
        return;
    const double top = 255.0 / 256.0;
    const double a0 = (double)tf[i * 4u + 3u], a1 = (double)tf[i * 4u + 7u];
    const double c0[3] = { (double)tf[i * 4u], (double)tf[i * 4u + 1u], (double)tf[i * 4u + 2u] };
    const double c1[3] = { (double)tf[i * 4u + 4u], (double)tf[i * 4u + 5u], (double)tf[i * 4u + 6u] };
    double cut[3] = { s, e, e };
    int pieces = 1;
    if( ( a0 < top ) != ( a1 < top ) )
    {
        const double t = ( top - a0 ) / ( a1 - a0 );
        if( t > s && t < e )
        {
            cut[1] = t;
            pieces = 2;
        }
    }
    for( int p = 0; p < pieces; ++p )
    {
        const double p0 = cut[p], p1 = cut[p + 1];
        const double mid = a0 + ( a1 - a0 ) * ( 0.5 * ( p0 + p1 ) );
        double ua = 1.0 / 256.0, ub = 1.0 / 256.0;
        if( mid < top ) /* the piece lies on the unclamped side: its ends may touch the crossing */
        {
            const double q0 = a0 + ( a1 - a0 ) * p0, q1 = a0 + ( a1 - a0 ) * p1;
            ua = 1.0 - ( q0 < top ? q0 : top );
            ub = 1.0 - ( q1 < top ? q1 : top );
        }
        const double ca[3] = { c0[0] + ( c1[0] - c0[0] ) * p0, c0[1] + ( c1[1] - c0[1] ) * p0, c0[2] + ( c1[2] - c0[2] ) * p0 };
        const double cb[3] = { c0[0] + ( c1[0] - c0[0] ) * p1, c0[1] + ( c1[1] - c0[1] ) * p1, c0[2] + ( c1[2] - c0[2] ) * p1 };
        vrc_preint_piece( p1 - p0, ua, ub, ca, cb, acc );
    }
}

/* beyond the first or last texel centre the transfer function is that texel */
VRC_HD void vrc_preint_outside( const float* tf, uint32_t i, double len, vrc_preint_sum& acc )
{
    if( !( len > 0.0 ) )
        return;
    const double top = 255.0 / 256.0;
    const double a = (double)tf[i * 4u + 3u];
    const double tau = -log( 1.0 - ( a < top ? a : top ) );
    acc.i += len * tau;
    acc.r += len * tau * (double)tf[i * 4u];
    acc.g += len * tau * (double)tf[i * 4u + 1u];
    acc.b += len * tau * (double)tf[i * 4u + 2u];
}

/* the plain classification at texel coordinate x, in float64 with exact weights: E(x, x) */
VRC_HD vrc_f4 vrc_preint_plain( const float* tf, double x, double k )
{
    const double top = 255.0 / 256.0;
    const double xc = x < 0.0 ? 0.0 : ( x > 255.0 ? 255.0 : x );
    const uint32_t i0 = xc < 255.0 ? (uint32_t)xc : 254u;
    const double w = xc - (double)i0;
    const double a = (double)tf[i0 * 4u + 3u] + ( (double)tf[i0 * 4u + 7u] - (double)tf[i0 * 4u + 3u] ) * w;
    const double alpha = 1.0 - pow( 1.0 - ( a < top ? a : top ), k );
    vrc_f4 e;
    e.x = (float)( ( (double)tf[i0 * 4u] + ( (double)tf[i0 * 4u + 4u] - (double)tf[i0 * 4u] ) * w ) * alpha );
    e.y = (float)( ( (double)tf[i0 * 4u + 1u] + ( (double)tf[i0 * 4u + 5u] - (double)tf[i0 * 4u + 1u] ) * w ) * alpha );
    e.z = (float)( ( (double)tf[i0 * 4u + 2u] + ( (double)tf[i0 * 4u + 6u] - (double)tf[i0 * 4u + 2u] ) * w ) * alpha );
    e.w = (float)alpha;
    return e;
}

/* prefix[i] = the integrals over [0, i], i = 0 ... 255, summed in texel order */
VRC_HD void vrc_preint_prefix( const float* tf, vrc_preint_sum* prefix )
{
    vrc_preint_sum run = { 0.0, 0.0, 0.0, 0.0 };
    prefix[0] = run;
    for( uint32_t i = 0; i + 1u < VRC_PREINT_DIM; ++i )
    {
        vrc_preint_sum one = { 0.0, 0.0, 0.0, 0.0 };
        vrc_preint_span( tf, i, 0.0, 1.0, one );
        run.i += one.i;
        run.r += one.r;
        run.g += one.g;
        run.b += one.b;
        prefix[i + 1u] = run;
    }
}

/* E(xf, xb), xf != xb as texel coordinates (unclamped); the smaller one is always integrated from, so that the entry is
 * symmetric bit for bit */
VRC_HD vrc_f4 vrc_preint_entry( const float* tf, const vrc_preint_sum* prefix, double xf, double xb, double k )
{
    const double lo = xf < xb ? xf : xb, hi = xf < xb ? xb : xf;
    vrc_preint_sum acc = { 0.0, 0.0, 0.0, 0.0 };
    vrc_preint_outside( tf, 0u, ( hi < 0.0 ? hi : 0.0 ) - lo, acc );
    vrc_preint_outside( tf, 255u, hi - ( lo > 255.0 ? lo : 255.0 ), acc );
    const double cl = lo < 0.0 ? 0.0 : ( lo > 255.0 ? 255.0 : lo ), ch = hi < 0.0 ? 0.0 : ( hi > 255.0 ? 255.0 : hi );
    if( ch > cl )
    {
        const uint32_t il = cl < 255.0 ? (uint32_t)cl : 254u, ih = ch < 255.0 ? (uint32_t)ch : 254u;
        if( il == ih )
            vrc_preint_span( tf, il, cl - (double)il, ch - (double)il, acc );
        else
        {
            vrc_preint_span( tf, il, cl - (double)il, 1.0, acc );
            acc.i += prefix[ih].i - prefix[il + 1u].i;
            acc.r += prefix[ih].r - prefix[il + 1u].r;
            acc.g += prefix[ih].g - prefix[il + 1u].g;
            acc.b += prefix[ih].b - prefix[il + 1u].b;
            vrc_preint_span( tf, ih, 0.0, ch - (double)ih, acc );
        }
    }
    vrc_f4 e = { 0.f, 0.f, 0.f, 0.f };
    if( !( acc.i > 0.0 ) )
        return e;
    const double alpha = -expm1( -k * ( acc.i / ( hi - lo ) ) );
    e.x = (float)( acc.r / acc.i * alpha );
    e.y = (float)( acc.g / acc.i * alpha );
    e.z = (float)( acc.b / acc.i * alpha );
    e.w = (float)alpha;
    return e;
}

/* the texel coordinate of stored value d as vrc_classify forms it, in float64 (the value-indexed table) */
VRC_HD double vrc_preint_value_coord( uint32_t d, const vrc_lut_params& p )
{
    return ( (double)d - (double)p.rangeMin ) / ( (double)p.rangeMax - (double)p.rangeMin ) * 256.0 - 0.5;
}

/* entry (row, col) of the table of `kind`; lut: the classified table, whose entries the diagonal of the value-indexed
 * table copies */
VRC_HD vrc_f4 vrc_preint_table_entry( const float* tf, const vrc_f4* lut, const vrc_preint_sum* prefix, vrc_lut_params p,
                                      int kind, uint32_t row, uint32_t col )
{
    const double k = (double)p.alphaCorrection;
    if( kind == VRC_PREINT_VALUE )
    {
        if( row == col )
            return lut[row];
        return vrc_preint_entry( tf, prefix, vrc_preint_value_coord( row, p ), vrc_preint_value_coord( col, p ), k );
    }
    if( row == col )
        return vrc_preint_plain( tf, (double)row, k );
    return vrc_preint_entry( tf, prefix, (double)row, (double)col, k );
}

/* the texel coordinate of a sample of the texel-indexed table: vrc_classify's, clamped to the texel centres (NaN: 0) */
VRC_HD float vrc_preint_coord( float d, const vrc_classifier& k )
{
    VRC_FAST_FP
    return fminf( fmaxf( d * k.mult + k.add, 0.0f ), 255.0f );
}

/* the texel-indexed table read bilinearly at (xf, xb), both in [0, 255]: exact float32 weights, taps clamped to 255,
 *   E = (1 - wb) ((1 - wf) T[i0][j0] + wf T[i1][j0]) + wb ((1 - wf) T[i0][j1] + wf T[i1][j1]) */
VRC_HD vrc_f4 vrc_preint_read( const vrc_f4* table, float xf, float xb )
{
    const float ff = floorf( xf ), fb = floorf( xb );
    const float wf = xf - ff, wb = xb - fb;
    const float vf = 1.0f - wf, vb = 1.0f - wb;
    const uint32_t i0 = (uint32_t)ff, j0 = (uint32_t)fb;
    const uint32_t i1 = i0 < 255u ? i0 + 1u : 255u, j1 = j0 < 255u ? j0 + 1u : 255u;
    const vrc_f4 t00 = table[i0 * VRC_PREINT_DIM + j0], t10 = table[i1 * VRC_PREINT_DIM + j0];
    const vrc_f4 t01 = table[i0 * VRC_PREINT_DIM + j1], t11 = table[i1 * VRC_PREINT_DIM + j1];
    vrc_f4 e;
    e.x = VRC_LERP2( vb, VRC_LERP2( vf, t00.x, wf, t10.x ), wb, VRC_LERP2( vf, t01.x, wf, t11.x ) );
    e.y = VRC_LERP2( vb, VRC_LERP2( vf, t00.y, wf, t10.y ), wb, VRC_LERP2( vf, t01.y, wf, t11.y ) );
    e.z = VRC_LERP2( vb, VRC_LERP2( vf, t00.z, wf, t10.z ), wb, VRC_LERP2( vf, t01.z, wf, t11.z ) );
    e.w = VRC_LERP2( vb, VRC_LERP2( vf, t00.w, wf, t10.w ), wb, VRC_LERP2( vf, t01.w, wf, t11.w ) );
    return e;
}

/* The table reads of a group: e[k] = the table's entry for the step that ends in sample k, by the value before it and its
 * own (VALUE: the stored bytes dv[]; otherwise the texel coordinates x[]).  carry: the value of the sample before the
 * group; first: the group opens a visit, whose sample 0 is paired with itself.  MASKED: only the first cnt >= 1 are the
 * reference's; the others read entry (0, 0), come out as zeros (an exact no-op in the blend) and do not move carry */
template < bool VALUE, int N, bool MASKED >
VRC_HD void vrc_preint_entries( const vrc_f4* __restrict__ table, uint32_t cnt, [[maybe_unused]] const float* x,
                                [[maybe_unused]] const uint32_t* dv, float& carry, bool& first, vrc_f4* e )
{
    const vrc_f4 z = { 0.f, 0.f, 0.f, 0.f };
    if constexpr( VALUE )
    {
        uint32_t before = first ? dv[0] : (uint32_t)carry;
        vrc_f4 t[N];
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
            const bool taken = !MASKED || (uint32_t)k < cnt;
            t[k] = table[taken ? before * VRC_PREINT_DIM + dv[k] : 0u];
            before = taken ? dv[k] : before;
        }
#pragma unroll
        for( int k = 0; k < N; ++k )
            e[k] = ( !MASKED || (uint32_t)k < cnt ) ? t[k] : z;
        carry = (float)before;
    }
    else
    {
        float before = first ? x[0] : carry;
#pragma unroll
        for( int k = 0; k < N; ++k )
        {
            const bool taken = !MASKED || (uint32_t)k < cnt;
            const vrc_f4 t = vrc_preint_read( table, taken ? before : 0.0f, taken ? x[k] : 0.0f );
            e[k] = taken ? t : z;
            before = taken ? x[k] : before;
        }
        carry = before;
    }
    first = false;
}

/* the pre-integrated mode of vrc_group_segment, for one brick visit: the front, then the table reads.  The previous value
 * is not carried from one brick visit to the next */
template < bool CLAMP, bool FIXED, bool TRILINEAR, bool VALUE, typename ATLAS_T >
struct vrc_preint_policy
{
    static_assert( !VALUE || ( !TRILINEAR && sizeof( ATLAS_T ) == 1 ), "the value-indexed table takes stored bytes" );
    static constexpr bool NOTES = false;
    const vrc_f4* __restrict__ table;
    const vrc_classifier& cls;
    float carry;
    bool first;

    template < int N, bool MASKED >
    VRC_HD void group( const vrc_sampler& sm, vrc_f3& pos, const vrc_f3& step, vrc_fixpos& fp,
                       const ATLAS_T* __restrict__ atlas, uint32_t cnt, vrc_f4* e )
    {
        typedef typename vrc_group_value< TRILINEAR, ATLAS_T >::type V;
        [[maybe_unused]] float x[N];     /* the texel coordinates of the samples, or (VALUE) ... */
        [[maybe_unused]] uint32_t dv[N]; /* ... their stored bytes */
        vrc_group_values< CLAMP, FIXED, TRILINEAR, ATLAS_T, N, MASKED, false >( sm, pos, step, fp, atlas, cnt, [&]( int k, V d ) {
            if constexpr( VALUE )
                dv[k] = (uint32_t)d;
            else
                x[k] = vrc_preint_coord( (float)d, cls );
        } );
        vrc_preint_entries< VALUE, N, MASKED >( table, cnt, x, dv, carry, first, e );
    }
};

/* One brick of one ray of a pre-integrated frame: vrc_brick_visit around its marches.  A slot of bytes known to hold one
 * value v is marched by the plain uniform march from lut[v] (the diagonal of the value-indexed table is a copy of that
 * table: E(v, v) for every sample of the visit); lut is read by that march alone */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, bool BIG, typename SRC >
VRC_HD bool vrc_preint_brick( const vrc_frame& f, const vrc_dev_node& n, const SRC& src, const ATLAS_T* __restrict__ atlas,
                              const vrc_f4* lut, const vrc_classifier& cls, vrc_f4& color, uint32_t& nSamples )
{
    static_assert( vrc_mode_is_preint( MODE ), "a pre-integrated mode" );
    constexpr bool TRILINEAR = MODE == VRC_MODE_PREINT_TRILINEAR;
    constexpr bool VALUE = !TRILINEAR && sizeof( ATLAS_T ) == 1;
    return vrc_brick_visit< BIG, VALUE >(
        f, n, src, atlas,
        [&]( const vrc_dev_node& m, const vrc_segment& s, const ATLAS_T* __restrict__ a, uint32_t v ) {
            return vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, VRC_GROUP, vrc_f4, false, true >(
                f, m, s, a, lut, color, nSamples, 0.0f, nullptr, lut[v] );
        },
        [&]( const vrc_dev_node& m, const vrc_segment& s, const ATLAS_T* __restrict__ a ) {
            vrc_preint_policy< CLAMP, FIXED, TRILINEAR, VALUE, ATLAS_T > p = { f.preintTable, cls, 0.0f, true };
            return vrc_group_segment< COUNT, FIXED, VALUE ? VRC_PREINT_GROUP : VRC_PREINT_GROUP_TEXEL >( f, m, s, a, p, color,
                                                                                                         nSamples );
        } );
}

/* ------------------------------------------------------------------------------------------
 * One brick of one ray of a shaded or a depth-tracking frame: vrc_brick_visit around the mode's marches.  dir: the ray's unit
 * direction (the shaded modes); cdepth: the ray's crossing state (the depth-tracking modes).
 * A slot of bytes known to hold one value v is marched from lut[v] by the plain uniform march: there a shaded frame has
 * G = 0 and s = 1; the depth-tracking modes find the crossing in it as well (vrc_cdepth_uniform).
 * ---------------------------------------------------------------------------------------- */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, bool BIG, typename SRC >
VRC_HD bool vrc_extension_brick( const vrc_frame& f, const vrc_dev_node& n, const SRC& src, [[maybe_unused]] const vrc_f3& dir,
                                 const ATLAS_T* __restrict__ atlas, const vrc_f4* lut, const vrc_classifier& cls,
                                 vrc_f4& color, uint32_t& nSamples, [[maybe_unused]] vrc_cdepth_state* cdepth )
{
    static_assert( vrc_mode_is_shade( MODE ) || vrc_mode_is_cdepth( MODE ), "a shaded or a depth-tracking mode" );
    constexpr bool TRILINEAR = MODE == VRC_MODE_SHADE_TRILINEAR || MODE == VRC_MODE_CDEPTH_TRILINEAR;
    constexpr bool BYTES = !TRILINEAR && sizeof( ATLAS_T ) == 1; /* the forms that look at the slot's word */
    [[maybe_unused]] const auto plain = [&]( const vrc_dev_node& m, const vrc_segment& s, const ATLAS_T* __restrict__ a,
                                             uint32_t v ) {
        return vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, VRC_GROUP, vrc_f4, false, true >(
            f, m, s, a, lut, color, nSamples, 0.0f, nullptr, lut[v] );
    };
    if constexpr( vrc_mode_is_shade( MODE ) )
        return vrc_brick_visit< BIG, BYTES >(
            f, n, src, atlas, plain, [&]( const vrc_dev_node& m, const vrc_segment& s, const ATLAS_T* __restrict__ a ) {
                vrc_shade_policy< CLAMP, FIXED, TRILINEAR, !BYTES, ATLAS_T > p = { f, lut, cls, dir };
                return vrc_group_segment< COUNT, FIXED, VRC_SHADE_GROUP >( f, m, s, a, p, color, nSamples );
            } );
    else
    {
        constexpr int GROUP = TRILINEAR          ? VRC_CDEPTH_GROUP_TRILINEAR
                              : BYTES && !CLAMP ? VRC_CDEPTH_GROUP
                                                : VRC_CDEPTH_GROUP_CLASSIFIED;
        return vrc_brick_visit< BIG, BYTES >(
            f, n, src, atlas,
            [&]( const vrc_dev_node&, const vrc_segment& s, const ATLAS_T*, uint32_t v ) {
                return vrc_cdepth_uniform< COUNT >( f, s, lut[v], v, color, nSamples, *cdepth );
            },
            [&]( const vrc_dev_node& m, const vrc_segment& s, const ATLAS_T* __restrict__ a ) {
                vrc_cdepth_policy< CLAMP, FIXED, TRILINEAR, !BYTES, ATLAS_T, GROUP > p = { lut,     cls,        *cdepth, f.cdepthTau,
                                                                                         s.tNear, f.stepSize, {} };
                return vrc_group_segment< COUNT, FIXED, GROUP >( f, m, s, a, p, color, nSamples );
            } );
    }
}

/* ------------------------------------------------------------------------------------------
 * Reference-order pixel: the O(nodeCount) loop of Renderer.cu:172-227, nodes in host order.
 * ---------------------------------------------------------------------------------------- */
/* MODE: how a sample is fetched and classified.
 *   VRC_MODE_TABLE      point sample of a u8 volume through the classified table (257 entries):
 *                       the reference path;
 *   VRC_MODE_TRILINEAR  trilinear fetch, per-sample classification (lut = padded transfer function);
 *   VRC_MODE_POINT      point sample, per-sample classification (16-bit voxels). */
#define VRC_MODE_GREY 3 /* VRC_MODE_TABLE with a grey transfer function (r == g == b in every entry): two-float table
                         * entries and colours, bit-identical frames, half the table bytes and blend work */
#define VRC_MODE_POINT_GREY 4 /* VRC_MODE_POINT with a grey transfer function, as VRC_MODE_GREY is to VRC_MODE_TABLE */
#define VRC_MODE_TABLE 0
#define VRC_MODE_TRILINEAR 1
#define VRC_MODE_POINT 2
#define VRC_MODE_PACKED 5      /* trilinear through the tap-packed atlas (vrc_march_segment_packed): ATLAS_T = uint32_t,
                                * lut = the vrc_cls8_entry table */
#define VRC_MODE_PACKED_GREY 6 /* the same for a grey transfer function: (grey, alpha) colours, paired table entries */
#define VRC_MODE_WALK_RECORD 9 /* no march: the grid walk records its visits (vrc_frame::walkCache; 7 and 8 are the MIP modes) */

/* BIG: the atlas holds more than 2^32 voxels.  Offsets inside a slot stay 32-bit; the slot's
 * 64-bit base moves into the lane's atlas pointer (one 64-bit add per gather instead of a 32-bit
 * one), so the default kernels keep their scalar base + 32-bit offset addressing. */
/* SRC: vrc_segment_ready, vrc_segment_from_interval or vrc_segment_from_walk.  One body for all: the slot word, its ballot and every march are
 * where they were; only the place the segment's arithmetic is done differs */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP, bool BIG, typename SRC >
VRC_HD bool vrc_march_brick_from( const vrc_frame& f, const vrc_dev_node& n, const SRC& src,
                                  const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                                  const vrc_classifier& cls, vrc_f4& color, uint32_t& nSamples,
                                  float levelStep )
{
    if constexpr( MODE == VRC_MODE_PACKED || MODE == VRC_MODE_PACKED_GREY )
    {
        const vrc_segment& s = src.full();
        /* (BIG here: a packed atlas of more than 4 GiB, or of an atlas of more than 2^32 voxels -- 64-bit lane pointers.
         * ATLAS_T is a tag: uint32_t = the packed form of 8-bit voxels, uint64_t = of 16-bit voxels) */
        static_assert( ( sizeof( ATLAS_T ) == 4 || sizeof( ATLAS_T ) == 8 ) && !CLAMP, "the packed atlas: overlap >= 1" );
        constexpr int TB = sizeof( ATLAS_T ) == 8 ? 4 : 2;
        const vrc_cls8 kc = vrc_make_cls8( cls );
        if constexpr( MODE == VRC_MODE_PACKED_GREY )
        {
            vrc_f2 c = { color.x, color.w };
            const bool done = vrc_march_segment_packed< COUNT, GROUP, vrc_f2, BIG, TB >( f, n, s, atlas, lut, kc, c, nSamples, levelStep );
            color.x = color.y = color.z = c.x;
            color.w = c.w;
            return done;
        }
        else
            return vrc_march_segment_packed< COUNT, GROUP, vrc_f4, BIG, TB >( f, n, s, atlas, lut, kc, color, nSamples, levelStep );
    }
    else if( BIG )
    {
        vrc_dev_node local = n;
        local.slotBase = 0u;
        const ATLAS_T* slot = atlas + ( ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase );
        return vrc_march_brick_from< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, false, SRC >( f, local, src, slot, lut, cls,
                                                                                          color, nSamples, levelStep );
    }
    if constexpr( ( MODE == VRC_MODE_TABLE || MODE == VRC_MODE_GREY ) && sizeof( ATLAS_T ) == 1 )
    {
        /* A brick whose upload found one value in every voxel (the slot's uniformity word, written by the repack kernel
         * on the stream and under the fences of the voxels themselves) is marched from that value's table entry: no
         * addresses, no gathers, no table reads.  Taken by the whole wave or not at all -- a lane in a uniform brick
         * of a wave that also holds other bricks gathers its constant voxels like the rest, the same samples either
         * way.  Trilinear, 16-bit and per-sample classified forms do not look at the word. */
        uint32_t word = 0u;
        if( f.slotInfo != nullptr && n.slotInfoIndex != 0u )
            word = f.slotInfo[n.slotInfoIndex - 1u];
        bool general = !vrc_slot_holds_one_value( word );
#if defined( __HIP_DEVICE_COMPILE__ )
        general = __builtin_amdgcn_ballot_w64( general ) != 0ull;
#endif
        if( !general )
        {
            const vrc_segment& s = src.distOnly();
            const uint32_t v = word & 0xFFu;
            if constexpr( MODE == VRC_MODE_GREY )
            {
                const vrc_f2* const lut2 = reinterpret_cast< const vrc_f2* >( lut );
                vrc_f2 c = { color.x, color.w };
                const bool done = vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, GROUP, vrc_f2, false, true >(
                    f, n, s, atlas, lut2, c, nSamples, levelStep, nullptr, lut2[v] );
                color.x = color.y = color.z = c.x;
                color.w = c.w;
                return done;
            }
            else
                return vrc_march_segment_as< CLAMP, COUNT, FIXED, ATLAS_T, GROUP, vrc_f4, false, true >(
                    f, n, s, atlas, lut, color, nSamples, levelStep, nullptr, lut[v] );
        }
    }
    const vrc_segment& s = src.full();
    if constexpr( MODE == VRC_MODE_GREY )
        return vrc_march_segment< CLAMP, COUNT, FIXED, ATLAS_T, GROUP, true >( f, n, s, atlas, lut, color, nSamples,
                                                                             levelStep );
    else if constexpr( MODE == VRC_MODE_POINT_GREY )
    {
        /* lut holds the padded transfer function as (grey, alpha) pairs; the pixel came in grey and leaves grey */
        vrc_f2 c = { color.x, color.w };
        const bool done = vrc_march_segment_as< CLAMP, COUNT, true, ATLAS_T, GROUP, vrc_f2, true >(
            f, n, s, atlas, reinterpret_cast< const vrc_f2* >( lut ), c, nSamples, levelStep, &cls );
        color.x = color.y = color.z = c.x;
        color.w = c.w;
        return done;
    }
    else if constexpr( MODE == VRC_MODE_POINT && FIXED )
        /* point sampling with per-sample classification (16-bit voxels) through the grouped march of the table
         * form: whole groups without per-sample masks, fixed-point stepping, address tables; only the table read
         * is replaced by vrc_classify */
        return vrc_march_segment_as< CLAMP, COUNT, true, ATLAS_T, GROUP, vrc_f4, true >( f, n, s, atlas, lut, color,
                                                                                       nSamples, levelStep, &cls );
    else if constexpr( MODE != VRC_MODE_TABLE )
        return vrc_march_segment_linear< CLAMP, COUNT, MODE == VRC_MODE_TRILINEAR, ATLAS_T >(
            f, n, s, atlas, lut, cls, color, nSamples, levelStep );
    else
        return vrc_march_segment< CLAMP, COUNT, FIXED, ATLAS_T, GROUP >( f, n, s, atlas, lut, color, nSamples,
                                                                       levelStep );
}

template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD bool vrc_march_brick( const vrc_frame& f, const vrc_dev_node& n, const vrc_segment& s,
                             const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                             const vrc_classifier& cls, vrc_f4& color, uint32_t& nSamples,
                             float levelStep = 0.0f )
{
    const vrc_segment_ready src = { s };
    return vrc_march_brick_from< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG, vrc_segment_ready >(
        f, n, src, atlas, lut, cls, color, nSamples, levelStep );
}

/* ... on a brick interval of the frame's step: the segment is completed where the march needs it */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD bool vrc_march_brick( const vrc_frame& f, const vrc_dev_node& n, const vrc_ray& r, const vrc_interval& iv,
                             const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                             const vrc_classifier& cls, vrc_f4& color, uint32_t& nSamples )
{
#if defined( VRC_WALK_VISIT_HOOK ) && !defined( __HIPCC__ )
    /* host test builds only (tests/cpu_harness/walk_cache_harness.cpp): every visit the walk hands to a march */
    VRC_WALK_VISIT_HOOK( n, r, iv );
#endif
    const vrc_segment_from_interval src = { r, iv, f.stepSize };
    return vrc_march_brick_from< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG, vrc_segment_from_interval >(
        f, n, src, atlas, lut, cls, color, nSamples, 0.0f );
}

/* ---- tile culling for the reference-order loop -------------------------------------------------------------
 * The reference tests every brick of the list against every ray (Renderer.cu:172-181).  A wave is an 8x8 pixel
 * tile: the bricks none of its rays can hit are found once per wave -- 64 bricks per step against the pyramid
 * through the tile's corner pixels (one pixel of margin) -- and the lanes then run the reference's loop over the
 * remaining bricks, in the list's order, with the reference's own slab test per ray.  A brick that is not hit is a
 * `continue` in the reference (the hit test comes before the `break` test, :181-186), so leaving it out changes
 * nothing: same bricks marched, same order, same samples. */
struct vrc_tile_pyramid
{
    vrc_f3 eye;
    vrc_f3 n[4]; /* inward normals of the four side planes through the eye */
};
VRC_HD vrc_f3 vrc_pixel_direction( const vrc_frame& f, float wx, float wy )
{
    const float nx = 2.0f * ( wx + f.pixelOffX - f.vpX - ( f.vpW / 2.0f ) ) / f.vpW;
    const float ny = 2.0f * ( wy + f.pixelOffY - f.vpY - ( f.vpH / 2.0f ) ) / f.vpH;
    const vrc_f4 ndc = { nx, ny, 1.0f, 1.0f };
    const vrc_f4 e = vrc_mul44( f.invProj, ndc );
    const vrc_f4 eyeSpace = { e.x / e.w, e.y / e.w, e.z / e.w, 1.0f };
    const vrc_f4 world = vrc_mul44( f.invView, eyeSpace );
    const vrc_f3 d = { world.x - f.eye[0], world.y - f.eye[1], world.z - f.eye[2] };
    return d;
}
VRC_HD vrc_f3 vrc_cross( vrc_f3 a, vrc_f3 b )
{
    const vrc_f3 c = { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x };
    return c;
}
/* pixels [x0, x1] x [y0, y1] (window coordinates of pixel corners, frame rows) */
VRC_HD vrc_tile_pyramid vrc_make_tile_pyramid( const vrc_frame& f, float x0, float y0, float x1, float y1 )
{
    vrc_tile_pyramid p;
    p.eye.x = f.eye[0];
    p.eye.y = f.eye[1];
    p.eye.z = f.eye[2];
    const vrc_f3 d[4] = { vrc_pixel_direction( f, x0, y0 ), vrc_pixel_direction( f, x1, y0 ),
                          vrc_pixel_direction( f, x1, y1 ), vrc_pixel_direction( f, x0, y1 ) };
    for( int k = 0; k < 4; ++k )
    {
        vrc_f3 n = vrc_cross( d[k], d[( k + 1 ) & 3] );
        if( vrc_dot( n, d[( k + 2 ) & 3] ) < 0.0f ) /* whichever way the projection winds the corners */
        {
            n.x = -n.x;
            n.y = -n.y;
            n.z = -n.z;
        }
        p.n[k] = n;
    }
    return p;
}
/* false: the box lies entirely outside one side plane, no ray of the tile can hit it */
VRC_HD bool vrc_pyramid_may_hit( const vrc_tile_pyramid& p, const float bmin[3], const float bsize[3] )
{
    const float lo[3] = { bmin[0] - p.eye.x, bmin[1] - p.eye.y, bmin[2] - p.eye.z };
    const float hi[3] = { lo[0] + bsize[0], lo[1] + bsize[1], lo[2] + bsize[2] };
    for( int k = 0; k < 4; ++k )
    {
        const float nn[3] = { p.n[k].x, p.n[k].y, p.n[k].z };
        float s = 0.0f, mag = 0.0f;
        for( int a = 0; a < 3; ++a )
        {
            const float u = nn[a] * lo[a], v = nn[a] * hi[a];
            s += u > v ? u : v;
            mag += ( u < 0.f ? -u : u ) + ( v < 0.f ? -v : v );
        }
        if( s < -1e-5f * mag ) /* the vertex furthest inside is outside, by more than rounding */
            return false;
    }
    return true;
}
#define VRC_TILE_CANDIDATES 1024u /* per wave; a tile that could hit more runs the plain loop */

/* glRaycaster with nSamplesPerPixel > 1 (fragRaycast.glsl:113-215; one draw per brick, in the host's order): for
 * every brick the fragment casts n rays through gl_FragCoord + (rand, rand) / 2, each marches THIS brick starting
 * from the pixel's colour so far, and the pixel becomes the average of the n results (:212-214).  A `discard` inside
 * the loop (a sub-ray that misses the volume or the brick, :140-143, :159-160, :176-177) discards the fragment: the
 * brick then leaves the pixel as it was.  Sub-sample 0 has rand(0,0) = 0: the pixel centre. */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD void vrc_pixel_gl_supersampled( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                       const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                                       const vrc_classifier& cls, vrc_f4* __restrict__ pixelBuffer, uint32_t px,
                                       uint32_t py, uint32_t& nSamples, const uint16_t* candidates,
                                       uint32_t nCandidates )
{
    VRC_STRICT_FP
    const uint32_t row = f.rowMap ? f.rowMap[py] : py;
    const uint32_t pixelPos = py * f.width + px;
    const float fx = (float)px + f.pixelOffX, fy = (float)row + f.pixelOffY; /* gl_FragCoord.xy */
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    vrc_f4 color = f.clearFirst ? zero : pixelBuffer[pixelPos];
    const uint32_t n = f.samplesPerPixel;
    const float fn = (float)n;
    const uint32_t nLoop = candidates ? nCandidates : f.nodeCount;
    for( uint32_t c = 0; c < nLoop; ++c )
    {
        if( color.w > VRC_EARLY_EXIT ) /* :115-117: this and every later brick's fragment is discarded */
            break;
        const uint32_t i = candidates ? (uint32_t)candidates[c] : c;
        const vrc_dev_node node = nodes[i];
        vrc_f4 sum = zero;
        bool discard = false;
        uint32_t cnt = 0;
        for( uint32_t k = 0; k < n; ++k )
        {
            const float fk = (float)k;
            const float dx = vrc_gl_rand( fx * fk, fy * fk ) / 2.0f;
            const float dy = vrc_gl_rand( fx * 2.0f * fk, fy * 2.0f * fk ) / 2.0f;
            const vrc_ray r = vrc_setup_ray_at( f, fx + dx, fy + dy );
            vrc_segment s;
            bool stop;
            if( !r.hit || !vrc_brick_segment( f, r, node, f.stepSize, &s, &stop ) )
            {
                discard = true;
                break;
            }
            vrc_f4 local = color;
            (void)vrc_march_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, node, s, atlas, lut, cls, local, cnt );
            sum.x += local.x;
            sum.y += local.y;
            sum.z += local.z;
            sum.w += local.w;
        }
        if( !discard )
        {
            color.x = sum.x / fn;
            color.y = sum.y / fn;
            color.z = sum.z / fn;
            color.w = sum.w / fn;
            if( COUNT )
                nSamples += cnt;
        }
    }
    pixelBuffer[pixelPos] = color;
}

template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD void vrc_pixel_reference_order( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                       const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                                       const vrc_classifier& cls,
                                       vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py,
                                       uint32_t& nSamples, const uint16_t* candidates = nullptr,
                                       uint32_t nCandidates = 0, vrc_cdepth_state* cdepth = nullptr )
{
    /* (cdepth: the ray's crossing state, the depth-tracking composite modes only) */
    if constexpr( !vrc_mode_is_shade( MODE ) && !vrc_mode_is_cdepth( MODE ) && !vrc_mode_is_preint( MODE ) ) /* (a shaded frame is defined on the cudaRaycaster variant's sample set) */
        if( f.variant == VRC_VARIANT_GL && f.samplesPerPixel > 1u )
        {
            vrc_pixel_gl_supersampled< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, nodes, atlas, lut, cls, pixelBuffer,
                                                                                       px, py, nSamples, candidates, nCandidates );
            return;
        }
    const vrc_ray r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    if( !r.hit )
    {
        if( f.clearFirst )
            pixelBuffer[pixelPos] = zero;
        return; /* Renderer.cu:129-130, :148-149: pixel left untouched (= cleared) */
    }
    vrc_f4 color = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( color.w > VRC_EARLY_EXIT ) /* Renderer.cu:152-155 */
        return;
    /* candidates: the bricks of the list a ray of this wave's tile can hit, in list order (tile culling, above) */
    const uint32_t nLoop = candidates ? nCandidates : f.nodeCount;
    for( uint32_t c = 0; c < nLoop; ++c )
    {
        const uint32_t i = candidates ? (uint32_t)candidates[c] : c;
        const vrc_dev_node n = nodes[i];
        vrc_segment s;
        bool stop;
        if( !vrc_brick_segment( f, r, n, f.stepSize, &s, &stop ) )
        {
            if( stop )
                break;
            continue;
        }
        if constexpr( vrc_mode_is_shade( MODE ) || vrc_mode_is_cdepth( MODE ) )
        {
            const vrc_segment_ready src = { s };
            if( vrc_extension_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, BIG, vrc_segment_ready >( f, n, src, r.dir, atlas, lut,
                                                                                                  cls, color, nSamples, cdepth ) )
                break;
        }
        else if constexpr( vrc_mode_is_preint( MODE ) )
        {
            const vrc_segment_ready src = { s };
            if( vrc_preint_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, BIG, vrc_segment_ready >( f, n, src, atlas, lut, cls, color,
                                                                                               nSamples ) )
                break;
        }
        else if( vrc_march_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, n, s, atlas, lut, cls, color,
                                                                     nSamples ) )
            break;
    }
    pixelBuffer[pixelPos] = color; /* Renderer.cu:229 */
}

/* ------------------------------------------------------------------------------------------
 * Grid-DDA pixel: same per-brick arithmetic, but the bricks a ray meets are enumerated by a
 * 3-D DDA over the brick grid (cell -> node index table) instead of testing every node.
 * For a regular single-LOD grid the along-ray order equals the reference's host order for
 * every pair of bricks that share a ray ("brick order").
 * ---------------------------------------------------------------------------------------- */
/* the axis the view looks along most, and which way: the slabs of vrc_ray_grid_dda's parts */
VRC_HD int vrc_part_dir( const vrc_frame& f )
{
    const vrc_ray c = vrc_setup_ray( f, f.width / 2u, (uint32_t)( f.vpH * 0.5f ) );
    const float ax = c.dir.x < 0.f ? -c.dir.x : c.dir.x, ay = c.dir.y < 0.f ? -c.dir.y : c.dir.y,
                az = c.dir.z < 0.f ? -c.dir.z : c.dir.z;
    const int a = ax >= ay && ax >= az ? 0 : ( ay >= az ? 1 : 2 );
    const float d = a == 0 ? c.dir.x : ( a == 1 ? c.dir.y : c.dir.z );
    return a | ( d < 0.f ? 4 : 0 );
}

/* The walk of one prepared ray; color is read-modify-write.  part: -1 = every brick the ray meets; 0 .. parts-1 =
 * only the bricks met in that one of `parts` equal slabs of the brick grid along axis partDir & 3, counted in the
 * direction the view looks along it (partDir & 4: towards smaller coordinates; vrc_part_dir).  The slab is a
 * property of the grid cell, the same for every ray: the lanes of a wave agree on which launch marches a brick.
 * partDir < 0 (two parts): the halves of the ray's own interval inside the grid instead.
 * Every brick is marched whole in exactly one part, and a brick's part never falls below that of a brick met
 * before it, so marching the parts one after the other composites the reference's samples in the reference's
 * order.  Two users: the depth split (two waves march the two halves of a tile's rays at the same time and the
 * halves are composited with `over`) and ray compaction (VRC_OPT_ERT_COMPACTION: one launch per part, the rays
 * that early termination has not ended are packed into full waves for the next).
 * Returns whether the ray is still alive (it meets the grid and its opacity is below the early-exit threshold). */
template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD bool vrc_ray_grid_dda( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node* __restrict__ nodes,
                              const int32_t* __restrict__ gridTable, const ATLAS_T* __restrict__ atlas,
                              const vrc_f4* lut, const vrc_classifier& cls, vrc_f4& color, uint32_t& nSamples,
                              int part = -1, int parts = 2, int partDir = 2, uint32_t* walkOut = nullptr,
                              vrc_cdepth_state* cdepth = nullptr )
{
    /* (cdepth: the ray's crossing state, the depth-tracking composite modes only) */
    /* (walkOut: VRC_MODE_WALK_RECORD only -- the ray's word of the walk cache's plane 0; nSamples then counts visits) */
    /* ray interval inside the brick grid */
    const vrc_f3 gmin = { f.gridMin[0], f.gridMin[1], f.gridMin[2] };
    const vrc_f3 gmax = { f.gridMin[0] + f.cellSize[0] * (float)f.gridDim[0],
                          f.gridMin[1] + f.cellSize[1] * (float)f.gridDim[1],
                          f.gridMin[2] + f.cellSize[2] * (float)f.gridDim[2] };
    float t0, t1;
    bool any = vrc_intersect_box( r.origin, r.invDir, gmin, gmax, &t0, &t1 );
    /* the GLSL twin does not clamp a brick's interval to the global box (fragRaycast.glsl:149-150):
     * bricks of the tree that reach past the volume (ragged trees) are sampled there too */
    if( f.variant == VRC_VARIANT_GL )
        t0 = fmaxf( t0, fmaxf( r.tNearPlane, 0.0f ) );
    else
    {
        t0 = fmaxf( fmaxf( t0, r.tNearGlobal ), fmaxf( r.tNearPlane, 0.0f ) );
        t1 = fminf( t1, r.tFarGlobal );
    }
    if( any && t0 <= t1 )
    {
        const float o[3] = { r.origin.x, r.origin.y, r.origin.z };
        const float d[3] = { r.dir.x, r.dir.y, r.dir.z };
        const float id[3] = { r.invDir.x, r.invDir.y, r.invDir.z };
        /* Which bricks does the ray meet?  Those of the cells it runs through -- and, where it enters or leaves
         * a cell through an edge or a corner of the grid (two or three of the entry / exit parameters equal
         * to within rounding), the bricks of the cells around that edge or corner.  In exact arithmetic the
         * ray has no extent in those; the reference tests every brick with its float slab test
         * (Renderer.cu:56-80, :179-181), and one that comes out with tfar a last bit above tnear gets its one
         * sample (:208).  Handing the same cells to the same arithmetic (vrc_brick_segment) reproduces that,
         * instead of depending on which of the tied faces this walk happens to cross first: the walk
         * composites the reference's samples, one for one. */
        int cell[3], stepDir[3];
        float tMax[3], tDelta[3];
        const float tolE = fabsf( t0 ) * 2e-6f;
        uint32_t back = 0u; /* axes on whose cell faces the ray is at t0: it also touches the cells behind them */
#pragma unroll
        for( int a = 0; a < 3; ++a )
        {
            const float p = o[a] + d[a] * t0;
            const float u = ( p - f.gridMin[a] ) * f.invCellSize[a];
            const bool pos = d[a] > 0.0f;
            stepDir[a] = pos ? 1 : -1;
            /* on a cell face at t0 (the ray enters the grid through an edge, or starts on a face): the walk
             * starts in the cell the ray goes on into, so that no cell is left at the parameter it was
             * entered at */
            const float kf = rintf( u );
            const float tFace = ( ( f.gridMin[a] + f.cellSize[a] * kf ) - o[a] ) * id[a];
            int c = (int)floorf( u );
            const int cOn = (int)kf - ( pos ? 0 : 1 );
            if( fabsf( tFace - t0 ) <= tolE && cOn >= 0 && cOn <= f.gridDim[a] - 1 )
            {
                c = cOn;
                back |= 1u << a;
            }
            c = c < 0 ? 0 : ( c > f.gridDim[a] - 1 ? f.gridDim[a] - 1 : c );
            cell[a] = c;
            const float boundary = f.gridMin[a] + f.cellSize[a] * (float)( pos ? c + 1 : c );
            tMax[a] = ( boundary - o[a] ) * id[a];
            tDelta[a] = f.cellSize[a] * fabsf( id[a] );
        }
        /* bricks already handed to the slab test: a brick is convex, once left it is never entered again,
         * but a coarse brick that spans several cells is met in each of them */
        int32_t recent[4] = { -1, -1, -1, -1 };
        const int maxSteps = f.gridDim[0] + f.gridDim[1] + f.gridDim[2] + 3;
        bool finished = false;
        int lastPart = 0;
        auto visit = [&]( int cx, int cy, int cz ) {
            const int32_t node = gridTable[( cz * f.gridDim[1] + cy ) * f.gridDim[0] + cx];
            if( node < 0 || node == recent[0] || node == recent[1] || node == recent[2] || node == recent[3] )
                return;
            recent[3] = recent[2];
            recent[2] = recent[1];
            recent[1] = recent[0];
            recent[0] = node;
            const vrc_dev_node n = nodes[node];
            vrc_interval iv;
            bool stop;
            if( vrc_brick_interval( f, r, n, f.stepSize, &iv, &stop ) )
            {
                if( part >= 0 )
                {
                    int sp;
                    if( partDir < 0 )
                        /* by ray parameter: the brick's segment starts in the near / far half of THIS ray's interval
                         * inside the grid -- halves of equal length for every ray (what the depth split wants: the
                         * longer half is the latency), at the price that the lanes of a wave disagree about the
                         * brick the middle falls into */
                        sp = iv.tNear < 0.5f * ( t0 + t1 ) ? 0 : 1; /* (the segment's tNear) */
                    else
                    {
                        const int ax = partDir & 3;
                        const int dim = f.gridDim[ax];
                        const int c = ax == 0 ? cx : ( ax == 1 ? cy : cz );
                        sp = ( ( ( partDir & 4 ) ? dim - 1 - c : c ) * parts ) / dim;
                    }
                    sp = sp > lastPart ? sp : lastPart;
                    lastPart = sp;
                    if( sp > part )
                        finished = true; /* nothing of this part lies behind a brick of a later one */
                    if( sp != part )
                        return; /* another part's brick */
                }
                if constexpr( MODE == VRC_MODE_WALK_RECORD )
                {
                    /* where every other mode marches: the visit is stored (the count pass, walkK = 0, stores none) and
                     * counted; nothing ends the list but `stop` and the end of the walk */
                    if( nSamples < f.walkK )
                    {
                        uint32_t* const w = walkOut + ( 1u + 4u * nSamples ) * f.walkPlane;
                        w[0] = (uint32_t)node;
                        const float dist = vrc_segment_dist( r, iv );
                        uint32_t second = vrc_float_bits( dist );
                        if( f.walkLean != 0u ) /* (the count pass found that every visit packs) */
                            (void)vrc_walk_lean_word( dist, f.stepSize, n.slotInfoIndex, &second );
                        w[f.walkPlane] = second;
                        w[2u * f.walkPlane] = vrc_float_bits( iv.tNear );
                        w[3u * f.walkPlane] = vrc_float_bits( iv.tFar );
                    }
                    else if( f.walkK == 0u )
                    {
                        /* the count pass also says how many of the visits meet a brick that vrc_march_brick_from would
                         * gather (color.x, otherwise unused here, carries the number): the host keeps a view of mostly
                         * such visits on the walk.  Nothing of the lists depends on it */
                        uint32_t word = 0u;
                        if( f.slotInfo != nullptr && n.slotInfoIndex != 0u )
                            word = f.slotInfo[n.slotInfoIndex - 1u];
                        if( !vrc_slot_holds_one_value( word ) )
                            color.x += 1.0f; /* (exact: a ray visits far fewer than 2^24 bricks) */
                        /* ... and, asked by walkLean, whether a visit fails to pack (color.y != 0) */
                        uint32_t packed;
                        if( f.walkLean != 0u &&
                            !vrc_walk_lean_word( vrc_segment_dist( r, iv ), f.stepSize, n.slotInfoIndex, &packed ) )
                            color.y = 1.0f;
                    }
                    ++nSamples;
                }
                else if constexpr( vrc_mode_is_mip( MODE ) )
                {
                    vrc_segment s;
                    vrc_segment_complete( r, iv, f.stepSize, &s );
                    if( vrc_mip_brick< CLAMP, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, n, s, atlas, color, nSamples, (uint32_t)node ) ) /* (color: the ray's MIP state) */
                        finished = true; /* (an isosurface frame: every brick from here on lies behind the ray's hit) */
                }
                else if constexpr( vrc_mode_is_shade( MODE ) || vrc_mode_is_cdepth( MODE ) )
                {
                    const vrc_segment_from_interval src = { r, iv, f.stepSize };
                    if( vrc_extension_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, BIG, vrc_segment_from_interval >(
                            f, n, src, r.dir, atlas, lut, cls, color, nSamples, cdepth ) )
                        finished = true;
                }
                else if constexpr( vrc_mode_is_preint( MODE ) )
                {
                    const vrc_segment_from_interval src = { r, iv, f.stepSize };
                    if( vrc_preint_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, BIG, vrc_segment_from_interval >(
                            f, n, src, atlas, lut, cls, color, nSamples ) )
                        finished = true;
                }
                else if( vrc_march_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, n, r, iv, atlas, lut, cls, color,
                                                                                       nSamples ) )
                    finished = true;
            }
            else if( stop )
                finished = true;
        };
        /* work list of the cells around an edge / corner, one bit per cell, in the order they are met:
         *   bits 0-6   cell - (subset of the entry-tied axes): subsets 7, 3, 5, 6, 1, 2, 4
         *   bits 8-13  cell + (proper subset of the exit-tied axes): subsets 1, 2, 4, 3, 5, 6
         * the 64-bit constants hold, per 3-bit axis set, the bits whose subset lies inside it */
        uint32_t pending = (uint32_t)( ( 0x7F68544032201000ull >> ( back * 8u ) ) & 0x7Fu );
        uint32_t tied = 0u; /* axes whose faces the ray leaves the current cell through */
        bool multi = false; /* more than one of them */
        for( int it = 0; it < maxSteps; ++it )
        {
            /* rare, and taken by the whole wave or not at all: the cells around the edge / corner the ray
             * entered the first cell through (first iteration) or left the last cell through */
            bool rare = pending != 0u || multi;
#if defined( __HIP_DEVICE_COMPILE__ )
            rare = __builtin_amdgcn_ballot_w64( rare ) != 0ull;
#endif
            if( rare )
            {
                if( multi )
                    pending |= (uint32_t)( ( 0x3F06050003000000ull >> ( tied * 8u ) ) & 0x3Fu ) << 8;
                while( pending != 0u && !finished )
                {
#if defined( __HIP_DEVICE_COMPILE__ )
                    const uint32_t slot = (uint32_t)__builtin_ctz( pending );
#else
                    uint32_t slot = 0;
                    while( !( ( pending >> slot ) & 1u ) )
                        ++slot;
#endif
                    pending &= pending - 1u;
                    const uint32_t sub = slot < 7u ? ( 0x4216537u >> ( slot * 4u ) ) & 7u
                                                   : ( 0x653421u >> ( ( slot - 8u ) * 4u ) ) & 7u;
                    const int sgn = slot < 7u ? -1 : 1;
                    const int cx = cell[0] + ( ( sub & 1u ) ? sgn * stepDir[0] : 0 );
                    const int cy = cell[1] + ( ( sub & 2u ) ? sgn * stepDir[1] : 0 );
                    const int cz = cell[2] + ( ( sub & 4u ) ? sgn * stepDir[2] : 0 );
                    if( cx >= 0 && cx < f.gridDim[0] && cy >= 0 && cy < f.gridDim[1] && cz >= 0 && cz < f.gridDim[2] )
                        visit( cx, cy, cz );
                }
                pending = 0u;
            }
            if( finished )
                break;
            /* through every tied face at once */
            if( tied & 1u )
            {
                cell[0] += stepDir[0];
                tMax[0] += tDelta[0];
            }
            if( tied & 2u )
            {
                cell[1] += stepDir[1];
                tMax[1] += tDelta[1];
            }
            if( tied & 4u )
            {
                cell[2] += stepDir[2];
                tMax[2] += tDelta[2];
            }
            if( cell[0] < 0 || cell[0] >= f.gridDim[0] || cell[1] < 0 || cell[1] >= f.gridDim[1] ||
                cell[2] < 0 || cell[2] >= f.gridDim[2] )
                break;
            visit( cell[0], cell[1], cell[2] );
            if( finished )
                break;
            const float tNext = fminf( fminf( tMax[0], tMax[1] ), tMax[2] );
            if( tNext > t1 ) /* the ray ends inside this cell */
                break;
            const float thr = tNext + fabsf( tNext ) * 2e-6f;
            tied = ( tMax[0] <= thr ? 1u : 0u ) | ( tMax[1] <= thr ? 2u : 0u ) | ( tMax[2] <= thr ? 4u : 0u );
            multi = ( tied & ( tied - 1u ) ) != 0u;
        }
        return !( color.w > VRC_EARLY_EXIT );
    }
    return false;
}

template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD void vrc_pixel_grid_dda( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                const int32_t* __restrict__ gridTable,
                                const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                                const vrc_classifier& cls,
                                vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py,
                                uint32_t& nSamples, uint32_t rayIndex = 0u, vrc_cdepth_state* cdepth = nullptr )
{
    /* rayIndex: tile * 64 + lane, the pixel's word in every plane of the ray cache (vrc_frame::rayCache; read only when
     * f.rayMode is not 0).  The mode is a frame constant, so the whole wave takes one side.  Both sides end in the same
     * `r` and run into the same code below -- no second exit: a loaded wave without a hit skips the other nine loads
     * and leaves through the miss path as a computed one does (an early return here cost every grid-walk instance
     * three registers, and the ones at their occupancy's limit scratch or a wave) */
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    vrc_ray r;
    if( f.rayMode == VRC_RAY_LOAD )
    {
        const float* const rc = f.rayCache + rayIndex;
        const uint32_t P = f.rayCachePlane;
        r.hit = vrc_float_bits( rc[9u * P] ) != 0u;
        bool any = r.hit;
#if defined( __HIP_DEVICE_COMPILE__ )
        any = __builtin_amdgcn_ballot_w64( any ) != 0ull;
#endif
        r.origin.x = f.eye[0];
        r.origin.y = f.eye[1];
        r.origin.z = f.eye[2];
        r.dir.x = r.dir.y = r.dir.z = r.invDir.x = r.invDir.y = r.invDir.z = 0.0f;
        r.tNearGlobal = r.tFarGlobal = r.tNearPlane = 0.0f;
        if( any ) /* (a wave whose rays all miss the volume reads nothing else of them) */
        {
            r.dir.x = rc[0];
            r.dir.y = rc[P];
            r.dir.z = rc[2u * P];
            r.invDir.x = rc[3u * P];
            r.invDir.y = rc[4u * P];
            r.invDir.z = rc[5u * P];
            r.tNearGlobal = rc[6u * P];
            r.tFarGlobal = rc[7u * P];
            r.tNearPlane = rc[8u * P];
        }
    }
    else
    {
        r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
        if( f.rayMode == VRC_RAY_STORE )
        {
            float* const rc = f.rayCache + rayIndex;
            const uint32_t P = f.rayCachePlane;
            rc[0] = r.dir.x;
            rc[P] = r.dir.y;
            rc[2u * P] = r.dir.z;
            rc[3u * P] = r.invDir.x;
            rc[4u * P] = r.invDir.y;
            rc[5u * P] = r.invDir.z;
            rc[6u * P] = r.tNearGlobal;
            rc[7u * P] = r.tFarGlobal;
            rc[8u * P] = r.tNearPlane;
            rc[9u * P] = vrc_bits_float( r.hit ? 1u : 0u );
        }
    }
    if( !r.hit )
    {
        if( f.clearFirst )
            pixelBuffer[pixelPos] = zero;
        return;
    }
    vrc_f4 color = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( color.w > VRC_EARLY_EXIT )
        return;
    vrc_ray_grid_dda< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, r, nodes, gridTable, atlas, lut, cls, color,
                                                                   nSamples, -1, 2, 2, nullptr, cdepth );
    pixelBuffer[pixelPos] = color;
}

/* ------------------------------------------------------------------------------------------
 * The walk cache (vrc_frame::walkCache): the grid walk recorded once, and the march replayed from the record.
 * ---------------------------------------------------------------------------------------- */
/* the ray of pixel rayIndex as the ray cache holds it (f.rayMode == VRC_RAY_LOAD): the bits vrc_setup_ray returned */
VRC_HD vrc_ray vrc_ray_from_cache( const vrc_frame& f, uint32_t rayIndex )
{
    const float* const rc = f.rayCache + rayIndex;
    const uint32_t P = f.rayCachePlane;
    vrc_ray r;
    r.origin.x = f.eye[0];
    r.origin.y = f.eye[1];
    r.origin.z = f.eye[2];
    r.dir.x = rc[0];
    r.dir.y = rc[P];
    r.dir.z = rc[2u * P];
    r.invDir.x = rc[3u * P];
    r.invDir.y = rc[4u * P];
    r.invDir.z = rc[5u * P];
    r.tNearGlobal = rc[6u * P];
    r.tFarGlobal = rc[7u * P];
    r.tNearPlane = rc[8u * P];
    r.hit = vrc_float_bits( rc[9u * P] ) != 0u;
    return r;
}

/* Record form of vrc_pixel_grid_dda: the same walk of the same ray, whose visits are stored and counted instead of
 * marched.  Returns the number of visits; the caller stores it in plane 0 (record pass) or folds it into the frame's
 * maximum (count pass).  The pixel buffer is not read: a list is complete whatever the frame composites onto, and
 * whatever the transfer function ends early.  gathers (count pass only): how many of the visits meet a brick that is not
 * known to be uniform, by the slot words as they are now; notLean (count pass of a frame with walkLean set): 1 when a
 * visit of the ray does not pack (vrc_walk_lean_word) */
VRC_HD uint32_t vrc_pixel_walk_record( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                       const int32_t* __restrict__ gridTable, uint32_t rayIndex,
                                       uint32_t* gathers = nullptr, uint32_t* notLean = nullptr )
{
    const vrc_ray r = vrc_ray_from_cache( f, rayIndex );
    uint32_t count = 0u;
    vrc_f4 none = { 0.f, 0.f, 0.f, 0.f };
    if( r.hit )
    {
        const vrc_classifier cls = {};
        vrc_ray_grid_dda< false, false, true, VRC_MODE_WALK_RECORD, uint8_t, VRC_GROUP, false >(
            f, r, nodes, gridTable, nullptr, nullptr, cls, none, count, -1, 2, 2, f.walkCache + rayIndex );
    }
    if( gathers )
        *gathers = (uint32_t)none.x;
    if( notLean )
        *notLean = none.y != 0.0f ? 1u : 0u;
    return count;
}

/* The third segment source (beside vrc_segment_ready and vrc_segment_from_interval): visit `at` of a recorded list.
 * distOnly(): the stored dist -- the uniform march needs no ray; full(): the stored interval completed from the ray of
 * the ray cache, exactly as vrc_march_brick completes an interval of the walk (vrc_segment_complete reads the ray's
 * origin and direction).  A wave whose bricks are all uniform never reads ray or interval.  `early`: the caller issued
 * the five loads already, at the top of the visit and in front of the node and slot-word fetches that decide whether
 * they are needed (vrc_pixel_walk_replay: it does so when the wave's visit before took the gather march); else they
 * are made here, where the wave first needs them.  `gathered`: set when a march asked for the whole segment -- what
 * the caller's next visit goes by; the uniform march never touches it */
struct vrc_walk_early
{
    bool have;
    float tNear, tFar;
    vrc_f3 dir;
};
VRC_HD vrc_walk_early vrc_walk_load_early( const vrc_frame& f, uint32_t rayIndex, const uint32_t* at )
{
    const float* const rc = f.rayCache + rayIndex;
    vrc_walk_early e;
    e.have = true;
    e.tNear = vrc_bits_float( at[2u * f.walkPlane] );
    e.tFar = vrc_bits_float( at[3u * f.walkPlane] );
    e.dir.x = rc[0];
    e.dir.y = rc[f.rayCachePlane];
    e.dir.z = rc[2u * f.rayCachePlane];
    return e;
}
struct vrc_segment_from_walk
{
    const vrc_frame& f;
    uint32_t rayIndex;
    const uint32_t* at; /* the visit's word of its first plane (node) */
    float dist;
    const vrc_walk_early& early;
    bool* gathered;
    VRC_HD vrc_segment full() const
    {
        *gathered = true;
        const vrc_walk_early e = early.have ? early : vrc_walk_load_early( f, rayIndex, at );
        vrc_ray r;
        r.origin.x = f.eye[0];
        r.origin.y = f.eye[1];
        r.origin.z = f.eye[2];
        r.dir = e.dir;
        r.invDir = e.dir; /* (not read by the completion) */
        r.tNearGlobal = r.tFarGlobal = r.tNearPlane = 0.0f;
        r.hit = true;
        const vrc_interval iv = { e.tNear, e.tFar };
        vrc_segment s;
        vrc_segment_complete( r, iv, f.stepSize, &s );
        return s;
    }
    VRC_HD vrc_segment distOnly() const
    {
        const vrc_f3 zero = { 0.0f, 0.0f, 0.0f };
        vrc_segment s = { zero, zero, dist, 0.0f };
        return s;
    }
};

/* The pixel a replayed march leaves (both replay functions: the final store and the clear of a ray without visits).
 * A frame's worth of plain stores stays in the L2s as dirty lines -- 16 bytes per pixel, about as much per XCD as half
 * its L2 holds at 1024 x 1024 -- and the release at the end of the kernel writes them back before the next packet of
 * the stream may start.  vrc_frame::storeThrough = 1 sends the four floats through the L2 instead: one 16-byte store
 * marked sc1 (write-through, the line is not kept), so the frame streams out while the march runs and the kernel ends
 * on an L2 that holds nothing of it.  The eight lanes of a tile row write one whole 128-byte line.  The store goes
 * through a buffer resource over the pixel buffer -- base and size are kernel arguments, so the descriptor is scalar --
 * of width * height * 16 bytes: an offset outside the frame is dropped by the range check, not written.  The choice is
 * the frame's, the same in every lane: a scalar branch.  On the host (the CPU harnesses) it is the assignment.
 * The pixel comes by value: taken by reference, `zero` of the callers becomes an object with an address and the
 * replay of the other form picks its first colour through a pointer into scratch (20 bytes per lane, as compiled).
 * The plain store's index passes through a lane move that moves nothing (quad_perm 0, 1, 2, 3: every lane reads itself),
 * so that its 64-bit address is formed at the store.  Without it the compiler keeps the address it formed for the
 * pixel's load (clearFirst = 0) alive across the visit loop beside the 32-bit offset the other store needs -- three
 * registers where the loop held two, one more in every instance, and the counted grey instance of the other form in
 * groups of 24 goes from 90 to 99 and loses its fifth wave.  With it the loop holds the pixel's number alone: every
 * instance needs as many registers as before or up to two fewer (one needs one more, within its waves) */
VRC_HD void vrc_store_pixel( const vrc_frame& f, vrc_f4* __restrict__ pixelBuffer, uint32_t pixelPos, const vrc_f4 c )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    if( f.storeThrough != 0u )
    {
        typedef uint32_t vrc_u4 __attribute__( ( ext_vector_type( 4 ) ) );
        const vrc_u4 bits = { vrc_float_bits( c.x ), vrc_float_bits( c.y ), vrc_float_bits( c.z ), vrc_float_bits( c.w ) };
        __builtin_amdgcn_raw_buffer_store_b128(
            bits, __builtin_amdgcn_make_buffer_rsrc( pixelBuffer, 0, (int)( f.width * f.height * 16u ), 0x00020000 ),
            (int)( pixelPos * 16u ), 0, 16 /* sc1 */ );
        return;
    }
    pixelBuffer[(uint32_t)__builtin_amdgcn_update_dpp( 0, (int)pixelPos, 0xE4, 0xF, 0xF, false )] = c;
#else
    (void)f;
    pixelBuffer[pixelPos] = c;
#endif
}

/* Replay form of vrc_pixel_grid_dda for the instances of the uniform-brick march (8-bit atlas, fixed-point stepping, no
 * clamp, 32-bit slot bases): the pixel's clear, early exit and store are the walk's, and every recorded visit goes to
 * the one visit body vrc_march_brick_from -- the slot word, its ballot, both uniform marches, the gather march and the
 * early exit are that code.  A ray without visits leaves the pixel as the walk does: cleared where the frame clears,
 * untouched where it does not (a hit ray that met no brick stored the colour it had loaded).  The count is clamped by
 * walkK and the node index by the table, so no list content can run the loop away or reach past the node table.  The
 * node and dist loads of visit k + 1 are issued before the march of visit k.  What only the gather march needs -- the
 * interval and the ray's direction -- is loaded at the top of a visit when the wave's visit before took the gather march
 * (bricks of a kind come in runs), so that those loads overlap the node and slot-word fetches; the prediction decides
 * nothing but when five loads are issued, and costs a wave of uniform bricks nothing */
template < bool COUNT, int MODE, int GROUP >
VRC_HD void vrc_pixel_walk_replay( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                   const uint8_t* __restrict__ atlas, const vrc_f4* lut, const vrc_classifier& cls,
                                   vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py, uint32_t& nSamples,
                                   uint32_t rayIndex )
{
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    const uint32_t P = f.walkPlane;
    const uint32_t* const wc = f.walkCache + rayIndex;
    uint32_t count = wc[0];
    count = count < f.walkK ? count : f.walkK;
    if( count == 0u )
    {
        if( f.clearFirst )
            vrc_store_pixel( f, pixelBuffer, pixelPos, zero );
        return;
    }
    vrc_f4 color = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( color.w > VRC_EARLY_EXIT )
        return;
    const uint32_t lastNode = f.nodeCount - 1u;
    const uint32_t* at = wc + P;
    uint32_t node = at[0];
    float dist = vrc_bits_float( at[P] );
    bool gathered = false; /* did the visit before take the gather march?  (the whole wave takes it or none of it) */
    for( uint32_t k = 0u; k < count; ++k )
    {
        const uint32_t* const next = at + 4u * P;
        uint32_t nodeNext = 0u;
        float distNext = 0.0f;
        if( k + 1u < count )
        {
            nodeNext = next[0];
            distNext = vrc_bits_float( next[P] );
        }
        vrc_walk_early early = { false, 0.0f, 0.0f, { 0.0f, 0.0f, 0.0f } };
        if( gathered )
            early = vrc_walk_load_early( f, rayIndex, at );
        gathered = false;
        const vrc_dev_node n = nodes[node < lastNode ? node : lastNode];
        const vrc_segment_from_walk src = { f, rayIndex, at, dist, early, &gathered };
        if( vrc_march_brick_from< false, COUNT, true, MODE, uint8_t, GROUP, false, vrc_segment_from_walk >(
                f, n, src, atlas, lut, cls, color, nSamples, 0.0f ) )
            break;
        at = next;
        node = nodeNext;
        dist = distNext;
    }
    vrc_store_pixel( f, pixelBuffer, pixelPos, color );
}

/* The replay of a lean list (vrc_frame::walkLean): the pixel's clear, early exit and store, the order of the visits,
 * the slot word's rule (0 without slotInfo or without an index), its ballot and the gather march are
 * vrc_pixel_walk_replay's; what a frame cannot change is read from the list instead of being fetched and computed
 * again.  The slot word's address comes from the list, so the node is not fetched in front of the ballot, and a
 * uniform visit marches the n of its word: no node, no dist, no vrc_exact_step_count, no second ballot (every visit of
 * a lean list counts exactly, so the wave would always have taken the counted form).  A visit that gathers fetches its
 * node, interval and ray inside its own branch (no prediction from the visit before) and runs the same march on the
 * same segment.  In flight across the march of visit k: the list word of visit k + 2 and the slot word of visit k + 1.
 * Neither load stands under a branch -- the list word comes from visit min(k + 2, walkK - 1) (vrc_lean_list_word), the
 * slot word through a pointer that is always valid (vrc_lean_slot_load) -- because a load that a path may skip leaves
 * the compiler one safe wait for the values of the visit before, vmcnt(0), right behind the loads just issued.  As
 * compiled for gfx950 the loop waits at its top for the two loads of the visit before, issues the two new ones, and
 * meets no vector-memory wait before its latch.  The index is clamped by walkSlots
 * as the node is by the table, so no list content reaches past slotInfo.  The colour stays in the march's own form
 * (two floats under a grey table) across the visits and is widened once, at the store: what every march of the
 * other form does on its way out */
template < int MODE > struct vrc_lean_colour { typedef vrc_f4 type; };
template <> struct vrc_lean_colour< VRC_MODE_GREY > { typedef vrc_f2 type; };
VRC_HD vrc_f2 vrc_lean_narrow( const vrc_f4& c, const vrc_f2* ) { return vrc_f2{ c.x, c.w }; }
VRC_HD vrc_f4 vrc_lean_narrow( const vrc_f4& c, const vrc_f4* ) { return c; }
VRC_HD vrc_f4 vrc_lean_widen( const vrc_f2& c ) { return vrc_f4{ c.x, c.x, c.x, c.w }; }
VRC_HD vrc_f4 vrc_lean_widen( const vrc_f4& c ) { return c; }
/* the slot word of a list word, in two steps so that the load can be issued a visit ahead and nothing waits for it
 * before the visit that reads it: the load and the rule.  The load is unconditional, so that no branch stands between
 * it and the march it is to overlap: it reads through a pointer that is always valid -- a word of slotInfo (index
 * clamped by walkSlots; a lean frame has walkSlots >= 1) or, for a frame without slotInfo (VRC_OPT_UNIFORM_BRICKS = 0
 * over lean lists), word 0 of the lists themselves -- and the rule selects: 0 without slotInfo or without an index */
VRC_HD uint32_t vrc_lean_slot_load( const vrc_frame& f, uint32_t packed )
{
    const uint32_t idx = packed & ( ( 1u << VRC_WALK_LEAN_INDEX_BITS ) - 1u );
    const bool have = f.slotInfo != nullptr;
    const uint32_t* const from = have ? f.slotInfo : f.walkCache;
    const uint32_t last = have ? f.walkSlots - 1u : 0u;
    const uint32_t i = idx != 0u ? idx - 1u : 0u;
    return from[i < last ? i : last];
}
VRC_HD uint32_t vrc_lean_slot_word( const vrc_frame& f, uint32_t packed, uint32_t loaded )
{
    return ( f.slotInfo != nullptr && ( packed & ( ( 1u << VRC_WALK_LEAN_INDEX_BITS ) - 1u ) ) != 0u ) ? loaded : 0u;
}
/* The list word (second plane) of visit v of a ray, v clamped to the last visit the planes hold.  The invariant the
 * unconditional reads rest on: the planes hold walkK >= 1 visits for EVERY ray of EVERY whole tile -- (1 + 4 walkK) x
 * walkPlane words, walkPlane = tiles x 64, rayIndex < walkPlane (vrc_render sizes them so; vrc_k_walk_record writes
 * plane 0 of every lane of a tile, those outside the frame included) -- so visit min(v, walkK - 1) of any ray index
 * below walkPlane is an allocated word, whatever the ray's count says.  A word read past the ray's count may hold
 * anything: it is never marched (the loop ends at count), and as a slot index it is clamped like any other.  v is the
 * same in every lane of a wave, so the clamp is scalar work */
VRC_HD uint32_t vrc_lean_list_word( const vrc_frame& f, uint32_t rayIndex, uint32_t v )
{
    const uint32_t lastVisit = f.walkK - 1u;
    const size_t plane = 2u + 4u * (size_t)( v < lastVisit ? v : lastVisit );
    return f.walkCache[(size_t)rayIndex + plane * f.walkPlane];
}

/* The pixel of lane `lane` of tile `tile` in the replay (Morton lane order, tiles of 8 x 8 row-major over tilesX), in two
 * parts: the tile's origin is the wave's -- the kernel hands it a tile number that is the same in every lane, so the
 * division stays off the vector unit -- and the lane adds its 3 + 3 bits */
VRC_HD void vrc_replay_tile_origin( uint32_t tile, uint32_t tilesX, uint32_t& x0, uint32_t& y0 )
{
    const uint32_t ty = tile / tilesX;
    x0 = ( tile - ty * tilesX ) * 8u;
    y0 = ty * 8u;
}
VRC_HD void vrc_replay_lane_pixel( uint32_t x0, uint32_t y0, uint32_t lane, uint32_t& px, uint32_t& py )
{
    px = x0 + ( ( lane & 1u ) | ( ( lane >> 1 ) & 2u ) | ( ( lane >> 2 ) & 4u ) );
    py = y0 + ( ( ( lane >> 1 ) & 1u ) | ( ( lane >> 2 ) & 2u ) | ( ( lane >> 3 ) & 4u ) );
}

/* The resolved word of visit v of a ray (vrc_frame::walkResolved, VRC_OPT_WALK_RESOLVED): what the uniform-only replay
 * makes of the visit's list word and slot word in every frame, made once.  The step count n stays in the 12 bits the
 * list word has it in; the low byte is the slot word's value (vrc_lean_slot_word of the word vrc_lean_slot_load reads:
 * the same clamp, the same rule); VRC_WALK_RESOLVED_ONE is set iff the visit is below the ray's count and the slot word
 * holds one value -- iff the uniform-only replay marches it.  A clear bit ends the ray's list there, as the count or a
 * word that does not hold one value does.  Visits stay one to one: v < walkK, any ray index below walkPlane (the
 * invariant of vrc_lean_list_word) */
#define VRC_WALK_RESOLVED_ONE 0x100u
VRC_HD uint32_t vrc_walk_resolved_word( const vrc_frame& f, uint32_t rayIndex, uint32_t v )
{
    const uint32_t listed = f.walkCache[rayIndex];
    const uint32_t packed = vrc_lean_list_word( f, rayIndex, v );
    const uint32_t word = vrc_lean_slot_word( f, packed, vrc_lean_slot_load( f, packed ) );
    const uint32_t one = ( v < listed && vrc_slot_holds_one_value( word ) ) ? VRC_WALK_RESOLVED_ONE : 0u;
    return ( packed & ~( ( 1u << VRC_WALK_LEAN_INDEX_BITS ) - 1u ) ) | one | ( word & 0xFFu );
}
/* ... and its load, v clamped to the last plane as vrc_lean_list_word clamps it: unconditional for the same reason */
VRC_HD uint32_t vrc_walk_resolved_load( const vrc_frame& f, uint32_t rayIndex, uint32_t v )
{
    const uint32_t lastVisit = f.walkK - 1u;
    return f.walkResolved[(size_t)rayIndex + (size_t)( v < lastVisit ? v : lastVisit ) * f.walkPlane];
}

/* The uniform-only replay from resolved words (vrc_frame::walkResolved != NULL; the uncounted instances).  The pixel's
 * clear, early exit and store, the first visit from the table and the march of every visit are those of
 * vrc_pixel_walk_replay_lean< false, ..., true > below; a visit is one word -- no slot word to load, no rule, no clamp of
 * an index -- and the loop ends at the first word whose bit is clear, which is where that function's count or its test
 * of the slot word ends it (a ray that ended in the peel is given such a word).  The count and the words of visits 0
 * and 1 are asked for together; across the march of visit k the word of visit k + 2 is in flight, its load under no
 * branch (profiles/r13_lean_prefetch.txt) */
template < int MODE >
VRC_HD void vrc_pixel_walk_replay_resolved( const vrc_frame& f, const vrc_f4* lut, vrc_f4* __restrict__ pixelBuffer,
                                            uint32_t px, uint32_t py, uint32_t rayIndex )
{
    typedef typename vrc_lean_colour< MODE >::type E;
    const E* const tab = reinterpret_cast< const E* >( lut );
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    uint32_t listed = f.walkCache[rayIndex];
    uint32_t res = vrc_walk_resolved_load( f, rayIndex, 0u );
    uint32_t resNext = vrc_walk_resolved_load( f, rayIndex, 1u );
#if defined( __HIP_DEVICE_COMPILE__ )
    /* (the three loads in front of the count's branch, one wait for all of them: left alone the compiler sinks the
     * words' loads behind that branch and the ray waits twice) */
    asm volatile( "" : "+v"( listed ), "+v"( res ), "+v"( resNext ) );
#endif
    if( listed == 0u ) /* (walkK >= 1: the count clamped by it is zero iff this is) */
    {
        if( f.clearFirst )
            vrc_store_pixel( f, pixelBuffer, pixelPos, zero );
        return;
    }
    const vrc_f4 start = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( start.w > VRC_EARLY_EXIT )
        return;
    E color = vrc_lean_narrow( start, (const E*)nullptr );
    const bool freeMarch = f.leanFree != 0u;
    const uint32_t K = f.walkK;
    uint32_t nSamples = 0u; /* (uncounted) */
    uint32_t k = 0u;
    const E* const first = static_cast< const E* >( f.firstVisit );
    if( first != nullptr && f.clearFirst ) /* (the frame's: the same in every lane) */
    {
        const uint32_t resAfter = vrc_walk_resolved_load( f, rayIndex, 2u );
        const uint32_t n = res >> VRC_WALK_LEAN_INDEX_BITS;
        const bool one = ( res & VRC_WALK_RESOLVED_ONE ) != 0u;
        bool done = true;
        if( one && n < VRC_FIRST_VISIT_ROWS )
        {
            color = first[( res & 0xFFu ) * VRC_FIRST_VISIT_ROWS + n];
            done = color.w > VRC_EARLY_EXIT;
        }
        else if( one )
            done = vrc_march_uniform_lean< false, E >( color, tab[res & 0xFFu], n, nSamples, freeMarch );
        res = done ? 0u : resNext;
        resNext = resAfter;
        k = 1u; /* (the same in every lane of the wave) */
    }
    for( ; k < K; ++k )
    {
        const uint32_t resAfter = vrc_walk_resolved_load( f, rayIndex, k + 2u );
        if( ( res & VRC_WALK_RESOLVED_ONE ) == 0u )
            break;
        if( vrc_march_uniform_lean< false, E >( color, tab[res & 0xFFu], res >> VRC_WALK_LEAN_INDEX_BITS, nSamples, freeMarch ) )
            break;
        res = resNext;
        resNext = resAfter;
    }
    vrc_store_pixel( f, pixelBuffer, pixelPos, vrc_lean_widen( color ) );
}

/* UNIFORM_ONLY: the same replay for a frame none of whose visits gathers (vrc_frame::walkLean = VRC_WALK_LEAN_UNIFORM:
 * the count pass of these lists found no such visit, and the host has seen no upload and no other slotInfo since).  The
 * wave then never asks whether one of its lanes gathers -- no ballot -- and the gather march is not in the function:
 * what is left is the loads, the rule and vrc_march_uniform_lean, in 20 registers where the other form holds the gather
 * march's 79 across the loop.  A word that does not hold one value after all (the host's rule is what keeps it from
 * happening) is clamped like any other and ends the ray's list at that visit: nothing is read through it.
 * The first visit from the table (vrc_frame::firstVisit, vrc_first_visit_row): peeled in front of the visit loop, in the
 * uncounted instances -- a counted frame marches every visit, its sample count being the oracle's yardstick.  The list
 * words of visits 0 and 1 and the slot word of visit 0 are loaded as ever; in a frame that starts from zero and has a
 * table, a lane whose slot word holds one value and whose n is below the rows takes color = T[word & 0xFF][n],
 * done = color.w > VRC_EARLY_EXIT -- what vrc_march_uniform_lean leaves from zero, bit for bit.  Uniform-only: any other
 * lane (n >= ROWS, a word that does not hold one value) runs the visit's body in the peel.  The form that can gather
 * peels per wave instead: where every lane of the wave can take its colour from the table the wave does, and where one
 * cannot the whole wave starts the loop at visit 0 as it always did -- the visit's body with its gather march stands in
 * the function once, and the instances keep their registers and waves (with the body in the peel as well the
 * grey instance in groups of 24 went from 89 to 98 registers and lost its fifth wave).  Behind the peel the loop starts
 * at visit 1 with its prefetch state as if visit 0 had been an iteration; the visit number stays the wave's (a ray that
 * ended in the peel is masked out of the loop, not given a count of its own: a per-lane number turns the clamp of the
 * list word's plane into vector work and moves the loop's wait to its latch).  The table's load stands in front of the
 * loop, never in it under a condition: a load that a path may skip leaves the compiler one safe wait, vmcnt(0), behind
 * the loop's own loads (profiles/r13_lean_prefetch.txt) */
template < bool COUNT, int MODE, int GROUP, bool UNIFORM_ONLY = false >
VRC_HD void vrc_pixel_walk_replay_lean( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                                        const uint8_t* __restrict__ atlas, const vrc_f4* lut, const vrc_classifier& cls,
                                        vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py, uint32_t& nSamples,
                                        uint32_t rayIndex )
{
    typedef typename vrc_lean_colour< MODE >::type E;
    (void)cls;
    if constexpr( UNIFORM_ONLY && !COUNT )
    {
        if( f.walkResolved != nullptr ) /* (the frame's: a scalar branch) */
        {
            vrc_pixel_walk_replay_resolved< MODE >( f, lut, pixelBuffer, px, py, rayIndex );
            return;
        }
    }
    const E* const tab = reinterpret_cast< const E* >( lut );
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    const uint32_t listed = f.walkCache[rayIndex];
    const uint32_t count = listed < f.walkK ? listed : f.walkK;
    if( count == 0u )
    {
        if( f.clearFirst )
            vrc_store_pixel( f, pixelBuffer, pixelPos, zero );
        return;
    }
    const vrc_f4 start = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( start.w > VRC_EARLY_EXIT )
        return;
    E color = vrc_lean_narrow( start, (const E*)nullptr );
    const uint32_t lastNode = f.nodeCount - 1u;
    const bool freeMarch = f.leanFree != 0u; /* (the frame's: a scalar branch in front of the per-lane test) */
    /* the words of the first two visits: unconditional like the loop's (a list of one visit reads its word twice) */
    uint32_t packed = vrc_lean_list_word( f, rayIndex, 0u );
    uint32_t packedNext = vrc_lean_list_word( f, rayIndex, 1u );
    uint32_t loaded = vrc_lean_slot_load( f, packed );
    uint32_t k = 0u;
    bool ended = false; /* the ray ends at its first visit: it runs no visit of the loop */
    if constexpr( !COUNT )
    {
        const E* const first = static_cast< const E* >( f.firstVisit );
        if( first != nullptr && f.clearFirst ) /* (the frame's: the same in every lane) */
        {
            const uint32_t word = vrc_lean_slot_word( f, packed, loaded );
            const uint32_t n = packed >> VRC_WALK_LEAN_INDEX_BITS;
            const bool one = vrc_slot_holds_one_value( word );
            const bool row = n < VRC_FIRST_VISIT_ROWS;
            bool peel = true;
            if constexpr( !UNIFORM_ONLY )
            {
                peel = one && row;
#if defined( __HIP_DEVICE_COMPILE__ )
                peel = __builtin_amdgcn_ballot_w64( !peel ) == 0ull;
#endif
            }
            if( peel )
            {
                const uint32_t loadedNext = vrc_lean_slot_load( f, packedNext );
                const uint32_t packedAfter = vrc_lean_list_word( f, rayIndex, 2u );
                bool done = true; /* (uniform-only: a word that does not hold one value ends the list, as in the loop) */
                if( one && row )
                {
                    color = first[( word & 0xFFu ) * VRC_FIRST_VISIT_ROWS + n];
                    done = color.w > VRC_EARLY_EXIT;
                }
                else if constexpr( UNIFORM_ONLY )
                {
                    if( one )
                        done = vrc_march_uniform_lean< COUNT, E >( color, tab[word & 0xFFu], n, nSamples, freeMarch );
                }
                packed = packedNext;
                packedNext = packedAfter;
                loaded = loadedNext;
                k = 1u; /* (the same in every lane of the wave, as in the loop) */
                ended = done;
            }
        }
    }
    for( const uint32_t visits = ended ? 0u : count; k < visits; ++k )
    {
        /* the two prefetches, neither under a branch (the slot word first: its address is a list word that arrived a
         * visit ago) */
        const uint32_t loadedNext = vrc_lean_slot_load( f, packedNext );
        const uint32_t packedAfter = vrc_lean_list_word( f, rayIndex, k + 2u );
        const uint32_t word = vrc_lean_slot_word( f, packed, loaded );
        const uint32_t n = packed >> VRC_WALK_LEAN_INDEX_BITS;
        bool general = !vrc_slot_holds_one_value( word );
        bool done;
        if constexpr( UNIFORM_ONLY )
        {
            /* no ballot, and no gather march in the function: such a word ends the list */
            if( general )
                break;
            done = vrc_march_uniform_lean< COUNT, E >( color, tab[word & 0xFFu], n, nSamples, freeMarch );
        }
        else
        {
#if defined( __HIP_DEVICE_COMPILE__ )
            general = __builtin_amdgcn_ballot_w64( general ) != 0ull;
#endif
            if( !general )
                done = vrc_march_uniform_lean< COUNT, E >( color, tab[word & 0xFFu], n, nSamples, freeMarch );
            else
            {
                /* the gather visit's own loads, all inside its branch: the interval and the ray's direction are asked
                 * for in front of the node, so the five of them travel while the node index and the node arrive */
                const uint32_t* const at = f.walkCache + ( (size_t)rayIndex + ( 1u + 4u * (size_t)k ) * f.walkPlane );
                const vrc_walk_early early = vrc_walk_load_early( f, rayIndex, at );
                const uint32_t node = at[0];
                const vrc_dev_node nd = nodes[node < lastNode ? node : lastNode];
                bool gathered = false;
                const vrc_segment_from_walk src = { f, rayIndex, at, 0.0f, early, &gathered };
                done = vrc_march_segment_as< false, COUNT, true, uint8_t, GROUP, E >( f, nd, src.full(), atlas, tab,
                                                                                      color, nSamples, 0.0f );
            }
        }
        if( done )
            break;
        packed = packedNext;
        packedNext = packedAfter;
        loaded = loadedNext;
    }
    vrc_store_pixel( f, pixelBuffer, pixelPos, vrc_lean_widen( color ) );
}

/* ------------------------------------------------------------------------------------------
 * EXTENSION: per-ray adaptive LOD (BASELINE C5; vrc_set_ray_lod).  The reference selects the LOD
 * per brick on the host: a brick is fine enough when its voxels, seen from the point of its box
 * nearest to the near plane, are at most screenSpaceError pixels wide
 * (livre/core/render/SelectVisibles.cpp:52-68: pixelPerVoxel * near / (near + distance) <= sse).
 * Here the same criterion is evaluated along the ray.  The node list is a hierarchy (a cut of the
 * octree plus ancestors, all resident, boxes may nest); with voxel size vw0 * 2^j at level j and
 * eye-space depth / near = t / tNearPlane along a ray, level j is fine enough from
 *     T_j = tNearPlane * lodBase * 2^j,   lodBase = vw0 / (screenSpaceError * worldSpacePerPixel).
 * Every level is a regular grid of bricks (border bricks may be smaller; the levels of a ragged
 * tree need not align with each other).  The ray hops from brick to brick: at parameter te it
 * wants level k = #{ j >= 1 : T_j <= te } and takes, at the point o + d*(te + eps), the brick of
 * the first level that has one there in the order k, k+1, ..., K-1, k-1, ..., 0; the run ends
 * where the ray leaves that brick's box (the finest level's cell where there is no brick) and
 * the level is chosen anew.  A run is marched like a reference brick segment
 * (Renderer.cu:195-223: sampling restarts at the run's entry point, here eps inside the brick so
 * that the first sample does not sit on a voxel face) with step stepSize * 2^j and
 * opacity exponent alphaCorrection * 2^j (classified table of level j: lut + j * 257; classifier
 * exponent scaled for the per-sample modes), so a level-j brick costs 2^-j of the samples and
 * the opacity of a homogeneous stretch does not depend on the level it is sampled at.
 * gridTable holds the cell -> node table of every level (f.lodTable offsets).  CUDA variant only.
 * ---------------------------------------------------------------------------------------- */

VRC_HD vrc_segment vrc_run_segment( const vrc_ray& r, float tA, float tB, float stepSize )
{
    VRC_STRICT_FP
    /* the tail of vrc_brick_segment (Renderer.cu:195-201) for an explicit interval */
    const vrc_f3 rayStart = { r.origin.x + r.dir.x * tA, r.origin.y + r.dir.y * tA,
                              r.origin.z + r.dir.z * tA };
    const vrc_f3 rayStop = { r.origin.x + r.dir.x * tB, r.origin.y + r.dir.y * tB,
                             r.origin.z + r.dir.z * tB };
    const vrc_f3 diff = { rayStop.x - rayStart.x, rayStop.y - rayStart.y, rayStop.z - rayStart.z };
    const float d2 = vrc_dot( diff, diff );
    vrc_segment s;
    s.pos = rayStart;
    s.tNear = tA;
    if( d2 > 0.0f )
    {
        const float invLen = 1.0f / sqrtf( d2 );
        s.step.x = diff.x * invLen * stepSize;
        s.step.y = diff.y * invLen * stepSize;
        s.step.z = diff.z * invLen * stepSize;
        s.dist = sqrtf( d2 );
    }
    else
    {
        s.step.x = s.step.y = s.step.z = 0.0f;
        s.dist = 0.0f;
    }
    return s;
}

/* T_0 of the ray: level j is fine enough from T_0 * 2^j on */
VRC_HD float vrc_ray_lod_base( const vrc_frame& f, const vrc_ray& r )
{
    VRC_STRICT_FP
    return r.tNearPlane * f.lodBase;
}

/* One hop of the per-ray LOD walk at ray parameter te: the brick the ray is in at te + eps (its index in
 * `nodes`, copied to n; -1: no level has a brick there), the parameter tp of the run's first sample and tB
 * where the ray leaves the brick's box (no brick: the finest level's grid cell).  Shared by
 * vrc_pixel_ray_lod and the LDS-staged kernel (vrc_kernels_lds.hip): same bits in both. */
VRC_HD int32_t vrc_ray_lod_hop( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node* __restrict__ nodes,
                                const int32_t* __restrict__ gridTable, float tBase, float te, float t1,
                                vrc_dev_node& n, float& tp, float& tB )
{
    const int K = (int)f.lodLevels;
    const float o[3] = { r.origin.x, r.origin.y, r.origin.z };
    const float d[3] = { r.dir.x, r.dir.y, r.dir.z };
    const float id[3] = { r.invDir.x, r.invDir.y, r.invDir.z };
    int k = 0;
    float T = tBase;
    for( int j = 1; j < K; ++j )
    {
        T = T + T; /* T_j, exact */
        k += T <= te ? 1 : 0;
    }
    float p[3];
    {
        VRC_STRICT_FP
        tp = te + f.lodEps;
        p[0] = o[0] + d[0] * tp;
        p[1] = o[1] + d[1] * tp;
        p[2] = o[2] + d[2] * tp;
    }
    int32_t node = -1;
    for( int s = 0; s < K && node < 0; ++s )
    {
        const int lv = s < K - k ? k + s : K - 1 - s; /* k..K-1, then k-1..0 */
        int c[3];
#pragma unroll
        for( int a = 0; a < 3; ++a )
        {
            VRC_STRICT_FP
            c[a] = (int)floorf( ( p[a] - f.gridMin[a] ) * f.lodInvCell[lv][a] );
            c[a] = c[a] < 0 ? 0 : ( c[a] > f.lodDim[lv][a] - 1 ? f.lodDim[lv][a] - 1 : c[a] );
        }
        node = gridTable[f.lodTable[lv] + ( c[2] * f.lodDim[lv][1] + c[1] ) * f.lodDim[lv][0] + c[0]];
    }
    /* where the ray leaves the brick (no brick here: the finest level's grid cell) */
    float bmin[3], bmax[3];
    if( node >= 0 )
    {
        n = nodes[node];
#pragma unroll
        for( int a = 0; a < 3; ++a )
        {
            bmin[a] = n.aabbMin[a];
            bmax[a] = n.aabbMin[a] + n.aabbSize[a];
        }
    }
    else
    {
#pragma unroll
        for( int a = 0; a < 3; ++a )
        {
            VRC_STRICT_FP
            int c = (int)floorf( ( p[a] - f.gridMin[a] ) * f.invCellSize[a] );
            c = c < 0 ? 0 : ( c > f.gridDim[a] - 1 ? f.gridDim[a] - 1 : c );
            bmin[a] = f.gridMin[a] + f.cellSize[a] * (float)c;
            bmax[a] = f.gridMin[a] + f.cellSize[a] * (float)( c + 1 );
        }
    }
    {
        VRC_STRICT_FP
        float tX = ( ( d[0] > 0.0f ? bmax[0] : bmin[0] ) - o[0] ) * id[0];
        tX = fminf( tX, ( ( d[1] > 0.0f ? bmax[1] : bmin[1] ) - o[1] ) * id[1] );
        tX = fminf( tX, ( ( d[2] > 0.0f ? bmax[2] : bmin[2] ) - o[2] ) * id[2] );
        tB = fminf( fmaxf( tX, tp ), t1 ); /* always forward */
    }
    return node;
}

/* the interval of the hierarchy's box a ray crosses (false: none) */
VRC_HD bool vrc_ray_lod_interval( const vrc_frame& f, const vrc_ray& r, float& t0, float& t1 )
{
    const vrc_f3 gmin = { f.gridMin[0], f.gridMin[1], f.gridMin[2] };
    const vrc_f3 gmax = { f.lodMax[0], f.lodMax[1], f.lodMax[2] };
    const bool any = vrc_intersect_box( r.origin, r.invDir, gmin, gmax, &t0, &t1 );
    t0 = fmaxf( fmaxf( t0, r.tNearGlobal ), fmaxf( r.tNearPlane, 0.0f ) );
    t1 = fminf( t1, r.tFarGlobal );
    return any && t0 < t1;
}
VRC_HD int vrc_ray_lod_max_hops( const vrc_frame& f )
{
    return 3 * ( f.gridDim[0] + f.gridDim[1] + f.gridDim[2] ) + 16;
}

template < bool CLAMP, bool COUNT, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD void vrc_pixel_ray_lod( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                               const int32_t* __restrict__ gridTable,
                               const ATLAS_T* __restrict__ atlas, const vrc_f4* lut,
                               const vrc_classifier& cls,
                               vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py,
                               uint32_t& nSamples )
{
    const vrc_ray r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    if( !r.hit )
    {
        if( f.clearFirst )
            pixelBuffer[pixelPos] = zero;
        return;
    }
    vrc_f4 color = f.clearFirst ? zero : pixelBuffer[pixelPos];
    if( color.w > VRC_EARLY_EXIT )
        return;

    float t0, t1;
    if( vrc_ray_lod_interval( f, r, t0, t1 ) )
    {
        const float tBase = vrc_ray_lod_base( f, r );
        const int maxHops = vrc_ray_lod_max_hops( f );
        float te = t0;
        for( int hop = 0; hop < maxHops && te < t1; ++hop )
        {
            vrc_dev_node n;
            float tp, tB;
            const int32_t node = vrc_ray_lod_hop( f, r, nodes, gridTable, tBase, te, t1, n, tp, tB );
            if( node >= 0 )
            {
                const float scale = (float)( 1u << n.level );
                const float levelStep = f.stepSize * scale;
                const vrc_segment s = vrc_run_segment( r, tp, tB, levelStep ); /* first sample eps inside */
                vrc_classifier lc = cls;
                lc.alphaCorrection = cls.alphaCorrection * scale;
                /* the level's classified table (257 entries of four floats, or of two in the grey form) */
                const vrc_f4* ll = MODE == VRC_MODE_TABLE ? lut + n.level * VRC_LUT_ENTRIES
                                   : MODE == VRC_MODE_GREY
                                       ? reinterpret_cast< const vrc_f4* >( reinterpret_cast< const vrc_f2* >( lut ) +
                                                                            n.level * VRC_LUT_ENTRIES )
                                       : lut;
                if( vrc_march_brick< CLAMP, COUNT, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, n, s, atlas, ll, lc, color,
                                                                             nSamples, levelStep ) )
                    break;
            }
            te = tB;
        }
    }
    pixelBuffer[pixelPos] = color;
}

/* the depth cue of a MIP pixel: w = 1 - strength * u, u = where D lies in the ray's own interval [tNearGlobal, tFarGlobal]
 * (vrc_setup_ray's), clamped to [0, 1]; u = 0 where that interval is empty, 1 for D = +infinity.  Float, in this order. */
VRC_HD float vrc_mip_cue_weight( float strength, float depth, float tNearGlobal, float tFarGlobal )
{
    VRC_STRICT_FP
    const float span = tFarGlobal - tNearGlobal;
    float u = 0.0f;
    if( span > 0.0f )
    {
        u = ( depth - tNearGlobal ) / span;
        u = u > 0.0f ? u : 0.0f; /* (a NaN -- an infinite interval -- reads 0) */
        u = u < 1.0f ? u : 1.0f;
    }
    const float su = strength * u;
    return 1.0f - su;
}

/* ------------------------------------------------------------------------------------------
 * MIP pixel: the bricks of the ray as the composite pixel finds them (DDA: the grid walk; else the list in its order,
 * with the reference's `break` where a brick's tNear lies beyond the ray's interval, which is part of the sample set's
 * definition), one classification at the end.  tfp: the padded transfer function in global memory, read twice per
 * ray.  Passes of one frame meet in vrc_frame::mipMax: the first pass writes it, later ones start from it, and after
 * every pass the pixel is that of the maximum so far.  A ray without samples leaves its pixel cleared.
 * The other folds (vrc_mode_fold( MODE )): the minimum meets in mipMax too, starting from the other end; the mean meets
 * in vrc_frame::meanSum / meanCount, and its pixel is the classification of sum / count -- the quotient formed in
 * double and rounded to float once, of the stored values: the classifier carries an offset-binary atlas's shift.
 * ---------------------------------------------------------------------------------------- */
template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, int GROUP = VRC_GROUP, bool BIG = false >
VRC_HD void vrc_pixel_mip( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                           const int32_t* __restrict__ gridTable, const ATLAS_T* __restrict__ atlas,
                           const vrc_f4* __restrict__ tfp, const vrc_classifier& cls,
                           vrc_f4* __restrict__ pixelBuffer, uint32_t px, uint32_t py, uint32_t& nSamples,
                           const uint16_t* candidates = nullptr, uint32_t nCandidates = 0 )
{
    static_assert( vrc_mode_is_mip( MODE ), "a MIP mode" );
    constexpr int FOLD = vrc_mode_fold( MODE );
    constexpr bool FLOAT_M = vrc_mode_base( MODE ) == VRC_MODE_MIP_TRILINEAR || sizeof( ATLAS_T ) == 4;
    constexpr bool DEPTH = vrc_mode_depth( MODE );
    static_assert( !DEPTH || FOLD != VRC_FOLD_MEAN, "the mean has no position" );
    const vrc_ray r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
    const uint32_t pixelPos = py * f.width + px;
    const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
    uint32_t bits = VRC_MIP_EMPTY;
    float depth = vrc_bits_float( 0x7F800000u ); /* (depth tracking: D, +infinity while no sample equals M) */
    uint32_t meanLo = 0u, meanHi = 0u, meanCount = 0u; /* (the mean fold's state; an integer 0 and a double 0 alike) */
    uint32_t where = 0u, hitNode = 0u; /* (the first-crossing fold: where this pass's hit was read, vrc_iso_brick) */
    if( r.hit )
    {
        vrc_f4 state = zero;
        const uint32_t before = nSamples;
        if constexpr( FOLD == VRC_FOLD_MEAN )
        {
            if( !f.mipFirst )
            {
                const unsigned long long b = f.meanSum[pixelPos];
                meanLo = (uint32_t)b;
                meanHi = (uint32_t)( b >> 32 );
                meanCount = f.meanCount[pixelPos];
            }
            state.x = vrc_bits_float( meanLo );
            state.y = vrc_bits_float( meanHi );
        }
        else if constexpr( FOLD == VRC_FOLD_FIRST )
        {
            if( !f.mipFirst )
                bits = f.mipMax[pixelPos];
            if( bits != VRC_MIP_EMPTY )
                depth = f.mipDepth[pixelPos];
            state.x = vrc_bits_float( bits );
            state.z = depth;
        }
        else
        {
            if( !f.mipFirst )
                bits = f.mipMax[pixelPos];
            if( bits != VRC_MIP_EMPTY )
            {
                state.x = vrc_bits_float( bits );
                state.y = 1.0f;
                if constexpr( DEPTH )
                    depth = f.mipDepth[pixelPos]; /* (a later pass: the first has bits = VRC_MIP_EMPTY here) */
            }
            else if( FOLD == VRC_FOLD_MIN )
                state.x = vrc_bits_float( FLOAT_M ? 0x7F800000u : 0xFFFFFFFFu ); /* +infinity, or above every voxel */
            else if( FLOAT_M )
                state.x = vrc_bits_float( 0xFF800000u ); /* a float M starts at -infinity */
            if constexpr( DEPTH )
                state.z = depth;
        }
        if constexpr( DDA )
            vrc_ray_grid_dda< CLAMP, true, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, r, nodes, gridTable, atlas, tfp, cls, state,
                                                                             nSamples );
        else
        {
            /* the loop of vrc_pixel_reference_order */
            const uint32_t nLoop = candidates ? nCandidates : f.nodeCount;
            for( uint32_t c = 0; c < nLoop; ++c )
            {
                const uint32_t i = candidates ? (uint32_t)candidates[c] : c;
                const vrc_dev_node n = nodes[i];
                vrc_segment s;
                bool stop;
                if( !vrc_brick_segment( f, r, n, f.stepSize, &s, &stop ) )
                {
                    if( stop )
                        break;
                    continue;
                }
                vrc_mip_brick< CLAMP, FIXED, MODE, ATLAS_T, GROUP, BIG >( f, n, s, atlas, state, nSamples, i );
            }
        }
        if constexpr( FOLD == VRC_FOLD_FIRST )
        {
            where = vrc_float_bits( state.y );
            if( where != 0u )
            {
                bits = vrc_float_bits( state.x );
                depth = state.z;
                hitNode = vrc_float_bits( state.w );
            }
        }
        else if constexpr( FOLD == VRC_FOLD_MEAN )
        {
            meanLo = vrc_float_bits( state.x );
            meanHi = vrc_float_bits( state.y );
            meanCount += nSamples - before;
        }
        else
        {
            bits = state.y != 0.0f ? vrc_float_bits( state.x ) : VRC_MIP_EMPTY;
            if constexpr( DEPTH )
                depth = state.y != 0.0f ? state.z : depth;
        }
    }
    if constexpr( FOLD == VRC_FOLD_FIRST )
    {
        /* the gradient: gathered where this pass lowered D (its nodes, its atlas), else what the passes before left */
        float g[3] = { 0.0f, 0.0f, 0.0f };
        if( where != 0u )
        {
            if( where != VRC_ISO_WHERE_UNIFORM && hitNode < f.nodeCount )
                vrc_iso_gradient< ATLAS_T, BIG >( f, nodes[hitNode], atlas, where - 1u, g );
        }
        else if( bits != VRC_MIP_EMPTY )
        {
            g[0] = f.isoGrad[3u * pixelPos];
            g[1] = f.isoGrad[3u * pixelPos + 1u];
            g[2] = f.isoGrad[3u * pixelPos + 2u];
        }
        f.mipMax[pixelPos] = bits;
        f.mipDepth[pixelPos] = depth;
        f.isoGrad[3u * pixelPos] = g[0];
        f.isoGrad[3u * pixelPos + 1u] = g[1];
        f.isoGrad[3u * pixelPos + 2u] = g[2];
        if( bits != VRC_MIP_EMPTY )
        {
            const vrc_f4 e = vrc_classify_mip( tfp, f.isoClassify, cls );
            const float sh = vrc_iso_shade( g, r.dir, f.isoAmbient );
            vrc_f4 p;
            p.x = e.x * sh;
            p.y = e.y * sh;
            p.z = e.z * sh;
            p.w = e.w;
            pixelBuffer[pixelPos] = p;
        }
        else if( f.clearFirst )
            pixelBuffer[pixelPos] = zero;
    }
    else if constexpr( FOLD == VRC_FOLD_MEAN )
    {
        f.meanSum[pixelPos] = ( (unsigned long long)meanHi << 32 ) | meanLo;
        f.meanCount[pixelPos] = meanCount;
        if( meanCount != 0u )
            pixelBuffer[pixelPos] = vrc_classify_mip( tfp, vrc_mean_value< !FLOAT_M >( meanLo, meanHi, meanCount, 0.0 ), cls );
        else if( f.clearFirst )
            pixelBuffer[pixelPos] = zero;
    }
    else
    {
        f.mipMax[pixelPos] = bits;
        if( bits != VRC_MIP_EMPTY )
        {
            float d;
            if constexpr( !FLOAT_M )
                d = (float)bits;
            else
                d = vrc_bits_float( bits );
            if constexpr( DEPTH )
            {
                f.mipDepth[pixelPos] = depth;
                vrc_f4 e = vrc_classify_mip( tfp, d, cls );
                if( f.mipCue > 0.0f )
                {
                    const float w = vrc_mip_cue_weight( f.mipCue, depth, r.tNearGlobal, r.tFarGlobal );
                    e.x = w * e.x;
                    e.y = w * e.y;
                    e.z = w * e.z;
                    e.w = w * e.w;
                }
                pixelBuffer[pixelPos] = e;
            }
            else
            pixelBuffer[pixelPos] = vrc_classify_mip( tfp, d, cls );
        }
        else
        {
            if constexpr( DEPTH )
                f.mipDepth[pixelPos] = vrc_bits_float( 0x7F800000u );
            if( f.clearFirst )
                pixelBuffer[pixelPos] = zero;
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * Slice pixel (include/vrc_hip.h, "A slice frame"): one sample per ray, where it meets vrc_frame::slicePlane.  No march,
 * no step, no lattice: the ray parameter of the plane, the position, the node whose box contains it, one point sample or
 * eight taps, one classification.  The passes of a frame meet in vrc_frame::mipMax (the bits of V) and mipDepth
 * (D = t_p): the first pass writes both for every pixel, a later one samples only where D is still +infinity.
 * ---------------------------------------------------------------------------------------- */
/* the ray of pixel rayIndex into the ray cache (f.rayMode == VRC_RAY_STORE): what vrc_ray_from_cache reads, plane for
 * plane what vrc_pixel_grid_dda stores */
VRC_HD void vrc_ray_to_cache( const vrc_frame& f, uint32_t rayIndex, const vrc_ray& r )
{
    float* const rc = f.rayCache + rayIndex;
    const uint32_t P = f.rayCachePlane;
    rc[0] = r.dir.x;
    rc[P] = r.dir.y;
    rc[2u * P] = r.dir.z;
    rc[3u * P] = r.invDir.x;
    rc[4u * P] = r.invDir.y;
    rc[5u * P] = r.invDir.z;
    rc[6u * P] = r.tNearGlobal;
    rc[7u * P] = r.tFarGlobal;
    rc[8u * P] = r.tNearPlane;
    rc[9u * P] = vrc_bits_float( r.hit ? 1u : 0u );
}

/* how far the containment test on the ray is widened: a few units in the last place of t */
VRC_HD float vrc_slice_tolerance( float t )
{
    VRC_STRICT_FP
    const float a = fabsf( t );
    return 2e-6f * ( a > 1.0f ? a : 1.0f );
}

/* the ray parameter at which r meets the plane, where the pixel takes its sample at all: the clip planes' expressions in
 * their order, without their VRC_EPSILON -- a ray in the plane takes none */
VRC_HD bool vrc_slice_parameter( const vrc_frame& f, const vrc_ray& r, float& t )
{
    VRC_STRICT_FP
    t = 0.0f;
    if( !r.hit )
        return false;
    const vrc_f3 n = { f.slicePlane[0], f.slicePlane[1], f.slicePlane[2] };
    const float rn = vrc_dot( r.dir, n );
    if( rn == 0.0f )
        return false;
    t = -( vrc_dot( n, r.origin ) + f.slicePlane[3] ) / rn;
    const float lo = fmaxf( r.tNearGlobal, r.tNearPlane );
    return lo <= t && t <= r.tFarGlobal; /* (a NaN takes no sample) */
}

/* does the box contain the ray's point at t?  Decided on the ray: t in the slab test's interval, widened by tol on both
 * sides, faces included */
VRC_HD bool vrc_slice_box_contains( const vrc_ray& r, const float* aabbMin, const float* aabbSize, float t, float tol )
{
    VRC_STRICT_FP
    const vrc_f3 boxMin = { aabbMin[0], aabbMin[1], aabbMin[2] };
    const vrc_f3 boxMax = { boxMin.x + aabbSize[0], boxMin.y + aabbSize[1], boxMin.z + aabbSize[2] };
    float tn = 0.0f, tf = 0.0f;
    (void)vrc_intersect_box( r.origin, r.invDir, boxMin, boxMax, &tn, &tf );
    return tn - tol <= t && t <= tf + tol;
}

/* the slot-local coordinate of a world position along one axis, clamped to the slot: every operation rounded */
VRC_HD float vrc_slice_local( float p, float boxMin, float voxPerWorld, float localOrigin, float hi )
{
    VRC_STRICT_FP
    const float d = p - boxMin;
    const float s = d * voxPerWorld;
    const float l = s + localOrigin;
    return fminf( fmaxf( l, 0.0f ), hi );
}

/* Grid form: the node of the brick-grid cell that holds P, looked up and not walked to; where that cell is empty or its
 * brick does not hold the ray's point at t (rounding put P across a cell face), the cells on the nearer side of P along
 * every axis, all seven combinations.  -1: no node of this pass contains P */
VRC_HD int32_t vrc_slice_grid_node( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node* __restrict__ nodes,
                                    const int32_t* __restrict__ gridTable, const vrc_f3& P, float t, float tol )
{
    const float p[3] = { P.x, P.y, P.z };
    int cell[3], other[3];
#pragma unroll
    for( int a = 0; a < 3; ++a )
    {
        VRC_STRICT_FP
        const float u = ( p[a] - f.gridMin[a] ) * f.invCellSize[a];
        const float fl = floorf( u );
        const int last = f.gridDim[a] - 1;
        const int c = fl > 0.0f ? ( fl < (float)last ? (int)fl : last ) : 0; /* (a NaN reads cell 0) */
        int o = ( u - fl ) < 0.5f ? c - 1 : c + 1;
        o = o < 0 ? 0 : ( o > last ? last : o );
        cell[a] = c;
        other[a] = o;
    }
    for( uint32_t m = 0; m < 8u; ++m )
    {
        if( ( ( m & 1u ) && other[0] == cell[0] ) || ( ( m & 2u ) && other[1] == cell[1] ) || ( ( m & 4u ) && other[2] == cell[2] ) )
            continue;
        const int cx = ( m & 1u ) ? other[0] : cell[0], cy = ( m & 2u ) ? other[1] : cell[1], cz = ( m & 4u ) ? other[2] : cell[2];
        const int32_t node = gridTable[( cz * f.gridDim[1] + cy ) * f.gridDim[0] + cx];
        if( node >= 0 && vrc_slice_box_contains( r, nodes[node].aabbMin, nodes[node].aabbSize, t, tol ) )
            return node;
    }
    return -1;
}

/* the sample of node n at P as the bits the running word holds: the stored voxel of a point sample of the 8- and 16-bit
 * atlases (an integer), the bits of a float otherwise -- all ones, which means "not sampled" there, is a NaN and is held as
 * another.  BIG: as vrc_projection_march, the slot's 64-bit base moves into the pointer */
template < bool LINEAR, typename ATLAS_T, bool BIG >
VRC_HD uint32_t vrc_slice_sample( const vrc_frame& f, const vrc_dev_node& n, const ATLAS_T* __restrict__ atlas, const vrc_f3& P )
{
    if constexpr( !LINEAR && sizeof( ATLAS_T ) <= 2 )
    {
        if( f.slotInfo != nullptr && n.slotInfoIndex != 0u )
        {
            const uint32_t word = f.slotInfo[n.slotInfoIndex - 1u];
            if( vrc_slot_holds_one_value( word ) )
                return word & VRC_SLOT_VALUE_MASK;
        }
    }
    vrc_dev_node local = n;
    const ATLAS_T* slot = atlas;
    if( BIG )
    {
        local.slotBase = 0u;
        slot = atlas + ( ( (uint64_t)n.slotBaseHi << 32 ) | n.slotBase );
    }
    const vrc_sampler sm = vrc_make_sampler( local, f );
    const float lx = vrc_slice_local( P.x, sm.minx, sm.kx, sm.ox, sm.hix );
    const float ly = vrc_slice_local( P.y, sm.miny, sm.ky, sm.oy, sm.hiy );
    const float lz = vrc_slice_local( P.z, sm.minz, sm.kz, sm.oz, sm.hiz );
    uint32_t bits;
    if constexpr( LINEAR )
    {
        const vrc_taps tp = vrc_trilinear_taps< true >( sm, lx, ly, lz );
        float v[8];
#pragma unroll
        for( int c = 0; c < 8; ++c )
            v[c] = (float)vrc_gather( slot, tp.ax[c & 1] + tp.ay[( c >> 1 ) & 1] + tp.az[c >> 2] );
        bits = vrc_float_bits( vrc_trilerp( v, tp.wx, tp.wy, tp.wz ) );
    }
    else
    {
        const ATLAS_T v = vrc_gather( slot, vrc_voxel_address( sm, (uint32_t)(int)lx, (uint32_t)(int)ly, (uint32_t)(int)lz ) );
        if constexpr( sizeof( ATLAS_T ) == 4 )
            bits = vrc_float_bits( v );
        else
            return (uint32_t)v;
    }
    return bits == VRC_MIP_EMPTY ? 0x7FC00000u : bits;
}

template < bool GRID, bool LINEAR, typename ATLAS_T, bool BIG >
VRC_HD void vrc_pixel_slice( const vrc_frame& f, const vrc_dev_node* __restrict__ nodes,
                             const int32_t* __restrict__ gridTable, const ATLAS_T* __restrict__ atlas,
                             const vrc_f4* __restrict__ tfp, const vrc_classifier& cls, vrc_f4* __restrict__ pixelBuffer,
                             uint32_t px, uint32_t py, uint32_t& nSamples, const uint16_t* candidates = nullptr,
                             uint32_t nCandidates = 0, uint32_t rayIndex = 0u )
{
    constexpr bool FLOAT_V = LINEAR || sizeof( ATLAS_T ) == 4;
    const uint32_t pixelPos = py * f.width + px;
    const float inf = vrc_bits_float( 0x7F800000u );
    /* the grid form keeps its rays in the ray cache as vrc_pixel_grid_dda does (the same planes, the same bits) */
    vrc_ray r;
    if( GRID && f.rayMode == VRC_RAY_LOAD )
        r = vrc_ray_from_cache( f, rayIndex );
    else
    {
        r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
        if( GRID && f.rayMode == VRC_RAY_STORE )
            vrc_ray_to_cache( f, rayIndex, r );
    }
    uint32_t bits = VRC_MIP_EMPTY;
    float depth = inf;
    if( !f.mipFirst )
    {
        bits = f.mipMax[pixelPos];
        depth = f.mipDepth[pixelPos];
    }
    bool sampled = false;
    float t;
    if( !( depth < inf ) && vrc_slice_parameter( f, r, t ) )
    {
        vrc_f3 P;
        {
            VRC_STRICT_FP
            P.x = r.origin.x + r.dir.x * t;
            P.y = r.origin.y + r.dir.y * t;
            P.z = r.origin.z + r.dir.z * t;
        }
        const float tol = vrc_slice_tolerance( t );
        int32_t node = -1;
        if constexpr( GRID )
            node = vrc_slice_grid_node( f, r, nodes, gridTable, P, t, tol );
        else
        {
            /* every node is a candidate, in list order, the first that contains P: no `break` at a brick beyond the
             * ray's interval (a brick the tile culling left out is hit by none of the tile's rays) */
            const uint32_t nLoop = candidates ? nCandidates : f.nodeCount;
            for( uint32_t c = 0; c < nLoop && node < 0; ++c )
            {
                const uint32_t i = candidates ? (uint32_t)candidates[c] : c;
                if( vrc_slice_box_contains( r, nodes[i].aabbMin, nodes[i].aabbSize, t, tol ) )
                    node = (int32_t)i;
            }
        }
        if( node >= 0 )
        {
            bits = vrc_slice_sample< LINEAR, ATLAS_T, BIG >( f, nodes[node], atlas, P );
            depth = t;
            sampled = true;
            nSamples += 1u;
        }
    }
    if( f.mipFirst || sampled )
    {
        f.mipMax[pixelPos] = bits;
        f.mipDepth[pixelPos] = depth;
    }
    if( sampled )
    {
        float d;
        if constexpr( FLOAT_V )
            d = vrc_bits_float( bits );
        else
            d = (float)bits;
        pixelBuffer[pixelPos] = vrc_classify_mip( tfp, d, cls );
    }
    else if( f.clearFirst )
    {
        const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
        pixelBuffer[pixelPos] = zero;
    }
}

#endif /* VRC_CORE_H */
