/*
 * vrc_plan.h -- what vrc_render decides from options and facts alone (host only: no HIP, no vrc_ctx, no vrc_pool).
 *
 * The options and per-frame latches of a context as two plain structs, and five decisions over them: which frame a
 * pass renders (vrc_plan_mode), which kernel form marches it (vrc_plan_form, vrc_plan_use_lds), whether that is the
 * table walk kernel (vrc_plan_table_walk), how a replayed frame stores its pixels (vrc_plan_store_through) and whether
 * it takes its rays' first visits from a table (vrc_plan_first_visit, vrc_plan_first_visit_build) or may march a visit
 * without the exit test (vrc_plan_lean_free_march), or reads resolved visit words (vrc_plan_walk_resolved).  A
 * refusal is a code and a message; the ORDER of the refusals is part of the contract (tests/test_render_plan_cpu.py
 * holds both functions to the text they replaced, message for message).
 *
 * And the two caches of a still view, each as what it remembers between calls plus the functions that read and write
 * that memory -- the context keeps the device memory, the event and the frames, and assigns none of this itself:
 *   ray cache   vrc_ray_state; vrc_plan_ray_cache (compute, store or load), vrc_ray_stored, vrc_ray_forget;
 *   walk cache  vrc_walk_state, vrc_walk_facts, vrc_walk_counted, vrc_walk_plan; vrc_walk_open (what the frame ends, is
 *               it a repeat, is the count's answer wanted), vrc_walk_decide (count, record, replay or walk; the replay
 *               instance; the four riders; what to allocate and build), vrc_walk_commit (what is remembered, by how far
 *               the caller got), vrc_walk_launched (the transitions behind the launches), vrc_walk_forget.
 * tests/test_walk_plan_cpu.py drives both through generated sequences of renders beside the text they replaced.
 */
#ifndef VRC_PLAN_H
#define VRC_PLAN_H

#include "../../include/vrc_hip.h"

/* the VRC_OPT_* values of a context (vrc_set_option / vrc_get_option), at their defaults */
struct vrc_options
{
    int64_t kernel = VRC_KERNEL_AUTO, variant = VRC_VARIANT_CUDARAYCASTER;
    int64_t filter = 0, tfFracBits = 8, stepping = 1;
    int64_t count = 0, timing = 1, streamMarkers = 0; /* VRC_OPT_COUNT_SAMPLES, _KERNEL_TIMING, _STREAM_MARKERS */
    int64_t depthSplit = 0, ertParts = 0;             /* VRC_OPT_DEPTH_SPLIT, _ERT_COMPACTION */
    int64_t packedAtlas = 1, uniformBricks = 1, greyTable = 1, tileOrder = 1, rayCache = 1;
    int64_t walkCache = 1, walkBudget = VRC_WALK_CACHE_DEFAULT_BUDGET, walkUniformOnly = 1;
    int64_t projection = VRC_PROJECTION_COMPOSITE, mipSkip = 1, mipFold = VRC_MIP_FOLD_MAX;
    int64_t mipDepth = 0, mipDepthCue = 0;     /* VRC_OPT_MIP_DEPTH; _MIP_DEPTH_CUE, thousandths */
    int64_t shading = 0, shadingAmbient = 250; /* VRC_OPT_SHADING; _SHADING_AMBIENT, thousandths */
    int64_t compositeDepth = 0, preint = 0;    /* VRC_OPT_COMPOSITE_DEPTH, thousandths; _PREINTEGRATION */
    int64_t storeThrough = 1;                  /* VRC_OPT_STORE_THROUGH */
    int64_t firstVisitTable = 1;               /* VRC_OPT_FIRST_VISIT_TABLE */
    int64_t leanFreeMarch = 1;                 /* VRC_OPT_LEAN_FREE_MARCH */
    int64_t walkResolved = 1;                  /* VRC_OPT_WALK_RESOLVED */
};

/* what the frame's first vrc_render read of the options its later passes must not change (-1 / false: none yet; written
 * by the pass that reads the option, forgotten by vrc_pre_render).  projection: of the first pass; fold: of the first
 * MIP pass; depth, cue: of the first maximum / minimum pass; iso*: vrc_set_isosurface's two values at the first ISO
 * pass; shading .. preint: of the first composite pass; slice*: vrc_set_slice's plane at the first slice pass */
struct vrc_latches
{
    int64_t projection = -1, fold = -1, depth = -1, cue = -1;
    bool iso = false;
    float isoValue = 0.0f, isoAmbient = 0.0f;
    int64_t shading = -1, shadingAmbient = -1, compositeDepth = -1, preint = -1;
    bool slice = false;
    float slicePlane[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
};

struct vrc_refusal
{
    int code; /* VRC_OK: not refused */
    const char* msg;
};

/* the frame a pass renders */
struct vrc_mode
{
    bool iso = false, mip = false;           /* iso: a MIP frame with the first-crossing fold (mip is set too) */
    bool mipDepth = false, mean = false;     /* depth tracking: the maximum and the minimum only; the mean reads neither option */
    bool shade = false, cdepth = false, preint = false; /* the composite extensions: read by composite frames only */
    bool slice = false; /* a slice frame: one sample per ray where it meets vrc_set_slice's plane; none of the above is set */
    bool linear = false;
    /* samples classified one by one (padded transfer function in the table buffer) whenever the 257-entry classified
     * table cannot be used: continuous or 16-bit densities (MIP: the one classification per ray reads it too) */
    bool classify = false;
    /* the plain composite: none of the frames marched by the gather kernels of the extensions */
    bool plain() const { return !mip && !shade && !cdepth && !preint && !slice; }
};

/* A frame marched by the gather kernels of an extension is not defined for the staged and packed forms, per-ray LOD and
 * the glRaycaster variant: the three refusals every such mode has, in this order */
#define VRC_PLAN_GATHER_ONLY( form, name, cut )                                                                                  \
    { "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no " form " form; " name " is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)", \
      "vrc_render: vrc_set_ray_lod is on; " name " " cut " a per-brick cut",                                                    \
      "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; " name " is defined on the cudaRaycaster variant's sample set" }
struct vrc_gather_only
{
    const char *kernel, *rayLod, *variant;
};
static const vrc_gather_only vrc_plan_iso_only = VRC_PLAN_GATHER_ONLY( "isosurface", "VRC_OPT_PROJECTION = ISO", "renders" );
static const vrc_gather_only vrc_plan_mip_only = VRC_PLAN_GATHER_ONLY( "maximum-intensity", "VRC_OPT_PROJECTION = MIP", "renders" );
static const vrc_gather_only vrc_plan_slice_only = VRC_PLAN_GATHER_ONLY( "slice", "VRC_OPT_PROJECTION = SLICE", "renders" );
static const vrc_gather_only vrc_plan_cdepth_only = VRC_PLAN_GATHER_ONLY( "depth-tracking", "VRC_OPT_COMPOSITE_DEPTH", "tracks" );
static const vrc_gather_only vrc_plan_preint_only = VRC_PLAN_GATHER_ONLY( "pre-integrated", "VRC_OPT_PREINTEGRATION = 1", "renders" );
static const vrc_gather_only vrc_plan_shade_only = VRC_PLAN_GATHER_ONLY( "shaded", "VRC_OPT_SHADING = 1", "renders" );
#undef VRC_PLAN_GATHER_ONLY

inline bool vrc_plan_staged_kernel( const vrc_options& o ) { return o.kernel == VRC_KERNEL_LDS || o.kernel == VRC_KERNEL_PACKED; }

inline const char* vrc_plan_gather_only( const vrc_options& o, bool rayLod, const vrc_gather_only& r )
{
    return vrc_plan_staged_kernel( o ) ? r.kernel : rayLod ? r.rayLod : o.variant != VRC_VARIANT_CUDARAYCASTER ? r.variant : nullptr;
}

#define VRC_PLAN_REFUSE( text ) return vrc_refusal{ VRC_EINVAL, text }

/* an option the frame's first pass latched (-1: none yet) and this pass reads differently */
inline bool vrc_plan_changed( int64_t latched, int64_t now ) { return latched >= 0 && latched != now; }

/* Which frame is this pass, and may it be?  Reads the options, the latches of the passes before, vrc_set_ray_lod,
 * vrc_set_isosurface (isoSet: called at all, and its two values), the bytes of an atlas element and vrc_set_slice
 * (sliceSet: called at all, and its plane; read by a slice frame only).  Changes nothing: a refused pass has latched
 * nothing. */
inline vrc_refusal vrc_plan_mode( const vrc_options& o, const vrc_latches& l, bool rayLod, bool isoSet, float isoValue,
                                  float isoAmbient, uint32_t elemBytes, vrc_mode& m, bool sliceSet = false,
                                  const float* slicePlane = nullptr )
{
#define VRC_PLAN_BETWEEN " changed between vrc_pre_render and vrc_post_render; "
    m = vrc_mode();
    if( elemBytes == 4 && vrc_plan_staged_kernel( o ) )
        VRC_PLAN_REFUSE( "vrc_render: 32-bit and float voxels are marched by gathers; the LDS-staged and tap-packed "
                         "forms take 8- and 16-bit voxels (VRC_OPT_KERNEL = AUTO, REFERENCE_ORDER or GRID_DDA)" );
    /* an isosurface frame reads none of the MIP frame's options but VRC_OPT_MIP_SKIP, and is served and refused as one */
    m.iso = o.projection == VRC_PROJECTION_ISO;
    m.mip = o.projection == VRC_PROJECTION_MIP || m.iso;
    /* a slice frame reads none of the options of the MIP, isosurface and composite frames, and is served and refused as
     * a MIP frame is */
    m.slice = o.projection == VRC_PROJECTION_SLICE;
    const bool fold = m.mip && !m.iso; /* a MIP frame that reads VRC_OPT_MIP_FOLD */
    m.mean = fold && o.mipFold == VRC_MIP_FOLD_MEAN;
    if( vrc_plan_changed( l.projection, o.projection ) )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PROJECTION" VRC_PLAN_BETWEEN "the passes of one frame take one projection" );
    if( m.iso && !isoSet )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PROJECTION = ISO needs vrc_set_isosurface first" );
    if( m.iso && l.iso && ( l.isoValue != isoValue || l.isoAmbient != isoAmbient ) )
        VRC_PLAN_REFUSE( "vrc_render: vrc_set_isosurface changed iso_value or ambient between vrc_pre_render and "
                         "vrc_post_render; the passes of one frame take one isosurface" );
    if( m.slice && ( !sliceSet || slicePlane == nullptr ) )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PROJECTION = SLICE needs vrc_set_slice first" );
    if( m.slice && l.slice &&
        ( l.slicePlane[0] != slicePlane[0] || l.slicePlane[1] != slicePlane[1] || l.slicePlane[2] != slicePlane[2] ||
          l.slicePlane[3] != slicePlane[3] ) )
        VRC_PLAN_REFUSE( "vrc_render: vrc_set_slice changed the plane between vrc_pre_render and vrc_post_render; the "
                         "passes of one frame take one plane" );
    if( fold && vrc_plan_changed( l.fold, o.mipFold ) )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_MIP_FOLD" VRC_PLAN_BETWEEN "the passes of one frame take one fold" );
    m.mipDepth = m.iso || ( fold && !m.mean && ( o.mipDepth != 0 || o.mipDepthCue > 0 ) );
    if( fold && !m.mean )
    {
        if( vrc_plan_changed( l.depth, o.mipDepth ) )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_MIP_DEPTH" VRC_PLAN_BETWEEN "the passes of one frame all keep the depth or none does" );
        if( vrc_plan_changed( l.cue, o.mipDepthCue ) )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_MIP_DEPTH_CUE" VRC_PLAN_BETWEEN "the passes of one frame take one cue strength" );
    }
    const char* no = nullptr;
    /* what the maximum-intensity projection is not defined for (include/vrc_hip.h) */
    if( m.mip && ( no = vrc_plan_gather_only( o, rayLod, m.iso ? vrc_plan_iso_only : vrc_plan_mip_only ) ) )
        VRC_PLAN_REFUSE( no );
    if( m.slice && ( no = vrc_plan_gather_only( o, rayLod, vrc_plan_slice_only ) ) )
        VRC_PLAN_REFUSE( no );
    const bool composite = !m.mip && !m.slice; /* a frame that reads the composite extensions' options */
    m.shade = composite && o.shading != 0;
    m.cdepth = composite && o.compositeDepth != 0;
    m.preint = composite && o.preint != 0;
    if( composite )
    {
        if( vrc_plan_changed( l.shading, o.shading ) )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_SHADING" VRC_PLAN_BETWEEN "the passes of one frame are all shaded or none is" );
        if( vrc_plan_changed( l.shadingAmbient, o.shadingAmbient ) )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_SHADING_AMBIENT" VRC_PLAN_BETWEEN "the passes of one frame take one ambient share" );
        if( vrc_plan_changed( l.compositeDepth, o.compositeDepth ) )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_COMPOSITE_DEPTH" VRC_PLAN_BETWEEN "the passes of one frame cross one threshold" );
    }
    if( m.cdepth )
    {
        if( m.shade )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_COMPOSITE_DEPTH; alpha does not "
                             "depend on shading: render the unshaded frame to pick in a shaded picture" );
        if( ( no = vrc_plan_gather_only( o, rayLod, vrc_plan_cdepth_only ) ) )
            VRC_PLAN_REFUSE( no );
    }
    if( composite && vrc_plan_changed( l.preint, o.preint ) )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PREINTEGRATION" VRC_PLAN_BETWEEN "the passes of one frame are all pre-integrated or none is" );
    if( m.preint )
    {
        if( m.shade )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_PREINTEGRATION; a step has no one "
                             "gradient: the two are not combined" );
        if( m.cdepth )
            VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_COMPOSITE_DEPTH together with VRC_OPT_PREINTEGRATION; the depth is "
                             "defined on the plain frame's alpha: the two are not combined" );
        if( ( no = vrc_plan_gather_only( o, rayLod, vrc_plan_preint_only ) ) )
            VRC_PLAN_REFUSE( no );
    }
    if( m.shade && ( no = vrc_plan_gather_only( o, rayLod, vrc_plan_shade_only ) ) )
        VRC_PLAN_REFUSE( no );
    m.linear = o.filter == VRC_FILTER_TRILINEAR;
    m.classify = m.linear || elemBytes != 1 || m.mip || m.slice;
    return vrc_refusal{ VRC_OK, nullptr };
#undef VRC_PLAN_BETWEEN
}

/* what the form of the march depends on beside the options and the mode: vrc_set_ray_lod, the cached node table
 * (vrc_host_tables), the call and the pool */
struct vrc_form_facts
{
    bool rayLod;
    bool gridOk, oneCell, lodOk, clamp;
    uint32_t nNodes, samplesPerPixel;
    uint32_t slotDim[3];
    uint32_t elemBytes;
    bool bigAtlas;
    bool packedPossible; /* pool_packed_possible */
};

enum vrc_packed_wish
{
    VRC_PACKED_NONE = 0,
    VRC_PACKED_WANTED,  /* VRC_KERNEL_AUTO, eligible: the packed form if the pool has (the memory for) the second atlas */
    VRC_PACKED_REQUIRED /* VRC_KERNEL_PACKED: that, or VRC_ENOMEM */
};

struct vrc_form
{
    bool glSuper = false;
    bool slotsFit8Bits = false;
    bool useDda = false;
    bool ldsEligible = false, ldsLodEligible = false;
    vrc_packed_wish packed = VRC_PACKED_NONE;
    bool usePacked = false, useLds = false; /* the caller's, once the pool has answered the wish (vrc_plan_use_lds) */
};

/* the last refusal of all: the required packed form, and the pool could not build its second atlas */
static const vrc_refusal vrc_plan_no_packed_memory = {
    VRC_ENOMEM, "vrc_render: no device memory for the tap-packed atlas (2.25 times the brick atlas)" };

inline vrc_refusal vrc_plan_form( const vrc_options& o, const vrc_mode& m, const vrc_form_facts& k, vrc_form& fm )
{
    fm = vrc_form();
    if( k.rayLod )
    {
        if( !k.lodOk )
            return vrc_refusal{ VRC_EHIERARCHY, "vrc_render: per-ray LOD needs a brick hierarchy (every level a regular grid of bricks, one brick per cell)" };
        if( o.variant != VRC_VARIANT_CUDARAYCASTER )
            VRC_PLAN_REFUSE( "vrc_render: per-ray LOD is defined for the cudaRaycaster variant only" );
        /* AUTO: the LDS-staged form for the trilinear filter where it applies, else the gather form; GRID_DDA asks for
         * the gather form, LDS for the staged one */
        if( o.kernel == VRC_KERNEL_REFERENCE_ORDER )
            VRC_PLAN_REFUSE( "vrc_render: per-ray LOD walks the hierarchy; VRC_OPT_KERNEL = AUTO, GRID_DDA (gathers), LDS or PACKED" );
    }
    fm.useDda = k.gridOk;
    /* AUTO keeps the reference's frame: bricks of one size are met by the grid walk in the reference's
     * order; a list that mixes brick sizes (an LOD cut) is composited in the host's centre-distance order,
     * which is not a visibility order for every ray (quirk Q6) -- the literal loop reproduces that as long
     * as testing every brick per ray is affordable.  GRID_DDA can always be asked for (true visibility
     * order); the trilinear filter (extension, no reference frame to keep) stays on the grid. */
    if( o.kernel == VRC_KERNEL_AUTO && fm.useDda && !k.oneCell && !m.linear && k.nNodes <= VRC_REFERENCE_ORDER_MAX_NODES )
        fm.useDda = false;
    /* glRaycaster with more than one sample per pixel (fragRaycast.glsl:121-129): the pixel is averaged brick by
     * brick in the host's order -- the reference-order loop is the only form that has a "brick by brick" */
    fm.glSuper = o.variant == VRC_VARIANT_GLRAYCASTER && k.samplesPerPixel > 1u;
    if( fm.glSuper )
    {
        if( o.kernel == VRC_KERNEL_GRID_DDA || o.kernel == VRC_KERNEL_LDS )
            VRC_PLAN_REFUSE( "vrc_render: the glRaycaster variant with samplesPerPixel > 1 is rendered by the "
                             "reference-order kernel (VRC_OPT_KERNEL = AUTO or REFERENCE_ORDER)" );
        fm.useDda = false;
    }
    if( o.kernel == VRC_KERNEL_REFERENCE_ORDER )
        fm.useDda = false;
    else if( o.kernel == VRC_KERNEL_GRID_DDA && !k.gridOk && !k.rayLod )
        VRC_PLAN_REFUSE( "vrc_render: node set is not grid-aligned; GRID_DDA unavailable" );
    /* LDS-staged kernel: brick-grid DDA + unclamped sampler (overlap >= 1).  AUTO takes it for
     * the trilinear filter (eight taps per sample), the gather kernel for point sampling. */
    /* its trilinear form takes the transfer-function texel and CUDA's 1.8 fixed-point lerp weight out of one
     * float -> integer conversion (vrc_kernels_lds.hip: lds_classify): other weight widths use the gather form */
    /* slot-local positions in 8.24 fixed point (fixed-point stepping, the per-axis address tables, the LDS kernel's boxes)
     * need every slot dimension to fit eight bits; pool creation bounds a slot's VOLUME only (2^24 voxels), so a flat
     * or long brick can exceed it: such pools march with float positions */
    fm.slotsFit8Bits = k.slotDim[0] <= 248u && k.slotDim[1] <= 248u && k.slotDim[2] <= 248u;
    /* 16-bit voxels: its trilinear form only (a 16-bit density does not index the classified table of the point form) */
    const bool ldsVoxels = fm.slotsFit8Bits && ( k.elemBytes == 1 || ( k.elemBytes == 2 && m.linear ) );
    /* atlases of more than 2^32 voxels (64-bit slot bases): its trilinear form only */
    fm.ldsEligible = k.gridOk && !k.clamp && ldsVoxels && ( !k.bigAtlas || m.linear ) && ( !m.linear || o.tfFracBits == 8 );
    if( !k.rayLod && o.kernel == VRC_KERNEL_LDS && !fm.ldsEligible )
        VRC_PLAN_REFUSE( "vrc_render: the LDS kernel needs a grid-aligned node set of 8-bit bricks in an atlas of at most 2^32 voxels (trilinear: 8- or 16-bit, any atlas, VRC_OPT_TF_FRAC_BITS = 8) with overlap >= 1" );
    /* per-ray LOD: the staged kernel's trilinear form only (samples classified one by one: no table per level) */
    fm.ldsLodEligible = k.rayLod && m.linear && !k.clamp && ldsVoxels && !k.bigAtlas && o.tfFracBits == 8;
    if( k.rayLod && o.kernel == VRC_KERNEL_LDS && !fm.ldsLodEligible )
        VRC_PLAN_REFUSE( "vrc_render: under per-ray LOD the LDS kernel needs the trilinear filter, 8- or 16-bit bricks with overlap >= 1 and VRC_OPT_TF_FRAC_BITS = 8" );
    /* tap-packed atlas (VRC_KERNEL_PACKED; vrc_core.h): the trilinear filter as two gathers per sample.  Needs what its
     * positions and its classifier need -- 8- or 16-bit bricks with overlap >= 1 in slots of at most 248 voxels a side,
     * VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping -- and 2.25 times the atlas in device memory; either brick
     * enumeration (grid walk where the node set is grid-aligned, else the reference-order loop) */
    const bool packedEligible = m.linear && !fm.glSuper && m.plain() && !k.clamp && fm.slotsFit8Bits && k.packedPossible &&
                                o.tfFracBits == 8 && o.stepping != 0;
    if( o.kernel == VRC_KERNEL_PACKED )
    {
        if( !packedEligible )
            VRC_PLAN_REFUSE( "vrc_render: the packed kernel needs the trilinear filter on 8- or 16-bit bricks with overlap >= 1 (slots of at most 248 voxels a side), VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping" );
        fm.packed = VRC_PACKED_REQUIRED;
    }
    else if( o.kernel == VRC_KERNEL_AUTO && packedEligible && o.packedAtlas )
        /* measured on C2: 1.2 against 1.7 ms along the axis, 1.5 against 2.4 at 30/20 degrees;
         * under per-ray LOD 1.4-2.1 x the staged form (profiles/r4_c5_trilinear_three_forms.txt); without the memory for
         * it the frame takes the staged form */
        fm.packed = VRC_PACKED_WANTED;
    return vrc_refusal{ VRC_OK, nullptr };
#undef VRC_PLAN_REFUSE
}

/* the LDS-staged form, once it is known whether the frame marches the packed atlas */
inline bool vrc_plan_use_lds( const vrc_options& o, const vrc_mode& m, const vrc_form_facts& k, const vrc_form& fm, bool usePacked )
{
    return k.rayLod ? ( fm.ldsLodEligible && o.kernel != VRC_KERNEL_GRID_DDA && !usePacked )
                    : !fm.glSuper && !usePacked && m.plain() &&
                          ( o.kernel == VRC_KERNEL_LDS || ( o.kernel == VRC_KERNEL_AUTO && m.linear && fm.ldsEligible ) );
}

/* the table-driven point-sampling walk kernel of the plain composite (fm.useLds set): what the depth split and ray
 * compaction exist for */
inline bool vrc_plan_table_walk( const vrc_options& o, const vrc_mode& m, const vrc_form_facts& k, const vrc_form& fm )
{
    return m.plain() && fm.useDda && !fm.useLds && !k.rayLod && !m.linear && k.elemBytes == 1 && !k.bigAtlas && !k.clamp &&
           o.stepping != 0 && fm.slotsFit8Bits;
}

/* write-through pixel stores (VRC_OPT_STORE_THROUGH; vrc_core.h: vrc_store_pixel): a replayed frame (walkUsed:
 * VRC_OPT_WALK_CACHE_USED of this pass, 4 = replay) whose pixel buffer, width * height * 16 bytes, a 32-bit buffer offset
 * spans -- 4 GiB and more keeps the plain stores */
inline bool vrc_plan_store_through( const vrc_options& o, int64_t walkUsed, uint32_t width, uint32_t height )
{
    return o.storeThrough != 0 && walkUsed == 4 && (uint64_t)width * height < ( 1ull << 28 ); /* (pixels of 16 bytes) */
}

/* the first-visit table (VRC_OPT_FIRST_VISIT_TABLE; vrc_core.h: vrc_first_visit_row, vrc_frame::firstVisit): a pass
 * takes the first uniform visit of its rays from the table where the option is on, the pass is a replayed lean frame
 * (walkUsed 4, walkLean != 0) that starts from zero (a later pass of a frame starts from the pixels so far, and takes
 * the four-float form at that: it neither reads nor rebuilds a grey frame's table), is not classified per sample, does
 * not count its samples -- the counted instances march every visit -- and the table is current: built for the
 * classified table's present generation, in the form (two floats or four) the pass marches */
struct vrc_first_visit_facts
{
    int64_t walkUsed; /* VRC_OPT_WALK_CACHE_USED of this pass */
    uint32_t walkLean;
    bool clearFirst;
    bool classify; /* vrc_mode::classify */
    bool current;
};
inline bool vrc_plan_first_visit_wanted( const vrc_options& o, const vrc_first_visit_facts& k )
{
    return o.firstVisitTable != 0 && k.walkUsed == 4 && k.walkLean != 0u && k.clearFirst && !k.classify && o.count == 0;
}
inline bool vrc_plan_first_visit( const vrc_options& o, const vrc_first_visit_facts& k )
{
    return vrc_plan_first_visit_wanted( o, k ) && k.current;
}
/* ... and a table that is not current is built by such a pass only if the vrc_render before it, in the same context,
 * rendered with the same generation of the classified table: someone dragging a transfer-function point over a still
 * view pays no build per edit -- one frame marches as ever, the next builds the table and uses it */
inline bool vrc_plan_first_visit_build( const vrc_options& o, const vrc_first_visit_facts& k, bool prevSameGeneration )
{
    return vrc_plan_first_visit_wanted( o, k ) && !k.current && prevSameGeneration;
}

/* the free body of the lean march (VRC_OPT_LEAN_FREE_MARCH; vrc_core.h: vrc_march_uniform_free, vrc_frame::leanFree):
 * where the option is on and the pass is a replayed lean frame (walkUsed 4, walkLean != 0) that is not classified per
 * sample and does not count its samples -- the counted instances hold no such body.  Whether the pass clears does not
 * matter: the per-lane test reads the alpha the visit starts from */
inline bool vrc_plan_lean_free_march( const vrc_options& o, int64_t walkUsed, uint32_t walkLean, bool classify )
{
    return o.leanFreeMarch != 0 && walkUsed == 4 && walkLean != 0u && !classify && o.count == 0;
}

/* the resolved visit words (VRC_OPT_WALK_RESOLVED; vrc_core.h: vrc_walk_resolved_word, vrc_frame::walkResolved): where
 * the option is on, the pass is handed the uniform-only instance (uniformOnly: vrc_frame::walkLean is
 * VRC_WALK_LEAN_UNIFORM -- a replayed lean frame, its lists, the pool's uploads and slotInfo those the count pass read),
 * does not count its samples -- the counted instances read the lists -- and the planes fit VRC_OPT_WALK_CACHE_BUDGET
 * beside the lists (fits).  Such a pass builds the planes if it has none for its lists, uploads and slotInfo */
inline bool vrc_plan_walk_resolved( const vrc_options& o, bool uniformOnly, bool fits )
{
    return o.walkResolved != 0 && uniformOnly && fits && o.count == 0;
}

/* ---------------------------------------------------------------------------------------- */
/* The values of vrc_core.h this header speaks of and does not include (a source that includes both checks them here) */
#ifndef VRC_RAY_COMPUTE
#define VRC_RAY_COMPUTE 0u
#define VRC_RAY_STORE 1u
#define VRC_RAY_LOAD 2u
#endif
#ifndef VRC_WALK_LEAN_UNIFORM
#define VRC_WALK_LEAN_UNIFORM 2u
#endif
static_assert( VRC_RAY_COMPUTE == 0u && VRC_RAY_STORE == 1u && VRC_RAY_LOAD == 2u && VRC_WALK_LEAN_UNIFORM == 2u,
               "vrc_plan.h and vrc_core.h name the same modes" );

/* ray cache (VRC_OPT_RAY_CACHE; vrc_core.h: vrc_frame::rayCache).  prevSet: there was a vrc_render before that could have
 * used the cache; valid: the planes hold the rays of exactly its frame constants */
struct vrc_ray_state
{
    bool valid = false, prevSet = false;
};

/* A frame whose ray constants differ from those of the vrc_render before (sameAsPrev: prevSet, and ray_constants_equal)
 * computes its rays -- a moving camera pays nothing; the first that repeats them also stores them, and the ones after
 * that load them.  A frame that cannot use the cache (eligible: vrc_api.hip) forgets the one before.  The planes a
 * storing frame writes are valid once its march is on the stream (vrc_ray_stored) */
inline uint32_t vrc_plan_ray_cache( vrc_ray_state& s, bool eligible, bool sameAsPrev )
{
    if( !eligible )
        s.valid = s.prevSet = false;
    else if( !sameAsPrev )
        s.valid = false;
    const uint32_t mode = !( eligible && sameAsPrev ) ? VRC_RAY_COMPUTE : s.valid ? VRC_RAY_LOAD : VRC_RAY_STORE;
    s.prevSet = eligible;
    return mode;
}
inline void vrc_ray_stored( vrc_ray_state& s ) { s.valid = true; }
/* whatever the planes were written under is gone: the stream, the row map's contents, the option */
inline void vrc_ray_forget( vrc_ray_state& s ) { s.valid = s.prevSet = false; }

/* walk cache (VRC_OPT_WALK_CACHE; vrc_core.h: vrc_frame::walkCache): a frame that loads its rays, of the instances the
 * replay march exists for (vrc_internal.h: vrc_walk_replay_eligible).  The first such frame that repeats the one before
 * also runs the count pass; the first one after its result has arrived (polled, never waited for) sizes the planes and
 * runs the record pass; the ones after that replay.  Both passes go on the stream in front of the march's timing pair
 * and are no marches: not timed, not counted as launches.
 * state: IDLE nothing known; COUNTING the count pass is on the stream, its result on the way behind the event; VALID the
 * planes hold the lists of the listed frame's constants over the node table as it is.  Nothing exists before the first
 * count pass: a camera that moves every frame allocates nothing.  The count pass runs only for a frame whose constants,
 * node list and (option at 1) pool uploads are those of the vrc_render before, prev*: what changes every call -- passes
 * over different node subsets, bricks streaming in -- launches nothing extra.
 * Whatever the lists depend on starts them over when it changes: the frame constants (vrc_walk_open), the node list,
 * the stream, the row map and the two options, where they are set (vrc_walk_forget); the transfer function, the
 * uniformity words and the pixel buffer's contents are not among them.  What the lists do not depend on may still decide
 * whether they are worth using: where every visit gathers the replay is no faster than the walk, and by 1 to 3 % slower
 * (profiles/r10_walk_cache.txt), so with the option at 1 a view more than half of whose visits gather, by the count pass
 * and the uniformity words it read, is not recorded and stays on the walk until the pool's uploads or
 * VRC_OPT_UNIFORM_BRICKS change; VRC_WALK_CACHE_ALWAYS replays whatever the bricks hold. */
enum
{
    VRC_WALK_IDLE = 0,
    VRC_WALK_COUNTING = 1,
    VRC_WALK_VALID = 2
};

/* what the walk cache remembers between calls, the first-visit table's part included */
struct vrc_walk_state
{
    int state = VRC_WALK_IDLE;
    uint32_t k = 0; /* visits per ray the planes hold */
    /* the form of the lists (vrc_core.h: vrc_frame::walkLean).  leanAsked: what the host saw when the count pass went
     * out -- a step that vrc_exact_step_count counts, a pool whose slot indices fit the word -- and so what that pass was
     * asked to check; part of what the lists are valid for.  lean: the form the record pass wrote */
    bool leanAsked = false, lean = false;
    /* what the count pass of the lists in the planes said of the slot words it read, those of gen and slotInfo --
     * compared for the uniform-only instance whatever VRC_OPT_WALK_CACHE says, because at VRC_WALK_CACHE_ALWAYS the
     * lists outlive an upload and that answer does not */
    unsigned long long gathers = 0;
    uint64_t gen = 0; /* gen, slotInfo: the uploads and the uniformity words the count pass read */
    const void* slotInfo = nullptr;
    bool prevSet = false; /* the vrc_render before: there was one, and its uploads (its frame: the context's) */
    uint64_t prevGen = 0;
    /* the resolved visit words (VRC_OPT_WALK_RESOLVED): k planes beside the lists, built from them and from the slot
     * words by the first frame that is handed the uniform-only instance without them.  resolvedValid: the planes hold the
     * words of the lists as recorded (a record pass ends it) under the uploads resolvedGen and the array
     * resolvedSlotInfo; a frame that finds another of the three takes the list words and drops the planes */
    bool resolvedValid = false;
    uint64_t resolvedGen = 0;
    const void* resolvedSlotInfo = nullptr;
    /* the first-visit table (VRC_OPT_FIRST_VISIT_TABLE).  It depends on the classified table alone -- transfer function,
     * opacity correction -- and on the form the frame marches, not on the view, the volume or the lists.  tableGen,
     * tableGrey: the generation (lutGen) and form it was built for (0: never).  tablePrevGen: the generation the
     * vrc_render before rendered with (0: none) */
    uint64_t tableGen = 0, tablePrevGen = 0;
    bool tableGrey = false;
};

/* what a call finds, and the plan may not work out itself */
struct vrc_walk_facts
{
    /* VRC_OPT_WALK_CACHE on, the ray cache in LOAD, vrc_walk_replay_eligible, nodes and a plane at all (the plan adds
     * that the planes of one visit fit: vrc_walk_fits) */
    bool eligibleSoFar;
    /* the form of the lists.  A lean list holds every visit's step count and slot index in one word of 12 + 20 bits.
     * What the host can see of that: the step is one vrc_exact_step_count counts (its own test, asked with a travel that
     * passes it), and the pool's slot indices fit.  The rest -- no visit whose count is inexact or takes more than 12
     * bits -- the count pass reports with the count */
    bool leanAsked;
    bool sameAsListed; /* walk_constants_equal: the frame the lists were counted for (read unless IDLE) and this one */
    bool sameAsPrev;   /* ... the frame of the vrc_render before (prevSet, and equal) and this one */
    bool sameNodes;    /* the node list of the vrc_render before, on the same pool */
    uint64_t uploadGen; /* the pool's (compared only where the choice goes by the bricks' content) */
    const void* slotInfo;
    size_t plane, nSlots; /* words of a plane of the lists; the pool's slots */
    uint32_t width, height;
    bool clearFirst, classify, greyTable; /* vrc_frame::clearFirst, vrc_mode::classify, vrc_raycast_args::greyTable */
    uint64_t lutGen;
};

/* the count pass's answer, once vrc_walk_open asked for it: has it arrived, and vrc_walk_count */
struct vrc_walk_counted
{
    bool ready = false;
    uint32_t longest = 0, notLean = 0;
    unsigned long long visits = 0, gathers = 0;
};

/* what a vrc_render does about the walk cache; the context keeps the last one, and VRC_OPT_*_USED read it */
struct vrc_walk_plan
{
    int64_t used = 0; /* VRC_OPT_WALK_CACHE_USED: 0 walk, 1 count, 2 waiting for the count, 3 record, 4 replay */
    bool count = false, record = false;   /* the passes to launch in front of the march */
    bool firstVisitBuild = false;         /* build the first-visit table, here and now */
    bool resolveBuild = false;            /* build the resolved visit words in front of the march */
    bool resolvedDrop = false;            /* the resolved planes the state holds are of something else */
    uint32_t walkK = 0, walkLean = 0, walkSlots = 0; /* vrc_frame's (count: walkLean alone, "check every visit") */
    unsigned long long gathers = 0;       /* of the lists the frame records or replays */
    int64_t leanUsed = 0, uniformUsed = 0; /* VRC_OPT_WALK_LEAN_USED, _WALK_UNIFORM_ONLY_USED */
    int64_t storeThrough = 0, firstVisit = 0, leanFree = 0, resolved = 0; /* the four riders' _USED */
    size_t listWords = 0, resolvedWords = 0; /* to allocate (0: nothing): the lists to record, the planes to build */
    bool lists() const { return record || used == 4; } /* the frame carries the lists' fields */
};

/* the planes of k visits: 32-bit word offsets in the kernels, and VRC_OPT_WALK_CACHE_BUDGET */
inline unsigned long long vrc_walk_list_words( size_t plane, uint32_t k ) { return ( 1ull + 4ull * k ) * plane; }
inline bool vrc_walk_fits( const vrc_options& o, size_t plane, uint32_t k )
{
    const unsigned long long words = vrc_walk_list_words( plane, k );
    return words <= 0xFFFFFFFFull && words * sizeof( uint32_t ) <= (unsigned long long)o.walkBudget;
}

/* The opening step.  Ends what this frame ends: lists of another frame, another form, or (byContent) other uploads or
 * uniformity words, and any lists where the frame is not eligible.  Notes whether the frame repeats the vrc_render
 * before, and becomes "the one before" itself.  Starts the plan: used is 4 over VALID lists, 2 over a count in flight,
 * 1 where an eligible repeat finds nothing, else 0 (eligible, IDLE and not a repeat: the next call counts if it is this
 * one again).  Returns whether the count's answer is wanted: the caller polls then, and only then */
inline bool vrc_walk_open( const vrc_options& o, vrc_walk_state& s, const vrc_walk_facts& k, vrc_walk_plan& pl )
{
    pl = vrc_walk_plan();
    const bool eligible = k.eligibleSoFar && vrc_walk_fits( o, k.plane, 1u );
    const bool byContent = o.walkCache != VRC_WALK_CACHE_ALWAYS;
    if( !eligible || ( s.state != VRC_WALK_IDLE &&
                       ( !k.sameAsListed || k.leanAsked != s.leanAsked ||
                         ( byContent && ( s.gen != k.uploadGen || s.slotInfo != k.slotInfo ) ) ) ) )
        s.state = VRC_WALK_IDLE;
    const bool repeats = k.sameNodes && s.prevSet && ( !byContent || s.prevGen == k.uploadGen ) && k.sameAsPrev;
    s.prevSet = true;
    s.prevGen = k.uploadGen;
    pl.used = !eligible ? 0 : s.state == VRC_WALK_VALID ? 4 : s.state == VRC_WALK_COUNTING ? 2 : repeats ? 1 : 0;
    pl.count = pl.used == 1;
    return pl.used == 2;
}

/* The deciding step: everything the frame does, written into the plan alone.  The caller allocates and builds what the
 * plan asks for (listWords; firstVisitBuild; resolvedWords), says how far it got (vrc_walk_commit) and fills the
 * frame's fields from the plan */
inline void vrc_walk_decide( const vrc_options& o, const vrc_walk_state& s, const vrc_walk_facts& k, const vrc_walk_counted& n,
                             vrc_walk_plan& pl )
{
    const bool byContent = o.walkCache != VRC_WALK_CACHE_ALWAYS;
    pl.walkK = s.k;
    pl.gathers = s.gathers;
    bool lean = s.lean;
    if( pl.used == 2 && n.ready )
    {
        const uint32_t longest = n.longest > 0u ? n.longest : 1u;
        if( !vrc_walk_fits( o, k.plane, longest ) )
            pl.used = 0; /* over the budget or the offset limit: this view stays on the walk */
        else if( byContent && 2u * n.gathers > n.visits )
            pl.used = 0; /* most visits gather: so does this one */
        else
        {
            pl.used = 3;
            pl.record = true;
            pl.listWords = (size_t)vrc_walk_list_words( k.plane, longest );
            pl.walkK = longest;
            pl.gathers = n.gathers;
            lean = s.leanAsked && n.notLean == 0u;
        }
    }
    if( pl.lists() )
    {
        pl.walkLean = lean ? 1u : 0u;
        pl.walkSlots = (uint32_t)k.nSlots;
        pl.leanUsed = ( lean && pl.used == 4 ) ? 1 : 0;
        /* the uniform-only instance (vrc_kernels_walk.hip): a replayed lean frame none of whose visits gathers -- by
         * the count pass of these lists, which is still the answer while the pool has taken no upload and the words are
         * the ones it read.  Where the lists outlive that (VRC_WALK_CACHE_ALWAYS) the frame goes back to the lean
         * instance and keeps them */
        if( pl.leanUsed && o.walkUniformOnly && pl.gathers == 0ull && s.gen == k.uploadGen && s.slotInfo == k.slotInfo )
        {
            pl.walkLean = VRC_WALK_LEAN_UNIFORM;
            pl.uniformUsed = 1;
        }
    }
    else
    {
        pl.walkK = 0u;
        pl.walkLean = ( pl.count && k.leanAsked ) ? 1u : 0u; /* (the count pass: check every visit) */
    }
    /* The riders: how the replay stores its pixels, takes a first visit, marches a visit, reads a visit.  None is among
     * what walk_constants_equal compares -- the lists do not depend on them -- so the frame's fields for them are set
     * behind the copies of the frame the context keeps */
    pl.storeThrough = vrc_plan_store_through( o, pl.used, k.width, k.height ) ? 1 : 0;
    /* the first-visit table is built on the stream behind the classified table it reads and in front of the march's
     * timing pair: no march, not timed, not counted as a launch */
    vrc_first_visit_facts fv = { pl.used, pl.walkLean, k.clearFirst, k.classify,
                                 s.tableGen != 0u && s.tableGen == k.lutGen && s.tableGrey == k.greyTable };
    pl.firstVisitBuild = vrc_plan_first_visit_build( o, fv, s.tablePrevGen == k.lutGen );
    fv.current = fv.current || pl.firstVisitBuild;
    pl.firstVisit = vrc_plan_first_visit( o, fv ) ? 1 : 0;
    pl.leanFree = vrc_plan_lean_free_march( o, pl.used, pl.walkLean, k.classify ) ? 1 : 0;
    /* the resolved planes are the lists' as recorded, under the uploads and the slotInfo the frame renders with -- what
     * a frame must find unchanged to be handed VRC_WALK_LEAN_UNIFORM at all -- and count against the budget beside the
     * lists.  The first such frame without them builds them (behind the pool's uploads and in front of the timing
     * pair: no march); planes of anything else are dropped, and so are they where the frame is not handed that
     * instance because the triple moved */
    pl.resolvedDrop = s.resolvedValid && ( pl.record || ( pl.used == 4 && ( s.resolvedGen != k.uploadGen || s.resolvedSlotInfo != k.slotInfo ) ) );
    const unsigned long long resolvedBytes = ( 1ull + 5ull * pl.walkK ) * k.plane * sizeof( uint32_t );
    pl.resolved = vrc_plan_walk_resolved( o, pl.walkLean == VRC_WALK_LEAN_UNIFORM, resolvedBytes <= (unsigned long long)o.walkBudget ) ? 1 : 0;
    pl.resolveBuild = pl.resolved && ( !s.resolvedValid || pl.resolvedDrop );
    pl.resolvedWords = pl.resolveBuild ? (size_t)pl.walkK * k.plane : 0u;
}

/* how far the caller got with what the plan asked for, in the order it goes about it */
enum vrc_walk_reached
{
    VRC_WALK_REACHED_NOTHING = 0, /* the poll, the count pass's three objects or the lists failed */
    VRC_WALK_REACHED_LISTS,       /* ... the build of the first-visit table failed */
    VRC_WALK_REACHED_TABLE,       /* ... the resolved planes could not grow */
    VRC_WALK_REACHED_ALL
};

/* The commit: what the state remembers of the plan, and `last`, the context's record of the call.  A vrc_render that
 * fails on the way remembers what it got to and nothing behind it: lists that could not grow leave the count in flight
 * with k, lean and gathers as they were, and the call reads back as one still waiting for it; planes that could not grow
 * leave resolvedGen and resolvedSlotInfo alone.  The read-backs of the riders such a call did not get to stay the call
 * before's */
inline void vrc_walk_commit( vrc_walk_state& s, const vrc_walk_facts& k, const vrc_walk_plan& pl, vrc_walk_reached reached,
                             vrc_walk_plan& last )
{
    const vrc_walk_plan before = last;
    last = pl;
    if( reached < VRC_WALK_REACHED_TABLE )
    {
        last.firstVisit = before.firstVisit;
        last.resolved = before.resolved;
        last.leanFree = 0;
    }
    if( reached == VRC_WALK_REACHED_NOTHING )
    {
        last.used = pl.record ? 2 : pl.count ? 0 : pl.used;
        last.leanUsed = last.uniformUsed = last.storeThrough = 0;
        return;
    }
    if( pl.count )
    {
        s.leanAsked = k.leanAsked;
        s.gen = k.uploadGen;
        s.slotInfo = k.slotInfo;
    }
    if( pl.record )
    {
        s.k = pl.walkK;
        s.lean = pl.walkLean != 0u;
        s.gathers = pl.gathers;
    }
    if( reached == VRC_WALK_REACHED_LISTS )
        return;
    if( pl.firstVisitBuild )
    {
        s.tableGen = k.lutGen;
        s.tableGrey = k.greyTable;
    }
    s.tablePrevGen = k.lutGen;
    if( pl.resolvedDrop )
        s.resolvedValid = false;
    if( pl.resolveBuild && reached == VRC_WALK_REACHED_ALL )
    {
        s.resolvedGen = k.uploadGen;
        s.resolvedSlotInfo = k.slotInfo;
    }
}

/* the three transitions behind the launches in front of the march, each once its launch succeeded: the count pass is on
 * the stream; the record pass is; the resolved planes' build is */
enum vrc_walk_launch
{
    VRC_WALK_LAUNCHED_COUNT,
    VRC_WALK_LAUNCHED_RECORD,
    VRC_WALK_LAUNCHED_RESOLVE
};
inline void vrc_walk_launched( vrc_walk_state& s, vrc_walk_launch what )
{
    if( what == VRC_WALK_LAUNCHED_COUNT )
        s.state = VRC_WALK_COUNTING;
    else if( what == VRC_WALK_LAUNCHED_RECORD )
        s.state = VRC_WALK_VALID;
    else
        s.resolvedValid = true;
}

/* start over: what the lists index or were written on is gone -- the node table, the stream, the row map, the option or
 * the budget they were made under.  (The resolved planes go with the next record pass; the repeat bookkeeping stays) */
inline void vrc_walk_forget( vrc_walk_state& s ) { s.state = VRC_WALK_IDLE; }

#endif /* VRC_PLAN_H */
