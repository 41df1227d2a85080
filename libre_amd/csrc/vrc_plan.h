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
 * pass; shading .. preint: of the first composite pass */
struct vrc_latches
{
    int64_t projection = -1, fold = -1, depth = -1, cue = -1;
    bool iso = false;
    float isoValue = 0.0f, isoAmbient = 0.0f;
    int64_t shading = -1, shadingAmbient = -1, compositeDepth = -1, preint = -1;
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
    bool linear = false;
    /* samples classified one by one (padded transfer function in the table buffer) whenever the 257-entry classified
     * table cannot be used: continuous or 16-bit densities (MIP: the one classification per ray reads it too) */
    bool classify = false;
    /* the plain composite: none of the frames marched by the gather kernels of the extensions */
    bool plain() const { return !mip && !shade && !cdepth && !preint; }
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
 * vrc_set_isosurface (isoSet: called at all, and its two values) and the bytes of an atlas element.  Changes nothing:
 * a refused pass has latched nothing. */
inline vrc_refusal vrc_plan_mode( const vrc_options& o, const vrc_latches& l, bool rayLod, bool isoSet, float isoValue,
                                  float isoAmbient, uint32_t elemBytes, vrc_mode& m )
{
#define VRC_PLAN_BETWEEN " changed between vrc_pre_render and vrc_post_render; "
    m = vrc_mode();
    if( elemBytes == 4 && vrc_plan_staged_kernel( o ) )
        VRC_PLAN_REFUSE( "vrc_render: 32-bit and float voxels are marched by gathers; the LDS-staged and tap-packed "
                         "forms take 8- and 16-bit voxels (VRC_OPT_KERNEL = AUTO, REFERENCE_ORDER or GRID_DDA)" );
    /* an isosurface frame reads none of the MIP frame's options but VRC_OPT_MIP_SKIP, and is served and refused as one */
    m.iso = o.projection == VRC_PROJECTION_ISO;
    m.mip = o.projection == VRC_PROJECTION_MIP || m.iso;
    const bool fold = m.mip && !m.iso; /* a MIP frame that reads VRC_OPT_MIP_FOLD */
    m.mean = fold && o.mipFold == VRC_MIP_FOLD_MEAN;
    if( vrc_plan_changed( l.projection, o.projection ) )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PROJECTION" VRC_PLAN_BETWEEN "the passes of one frame take one projection" );
    if( m.iso && !isoSet )
        VRC_PLAN_REFUSE( "vrc_render: VRC_OPT_PROJECTION = ISO needs vrc_set_isosurface first" );
    if( m.iso && l.iso && ( l.isoValue != isoValue || l.isoAmbient != isoAmbient ) )
        VRC_PLAN_REFUSE( "vrc_render: vrc_set_isosurface changed iso_value or ambient between vrc_pre_render and "
                         "vrc_post_render; the passes of one frame take one isosurface" );
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
    m.shade = !m.mip && o.shading != 0;
    m.cdepth = !m.mip && o.compositeDepth != 0;
    m.preint = !m.mip && o.preint != 0;
    if( !m.mip )
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
    if( !m.mip && vrc_plan_changed( l.preint, o.preint ) )
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
    m.classify = m.linear || elemBytes != 1 || m.mip;
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

#endif /* VRC_PLAN_H */
