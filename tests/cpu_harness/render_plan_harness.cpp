/*
 * render_plan_harness.cpp -- the two decisions of libre_amd/csrc/vrc_plan.h (vrc_plan_mode; vrc_plan_form with
 * vrc_plan_use_lds and the packed wish) against the text of vrc_render they replaced, for tests/test_render_plan_cpu.py.
 * TEST INFRASTRUCTURE ONLY.
 *
 * mode_before and form_before hold verbatim copies of the two blocks of vrc_render as they stood before it was split
 * into phases (between the BEGIN / END markers: the test counts the message literals there).  They run over stand-in
 * structs with the field names the context and the pool had; fail( code, msg ) records; pool_packed_possible and
 * pool_enable_packed are inputs, and the calls of the latter are counted.  Generated inputs go through both; what must
 * agree: the code, the message (strcmp), whether pool_enable_packed was called, and on success every derived flag.
 *
 * Built as a shared library and, with -DRENDER_PLAN_MAIN, as a stand-alone program for the sanitizer run.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../libre_amd/csrc/vrc_plan.h"

namespace
{
struct old_ctx
{
    int64_t optKernel, optFilter, optTfFracBits, optStepping, optVariant, optPackedAtlas;
    int64_t optProjection, optMipFold, optMipDepth, optMipDepthCue, optShading, optShadingAmbient, optCompositeDepth, optPreint;
    bool rayLod, isoSet;
    float isoValue, isoAmbient;
    int64_t frameProjection, frameFold, frameDepth, frameCue;
    bool frameIso;
    float frameIsoValue, frameIsoAmbient;
    int64_t frameShading, frameShadingAmbient, frameCompositeDepth, framePreint;
    bool cachedGridOk, cachedOneCell, cachedLodOk, cachedClamp;
};
struct old_pool
{
    uint32_t elemBytes;
    uint32_t slotDim[3];
    bool bigAtlas;
    bool packedPossible, enableSucceeds;
    int enableCalls;
};
struct old_render
{
    uint32_t samplesPerPixel;
};

int g_code;
const char* g_msg;
int fail( int code, const char* msg )
{
    g_code = code;
    g_msg = msg;
    return code;
}
bool pool_packed_possible( const old_pool* p ) { return p->packedPossible; }
bool pool_enable_packed( old_pool* p )
{
    ++p->enableCalls;
    return p->enableSucceeds;
}

struct flags
{
    bool iso, mip, mipDepth, shade, cdepth, preint, linear, classify;
    bool glSuper, slotsFit8Bits, useDda, usePacked, useLds;
};

int mode_before( const old_ctx* c, const old_pool* pool, flags& out )
{
    /* BEGIN MODE BLOCK */
    if( pool->elemBytes == 4 && ( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED ) )
        return fail( VRC_EINVAL, "vrc_render: 32-bit and float voxels are marched by gathers; the LDS-staged and tap-packed "
                                 "forms take 8- and 16-bit voxels (VRC_OPT_KERNEL = AUTO, REFERENCE_ORDER or GRID_DDA)" );
    /* an isosurface frame is a MIP frame with the first-crossing fold: it reads none of the MIP frame's options but
     * VRC_OPT_MIP_SKIP, and is served and refused as one */
    const bool iso = c->optProjection == VRC_PROJECTION_ISO;
    const bool mip = c->optProjection == VRC_PROJECTION_MIP || iso;
    if( c->frameProjection >= 0 && c->frameProjection != c->optProjection )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PROJECTION changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame take one projection" );
    if( iso && !c->isoSet )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PROJECTION = ISO needs vrc_set_isosurface first" );
    if( iso && c->frameIso && ( c->frameIsoValue != c->isoValue || c->frameIsoAmbient != c->isoAmbient ) )
        return fail( VRC_EINVAL, "vrc_render: vrc_set_isosurface changed iso_value or ambient between vrc_pre_render and "
                                 "vrc_post_render; the passes of one frame take one isosurface" );
    if( mip && !iso && c->frameFold >= 0 && c->frameFold != c->optMipFold )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_FOLD changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame take one fold" );
    /* depth tracking: the maximum and the minimum only; the mean reads neither option */
    const bool mipDepth = iso || ( mip && c->optMipFold != VRC_MIP_FOLD_MEAN && ( c->optMipDepth != 0 || c->optMipDepthCue > 0 ) );
    if( mip && !iso && c->optMipFold != VRC_MIP_FOLD_MEAN )
    {
        if( c->frameDepth >= 0 && c->frameDepth != c->optMipDepth )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_DEPTH changed between vrc_pre_render and vrc_post_render; the "
                                     "passes of one frame all keep the depth or none does" );
        if( c->frameCue >= 0 && c->frameCue != c->optMipDepthCue )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_DEPTH_CUE changed between vrc_pre_render and vrc_post_render; "
                                     "the passes of one frame take one cue strength" );
    }
    if( mip )
    {
        /* what the maximum-intensity projection is not defined for (include/vrc_hip.h) */
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, iso ? "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no isosurface form; "
                                           "VRC_OPT_PROJECTION = ISO is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)"
                                         : "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no maximum-intensity form; "
                                           "VRC_OPT_PROJECTION = MIP is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, iso ? "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PROJECTION = ISO renders a per-brick cut"
                                         : "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PROJECTION = MIP renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, iso ? "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PROJECTION = ISO is defined on the "
                                           "cudaRaycaster variant's sample set"
                                         : "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PROJECTION = MIP is defined on the "
                                           "cudaRaycaster variant's sample set" );
    }
    /* a shaded composite frame (include/vrc_hip.h, "A shaded composite frame"): read by composite frames only; served by
     * the gather marches of vrc_kernels_shade.hip and refused where those have no form */
    const bool shade = !mip && c->optShading != 0;
    if( !mip )
    {
        if( c->frameShading >= 0 && c->frameShading != c->optShading )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING changed between vrc_pre_render and vrc_post_render; the "
                                     "passes of one frame are all shaded or none is" );
        if( c->frameShadingAmbient >= 0 && c->frameShadingAmbient != c->optShadingAmbient )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING_AMBIENT changed between vrc_pre_render and vrc_post_render; "
                                     "the passes of one frame take one ambient share" );
    }
    /* the depth of a composite frame (include/vrc_hip.h, "The depth of a composite frame"): read by composite frames only;
     * served by the gather marches of vrc_kernels_cdepth.hip and refused where those have no form */
    const bool cdepth = !mip && c->optCompositeDepth != 0;
    if( !mip && c->frameCompositeDepth >= 0 && c->frameCompositeDepth != c->optCompositeDepth )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_COMPOSITE_DEPTH changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame cross one threshold" );
    if( cdepth )
    {
        if( shade )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_COMPOSITE_DEPTH; alpha does not "
                                     "depend on shading: render the unshaded frame to pick in a shaded picture" );
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no depth-tracking form; "
                                     "VRC_OPT_COMPOSITE_DEPTH is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_COMPOSITE_DEPTH tracks a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_COMPOSITE_DEPTH is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    /* a pre-integrated composite frame (include/vrc_hip.h, "A pre-integrated composite frame"): read by composite frames
     * only; served by the gather marches of vrc_kernels_preint.hip and refused where those have no form */
    const bool preint = !mip && c->optPreint != 0;
    if( !mip && c->framePreint >= 0 && c->framePreint != c->optPreint )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PREINTEGRATION changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame are all pre-integrated or none is" );
    if( preint )
    {
        if( shade )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_PREINTEGRATION; a step has no one "
                                     "gradient: the two are not combined" );
        if( cdepth )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_COMPOSITE_DEPTH together with VRC_OPT_PREINTEGRATION; the depth is "
                                     "defined on the plain frame's alpha: the two are not combined" );
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no pre-integrated form; "
                                     "VRC_OPT_PREINTEGRATION = 1 is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PREINTEGRATION = 1 renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PREINTEGRATION = 1 is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    if( shade )
    {
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no shaded form; VRC_OPT_SHADING = 1 is "
                                     "marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_SHADING = 1 renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_SHADING = 1 is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    const bool linear = c->optFilter == VRC_FILTER_TRILINEAR;
    /* samples classified one by one (padded transfer function in the table buffer) whenever the
     * 257-entry classified table cannot be used: continuous or 16-bit densities */
    /* (MIP: the one classification per ray reads the padded transfer function too) */
    const bool classify = linear || pool->elemBytes != 1 || mip;
    /* END MODE BLOCK */
    out.iso = iso;
    out.mip = mip;
    out.mipDepth = mipDepth;
    out.shade = shade;
    out.cdepth = cdepth;
    out.preint = preint;
    out.linear = linear;
    out.classify = classify;
    return fail( VRC_OK, nullptr );
}

int form_before( const old_ctx* c, old_pool* pool, const old_render* render, uint32_t nNodes, flags& out )
{
    const bool mip = out.mip, shade = out.shade, cdepth = out.cdepth, preint = out.preint, linear = out.linear;
    /* BEGIN FORM BLOCK */
    if( c->rayLod )
    {
        if( !c->cachedLodOk )
            return fail( VRC_EHIERARCHY, "vrc_render: per-ray LOD needs a brick hierarchy (every level a regular grid of bricks, one brick per cell)" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: per-ray LOD is defined for the cudaRaycaster variant only" );
        /* AUTO: the LDS-staged form for the trilinear filter where it applies, else the gather form; GRID_DDA asks for
         * the gather form, LDS for the staged one */
        if( c->optKernel == VRC_KERNEL_REFERENCE_ORDER )
            return fail( VRC_EINVAL, "vrc_render: per-ray LOD walks the hierarchy; VRC_OPT_KERNEL = AUTO, GRID_DDA (gathers), LDS or PACKED" );
    }
    bool useDda = c->cachedGridOk;
    /* AUTO keeps the reference's frame: bricks of one size are met by the grid walk in the reference's
     * order; a list that mixes brick sizes (an LOD cut) is composited in the host's centre-distance order,
     * which is not a visibility order for every ray (quirk Q6) -- the literal loop reproduces that as long
     * as testing every brick per ray is affordable.  GRID_DDA can always be asked for (true visibility
     * order); the trilinear filter (extension, no reference frame to keep) stays on the grid. */
    if( c->optKernel == VRC_KERNEL_AUTO && useDda && !c->cachedOneCell && !linear &&
        nNodes <= VRC_REFERENCE_ORDER_MAX_NODES )
        useDda = false;
    /* glRaycaster with more than one sample per pixel (fragRaycast.glsl:121-129): the pixel is averaged brick by
     * brick in the host's order -- the reference-order loop is the only form that has a "brick by brick" */
    const bool glSuper = c->optVariant == VRC_VARIANT_GLRAYCASTER && render->samplesPerPixel > 1u;
    if( glSuper )
    {
        if( c->optKernel == VRC_KERNEL_GRID_DDA || c->optKernel == VRC_KERNEL_LDS )
            return fail( VRC_EINVAL, "vrc_render: the glRaycaster variant with samplesPerPixel > 1 is rendered by the "
                                     "reference-order kernel (VRC_OPT_KERNEL = AUTO or REFERENCE_ORDER)" );
        useDda = false;
    }
    if( c->optKernel == VRC_KERNEL_REFERENCE_ORDER )
        useDda = false;
    else if( c->optKernel == VRC_KERNEL_GRID_DDA && !c->cachedGridOk && !c->rayLod )
        return fail( VRC_EINVAL, "vrc_render: node set is not grid-aligned; GRID_DDA unavailable" );
    /* LDS-staged kernel: brick-grid DDA + unclamped sampler (overlap >= 1).  AUTO takes it for
     * the trilinear filter (eight taps per sample), the gather kernel for point sampling. */
    /* its trilinear form takes the transfer-function texel and CUDA's 1.8 fixed-point lerp weight out of one
     * float -> integer conversion (vrc_kernels_lds.hip: lds_classify): other weight widths use the gather form */
    /* slot-local positions in 8.24 fixed point (fixed-point stepping, the per-axis address tables, the LDS kernel's boxes)
     * need every slot dimension to fit eight bits; pool creation bounds a slot's VOLUME only (2^24 voxels), so a flat
     * or long brick can exceed it: such pools march with float positions */
    const bool slotsFit8Bits = pool->slotDim[0] <= 248u && pool->slotDim[1] <= 248u && pool->slotDim[2] <= 248u;
    /* 16-bit voxels: its trilinear form only (a 16-bit density does not index the classified table of the point form) */
    const bool ldsVoxels = slotsFit8Bits && ( pool->elemBytes == 1 || ( pool->elemBytes == 2 && linear ) );
    /* atlases of more than 2^32 voxels (64-bit slot bases): its trilinear form only */
    const bool ldsEligible = c->cachedGridOk && !c->cachedClamp && ldsVoxels && ( !pool->bigAtlas || linear ) &&
                             ( !linear || c->optTfFracBits == 8 );
    if( !c->rayLod && c->optKernel == VRC_KERNEL_LDS && !ldsEligible )
        return fail( VRC_EINVAL, "vrc_render: the LDS kernel needs a grid-aligned node set of 8-bit bricks in an atlas of at most 2^32 voxels (trilinear: 8- or 16-bit, any atlas, VRC_OPT_TF_FRAC_BITS = 8) with overlap >= 1" );
    /* per-ray LOD: the staged kernel's trilinear form only (samples classified one by one: no table per level) */
    const bool ldsLodEligible = c->rayLod && linear && !c->cachedClamp && ldsVoxels && !pool->bigAtlas &&
                                c->optTfFracBits == 8;
    if( c->rayLod && c->optKernel == VRC_KERNEL_LDS && !ldsLodEligible )
        return fail( VRC_EINVAL, "vrc_render: under per-ray LOD the LDS kernel needs the trilinear filter, 8- or 16-bit bricks with overlap >= 1 and VRC_OPT_TF_FRAC_BITS = 8" );
    /* tap-packed atlas (VRC_KERNEL_PACKED; vrc_core.h): the trilinear filter as two gathers per sample.  Needs what its
     * positions and its classifier need -- 8- or 16-bit bricks with overlap >= 1 in slots of at most 248 voxels a side,
     * VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping -- and 2.25 times the atlas in device memory; either brick
     * enumeration (grid walk where the node set is grid-aligned, else the reference-order loop) */
    const bool packedEligible = linear && !glSuper && !mip && !shade && !cdepth && !preint && !c->cachedClamp && slotsFit8Bits &&
                                pool_packed_possible( pool ) && c->optTfFracBits == 8 && c->optStepping != 0;
    bool usePacked = false;
    if( c->optKernel == VRC_KERNEL_PACKED )
    {
        if( !packedEligible )
            return fail( VRC_EINVAL, "vrc_render: the packed kernel needs the trilinear filter on 8- or 16-bit bricks with overlap >= 1 (slots of at most 248 voxels a side), VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping" );
        if( !pool_enable_packed( pool ) )
            return fail( VRC_ENOMEM, "vrc_render: no device memory for the tap-packed atlas (2.25 times the brick atlas)" );
        usePacked = true;
    }
    else if( c->optKernel == VRC_KERNEL_AUTO && packedEligible && c->optPackedAtlas )
        /* measured on C2: 1.2 against 1.7 ms along the axis, 1.5 against 2.4 at 30/20 degrees;
         * under per-ray LOD 1.4-2.1 x the staged form (profiles/r4_c5_trilinear_three_forms.txt); without the memory for
         * it the frame takes the staged form below */
        usePacked = pool_enable_packed( pool );
    const bool useLds = c->rayLod ? ( ldsLodEligible && c->optKernel != VRC_KERNEL_GRID_DDA && !usePacked )
                                  : !glSuper && !usePacked && !mip && !shade && !cdepth && !preint && ( c->optKernel == VRC_KERNEL_LDS ||
                                                  ( c->optKernel == VRC_KERNEL_AUTO && linear && ldsEligible ) );
    /* END FORM BLOCK */
    out.glSuper = glSuper;
    out.slotsFit8Bits = slotsFit8Bits;
    out.useDda = useDda;
    out.usePacked = usePacked;
    out.useLds = useLds;
    return fail( VRC_OK, nullptr );
}

/* ---- the same two decisions through vrc_plan.h, as vrc_render makes them ---- */
vrc_options options_of( const old_ctx& c )
{
    vrc_options o;
    o.kernel = c.optKernel;
    o.filter = c.optFilter;
    o.tfFracBits = c.optTfFracBits;
    o.stepping = c.optStepping;
    o.variant = c.optVariant;
    o.packedAtlas = c.optPackedAtlas;
    o.projection = c.optProjection;
    o.mipFold = c.optMipFold;
    o.mipDepth = c.optMipDepth;
    o.mipDepthCue = c.optMipDepthCue;
    o.shading = c.optShading;
    o.shadingAmbient = c.optShadingAmbient;
    o.compositeDepth = c.optCompositeDepth;
    o.preint = c.optPreint;
    return o;
}

vrc_refusal mode_after( const old_ctx& c, const old_pool& pool, vrc_mode& m )
{
    vrc_latches l;
    l.projection = c.frameProjection;
    l.fold = c.frameFold;
    l.depth = c.frameDepth;
    l.cue = c.frameCue;
    l.iso = c.frameIso;
    l.isoValue = c.frameIsoValue;
    l.isoAmbient = c.frameIsoAmbient;
    l.shading = c.frameShading;
    l.shadingAmbient = c.frameShadingAmbient;
    l.compositeDepth = c.frameCompositeDepth;
    l.preint = c.framePreint;
    return vrc_plan_mode( options_of( c ), l, c.rayLod, c.isoSet, c.isoValue, c.isoAmbient, pool.elemBytes, m );
}

vrc_refusal form_after( const old_ctx& c, old_pool& pool, const old_render& render, uint32_t nNodes, const vrc_mode& m,
                        vrc_form& fm )
{
    const vrc_options o = options_of( c );
    vrc_form_facts k;
    k.rayLod = c.rayLod;
    k.gridOk = c.cachedGridOk;
    k.oneCell = c.cachedOneCell;
    k.lodOk = c.cachedLodOk;
    k.clamp = c.cachedClamp;
    k.nNodes = nNodes;
    k.samplesPerPixel = render.samplesPerPixel;
    for( int i = 0; i < 3; ++i )
        k.slotDim[i] = pool.slotDim[i];
    k.elemBytes = pool.elemBytes;
    k.bigAtlas = pool.bigAtlas;
    k.packedPossible = pool_packed_possible( &pool );
    const vrc_refusal r = vrc_plan_form( o, m, k, fm );
    if( r.code != VRC_OK )
        return r;
    fm.usePacked = fm.packed != VRC_PACKED_NONE && pool_enable_packed( &pool );
    if( fm.packed == VRC_PACKED_REQUIRED && !fm.usePacked )
        return vrc_plan_no_packed_memory;
    fm.useLds = vrc_plan_use_lds( o, m, k, fm, fm.usePacked );
    return r;
}

struct tally
{
    uint64_t cases = 0, refused = 0, bad = 0, enableCalls = 0;
    std::vector< const char* > seen; /* the distinct messages the copied text returned */
    void note( const char* msg )
    {
        for( const char* s : seen )
            if( std::strcmp( s, msg ) == 0 )
                return;
        seen.push_back( msg );
    }
    void write( uint64_t* out ) const
    {
        out[0] = cases;
        out[1] = refused;
        out[2] = bad;
        out[3] = enableCalls;
        out[4] = seen.size();
    }
};

bool same_refusal( int code, const char* msg, const vrc_refusal& r )
{
    if( code != r.code )
        return false;
    if( code == VRC_OK )
        return r.msg == nullptr;
    return r.msg && std::strcmp( msg, r.msg ) == 0;
}

void mode_case( const old_ctx& c, const old_pool& pool, tally& t )
{
    flags before = {};
    vrc_mode m;
    const int code = mode_before( &c, &pool, before );
    const char* const msg = g_msg;
    const vrc_refusal r = mode_after( c, pool, m );
    ++t.cases;
    bool ok = same_refusal( code, msg, r );
    if( code != VRC_OK )
    {
        ++t.refused;
        t.note( msg );
    }
    else if( ok )
        ok = before.iso == m.iso && before.mip == m.mip && before.mipDepth == m.mipDepth && before.shade == m.shade &&
             before.cdepth == m.cdepth && before.preint == m.preint && before.linear == m.linear &&
             before.classify == m.classify && m.mean == ( m.mip && !m.iso && c.optMipFold == VRC_MIP_FOLD_MEAN ) &&
             m.plain() == ( !before.mip && !before.shade && !before.cdepth && !before.preint );
    if( !ok && t.bad++ < 5u )
        std::fprintf( stderr, "mode: before %d \"%s\", after %d \"%s\"\n", code, msg ? msg : "", r.code, r.msg ? r.msg : "" );
}

void form_case( const old_ctx& c, const old_pool& pool0, const old_render& render, uint32_t nNodes, const flags& modeFlags,
                tally& t )
{
    old_pool poolBefore = pool0, poolAfter = pool0;
    flags before = modeFlags;
    vrc_mode m;
    m.mip = modeFlags.mip;
    m.shade = modeFlags.shade;
    m.cdepth = modeFlags.cdepth;
    m.preint = modeFlags.preint;
    m.linear = modeFlags.linear;
    vrc_form fm;
    const int code = form_before( &c, &poolBefore, &render, nNodes, before );
    const char* const msg = g_msg;
    const vrc_refusal r = form_after( c, poolAfter, render, nNodes, m, fm );
    ++t.cases;
    t.enableCalls += (uint64_t)poolBefore.enableCalls;
    bool ok = same_refusal( code, msg, r ) && poolBefore.enableCalls == poolAfter.enableCalls;
    if( code != VRC_OK )
    {
        ++t.refused;
        t.note( msg );
    }
    else if( ok )
        ok = before.glSuper == fm.glSuper && before.slotsFit8Bits == fm.slotsFit8Bits && before.useDda == fm.useDda &&
             before.usePacked == fm.usePacked && before.useLds == fm.useLds;
    if( !ok && t.bad++ < 5u )
        std::fprintf( stderr, "form: before %d \"%s\", after %d \"%s\"\n", code, msg ? msg : "", r.code, r.msg ? r.msg : "" );
}

const int64_t kKernels[5] = { VRC_KERNEL_AUTO, VRC_KERNEL_REFERENCE_ORDER, VRC_KERNEL_GRID_DDA, VRC_KERNEL_LDS, VRC_KERNEL_PACKED };
const int64_t kCue[2] = { 0, 500 }, kAmbient[2] = { 250, 300 }, kTau[2] = { 0, 500 };
const uint32_t kElem[3] = { 1, 2, 4 };
/* a prime that divides neither product: i -> i * kSpread mod product visits every case once, and every `stride`-th of
 * them is a sample across all inputs, whatever the stride shares with the radices */
const uint64_t kSpread = 1000003ull;

/* the options of mode case `i` of the full product (138240 of them) */
const uint64_t kModeProduct = 5ull * 3 * 3 * 3 * 1024;
void mode_options( uint64_t i, old_ctx& c, old_pool& pool )
{
    const auto take = [&]( uint64_t n ) {
        const uint64_t v = i % n;
        i /= n;
        return v;
    };
    c.optKernel = kKernels[take( 5 )];
    c.optProjection = (int64_t)take( 3 );
    c.optMipFold = (int64_t)take( 3 );
    pool.elemBytes = kElem[take( 3 )];
    c.optMipDepth = (int64_t)take( 2 );
    c.optMipDepthCue = kCue[take( 2 )];
    c.optShading = (int64_t)take( 2 );
    c.optShadingAmbient = kAmbient[take( 2 )];
    c.optCompositeDepth = kTau[take( 2 )];
    c.optPreint = (int64_t)take( 2 );
    c.rayLod = take( 2 ) != 0;
    c.optVariant = take( 2 ) ? VRC_VARIANT_GLRAYCASTER : VRC_VARIANT_CUDARAYCASTER;
    c.optFilter = take( 2 ) ? VRC_FILTER_TRILINEAR : VRC_FILTER_NEAREST;
    c.isoSet = take( 2 ) != 0;
    c.isoValue = 0.5f;
    c.isoAmbient = 0.25f;
}

/* latch state s: 0 all unset; 1 all equal to the options; 2 .. 11 one of the ten latches alone differing */
void mode_latches( int s, old_ctx& c )
{
    const bool set = s != 0;
    c.frameProjection = set ? c.optProjection : -1;
    c.frameFold = set ? c.optMipFold : -1;
    c.frameDepth = set ? c.optMipDepth : -1;
    c.frameCue = set ? c.optMipDepthCue : -1;
    c.frameIso = set;
    c.frameIsoValue = set ? c.isoValue : 0.0f;
    c.frameIsoAmbient = set ? c.isoAmbient : 0.0f;
    c.frameShading = set ? c.optShading : -1;
    c.frameShadingAmbient = set ? c.optShadingAmbient : -1;
    c.frameCompositeDepth = set ? c.optCompositeDepth : -1;
    c.framePreint = set ? c.optPreint : -1;
    switch( s )
    {
    case 2: c.frameProjection = ( c.optProjection + 1 ) % 3; break;
    case 3: c.frameFold = ( c.optMipFold + 1 ) % 3; break;
    case 4: c.frameDepth = 1 - c.optMipDepth; break;
    case 5: c.frameCue = 500 - c.optMipDepthCue; break;
    case 6: c.frameIsoValue = c.isoValue + 1.0f; break;
    case 7: c.frameIsoAmbient = c.isoAmbient + 0.5f; break;
    case 8: c.frameShading = 1 - c.optShading; break;
    case 9: c.frameShadingAmbient = 550 - c.optShadingAmbient; break;
    case 10: c.frameCompositeDepth = 500 - c.optCompositeDepth; break;
    case 11: c.framePreint = 1 - c.optPreint; break;
    default: break;
    }
}

uint64_t g_rng;
uint32_t rnd( uint32_t n ) /* splitmix64 */
{
    uint64_t z = ( g_rng += 0x9E3779B97F4A7C15ull );
    z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
    z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull;
    return (uint32_t)( ( ( z ^ ( z >> 31 ) ) >> 33 ) % n );
}
/* a latch over its unrestricted space: unset, or any value the option can take */
int64_t any_latch( const int64_t* values, uint32_t n )
{
    const uint32_t k = rnd( n + 1u );
    return k == n ? -1 : values[k];
}
} // namespace

extern "C" {

/* the full product of the mode block's inputs x 12 latch states (every `stride`-th case), then nRandom seeded draws
 * over the unrestricted latch space.  out: cases, refused, bad, 0, distinct messages of the copied text.  Returns bad */
uint64_t render_plan_mode_run( uint64_t seed, uint64_t nRandom, uint64_t stride, uint64_t* out )
{
    tally t;
    old_ctx c = {};
    old_pool pool = {};
    for( uint64_t i0 = 0; i0 < kModeProduct * 12ull; i0 += stride )
    {
        const uint64_t i = i0 * kSpread % ( kModeProduct * 12ull );
        mode_options( i / 12ull, c, pool );
        mode_latches( (int)( i % 12ull ), c );
        mode_case( c, pool, t );
    }
    g_rng = seed;
    const int64_t three[3] = { 0, 1, 2 }, two[2] = { 0, 1 };
    const float isoValues[2] = { 0.5f, 1.5f }, isoAmbients[2] = { 0.25f, 0.75f };
    for( uint64_t i = 0; i < nRandom; ++i )
    {
        mode_options( ( ( (uint64_t)rnd( 1u << 20 ) << 20 ) | rnd( 1u << 20 ) ) % kModeProduct, c, pool );
        c.frameProjection = any_latch( three, 3 );
        c.frameFold = any_latch( three, 3 );
        c.frameDepth = any_latch( two, 2 );
        c.frameCue = any_latch( kCue, 2 );
        c.frameIso = rnd( 2 ) != 0;
        c.frameIsoValue = isoValues[rnd( 2 )];
        c.frameIsoAmbient = isoAmbients[rnd( 2 )];
        c.frameShading = any_latch( two, 2 );
        c.frameShadingAmbient = any_latch( kAmbient, 2 );
        c.frameCompositeDepth = any_latch( kTau, 2 );
        c.framePreint = any_latch( two, 2 );
        mode_case( c, pool, t );
    }
    t.write( out );
    return t.bad;
}

/* the full product of the form block's inputs (every `stride`-th case).  out: cases, refused, bad, calls of
 * pool_enable_packed by the copied text, its distinct messages.  Returns bad */
uint64_t render_plan_form_run( uint64_t stride, uint64_t* out )
{
    tally t;
    const uint64_t product = 5ull * 5 * 3 * ( 1ull << 16 );
    for( uint64_t i0 = 0; i0 < product; i0 += stride )
    {
        uint64_t i = i0 * kSpread % product;
        const auto take = [&]( uint64_t n ) {
            const uint64_t v = i % n;
            i /= n;
            return v;
        };
        old_ctx c = {};
        old_pool pool = {};
        old_render render = {};
        flags mode = {};
        c.optKernel = kKernels[take( 5 )];
        const uint64_t kind = take( 5 ); /* plain, MIP, shade, composite depth, pre-integration */
        mode.mip = kind == 1;
        mode.shade = kind == 2;
        mode.cdepth = kind == 3;
        mode.preint = kind == 4;
        pool.elemBytes = kElem[take( 3 )];
        c.optVariant = take( 2 ) ? VRC_VARIANT_GLRAYCASTER : VRC_VARIANT_CUDARAYCASTER;
        render.samplesPerPixel = 1u + (uint32_t)take( 2 );
        c.rayLod = take( 2 ) != 0;
        mode.linear = take( 2 ) != 0;
        c.cachedGridOk = take( 2 ) != 0;
        c.cachedOneCell = take( 2 ) != 0;
        c.cachedLodOk = take( 2 ) != 0;
        c.cachedClamp = take( 2 ) != 0;
        const uint32_t nNodes = VRC_REFERENCE_ORDER_MAX_NODES + (uint32_t)take( 2 );
        pool.bigAtlas = take( 2 ) != 0;
        pool.slotDim[0] = 16u;
        pool.slotDim[1] = 248u + (uint32_t)take( 2 );
        pool.slotDim[2] = 16u;
        c.optTfFracBits = take( 2 ) ? 10 : 8;
        c.optStepping = (int64_t)take( 2 );
        c.optPackedAtlas = (int64_t)take( 2 );
        pool.packedPossible = take( 2 ) != 0;
        pool.enableSucceeds = take( 2 ) != 0;
        form_case( c, pool, render, nNodes, mode, t );
    }
    t.write( out );
    return t.bad;
}
}

#ifdef RENDER_PLAN_MAIN
int main( int argc, char** argv )
{
    const uint64_t stride = argc > 1 ? std::strtoull( argv[1], nullptr, 10 ) : 1ull;
    uint64_t m[5], f[5];
    const uint64_t bad = render_plan_mode_run( 2024, 1000000ull / stride, stride, m ) + render_plan_form_run( stride, f );
    std::printf( "mode cases %llu refused %llu bad %llu calls %llu messages %llu\n", (unsigned long long)m[0],
                 (unsigned long long)m[1], (unsigned long long)m[2], (unsigned long long)m[3], (unsigned long long)m[4] );
    std::printf( "form cases %llu refused %llu bad %llu calls %llu messages %llu\n", (unsigned long long)f[0],
                 (unsigned long long)f[1], (unsigned long long)f[2], (unsigned long long)f[3], (unsigned long long)f[4] );
    return bad ? 1 : 0;
}
#endif
