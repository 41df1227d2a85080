/*
 * vrc_kernels_slice.hip -- gfx950 kernels of a slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE; include/vrc_hip.h,
 * "A slice frame"): the kernel frame (vrc_kernel_frame.h) around vrc_pixel_slice, and nothing else.  A frame of another
 * projection launches nothing from this file.
 *
 * One sample per pixel: no march, so no stepping variant, no sample group and no clamped / unclamped pair -- the one
 * sample is always clamped to its slot.  That leaves GRID (the cell of the sample looked up in the brick grid -- a
 * look-up, there is no walk -- against the culled list of the reference-order form; it is what the frame's pieces take
 * for their DDA argument), LINEAR (eight taps against one), the atlas type and BIG: 24 instances, chosen by the short
 * ladder below and not by vrc_frame_launch_family, which would instantiate the steppings and the clamped sampler of a
 * march for nothing.
 *
 * No table in LDS (the pixel is classified once, from the padded transfer function in global memory) and no loop but
 * the reference-order form's search of the tile's candidates, whose 8 KiB per workgroup of four waves admit the eight
 * waves a SIMD holds: the instances carry no occupancy cap and no register budget of their own (DESIGN.md section 4.10
 * has their registers).  The sample counter is added to where the caller asked for it.
 */
#include "vrc_kernel_frame.h"

template < bool GRID, bool LINEAR, typename ATLAS_T, bool BIG >
__global__ __launch_bounds__( VRC_FRAME_WG_THREADS ) void vrc_k_raycast_slice(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const int32_t* __restrict__ gridTable,
    const ATLAS_T* __restrict__ atlas, const vrc_f4* __restrict__ tfp, const vrc_classifier cls,
    vrc_f4* __restrict__ pixelBuffer, unsigned long long* __restrict__ sampleCounter,
    const uint32_t* __restrict__ tileOrder, const uint32_t tilesX, const uint32_t nTiles )
{
    __shared__ uint16_t tileCand[GRID ? 1u : VRC_WAVES_PER_GROUP * VRC_TILE_CANDIDATES];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    /* the waves of the workgroup are independent */
    vrc_frame_tile t;
    if( !vrc_frame_find_tile( tileOrder, tilesX, nTiles, tid, lane, t ) )
        return;
    uint32_t nSamples = 0;
    uint32_t nCand;
    const uint16_t* const cand = vrc_frame_cull_tile< GRID >( f, nodes, tileCand, tid, lane, t.tx, t.ty, nCand );
    if( t.px < f.width && t.py < f.height )
        vrc_pixel_slice< GRID, LINEAR, ATLAS_T, BIG >( f, nodes, gridTable, atlas, tfp, cls, pixelBuffer, t.px, t.py, nSamples,
                                                      cand, nCand, t.tile * 64u + lane );
    if( sampleCounter != nullptr )
        vrc_frame_add_samples( sampleCounter, nSamples, lane );
}

/* one launch over the frame's tile schedule, noted for vrc_last_kernel with the kernel's own four template arguments */
template < bool GRID, bool LINEAR, typename ATLAS_T, bool BIG >
static hipError_t launch_slice( const vrc_raycast_args& a, hipStream_t stream )
{
    const uint32_t tilesX = ( a.frame.width + VRC_TILE_W - 1 ) / VRC_TILE_W;
    const uint32_t tilesY = ( a.frame.height + VRC_TILE_H - 1 ) / VRC_TILE_H;
    const uint32_t nTiles = tilesX * tilesY;
    if( nTiles == 0 )
        return hipSuccess;
    auto* const kernel = &vrc_k_raycast_slice< GRID, LINEAR, ATLAS_T, BIG >;
    vrc_internal_note_kernel( "vrc_k_raycast_slice<%s,%s,%s,%s>", GRID ? "true" : "false", LINEAR ? "true" : "false",
                              vrc_frame_atlas_name< ATLAS_T >(), BIG ? "true" : "false" );
    vrc_internal_note_kernel_fn( (const void*)kernel, (int)VRC_FRAME_WG_THREADS, 0 );
    vrc_launch_march( a, kernel, dim3( ( vrc_schedule_slots( tilesX, tilesY ) + VRC_WAVES_PER_GROUP - 1u ) / VRC_WAVES_PER_GROUP ),
                      dim3( VRC_FRAME_WG_THREADS ), 0, stream, a.frame, a.nodes, a.gridTable, (const ATLAS_T*)a.atlas, a.lut,
                      a.classifier, a.pixelBuffer, a.sampleCounter, a.tileOrder, tilesX, nTiles );
    return hipGetLastError();
}

template < typename ATLAS_T, bool BIG >
static hipError_t launch_slice_atlas( const vrc_raycast_args& a, hipStream_t stream )
{
    if( a.linear )
        return a.gridDda ? launch_slice< true, true, ATLAS_T, BIG >( a, stream ) : launch_slice< false, true, ATLAS_T, BIG >( a, stream );
    return a.gridDda ? launch_slice< true, false, ATLAS_T, BIG >( a, stream ) : launch_slice< false, false, ATLAS_T, BIG >( a, stream );
}

hipError_t vrc_launch_raycast_slice( const vrc_raycast_args& a, hipStream_t stream )
{
    if( VRC_TILE_W != 8u || a.lut == nullptr || a.frame.mipMax == nullptr || a.frame.mipDepth == nullptr )
        return hipErrorInvalidValue;
    if( a.gridDda && a.gridTable == nullptr )
        return hipErrorInvalidValue;
    switch( a.elemBytes )
    {
    case 1: return a.bigAtlas ? launch_slice_atlas< uint8_t, true >( a, stream ) : launch_slice_atlas< uint8_t, false >( a, stream );
    case 2: return a.bigAtlas ? launch_slice_atlas< uint16_t, true >( a, stream ) : launch_slice_atlas< uint16_t, false >( a, stream );
    case 4: return a.bigAtlas ? launch_slice_atlas< float, true >( a, stream ) : launch_slice_atlas< float, false >( a, stream );
    default: return hipErrorInvalidValue;
    }
}
