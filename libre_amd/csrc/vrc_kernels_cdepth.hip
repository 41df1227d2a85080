/*
 * vrc_kernels_cdepth.hip -- gfx950 kernels of a composite frame that keeps the depth at which every ray's opacity crosses
 * a threshold (VRC_OPT_COMPOSITE_DEPTH above 0; vrc_core.h: vrc_cdepth_policy under vrc_extension_brick), and nothing
 * else.  A frame with the option at 0, a shaded frame, a MIP frame and an isosurface frame launch nothing from this file.
 *
 * The kernel frame (vrc_kernel_frame.h) around the depth-tracking march, with the classified table (or the padded
 * transfer function) in LDS and the ray cache of the grid walk, samples always counted in a register.  Behind the march
 * the pixel's (D, V) is stored where this pass crossed and no pass before it had.
 */
#include "vrc_kernel_frame.h"

/* Waves per SIMD the compiler plans registers for (a register budget, not a residency limit; DESIGN.md has the table of
 * what every instance came out at).  LDS is 4 KiB of table, 3 KiB of address tables and, in the reference-order form,
 * 8 KiB of tile candidates per workgroup of four waves: it admits the 8 waves a SIMD holds, so the registers decide.
 *   point samples: at least 4 (128 VGPRs): a group holds 8 classified samples and their 8 densities (6 under the
 *     clamped sampler and where samples are classified one by one: 8 left up to 4 registers of scratch there);
 *   trilinear samples: at least 3, as the depth-tracking and first-crossing trilinear instances of vrc_kernels_mip.h --
 *     the 4 x 12 address parts and 32 taps of a group. */
#define VRC_CDEPTH_MIN_WAVES ( MODE == VRC_MODE_CDEPTH_TRILINEAR ? 3 : 4 )

template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
__global__ __launch_bounds__( VRC_FRAME_WG_THREADS ) __attribute__( ( amdgpu_waves_per_eu( VRC_CDEPTH_MIN_WAVES, 8 ) ) ) void vrc_k_raycast_cdepth(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const int32_t* __restrict__ gridTable,
    const ATLAS_T* __restrict__ atlas, const vrc_f4* __restrict__ lutGlobal, const vrc_classifier cls,
    vrc_f4* __restrict__ pixelBuffer, unsigned long long* __restrict__ sampleCounter,
    const uint32_t* __restrict__ tileOrder, const uint32_t tilesX, const uint32_t nTiles )
{
    __shared__ vrc_f4 lut[VRC_TFP_ENTRIES];
    __shared__ uint16_t tileCand[DDA ? 1u : VRC_WAVES_PER_GROUP * VRC_TILE_CANDIDATES];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    vrc_frame_fill_table( lut, lutGlobal, tid );
    if( FIXED )
        vrc_frame_fill_address_tables( f, tid );
    __syncthreads();
    /* from here on the waves of the workgroup are independent */
    vrc_frame_tile t;
    if( !vrc_frame_find_tile( tileOrder, tilesX, nTiles, tid, lane, t ) )
        return;
    uint32_t nSamples = 0;
    uint32_t nCand;
    const uint16_t* const cand = vrc_frame_cull_tile< DDA >( f, nodes, tileCand, tid, lane, t.tx, t.ty, nCand );
    if( t.px < f.width && t.py < f.height )
    {
        /* the pixel's pair: a first pass does not read it and leaves every pixel's; a later pass leaves the pair of a
         * pixel that had crossed alone, in the march (crossed from the start) and here */
        const uint32_t pixelPos = t.py * f.width + t.px;
        vrc_cdepth_state z = { vrc_bits_float( 0x7F800000u ), VRC_MIP_EMPTY, false };
        bool had = false;
        if( !f.mipFirst )
            had = f.mipDepth[pixelPos] < vrc_bits_float( 0x7F800000u );
        z.crossed = had;
        if( DDA )
            vrc_pixel_grid_dda< CLAMP, true, FIXED, MODE, ATLAS_T, VRC_CDEPTH_GROUP, BIG >(
                f, nodes, gridTable, atlas, lut, cls, pixelBuffer, t.px, t.py, nSamples, t.tile * 64u + lane, &z );
        else
            vrc_pixel_reference_order< CLAMP, true, FIXED, MODE, ATLAS_T, VRC_CDEPTH_GROUP, BIG >(
                f, nodes, atlas, lut, cls, pixelBuffer, t.px, t.py, nSamples, cand, nCand, &z );
        if( f.mipFirst || ( z.crossed && !had ) )
        {
            f.mipDepth[pixelPos] = z.d;
            f.mipMax[pixelPos] = z.v;
        }
    }
    if( sampleCounter != nullptr )
        vrc_frame_add_samples( sampleCounter, nSamples, lane );
}

struct vrc_cdepth_kernels
{
    static constexpr int POINT = VRC_MODE_CDEPTH, TRILINEAR = VRC_MODE_CDEPTH_TRILINEAR;
    static constexpr bool FIXED_BIG8 = false;
    template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
    static hipError_t launch( const vrc_raycast_args& a, hipStream_t stream )
    {
        return vrc_frame_launch< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >(
            "vrc_k_raycast_cdepth", &vrc_k_raycast_cdepth< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >, a, stream );
    }
};

hipError_t vrc_launch_raycast_cdepth( const vrc_raycast_args& a, hipStream_t stream )
{
    if( VRC_TILE_W != 8u || a.lut == nullptr || !a.cdepth || a.shade || a.packed || a.frame.mipMax == nullptr ||
        a.frame.mipDepth == nullptr )
        return hipErrorInvalidValue;
    return vrc_frame_launch_extension< vrc_cdepth_kernels >( a, stream );
}
