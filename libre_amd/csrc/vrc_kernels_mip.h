/*
 * vrc_kernels_mip.h -- the kernel of a MIP frame and its launchers, as templates: included by the translation unit of
 * every fold (vrc_kernels_mip.hip the maximum, vrc_kernels_minip.hip the minimum, vrc_kernels_meanip.hip the mean), each
 * of which instantiates its own fold's instances and nothing else -- the instances of one fold take about half a minute
 * to compile, and a change to one fold's code does not rebuild the others'.
 *
 * The kernel frame (vrc_kernel_frame.h) around another march body.  What it does not
 * have: a table in LDS (the pixel is classified once per ray, from the padded transfer function in global memory),
 * a transmittance, an early-exit test.  Per sample: the address, the gather and half a v_max3 (minimum: v_min3; mean:
 * half a v_add3, or one v_add_f64).
 *
 * Samples are always counted in a register (one add per group); the counter is only added to where the caller asked
 * for it -- half the instances of a COUNT template argument.
 */
#ifndef VRC_KERNELS_MIP_H
#define VRC_KERNELS_MIP_H

#include "vrc_kernel_frame.h"

/* Waves per SIMD the compiler plans registers for (amdgpu_waves_per_eu is a register budget, not a residency limit).
 * Without the classified table the LDS need is 3 KiB of address tables (plus 8 KiB of tile candidates in the
 * reference-order form) per workgroup of four waves: LDS admits more than the 8 waves a SIMD holds, so the registers an
 * instance ends up with decide how many waves are resident.
 *   point samples, fixed-point stepping, 32-bit slot bases: (5, 5), the composite gather kernel's choice.  They come out
 *     at 62-72 VGPRs, so 7-8 waves are resident; whether they want a limit of 5, as the composite gather kernel did
 *     (its sixth wave thrashes the vector L1), is not measured, and nothing enforces one.
 *   everything else (trilinear: 32 gathers and 4 x 12 address parts in flight; the float position chain; the clamped
 *     sampler; 64-bit slot bases): at least 4, as the composite forms that spilled at 5.
 *   trilinear samples with depth tracking (vrc_kernels_mipdepth.hip): at least 3.  The group's eight samples stay live
 *     past the fold for the index search, and at 4 (128 VGPRs) the grid-walk forms with the clamped sampler spilled
 *     12-16 bytes a lane; at 3 none does (DESIGN.md section 4.6 has the table).
 *   the first-crossing fold (vrc_kernels_iso.hip): as the fold-less rows above for point samples (74-101 VGPRs), at least
 *     3 for trilinear samples as with depth tracking -- the group's samples and taps stay live for the search (116-140
 *     VGPRs, no scratch; the table is in the same section). */
#define VRC_MIP_MIN_WAVES                                                                                          \
    ( ( vrc_mode_base( MODE ) == VRC_MODE_MIP && FIXED && !CLAMP && !BIG )                            ? 5          \
      : ( ( vrc_mode_depth( MODE ) || vrc_mode_fold( MODE ) == VRC_FOLD_FIRST ) && vrc_mode_base( MODE ) == VRC_MODE_MIP_TRILINEAR ) ? 3 : 4 )
#define VRC_MIP_MAX_WAVES ( ( vrc_mode_base( MODE ) == VRC_MODE_MIP && FIXED && !CLAMP && !BIG ) ? 5 : 8 )

template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
__global__ __launch_bounds__( VRC_FRAME_WG_THREADS ) __attribute__( ( amdgpu_waves_per_eu( VRC_MIP_MIN_WAVES, VRC_MIP_MAX_WAVES ) ) ) void vrc_k_raycast_mip(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const int32_t* __restrict__ gridTable,
    const ATLAS_T* __restrict__ atlas, const vrc_f4* __restrict__ tfp, const vrc_classifier cls,
    vrc_f4* __restrict__ pixelBuffer, unsigned long long* __restrict__ sampleCounter,
    const uint32_t* __restrict__ tileOrder, const uint32_t tilesX, const uint32_t nTiles )
{
    __shared__ uint16_t tileCand[DDA ? 1u : VRC_WAVES_PER_GROUP * VRC_TILE_CANDIDATES];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    if( FIXED )
    {
        vrc_frame_fill_address_tables( f, tid );
        __syncthreads();
    }
    /* from here on the waves of the workgroup are independent */
    vrc_frame_tile t;
    if( !vrc_frame_find_tile( tileOrder, tilesX, nTiles, tid, lane, t ) )
        return;
    uint32_t nSamples = 0;
    uint32_t nCand;
    const uint16_t* const cand = vrc_frame_cull_tile< DDA >( f, nodes, tileCand, tid, lane, t.tx, t.ty, nCand );
    if( t.px < f.width && t.py < f.height )
        vrc_pixel_mip< DDA, CLAMP, FIXED, MODE, ATLAS_T, VRC_GROUP, BIG >( f, nodes, gridTable, atlas, tfp, cls, pixelBuffer,
                                                                         t.px, t.py, nSamples, cand, nCand );
    if( sampleCounter != nullptr )
        vrc_frame_add_samples( sampleCounter, nSamples, lane );
}

/* the kernel family of one fold for the launch ladder of vrc_kernel_frame.h.  Point samples step in fixed point wherever
 * the caller asked for it, 8-bit voxels of an atlas of more than 2^32 voxels included */
template < int FOLD >
struct vrc_mip_kernels
{
    static constexpr int POINT = VRC_MODE_WITH_FOLD( VRC_MODE_MIP, FOLD ), TRILINEAR = VRC_MODE_WITH_FOLD( VRC_MODE_MIP_TRILINEAR, FOLD );
    static constexpr bool FIXED_BIG8 = true;
    template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
    static hipError_t launch( const vrc_raycast_args& a, hipStream_t stream )
    {
        return vrc_frame_launch< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >(
            "vrc_k_raycast_mip", &vrc_k_raycast_mip< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >, a, stream );
    }
};

/* the instances of one fold: what a translation unit's entry point is */
template < int FOLD >
static hipError_t launch_mip_fold( const vrc_raycast_args& a, hipStream_t stream )
{
    if( VRC_TILE_W != 8u || a.lut == nullptr )
        return hipErrorInvalidValue;
    if( FOLD == VRC_FOLD_MEAN ? ( a.frame.meanSum == nullptr || a.frame.meanCount == nullptr ) : a.frame.mipMax == nullptr )
        return hipErrorInvalidValue;
    if( FOLD == VRC_FOLD_FIRST && ( a.frame.mipDepth == nullptr || a.frame.isoGrad == nullptr ) )
        return hipErrorInvalidValue;
    return vrc_frame_launch_family< vrc_mip_kernels< FOLD > >( a, stream );
}

#endif
