/*
 * vrc_kernels_mipdepth.hip -- gfx950 kernels of a MIP frame that keeps the depth of the projected sample
 * (VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE): the instances of vrc_kernels_mip.h's kernel for the maximum and the minimum
 * with depth tracking (vrc_core.h: VRC_FOLD_DEPTH above the fold), and the small kernel that turns the running depth
 * into what vrc_get_projection_depths returns.  A frame without depth tracking launches nothing from this file.
 */
#include "vrc_kernels_mip.h"

hipError_t vrc_launch_raycast_mip_depth( const vrc_raycast_args& a, int fold, hipStream_t stream )
{
    if( a.frame.mipDepth == nullptr )
        return hipErrorInvalidValue;
    switch( fold )
    {
    case VRC_FOLD_MAX: return launch_mip_fold< VRC_FOLD_MAX + VRC_FOLD_DEPTH >( a, stream );
    case VRC_FOLD_MIN: return launch_mip_fold< VRC_FOLD_MIN + VRC_FOLD_DEPTH >( a, stream );
    default: return hipErrorInvalidValue; /* the mean has no position */
    }
}

/* host_t = D; host_xyz = origin + D * dir of the pixel's ray (the frame row under a row map), product and sum each
 * rounded */
__global__ void vrc_k_projection_depths( const vrc_frame f, const float* __restrict__ depth, const uint32_t pixels,
                                         float* __restrict__ t, float* __restrict__ xyz )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= pixels )
        return;
    const float d = depth[i];
    t[i] = d;
    if( xyz != nullptr )
    {
        VRC_STRICT_FP
        const uint32_t px = i % f.width, py = i / f.width;
        const vrc_ray r = vrc_setup_ray( f, px, f.rowMap ? f.rowMap[py] : py );
        const float ax = d * r.dir.x, ay = d * r.dir.y, az = d * r.dir.z;
        xyz[3u * i] = r.origin.x + ax;
        xyz[3u * i + 1u] = r.origin.y + ay;
        xyz[3u * i + 2u] = r.origin.z + az;
    }
}

hipError_t vrc_launch_projection_depths( const vrc_frame& f, const float* depth, uint32_t pixels, float* t, float* xyz,
                                         hipStream_t stream )
{
    if( pixels == 0u )
        return hipSuccess;
    if( depth == nullptr || t == nullptr || f.width == 0u || pixels != f.width * f.height )
        return hipErrorInvalidValue;
    hipLaunchKernelGGL( vrc_k_projection_depths, dim3( ( pixels + 255u ) / 256u ), dim3( 256 ), 0, stream, f, depth, pixels, t, xyz );
    return hipGetLastError();
}
