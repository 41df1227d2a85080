/*
 * vrc_kernels_mip.hip -- gfx950 kernels of the maximum-intensity projection (VRC_OPT_PROJECTION = VRC_PROJECTION_MIP,
 * VRC_OPT_MIP_FOLD = VRC_MIP_FOLD_MAX; include/vrc_hip.h defines the frame, vrc_core.h holds the per-ray code:
 * vrc_pixel_mip; vrc_kernels_mip.h the kernel and its launchers, which the other folds' translation units share).
 *
 * In a translation unit of its own: the composite kernels' code does not change with it.
 */
#include "vrc_kernels_mip.h"

hipError_t vrc_launch_raycast_mip( const vrc_raycast_args& a, hipStream_t stream )
{
    return launch_mip_fold< VRC_FOLD_MAX >( a, stream );
}
