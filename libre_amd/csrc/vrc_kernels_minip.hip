/*
 * vrc_kernels_minip.hip -- gfx950 kernels of the minimum-intensity projection (VRC_OPT_MIP_FOLD = VRC_MIP_FOLD_MIN):
 * the instances of vrc_kernels_mip.h's kernel for the fold that mirrors the maximum (vrc_core.h: VRC_FOLD_MIN).
 */
#include "vrc_kernels_mip.h"

hipError_t vrc_launch_raycast_minip( const vrc_raycast_args& a, hipStream_t stream )
{
    return launch_mip_fold< VRC_FOLD_MIN >( a, stream );
}
