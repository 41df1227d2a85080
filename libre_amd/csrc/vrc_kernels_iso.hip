/*
 * vrc_kernels_iso.hip -- gfx950 kernels of an isosurface frame (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO): the instances
 * of vrc_kernels_mip.h's kernel for the first-crossing fold (vrc_core.h: VRC_FOLD_FIRST), and nothing else.  A composite
 * or MIP frame launches nothing from this file.
 */
#include "vrc_kernels_mip.h"

hipError_t vrc_launch_raycast_iso( const vrc_raycast_args& a, hipStream_t stream )
{
    return launch_mip_fold< VRC_FOLD_FIRST >( a, stream );
}
