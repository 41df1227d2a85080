/*
 * vrc_kernels_meanip.hip -- gfx950 kernels of the mean-intensity projection (VRC_OPT_MIP_FOLD = VRC_MIP_FOLD_MEAN): the
 * instances of vrc_kernels_mip.h's kernel for the accumulating fold (vrc_core.h: VRC_FOLD_MEAN), and the small kernel
 * that turns the per-pixel state of any fold into the values and counts of vrc_get_projection_values.
 */
#include "vrc_kernels_mip.h"

hipError_t vrc_launch_raycast_meanip( const vrc_raycast_args& a, hipStream_t stream )
{
    return launch_mip_fold< VRC_FOLD_MEAN >( a, stream );
}

__global__ void vrc_k_projection_values( const vrc_projection_state st, float* __restrict__ values,
                                         uint32_t* __restrict__ counts )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= st.pixels )
        return;
    const bool mean = st.fold == VRC_FOLD_MEAN;
    float v;
    uint32_t n;
    vrc_projection_value( st.fold, st.floatState != 0u, st.shift, mean ? 0u : st.mipMax[i], mean ? st.meanSum[i] : 0ull,
                          mean ? st.meanCount[i] : 0u, v, n );
    values[i] = v;
    counts[i] = n;
}

hipError_t vrc_launch_projection_values( const vrc_projection_state& st, float* values, uint32_t* counts, hipStream_t stream )
{
    if( st.pixels == 0u )
        return hipSuccess;
    if( values == nullptr || counts == nullptr ||
        ( st.fold == VRC_FOLD_MEAN ? ( st.meanSum == nullptr || st.meanCount == nullptr ) : st.mipMax == nullptr ) )
        return hipErrorInvalidValue;
    hipLaunchKernelGGL( vrc_k_projection_values, dim3( ( st.pixels + 255u ) / 256u ), dim3( 256 ), 0, stream, st, values, counts );
    return hipGetLastError();
}
