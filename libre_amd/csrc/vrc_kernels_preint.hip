/*
 * vrc_kernels_preint.hip -- gfx950 kernels of a pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1; vrc_core.h:
 * vrc_preint_entry, vrc_preint_brick), and nothing else.  A frame with the option at 0, a MIP frame and an isosurface
 * frame launch nothing from this file.
 *
 * vrc_k_build_preint fills the frame's 256 x 256 table in float64, one block per row.  vrc_k_raycast_preint is the frame
 * of the composite kernel (vrc_kernels.hip: vrc_k_raycast) around the pre-integrated march: one wave64 = one 8x8 pixel
 * tile in Morton lane order, four tiles of a schedule unit per workgroup, the tile schedule, the tile culling of the
 * reference-order loop, the classified table (or the padded transfer function) in LDS, the per-axis address tables of
 * the fixed-point stepping, the ray cache of the grid walk.  The pre-integrated table stays in global memory (1 MiB: it
 * lives in the L2, and the reads of a march cluster at its diagonal).  Samples are always counted in a register; the
 * counter is only added to where the caller asked for it (vrc_kernels_mip.h does the same: half the instances).
 */
#include "vrc_kernel_frame.h" /* (the launchers' side: the kernel below keeps its own text) */

#define VRC_PREINT_WG_THREADS ( 64u * VRC_WAVES_PER_GROUP )

/* The table.  Block `row` fills row `row`: its 256 threads first integrate one texel interval each (thread i: the interval
 * between texel centres i and i + 1), thread 0 sums them in texel order into the prefix table in LDS (8 KiB; every block
 * the same bits), then thread `col` forms entry (row, col) from two partial intervals and one prefix difference.
 * Rebuilt on every transfer-function edit: 65 536 entries of a few logarithms each, not 65 536 x 255. */
__global__ __launch_bounds__( 256 ) void vrc_k_build_preint( const float* __restrict__ tf, const vrc_f4* __restrict__ lut,
                                                             vrc_f4* __restrict__ table, const vrc_lut_params p,
                                                             const int kind )
{
    __shared__ vrc_preint_sum prefix[VRC_PREINT_DIM];
    const uint32_t col = threadIdx.x, row = blockIdx.x;
    vrc_preint_sum one = { 0.0, 0.0, 0.0, 0.0 };
    if( col + 1u < VRC_PREINT_DIM )
        vrc_preint_span( tf, col, 0.0, 1.0, one );
    prefix[col] = one;
    __syncthreads();
    if( col == 0u )
    {
        /* vrc_preint_prefix's sum, over the intervals the block's threads integrated */
        vrc_preint_sum run = { 0.0, 0.0, 0.0, 0.0 };
        for( uint32_t i = 0; i < VRC_PREINT_DIM; ++i )
        {
            const vrc_preint_sum next = prefix[i];
            prefix[i] = run;
            run.i += next.i;
            run.r += next.r;
            run.g += next.g;
            run.b += next.b;
        }
    }
    __syncthreads();
    table[row * VRC_PREINT_DIM + col] = vrc_preint_table_entry( tf, lut, prefix, p, kind, row, col );
}

hipError_t vrc_launch_build_preint( const float* tf, const vrc_f4* lut, vrc_f4* table, vrc_lut_params p, int kind,
                                    hipStream_t stream )
{
    if( tf == nullptr || table == nullptr || ( kind == VRC_PREINT_VALUE && lut == nullptr ) )
        return hipErrorInvalidValue;
    hipLaunchKernelGGL( vrc_k_build_preint, dim3( VRC_PREINT_DIM ), dim3( VRC_PREINT_DIM ), 0, stream, tf, lut, table, p, kind );
    return hipGetLastError();
}

/* Waves per SIMD the compiler plans registers for (a register budget, not a residency limit; DESIGN.md has the table of
 * what every instance came out at).  LDS is 4 KiB of table, 3 KiB of address tables and, in the reference-order form,
 * 8 KiB of tile candidates per workgroup of four waves: it admits the 8 waves a SIMD holds, so the registers decide.
 *   point samples: at least 4 (128 VGPRs): a group holds 8 table entries, or (the texel-indexed table) 4 x 4 taps;
 *   trilinear samples: at least 3, as the shaded and depth-tracking trilinear instances -- the 4 x 12 address parts and
 *     32 taps of a group, then its 4 x 4 table taps. */
#define VRC_PREINT_MIN_WAVES ( MODE == VRC_MODE_PREINT_TRILINEAR ? 3 : 4 )

template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
__global__ __launch_bounds__( VRC_PREINT_WG_THREADS ) __attribute__( ( amdgpu_waves_per_eu( VRC_PREINT_MIN_WAVES, 8 ) ) ) void vrc_k_raycast_preint(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const int32_t* __restrict__ gridTable,
    const ATLAS_T* __restrict__ atlas, const vrc_f4* __restrict__ lutGlobal, const vrc_classifier cls,
    vrc_f4* __restrict__ pixelBuffer, unsigned long long* __restrict__ sampleCounter,
    const uint32_t* __restrict__ tileOrder, const uint32_t tilesX, const uint32_t nTiles )
{
    /* classified table (257 entries: what a uniform brick is marched from) or the padded transfer function (258) */
    __shared__ vrc_f4 lut[VRC_TFP_ENTRIES];
    __shared__ uint16_t tileCand[DDA ? 1u : VRC_WAVES_PER_GROUP * VRC_TILE_CANDIDATES];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    for( uint32_t i = tid; i < VRC_TFP_ENTRIES; i += VRC_PREINT_WG_THREADS )
        lut[i] = lutGlobal[i];
    if( FIXED )
    {
        const vrc_lay lay = vrc_make_lay( f.sbx, f.sby );
        for( uint32_t u = tid; u < 256u; u += VRC_PREINT_WG_THREADS )
        {
            vrc_addr_tab[u] = vrc_lay_x( lay, u );
            vrc_addr_tab[256u + u] = vrc_lay_y( lay, u );
            vrc_addr_tab[512u + u] = vrc_lay_z( lay, u );
        }
    }
    __syncthreads();
    /* from here on the waves of the workgroup are independent */
    const uint32_t slotIndex = blockIdx.x * VRC_WAVES_PER_GROUP + ( tid >> 6 );
    const uint32_t tilesY = nTiles / tilesX;
    if( slotIndex >= vrc_schedule_slots( tilesX, tilesY ) )
        return;
    const uint32_t tile = vrc_slot_tile( tileOrder, slotIndex, tilesX, tilesY );
    if( tile == VRC_NO_TILE )
        return;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    /* Morton lane order: four consecutive lanes are a 2x2 pixel quad (vrc_k_raycast) */
    const uint32_t lx = ( lane & 1u ) | ( ( lane >> 1 ) & 2u ) | ( ( lane >> 2 ) & 4u );
    const uint32_t ly = ( ( lane >> 1 ) & 1u ) | ( ( lane >> 2 ) & 2u ) | ( ( lane >> 3 ) & 4u );
    const uint32_t px = tx * VRC_TILE_W + lx;
    const uint32_t py = ty * VRC_TILE_H + ly;

    uint32_t nSamples = 0;
    /* reference-order loop: the bricks this tile's rays can hit at all, found once per wave (vrc_core.h, "tile
     * culling"; a brick that is not hit is a `continue`, so leaving it out changes no sample) */
    const uint16_t* cand = nullptr;
    uint32_t nCand = 0;
    if( !DDA && f.nodeCount > 8u && f.nodeCount <= 65535u )
    {
        uint16_t* const mine = tileCand + ( tid >> 6 ) * VRC_TILE_CANDIDATES;
        float r0 = 1e30f, r1 = -1e30f;
        for( uint32_t j = 0; j < VRC_TILE_H; ++j )
        {
            const uint32_t row = ty * VRC_TILE_H + j;
            if( row < f.height )
            {
                const float fr = (float)( f.rowMap ? f.rowMap[row] : row );
                r0 = fminf( r0, fr );
                r1 = fmaxf( r1, fr );
            }
        }
        const vrc_tile_pyramid pyr = vrc_make_tile_pyramid( f, (float)( tx * VRC_TILE_W ) - 1.0f, r0 - 1.0f,
                                                           (float)( tx * VRC_TILE_W + VRC_TILE_W ), r1 + 1.0f );
        for( uint32_t base = 0; base < f.nodeCount; base += 64u )
        {
            const uint32_t i = base + lane;
            bool in = false;
            if( i < f.nodeCount )
                in = vrc_pyramid_may_hit( pyr, nodes[i].aabbMin, nodes[i].aabbSize );
            const uint64_t m = __builtin_amdgcn_ballot_w64( in );
            const uint32_t at = nCand + __builtin_amdgcn_mbcnt_hi( (uint32_t)( m >> 32 ),
                                                                   __builtin_amdgcn_mbcnt_lo( (uint32_t)m, 0u ) );
            if( in && at < VRC_TILE_CANDIDATES )
                mine[at] = (uint16_t)i;
            nCand += (uint32_t)__builtin_popcountll( m );
        }
        __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
        __builtin_amdgcn_wave_barrier();
        if( nCand <= VRC_TILE_CANDIDATES )
            cand = mine;
    }
    if( px < f.width && py < f.height )
    {
        /* (GROUP of the pixel loops: not read by a pre-integrated mode, vrc_preint_brick chooses its own) */
        if( DDA )
            vrc_pixel_grid_dda< CLAMP, true, FIXED, MODE, ATLAS_T, VRC_PREINT_GROUP, BIG >(
                f, nodes, gridTable, atlas, lut, cls, pixelBuffer, px, py, nSamples, tile * 64u + lane );
        else
            vrc_pixel_reference_order< CLAMP, true, FIXED, MODE, ATLAS_T, VRC_PREINT_GROUP, BIG >(
                f, nodes, atlas, lut, cls, pixelBuffer, px, py, nSamples, cand, nCand );
    }
    if( sampleCounter != nullptr )
    {
        /* wave64 reduction, one atomic per wave */
        unsigned long long s = nSamples;
#pragma unroll
        for( int off = 32; off > 0; off >>= 1 )
            s += __shfl_down( s, off, 64 );
        if( lane == 0 && s != 0 )
            atomicAdd( sampleCounter, s );
    }
}

/* the kernel family for the launch ladder of vrc_kernel_frame.h: the sampler of the plain composite forms */
struct vrc_preint_kernels
{
    static constexpr int POINT = VRC_MODE_PREINT, TRILINEAR = VRC_MODE_PREINT_TRILINEAR;
    static constexpr bool FIXED_BIG8 = false;
    template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG >
    static hipError_t launch( const vrc_raycast_args& a, hipStream_t stream )
    {
        return vrc_frame_launch< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >(
            "vrc_k_raycast_preint", &vrc_k_raycast_preint< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG >, a, stream );
    }
};

hipError_t vrc_launch_raycast_preint( const vrc_raycast_args& a, hipStream_t stream )
{
    if( VRC_TILE_W != 8u || a.lut == nullptr || !a.preint || a.frame.preintTable == nullptr || a.packed )
        return hipErrorInvalidValue;
    return vrc_frame_launch_extension< vrc_preint_kernels >( a, stream );
}
