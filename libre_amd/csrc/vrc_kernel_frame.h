/*
 * vrc_kernel_frame.h -- the frame every tile kernel puts around its march, in pieces: one wave64 = one 8x8 pixel tile in
 * Morton lane order, four tiles of a schedule unit per workgroup, the tile schedule, the tile culling of the
 * reference-order loop, a table and the per-axis address tables of the fixed-point stepping in LDS, the sample count's
 * reduction; and what the launchers of such kernels share: one launch and one ladder from the frame's
 * options to the instance.  Included by vrc_kernels_mip.h, vrc_kernels_shade.hip, vrc_kernels_cdepth.hip and (the
 * launchers' side alone) vrc_kernels_preint.hip; the __shared__ arrays stay where the kernels declare them.
 * vrc_k_raycast (vrc_kernels.hip), whose frame this is, keeps its own text: its code object is held to the last byte,
 * and with the pieces called from here its registers are numbered differently.  vrc_k_raycast_preint keeps its own as
 * well: its 8-bit fixed-point grid-walk instance is 6-7 % slower over these pieces (profiles/r14_shared_march.txt).
 */
#ifndef VRC_KERNEL_FRAME_H
#define VRC_KERNEL_FRAME_H

#include "vrc_internal.h"

#include <type_traits>

#define VRC_FRAME_WG_THREADS ( 64u * VRC_WAVES_PER_GROUP )

/* the classified table (257 entries) or, where samples are classified one by one, the padded transfer function (258) */
__device__ __forceinline__ void vrc_frame_fill_table( vrc_f4* lut, const vrc_f4* lutGlobal, uint32_t tid )
{
    for( uint32_t i = tid; i < VRC_TFP_ENTRIES; i += VRC_FRAME_WG_THREADS )
        lut[i] = lutGlobal[i];
}

/* the per-axis address tables of the fixed-point stepping (vrc_core.h: vrc_addr_tab) */
__device__ __forceinline__ void vrc_frame_fill_address_tables( const vrc_frame& f, uint32_t tid )
{
    const vrc_lay lay = vrc_make_lay( f.sbx, f.sby );
    for( uint32_t u = tid; u < 256u; u += VRC_FRAME_WG_THREADS )
    {
        vrc_addr_tab[u] = vrc_lay_x( lay, u );
        vrc_addr_tab[256u + u] = vrc_lay_y( lay, u );
        vrc_addr_tab[512u + u] = vrc_lay_z( lay, u );
    }
}

/* the wave's tile and the lane's pixel */
struct vrc_frame_tile
{
    uint32_t tile, tx, ty, px, py;
};

/* Workgroup -> tile by the schedule of vrc_internal.h; false: the wave has no tile.  Morton lane order: four consecutive
 * lanes (the unit the texture addresser works on) are a 2x2 pixel quad, so their voxels usually share one 64-byte segment */
__device__ __forceinline__ bool vrc_frame_find_tile( const uint32_t* tileOrder, uint32_t tilesX, uint32_t nTiles,
                                                     uint32_t tid, uint32_t lane, vrc_frame_tile& t )
{
    const uint32_t slotIndex = blockIdx.x * VRC_WAVES_PER_GROUP + ( tid >> 6 );
    const uint32_t tilesY = nTiles / tilesX;
    if( slotIndex >= vrc_schedule_slots( tilesX, tilesY ) )
        return false;
    t.tile = vrc_slot_tile( tileOrder, slotIndex, tilesX, tilesY );
    if( t.tile == VRC_NO_TILE )
        return false;
    t.tx = t.tile % tilesX;
    t.ty = t.tile / tilesX;
    const uint32_t lx = ( lane & 1u ) | ( ( lane >> 1 ) & 2u ) | ( ( lane >> 2 ) & 4u );
    const uint32_t ly = ( ( lane >> 1 ) & 1u ) | ( ( lane >> 2 ) & 2u ) | ( ( lane >> 3 ) & 4u );
    t.px = t.tx * VRC_TILE_W + lx;
    t.py = t.ty * VRC_TILE_H + ly;
    return true;
}

/* Reference-order loop: the bricks this tile's rays can hit at all, found once per wave (vrc_core.h, "tile culling"; a
 * brick that is not hit is a `continue`, so leaving it out changes no sample): 64 bricks per step against the pyramid
 * through the tile's corner pixels, one pixel of margin.  tileCand: VRC_WAVES_PER_GROUP * VRC_TILE_CANDIDATES entries in
 * LDS.  Returns the wave's candidates, nCand of them, or null: the lanes run the whole list */
template < bool DDA >
__device__ __forceinline__ const uint16_t* vrc_frame_cull_tile( const vrc_frame& f, const vrc_dev_node* nodes,
                                                                uint16_t* tileCand, uint32_t tid, uint32_t lane, uint32_t tx,
                                                                uint32_t ty, uint32_t& nCand )
{
    const uint16_t* cand = nullptr;
    nCand = 0;
    if( !DDA && f.nodeCount > 8u && f.nodeCount <= 65535u )
    {
        uint16_t* const mine = tileCand + ( tid >> 6 ) * VRC_TILE_CANDIDATES;
        /* frame rows of the tile (row bands: local rows map to frame rows, not always consecutive ones) */
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
    return cand;
}

/* wave64 reduction of the lanes' sample counts, one atomic per wave */
__device__ __forceinline__ void vrc_frame_add_samples( unsigned long long* sampleCounter, uint32_t nSamples,
                                                       uint32_t lane )
{
    unsigned long long s = nSamples;
#pragma unroll
    for( int off = 32; off > 0; off >>= 1 )
        s += __shfl_down( s, off, 64 );
    if( lane == 0 && s != 0 )
        atomicAdd( sampleCounter, s );
}

/* ---- the launchers' side ---- */
template < typename ATLAS_T >
static inline const char* vrc_frame_atlas_name()
{
    return std::is_same< ATLAS_T, float >::value ? "float" : sizeof( ATLAS_T ) == 1 ? "unsigned char" : "unsigned short";
}

/* One launch of a tile kernel `name`< DDA, CLAMP, FIXED, MODE, ATLAS_T, BIG > over the frame's tile schedule, noted for
 * vrc_last_kernel */
template < bool DDA, bool CLAMP, bool FIXED, int MODE, typename ATLAS_T, bool BIG, typename... KArgs >
static hipError_t vrc_frame_launch( const char* name, void ( *kernel )( KArgs... ), const vrc_raycast_args& a, hipStream_t stream )
{
    const uint32_t tilesX = ( a.frame.width + VRC_TILE_W - 1 ) / VRC_TILE_W;
    const uint32_t tilesY = ( a.frame.height + VRC_TILE_H - 1 ) / VRC_TILE_H;
    const uint32_t nTiles = tilesX * tilesY;
    if( nTiles == 0 )
        return hipSuccess;
    vrc_internal_note_kernel( "%s<%s,%s,%s,%d,%s,%s>", name, DDA ? "true" : "false", CLAMP ? "true" : "false",
                              FIXED ? "true" : "false", (int)MODE, vrc_frame_atlas_name< ATLAS_T >(), BIG ? "true" : "false" );
    vrc_internal_note_kernel_fn( (const void*)kernel, (int)VRC_FRAME_WG_THREADS, 0 );
    vrc_launch_march( a, kernel, dim3( ( vrc_schedule_slots( tilesX, tilesY ) + VRC_WAVES_PER_GROUP - 1u ) / VRC_WAVES_PER_GROUP ),
                      dim3( VRC_FRAME_WG_THREADS ), 0, stream, a.frame, a.nodes, a.gridTable, (const ATLAS_T*)a.atlas, a.lut,
                      a.classifier, a.pixelBuffer, a.sampleCounter, a.tileOrder, tilesX, nTiles );
    return hipGetLastError();
}

/* The instances of a kernel family K (K::POINT, K::TRILINEAR: its two modes; K::launch< DDA, CLAMP, FIXED, MODE, ATLAS_T,
 * BIG >: one launch) by the sampler of the plain composite forms (vrc_launch_raycast): fixed-point stepping where the
 * caller asked for it and the slot has an overlap (point samples), the float chain with or without clamped addressing
 * otherwise; the trilinear gather form always steps in float.  K::FIXED_BIG8: do 8-bit point samples of an atlas of more
 * than 2^32 voxels step in fixed point too?  The projections': yes.  The composite extensions': no, in float, as
 * vrc_launch_raycast's BIG instances do -- they take the plain frame's sample positions */
template < typename K, int MODE, typename ATLAS_T, bool BIG >
static hipError_t vrc_frame_launch_sampler( const vrc_raycast_args& a, hipStream_t stream )
{
    if constexpr( MODE == K::POINT && ( K::FIXED_BIG8 || !BIG || sizeof( ATLAS_T ) >= 2 ) )
        if( a.fixedStepping && !a.clamp )
            return a.gridDda ? K::template launch< true, false, true, MODE, ATLAS_T, BIG >( a, stream )
                             : K::template launch< false, false, true, MODE, ATLAS_T, BIG >( a, stream );
    if( a.clamp )
        return a.gridDda ? K::template launch< true, true, false, MODE, ATLAS_T, BIG >( a, stream )
                         : K::template launch< false, true, false, MODE, ATLAS_T, BIG >( a, stream );
    return a.gridDda ? K::template launch< true, false, false, MODE, ATLAS_T, BIG >( a, stream )
                     : K::template launch< false, false, false, MODE, ATLAS_T, BIG >( a, stream );
}

template < typename K, typename ATLAS_T >
static hipError_t vrc_frame_launch_atlas( const vrc_raycast_args& a, hipStream_t stream )
{
    if( a.linear )
        return a.bigAtlas ? vrc_frame_launch_sampler< K, K::TRILINEAR, ATLAS_T, true >( a, stream )
                          : vrc_frame_launch_sampler< K, K::TRILINEAR, ATLAS_T, false >( a, stream );
    return a.bigAtlas ? vrc_frame_launch_sampler< K, K::POINT, ATLAS_T, true >( a, stream )
                      : vrc_frame_launch_sampler< K, K::POINT, ATLAS_T, false >( a, stream );
}

template < typename K >
static hipError_t vrc_frame_launch_family( const vrc_raycast_args& a, hipStream_t stream )
{
    switch( a.elemBytes )
    {
    case 1: return vrc_frame_launch_atlas< K, uint8_t >( a, stream );
    case 2: return vrc_frame_launch_atlas< K, uint16_t >( a, stream );
    case 4: return vrc_frame_launch_atlas< K, float >( a, stream );
    default: return hipErrorInvalidValue;
    }
}

template < typename K >
static hipError_t vrc_frame_launch_extension( const vrc_raycast_args& a, hipStream_t stream )
{
    if( a.gridDda && a.gridTable == nullptr )
        return hipErrorInvalidValue;
    return vrc_frame_launch_family< K >( a, stream );
}

#endif
