/*
 * vrc_kernels_walk.hip -- the walk cache (VRC_OPT_WALK_CACHE; vrc_core.h: vrc_frame::walkCache).
 *
 * Which bricks a ray visits, and the interval of each, depend on the ray, the brick grid, the node table and the frame
 * constants the slab test reads -- not on the transfer function, the voxels or early termination.  A view that stands
 * still over a resident brick set therefore walks the grid once:
 *   vrc_k_walk_record   the tile-scheduled grid walk (vrc_ray_grid_dda, the same tie cells, `pending`, `recent` and
 *                       `stop`) whose visit stores (node, dist, tNear, tFar) instead of marching.  Run twice: with
 *                       frame.walkK = 0 it only counts (vrc_walk_count, up to four atomics per wave), then the host sizes
 *                       the planes and the second run fills them.  Never a march: not timed, not counted as a launch.
 *   vrc_k_raycast_replay the march of a frame whose lists are valid: the tile schedule, lane order, pixel clear and
 *                       store, and sample counter of vrc_k_raycast around vrc_pixel_walk_replay, which hands every
 *                       recorded visit to the one visit body vrc_march_brick_from.  None of the walk's state (cell, tMax,
 *                       tDelta, recent, pending) exists in it.  Its LEAN instances replay the lean form of the lists
 *                       (vrc_frame::walkLean: a visit's second plane holds its step count and slot index instead of
 *                       dist) through vrc_pixel_walk_replay_lean, which neither fetches the node of a uniform visit nor
 *                       counts its steps again; the host picks the form per view (vrc_render), the count pass
 *                       reports whether every visit packs.
 *   vrc_k_walk_resolve  the resolved visit words of lean lists (vrc_frame::walkResolved): one word per visit from the
 *                       list word and the slot word, for the uncounted uniform-only instances of the replay.  Run once
 *                       per set of lists, uploads and slot words.  Not a march either.
 * Instances: the ones the uniform-brick march exists for -- the table-driven point-sampling march of 8-bit voxels with
 * fixed-point stepping (VRC_MODE_TABLE, VRC_MODE_GREY), counted and uncounted, in the group sizes vrc_launch_raycast
 * picks for them.  Every other frame keeps the walk.
 */
#include "vrc_internal.h"

#define VRC_WALK_WAVES VRC_WAVES_PER_GROUP /* the four tiles of a schedule unit (vrc_internal.h) */
#define VRC_WALK_THREADS ( 64u * VRC_WALK_WAVES )

/* Morton lane order of vrc_k_raycast: the ray cache and the walk cache are indexed tile * 64 + lane in it */
__device__ inline void vrc_walk_lane_pixel( uint32_t tile, uint32_t tilesX, uint32_t lane, uint32_t& px, uint32_t& py )
{
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    const uint32_t lx = ( lane & 1u ) | ( ( lane >> 1 ) & 2u ) | ( ( lane >> 2 ) & 4u );
    const uint32_t ly = ( ( lane >> 1 ) & 1u ) | ( ( lane >> 2 ) & 2u ) | ( ( lane >> 3 ) & 4u );
    px = tx * 8u + lx;
    py = ty * 8u + ly;
}

/* one wave per tile, tiles in row-major order (the pass runs once per view: no schedule) */
__global__ __launch_bounds__( VRC_WALK_THREADS ) void vrc_k_walk_record(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const int32_t* __restrict__ gridTable,
    vrc_walk_count* __restrict__ result, const uint32_t tilesX, const uint32_t nTiles )
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * VRC_WALK_WAVES + ( threadIdx.x >> 6 );
    if( tile >= nTiles )
        return;
    uint32_t px, py;
    vrc_walk_lane_pixel( tile, tilesX, lane, px, py );
    const uint32_t rayIndex = tile * 64u + lane;
    uint32_t count = 0u, gathers = 0u, notLean = 0u;
    if( px < f.width && py < f.height )
        count = vrc_pixel_walk_record( f, nodes, gridTable, rayIndex, &gathers, &notLean );
    if( f.walkK != 0u )
        f.walkCache[rayIndex] = count; /* (0 for a lane outside the frame: whole tiles) */
    else
    {
        /* the count pass's result (vrc_walk_count): the longest list, and over the whole frame the visits, those of
         * them that would gather, and whether one of them does not pack into a lean list's word; one atomic each per
         * wave */
        uint32_t m = count, sum = count, g = gathers; /* (64 lanes: the wave's sums fit 32 bits) */
#pragma unroll
        for( int off = 32; off > 0; off >>= 1 )
        {
            const uint32_t o = __shfl_down( m, off, 64 );
            m = o > m ? o : m;
            sum += __shfl_down( sum, off, 64 );
            g += __shfl_down( g, off, 64 );
        }
        const bool anyNotLean = __builtin_amdgcn_ballot_w64( notLean != 0u ) != 0ull;
        if( lane == 0u && m != 0u )
        {
            atomicMax( &result->longest, m );
            atomicAdd( &result->visits, (unsigned long long)sum );
            if( g != 0u )
                atomicAdd( &result->gathers, (unsigned long long)g );
            if( anyNotLean )
                atomicOr( &result->notLean, 1u );
        }
    }
}

hipError_t vrc_launch_walk_record( const vrc_raycast_args& a, vrc_walk_count* result, hipStream_t stream )
{
    const uint32_t tilesX = ( a.frame.width + 7u ) / 8u, tilesY = ( a.frame.height + 7u ) / 8u;
    const uint32_t nTiles = tilesX * tilesY;
    if( nTiles == 0 )
        return hipSuccess;
    if( !a.gridTable || a.frame.rayMode != VRC_RAY_LOAD || ( a.frame.walkK != 0u ? !a.frame.walkCache : !result ) )
        return hipErrorInvalidValue;
    hipLaunchKernelGGL( vrc_k_walk_record, dim3( ( nTiles + VRC_WALK_WAVES - 1u ) / VRC_WALK_WAVES ), dim3( VRC_WALK_THREADS ),
                        0, stream, a.frame, a.nodes, a.gridTable, result, tilesX, nTiles );
    return hipGetLastError();
}

/* The first-visit table (vrc_core.h: vrc_first_visit_row): one lane per entry of the classified table, each filling its
 * row from `start` -- zero, handed in as an argument so that the compiler composites the first sample as the march
 * does.  The entry is narrowed as vrc_k_raycast_replay narrows what it stages */
template < typename E >
__global__ __launch_bounds__( 64 ) void vrc_k_build_first_visit( const vrc_f4* __restrict__ lut, E* __restrict__ table, const E start )
{
    const uint32_t e = blockIdx.x * 64u + threadIdx.x;
    if( e < VRC_FIRST_VISIT_ENTRIES )
        vrc_first_visit_row< E >( table + (size_t)e * VRC_FIRST_VISIT_ROWS, vrc_lean_narrow( lut[e], (const E*)nullptr ), start );
}

hipError_t vrc_launch_build_first_visit( const vrc_f4* lut, void* table, bool grey, hipStream_t stream )
{
    if( !lut || !table )
        return hipErrorInvalidValue;
    const dim3 grid( ( VRC_FIRST_VISIT_ENTRIES + 63u ) / 64u ), block( 64 );
    if( grey )
        hipLaunchKernelGGL( vrc_k_build_first_visit< vrc_f2 >, grid, block, 0, stream, lut, static_cast< vrc_f2* >( table ),
                            vrc_f2{ 0.f, 0.f } );
    else
        hipLaunchKernelGGL( vrc_k_build_first_visit< vrc_f4 >, grid, block, 0, stream, lut, static_cast< vrc_f4* >( table ),
                            vrc_f4{ 0.f, 0.f, 0.f, 0.f } );
    return hipGetLastError();
}

/* The resolved visit words (vrc_core.h: vrc_walk_resolved_word, vrc_frame::walkResolved): one lane per ray index below
 * walkPlane, each writing the walkK words of its ray; visit by visit the lanes of a wave read and write neighbouring
 * words of one plane.  Reads the lists and the slot words as they are on the stream */
__global__ __launch_bounds__( 256 ) void vrc_k_walk_resolve( const vrc_frame f, uint32_t* __restrict__ resolved )
{
    const uint32_t rayIndex = blockIdx.x * 256u + threadIdx.x;
    if( rayIndex >= f.walkPlane )
        return;
    for( uint32_t v = 0u; v < f.walkK; ++v )
        resolved[(size_t)rayIndex + (size_t)v * f.walkPlane] = vrc_walk_resolved_word( f, rayIndex, v );
}

hipError_t vrc_launch_walk_resolve( const vrc_frame& f, uint32_t* resolved, hipStream_t stream )
{
    if( !resolved || !f.walkCache || f.walkK == 0u || f.walkPlane == 0u || f.walkLean == 0u || f.walkSlots == 0u )
        return hipErrorInvalidValue;
    hipLaunchKernelGGL( vrc_k_walk_resolve, dim3( ( f.walkPlane + 255u ) / 256u ), dim3( 256 ), 0, stream, f, resolved );
    return hipGetLastError();
}

/* waves per SIMD, as vrc_k_raycast says them for the walking instances of the same march (vrc_kernels.hip) -- except that
 * the grey form in groups of 14, the judged instance, is allowed a sixth wave.  The walking instance is held at five
 * because six thrash the L1 under its gathers; the replay needs 76 registers (79 with the sample counter), and
 * measured at five against six waves (profiles/r10_walk_cache.txt) the uniform-brick frame runs 8 % faster at six and
 * the gather path no slower */
#ifndef VRC_REPLAY_GREY_MAX_WAVES
#define VRC_REPLAY_GREY_MAX_WAVES 6
#endif
/* The uniform-only instances (UNIFORM: vrc_pixel_walk_replay_lean< ..., true >, a lean frame none of whose visits
 * gathers) hold no gather march and need 20 to 24 registers (50 to 54 counted), so the registers allow eight waves per SIMD and the
 * attribute asks for them; they stage the classified table alone -- nothing in them steps through a brick, so no
 * vrc_addr_tab.  Waves per SIMD and waves per workgroup as measured on C2 (profiles/r15_uniform_only.txt) */
#ifndef VRC_REPLAY_UNIFORM_MAX_WAVES
#define VRC_REPLAY_UNIFORM_MAX_WAVES 8
#endif
#ifndef VRC_REPLAY_UNIFORM_WG_WAVES
#define VRC_REPLAY_UNIFORM_WG_WAVES VRC_WALK_WAVES /* (1: every wave stages a table of its own and meets no barrier) */
#endif
/* GROUP: samples a lane of the gather march keeps in flight -- what vrc_launch_raycast picks for the walking instance */
#define VRC_REPLAY_K_MIN_WAVES ( UNIFORM ? VRC_REPLAY_UNIFORM_MAX_WAVES : ( GROUP > VRC_GREY_GROUP ? 2 : 5 ) )
#define VRC_REPLAY_K_MAX_WAVES \
    ( UNIFORM ? VRC_REPLAY_UNIFORM_MAX_WAVES \
              : ( GROUP > VRC_GREY_GROUP ? 8 : ( MODE == VRC_MODE_GREY ? VRC_REPLAY_GREY_MAX_WAVES : 5 ) ) )
#define VRC_REPLAY_K_WAVES ( UNIFORM ? VRC_REPLAY_UNIFORM_WG_WAVES : VRC_WALK_WAVES )
/* LEAN: the replay of a lean list (vrc_frame::walkLean, vrc_pixel_walk_replay_lean); everything around the pixel is
 * the same kernel.  UNIFORM (with LEAN): its uniform-only form */
template < bool COUNT, int MODE, int GROUP, bool LEAN = false, bool UNIFORM = false >
__global__ __launch_bounds__( 64u * VRC_REPLAY_K_WAVES ) __attribute__( ( amdgpu_waves_per_eu( VRC_REPLAY_K_MIN_WAVES, VRC_REPLAY_K_MAX_WAVES ) ) ) void vrc_k_raycast_replay(
    const vrc_frame f, const vrc_dev_node* __restrict__ nodes, const uint8_t* __restrict__ atlas,
    const vrc_f4* __restrict__ lutGlobal, const vrc_classifier cls, vrc_f4* __restrict__ pixelBuffer,
    unsigned long long* __restrict__ sampleCounter, const uint32_t* __restrict__ tileOrder, const uint32_t tilesX,
    const uint32_t nTiles )
{
    static_assert( LEAN || !UNIFORM, "the uniform-only form replays lean lists" );
    constexpr uint32_t WAVES = VRC_REPLAY_K_WAVES, THREADS = 64u * WAVES;
    static_assert( MODE == VRC_MODE_TABLE || MODE == VRC_MODE_GREY, "the instances of the uniform-brick march" );
    /* the classified table (257 entries), as vrc_k_raycast stages it */
    __shared__ vrc_f4 lut[VRC_CLS8_ENTRIES];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    if( MODE == VRC_MODE_GREY )
    {
        vrc_f2* const lut2 = reinterpret_cast< vrc_f2* >( lut );
        for( uint32_t i = tid; i < VRC_LUT_ENTRIES; i += THREADS )
        {
            const vrc_f4 e = lutGlobal[i];
            lut2[i] = vrc_f2{ e.x, e.w };
        }
    }
    else
    {
        for( uint32_t i = tid; i < VRC_TFP_ENTRIES; i += THREADS )
            lut[i] = lutGlobal[i];
    }
    if constexpr( !UNIFORM )
    {
        const vrc_lay lay = vrc_make_lay( f.sbx, f.sby );
        for( uint32_t u = tid; u < 256u; u += THREADS )
        {
            vrc_addr_tab[u] = vrc_lay_x( lay, u );
            vrc_addr_tab[256u + u] = vrc_lay_y( lay, u );
            vrc_addr_tab[512u + u] = vrc_lay_z( lay, u );
        }
    }
    __syncthreads();
    /* from here on the waves of the workgroup are independent */
    /* the slot and its tile are the wave's: said so, the schedule's read and the tile's division by tilesX are scalar
     * work, and a lane adds its own 3 + 3 bits (vrc_core.h: vrc_replay_tile_origin) */
    const uint32_t slotIndex = __builtin_amdgcn_readfirstlane( blockIdx.x * WAVES + ( tid >> 6 ) );
    const uint32_t tilesY = nTiles / tilesX;
    if( slotIndex >= vrc_schedule_slots( tilesX, tilesY ) )
        return;
    const uint32_t tile = __builtin_amdgcn_readfirstlane( vrc_slot_tile( tileOrder, slotIndex, tilesX, tilesY ) );
    if( tile == VRC_NO_TILE )
        return;
    uint32_t x0, y0, px, py;
    vrc_replay_tile_origin( tile, tilesX, x0, y0 );
    vrc_replay_lane_pixel( x0, y0, lane, px, py );

    uint32_t nSamples = 0;
    if( px < f.width && py < f.height )
    {
        if constexpr( LEAN )
            vrc_pixel_walk_replay_lean< COUNT, MODE, GROUP, UNIFORM >( f, nodes, atlas, lut, cls, pixelBuffer, px, py,
                                                                       nSamples, tile * 64u + lane );
        else
            vrc_pixel_walk_replay< COUNT, MODE, GROUP >( f, nodes, atlas, lut, cls, pixelBuffer, px, py, nSamples,
                                                         tile * 64u + lane );
    }
    if( COUNT )
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

template < bool COUNT, int MODE, int GROUP, bool LEAN, bool UNIFORM = false >
static hipError_t launch_replay( const vrc_raycast_args& a, hipStream_t stream )
{
    const uint32_t tilesX = ( a.frame.width + 7u ) / 8u, tilesY = ( a.frame.height + 7u ) / 8u;
    const uint32_t nTiles = tilesX * tilesY;
    if( nTiles == 0 )
        return hipSuccess;
    constexpr uint32_t WAVES = VRC_REPLAY_K_WAVES;
    /* (the uniform-only form is a lean form: its name ends as theirs does) */
    vrc_internal_note_kernel( "vrc_k_raycast_replay<%s,%d,unsigned char,%d%s%s>", COUNT ? "true" : "false", (int)MODE, (int)GROUP,
                              UNIFORM ? ",uniform" : "", LEAN ? ",lean" : "" );
    vrc_internal_note_kernel_fn( (const void*)&vrc_k_raycast_replay< COUNT, MODE, GROUP, LEAN, UNIFORM >, (int)( 64u * WAVES ), 0 );
    vrc_launch_march( a, &vrc_k_raycast_replay< COUNT, MODE, GROUP, LEAN, UNIFORM >,
                      dim3( ( vrc_schedule_slots( tilesX, tilesY ) + WAVES - 1u ) / WAVES ), dim3( 64u * WAVES ), 0, stream,
                      a.frame, a.nodes, (const uint8_t*)a.atlas, a.lut, a.classifier, a.pixelBuffer, a.sampleCounter,
                      a.tileOrder, tilesX, nTiles );
    return hipGetLastError();
}

/* (the form of the lists and the sample counter: run-time choices among instances) */
template < int MODE, int GROUP >
static hipError_t launch_replay( const vrc_raycast_args& a, hipStream_t stream )
{
    if( a.frame.walkLean == VRC_WALK_LEAN_UNIFORM )
        return a.sampleCounter ? launch_replay< true, MODE, GROUP, true, true >( a, stream )
                               : launch_replay< false, MODE, GROUP, true, true >( a, stream );
    if( a.frame.walkLean != 0u )
        return a.sampleCounter ? launch_replay< true, MODE, GROUP, true >( a, stream )
                               : launch_replay< false, MODE, GROUP, true >( a, stream );
    return a.sampleCounter ? launch_replay< true, MODE, GROUP, false >( a, stream )
                           : launch_replay< false, MODE, GROUP, false >( a, stream );
}

/* the frames vrc_launch_raycast would march with <true,false,COUNT,true,TABLE or GREY,unsigned char,GROUP,false>, in the
 * group size it would take (vrc_walk_replay_group): anything else is the caller's mistake, not a frame to walk quietly */
hipError_t vrc_launch_raycast_replay( const vrc_raycast_args& a, hipStream_t stream )
{
    if( !vrc_walk_replay_eligible( a ) || !a.frame.walkCache || a.frame.walkK == 0u || a.frame.rayMode != VRC_RAY_LOAD ||
        ( a.frame.walkLean != 0u && a.frame.walkSlots == 0u ) )
        return hipErrorInvalidValue;
    const int group = vrc_walk_replay_group( a );
    if( a.greyTable )
        return group == VRC_SMALL_GROUP ? launch_replay< VRC_MODE_GREY, VRC_SMALL_GROUP >( a, stream )
                                             : launch_replay< VRC_MODE_GREY, VRC_GREY_GROUP >( a, stream );
    return group == VRC_SMALL_GROUP ? launch_replay< VRC_MODE_TABLE, VRC_SMALL_GROUP >( a, stream )
                                         : launch_replay< VRC_MODE_TABLE, VRC_GROUP >( a, stream );
}
