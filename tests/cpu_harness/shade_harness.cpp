/*
 * shade_harness.cpp -- host build (g++) of the per-ray code of a shaded composite frame (libre_amd/csrc/vrc_core.h:
 * vrc_extension_brick under vrc_pixel_reference_order / vrc_pixel_grid_dda), for tests/test_shade_cpu.py.  TEST
 * INFRASTRUCTURE ONLY.  The same call renders the unshaded frame through the instances vrc_launch_raycast picks
 * (shading = 0), so that the two can be compared bit for bit.
 *
 * With -DSHADE_HARNESS_MAIN the file is a stand-alone program for the address and undefined-behaviour sanitizers: tiny
 * scenes whose atlases are allocated to the exact element count, rays along faces, edges and diagonals, every sampler.
 * It is the check that no neighbour gather of the gradient leaves its slot.
 */
#define VRC_SHADE_SKIP_HOOK 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

namespace
{
/* row-major atlas -> micro-blocked atlas, and the uniformity word of every slot reduced over its brick (8-bit voxels) */
template < typename T >
void upload( const void* rowMajor, const uint32_t atlasDim[3], const vrc_layout& lay, const uint32_t brick[3],
             std::vector< T >& atlas, std::vector< uint32_t >& info )
{
    const T* const src = static_cast< const T* >( rowMajor );
    atlas.resize( (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2] );
    const uint32_t nSlots = lay.slots[0] * lay.slots[1] * lay.slots[2];
    info.assign( nSlots, 0u );
    std::vector< T > first( nSlots );
    for( uint32_t z = 0; z < atlasDim[2]; ++z )
        for( uint32_t y = 0; y < atlasDim[1]; ++y )
            for( uint32_t x = 0; x < atlasDim[0]; ++x )
            {
                const T v = src[( (size_t)z * atlasDim[1] + y ) * atlasDim[0] + x];
                atlas[vrc_atlas_index( lay, x, y, z )] = v;
                const uint32_t i = x / lay.slotDim[0], j = y / lay.slotDim[1], k = z / lay.slotDim[2];
                const uint32_t lx = x - i * lay.slotDim[0], ly = y - j * lay.slotDim[1], lz = z - k * lay.slotDim[2];
                if( lx >= brick[0] || ly >= brick[1] || lz >= brick[2] || sizeof( T ) != 1 )
                    continue;
                const uint32_t slot = ( k * lay.slots[1] + j ) * lay.slots[0] + i;
                if( !( info[slot] & VRC_SLOT_KNOWN ) )
                {
                    first[slot] = v;
                    info[slot] = VRC_SLOT_KNOWN | (uint32_t)v;
                }
                else if( v != first[slot] )
                    info[slot] |= VRC_SLOT_MIXED;
            }
}

/* one pixel: the instance the launchers pick (vrc_launch_raycast / vrc_launch_raycast_shade) */
template < typename T >
void pixel( const vrc_frame& f, const vrc_host_tables& t, const T* atlas, const vrc_f4* table, const vrc_classifier& cls,
            vrc_f4* pb, uint32_t px, uint32_t py, uint32_t& n, bool grid, bool fixed, bool linear, bool shading )
{
#define ARGS_DDA f, t.nodes.data(), t.grid.data(), atlas, table, cls, pb, px, py, n
#define ARGS_REF f, t.nodes.data(), atlas, table, cls, pb, px, py, n
#define FORMS( MODE, FIXED )                                                                          \
    {                                                                                                 \
        if( grid && t.clamp ) vrc_pixel_grid_dda< true, true, false, MODE, T >( ARGS_DDA );           \
        else if( grid ) vrc_pixel_grid_dda< false, true, FIXED, MODE, T >( ARGS_DDA );                \
        else if( t.clamp ) vrc_pixel_reference_order< true, true, false, MODE, T >( ARGS_REF );       \
        else vrc_pixel_reference_order< false, true, FIXED, MODE, T >( ARGS_REF );                    \
    }
    constexpr int UNSHADED_POINT = sizeof( T ) == 1 ? VRC_MODE_TABLE : VRC_MODE_POINT;
    if( shading )
    {
        if( linear ) FORMS( VRC_MODE_SHADE_TRILINEAR, false )
        else if( fixed ) FORMS( VRC_MODE_SHADE, true )
        else FORMS( VRC_MODE_SHADE, false )
    }
    else
    {
        if( linear ) FORMS( VRC_MODE_TRILINEAR, false )
        else if( fixed ) FORMS( UNSHADED_POINT, true )
        else FORMS( UNSHADED_POINT, false )
    }
#undef FORMS
#undef ARGS_DDA
#undef ARGS_REF
}
} // namespace

/* form: bit 0 = grid walk (else reference order), bit 1 = fixed-point stepping, bit 3 = trilinear samples, bit 5 =
 * uniform bricks.  voxelBytes: 1, 2 or 4 (float).  first != 0: the frame's first pass (the pixel buffer is not read).
 * shading: VRC_OPT_SHADING; ambient: VRC_OPT_SHADING_AMBIENT / 1000; skip = 0: the gradient of transparent samples is
 * gathered too.  perPixel, withGradient, withoutGradient: W x H counts of this call (samples taken; of those, with and
 * without their six neighbour gathers), or null.  rays: W x H x 3 unit directions, or null. */
extern "C" int shade_harness_render( const void* atlasRowMajor, uint32_t voxelBytes, const uint32_t atlasDim[3],
                                    const uint32_t slotDim[3], const uint32_t brickDim[3], float* pixelBuffer, uint32_t W,
                                    uint32_t H, const float* planes, uint32_t nPlanes, const float* tf,
                                    const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                                    const vrc_render_data* render, int form, int fracBits, int first, int shading,
                                    float ambient, int skip, uint64_t* samplesOut, uint32_t* perPixel,
                                    uint32_t* withGradient, uint32_t* withoutGradient, float* rays )
{
    if( !( ambient >= 0.0f && ambient <= 1.0f ) )
        return 1;
    vrc_atlas_geom geom;
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        if( atlasDim[a] % 8u || slotDim[a] % 8u || atlasDim[a] % slotDim[a] )
            return 1;
        geom.atlasDim[a] = atlasDim[a];
        geom.slotDim[a] = slotDim[a];
        geom.slots[a] = lay.slots[a] = atlasDim[a] / slotDim[a];
        lay.slotDim[a] = slotDim[a];
    }
    std::vector< uint8_t > atlas8;
    std::vector< uint16_t > atlas16;
    std::vector< uint32_t > atlas32, info;
    if( voxelBytes == 1 )
        upload< uint8_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas8, info );
    else if( voxelBytes == 2 )
        upload< uint16_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas16, info );
    else if( voxelBytes == 4 )
        upload< uint32_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas32, info );
    else
        return 1;

    vrc_lut_params lp;
    lp.rangeMin = render->dataSourceRange[0];
    lp.rangeMax = render->dataSourceRange[1];
    lp.alphaCorrection = (float)render->maxSamplesPerRay / (float)render->samplesPerRay;
    lp.fracBits = fracBits;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > lut( VRC_TFP_ENTRIES ), tfp( VRC_TFP_ENTRIES );
    for( uint32_t d = 0; d < 256; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    lut[256] = lut[257] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
    }
    vrc_host_tables t;
    vrc_build_tables( geom, nodes, nNodes, t );
    const bool grid = ( form & 1 ) != 0, linear = ( form & 8 ) != 0;
    if( grid && !t.gridOk )
        return 2;
    const bool fixed = ( form & 2 ) != 0 && !linear && !t.clamp && slotDim[0] <= 248u && slotDim[1] <= 248u && slotDim[2] <= 248u;
    const vrc_f4* const table = ( linear || voxelBytes != 1 ) ? tfp.data() : lut.data();
    float pl[6][4];
    std::memset( pl, 0, sizeof( pl ) );
    for( uint32_t i = 0; i < nPlanes && i < 6; ++i )
        for( int k = 0; k < 4; ++k )
            pl[i][k] = planes[i * 4 + k];
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    vrc_fill_frame( f, *view, *render, geom, t.g, pl, nPlanes, nNodes, W, H, 0.f, 0.f );
    f.variant = VRC_VARIANT_CUDA;
    f.samplesPerPixel = 1u;
    f.clearFirst = first ? 1u : 0u;
    f.slotInfo = ( form & 32 ) ? info.data() : nullptr;
    f.shadeAmbient = shading ? ambient : 0.0f;
    vrc_shade_skip_hook = skip ? 1 : 0;

    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
            vrc_shade_gradients[0] = vrc_shade_gradients[1] = 0ull;
            if( voxelBytes == 4 )
                pixel< float >( f, t, reinterpret_cast< const float* >( atlas32.data() ), table, cls, pb, px, py, n, grid, fixed, linear, shading != 0 );
            else if( voxelBytes == 2 )
                pixel< uint16_t >( f, t, atlas16.data(), table, cls, pb, px, py, n, grid, fixed, linear, shading != 0 );
            else
                pixel< uint8_t >( f, t, atlas8.data(), table, cls, pb, px, py, n, grid, fixed, linear, shading != 0 );
            total += n;
            const size_t i = (size_t)py * W + px;
            if( perPixel )
                perPixel[i] = n;
            if( withGradient )
                withGradient[i] = (uint32_t)vrc_shade_gradients[1];
            if( withoutGradient )
                withoutGradient[i] = (uint32_t)vrc_shade_gradients[0];
            if( rays )
            {
                const vrc_ray r = vrc_setup_ray( f, px, py );
                rays[3 * i] = r.dir.x, rays[3 * i + 1] = r.dir.y, rays[3 * i + 2] = r.dir.z;
            }
        }
    vrc_shade_skip_hook = 1;
    if( samplesOut )
        *samplesOut = total;
    return 0;
}

#if defined( SHADE_HARNESS_MAIN )
/* ---- the stand-alone program ------------------------------------------------------------------------------------------- */
namespace
{
/* 2 x 2 x 2 bricks of 8^3 voxels in the unit cube at -0.5, overlap 0 (slots of 8^3: the clamped sampler) or 1 (slots of
 * 16^3); the atlas holds exactly slots x slot elements */
template < typename T >
struct tiny
{
    vrc_atlas_geom geom;
    std::vector< T > atlas;
    vrc_host_tables t;
    vrc_frame f;
};

template < typename T >
void build( tiny< T >& sc, uint32_t overlap, float stepSize )
{
    const uint32_t slot = overlap ? 16u : 8u;
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        sc.geom.slotDim[a] = lay.slotDim[a] = slot;
        sc.geom.slots[a] = lay.slots[a] = 2u;
        sc.geom.atlasDim[a] = 2u * slot;
    }
    sc.atlas.assign( (size_t)8u * slot * slot * slot, (T)0 ); /* exactly: no slack behind the last slot */
    std::vector< vrc_node_data > nodes( 8 );
    uint32_t i = 0;
    for( uint32_t z = 0; z < 2u; ++z )
        for( uint32_t y = 0; y < 2u; ++y )
            for( uint32_t x = 0; x < 2u; ++x, ++i )
            {
                const uint32_t c[3] = { x, y, z };
                for( int a = 0; a < 3; ++a )
                {
                    nodes[i].aabbMin[a] = -0.5f + 0.5f * (float)c[a];
                    nodes[i].aabbSize[a] = 0.5f;
                    nodes[i].textureMin[a] = (float)( c[a] * slot + overlap ) / (float)sc.geom.atlasDim[a];
                    nodes[i].textureSize[a] = 8.0f / (float)sc.geom.atlasDim[a];
                }
                for( uint32_t vz = 0; vz < slot; ++vz )
                    for( uint32_t vy = 0; vy < slot; ++vy )
                        for( uint32_t vx = 0; vx < slot; ++vx )
                        {
                            uint32_t h = ( i * 4096u + ( vz * 16u + vy ) * 16u + vx ) * 2654435761u;
                            h ^= h >> 15;
                            sc.atlas[vrc_atlas_index( lay, x * slot + vx, y * slot + vy, z * slot + vz )] = (T)( 20u + ( h >> 8 ) % 200u );
                        }
            }
    vrc_build_tables( sc.geom, nodes.data(), 8u, sc.t );
    vrc_frame& f = sc.f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = VRC_VARIANT_CUDA;
    f.stepSize = stepSize;
    f.width = f.height = 1u;
    f.nodeCount = 8u;
    f.sbx = f.sby = slot / 8u;
    f.samplesPerPixel = 1u;
    f.shadeAmbient = 0.25f;
    for( int a = 0; a < 3; ++a )
    {
        f.aabbMin[a] = -0.5f;
        f.aabbMax[a] = 0.5f;
        f.slotDim[a] = slot;
        f.gridMin[a] = sc.t.g.gridMin[a];
        f.cellSize[a] = sc.t.g.cellSize[a];
        f.invCellSize[a] = sc.t.g.invCellSize[a];
        f.gridDim[a] = sc.t.g.gridDim[a];
    }
}

vrc_ray make_ray( const float o[3], const float to[3] )
{
    vrc_ray r;
    float d[3] = { to[0] - o[0], to[1] - o[1], to[2] - o[2] };
    const float len = std::sqrt( d[0] * d[0] + d[1] * d[1] + d[2] * d[2] );
    for( int a = 0; a < 3; ++a )
    {
        d[a] /= len;
        if( d[a] == 0.0f )
            d[a] = VRC_EPSILON;
    }
    r.origin = vrc_f3{ o[0], o[1], o[2] };
    r.dir = vrc_f3{ d[0], d[1], d[2] };
    r.invDir = vrc_f3{ 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
    const vrc_f3 lo = { -0.5f, -0.5f, -0.5f }, hi = { 0.5f, 0.5f, 0.5f };
    r.hit = vrc_intersect_box( r.origin, r.invDir, lo, hi, &r.tNearGlobal, &r.tFarGlobal );
    r.tNearPlane = 0.0f;
    return r;
}

/* one ray through the bricks in list order, every sampler of the type; returns the samples taken */
template < typename T, bool CLAMP >
uint64_t march( const tiny< T >& sc, const vrc_ray& r, const vrc_f4* lut, const vrc_f4* tfp, const vrc_classifier& cls,
                double* sum )
{
    uint64_t total = 0;
    if( !r.hit )
        return 0;
    for( int form = 0; form < ( CLAMP ? 2 : 3 ); ++form ) /* 0: point, float chain; 1: trilinear; 2: point, fixed-point stepping */
    {
        vrc_f4 color = { 0.f, 0.f, 0.f, 0.f };
        uint32_t n = 0;
        for( uint32_t i = 0; i < sc.f.nodeCount; ++i )
        {
            vrc_segment s;
            bool stop;
            if( !vrc_brick_segment( sc.f, r, sc.t.nodes[i], sc.f.stepSize, &s, &stop ) )
            {
                if( stop )
                    break;
                continue;
            }
            const vrc_segment_ready src = { s };
            bool done;
            const vrc_f4* const table = sizeof( T ) == 1 ? lut : tfp;
            if( form == 1 )
                done = vrc_extension_brick< CLAMP, true, false, VRC_MODE_SHADE_TRILINEAR, T, false, vrc_segment_ready >(
                    sc.f, sc.t.nodes[i], src, r.dir, sc.atlas.data(), tfp, cls, color, n, nullptr );
            else if( form == 2 )
                done = vrc_extension_brick< false, true, !CLAMP, VRC_MODE_SHADE, T, false, vrc_segment_ready >(
                    sc.f, sc.t.nodes[i], src, r.dir, sc.atlas.data(), table, cls, color, n, nullptr );
            else
                done = vrc_extension_brick< CLAMP, true, false, VRC_MODE_SHADE, T, false, vrc_segment_ready >(
                    sc.f, sc.t.nodes[i], src, r.dir, sc.atlas.data(), table, cls, color, n, nullptr );
            if( done )
                break;
        }
        total += n;
        *sum += (double)color.x + (double)color.w;
    }
    return total;
}

template < typename T >
uint64_t run_type( double* sum, uint64_t* rays )
{
    float tf[256 * 4];
    for( int i = 0; i < 256; ++i )
    {
        const float v = (float)i / 255.0f;
        tf[i * 4 + 0] = v, tf[i * 4 + 1] = 1.0f - v, tf[i * 4 + 2] = 0.5f * v, tf[i * 4 + 3] = 0.05f * v;
    }
    vrc_lut_params lp;
    lp.rangeMin = 0.0f;
    lp.rangeMax = 255.0f;
    lp.alphaCorrection = 1.0f;
    lp.fracBits = 8;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > lut( VRC_TFP_ENTRIES ), tfp( VRC_TFP_ENTRIES );
    for( uint32_t d = 0; d < 256; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    lut[256] = lut[257] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
    }
    uint64_t total = 0;
    static const float steps[2] = { 1.0f / 32.0f, (float)( 1.0 / 37.0 ) };
    for( uint32_t overlap = 0; overlap < 2u; ++overlap )
        for( float step : steps )
        {
            tiny< T > sc;
            build( sc, overlap, step );
            if( sc.t.clamp != ( overlap == 0u ) )
                return ~0ull;
            /* rays through and along the outer faces, the inner brick faces, the edges and the corners, and the diagonals */
            static const float at[] = { -0.5f, -0.4999999f, -0.25f, -1e-7f, 0.0f, 1e-7f, 0.3f, 0.4999999f, 0.5f };
            for( int ax = 0; ax < 3; ++ax )
                for( float u : at )
                    for( float v : at )
                        for( int dir = 0; dir < 2; ++dir )
                        {
                            float o[3], to[3];
                            o[ax] = dir ? 1.5f : -1.5f;
                            to[ax] = dir ? -1.5f : 1.5f;
                            o[( ax + 1 ) % 3] = to[( ax + 1 ) % 3] = u;
                            o[( ax + 2 ) % 3] = to[( ax + 2 ) % 3] = v;
                            const vrc_ray r = make_ray( o, to );
                            total += overlap ? march< T, false >( sc, r, lut.data(), tfp.data(), cls, sum )
                                             : march< T, true >( sc, r, lut.data(), tfp.data(), cls, sum );
                            ++*rays;
                        }
            for( int c = 0; c < 8; ++c ) /* the space diagonals, both ways, and face diagonals in the outer faces */
                for( int k = 0; k < 3; ++k )
                {
                    float o[3], to[3];
                    for( int a = 0; a < 3; ++a )
                    {
                        const float sgn = ( ( c >> a ) & 1 ) ? 1.0f : -1.0f;
                        o[a] = 1.5f * sgn;
                        to[a] = -1.5f * sgn;
                    }
                    if( k > 0 )
                        o[k - 1] = to[k - 1] = ( c & 1 ) ? 0.5f : -0.5f;
                    const vrc_ray r = make_ray( o, to );
                    total += overlap ? march< T, false >( sc, r, lut.data(), tfp.data(), cls, sum )
                                     : march< T, true >( sc, r, lut.data(), tfp.data(), cls, sum );
                    ++*rays;
                }
            /* from inside, towards every corner */
            for( int c = 0; c < 8; ++c )
            {
                const float o[3] = { 0.01f, -0.02f, 0.03f };
                const float to[3] = { ( c & 1 ) ? 0.5f : -0.5f, ( c & 2 ) ? 0.5f : -0.5f, ( c & 4 ) ? 0.5f : -0.5f };
                const vrc_ray r = make_ray( o, to );
                total += overlap ? march< T, false >( sc, r, lut.data(), tfp.data(), cls, sum )
                                 : march< T, true >( sc, r, lut.data(), tfp.data(), cls, sum );
                ++*rays;
            }
        }
    return total;
}
} // namespace

int main()
{
    double sum = 0.0;
    uint64_t rays = 0;
    vrc_shade_skip_hook = 0; /* every sample gathers its six neighbours */
    const uint64_t a = run_type< uint8_t >( &sum, &rays );
    const uint64_t b = run_type< uint16_t >( &sum, &rays );
    const uint64_t c = run_type< float >( &sum, &rays );
    if( a == ~0ull || b == ~0ull || c == ~0ull )
        return 2;
    std::printf( "rays %llu samples %llu gradients %llu skipped %llu checksum %.6f\n", (unsigned long long)rays,
                 (unsigned long long)( a + b + c ), (unsigned long long)vrc_shade_gradients[1],
                 (unsigned long long)vrc_shade_gradients[0], sum );
    return ( a + b + c ) > 0 && vrc_shade_gradients[1] == a + b + c && std::isfinite( sum ) ? 0 : 1;
}
#endif
