/*
 * preint_harness.cpp -- host build (g++) of the code of a pre-integrated composite frame (libre_amd/csrc/vrc_core.h: the
 * table builder vrc_preint_table_entry and the march vrc_preint_brick under vrc_pixel_reference_order /
 * vrc_pixel_grid_dda), for tests/test_preint_cpu.py.  TEST INFRASTRUCTURE ONLY.  The same call renders the plain frame
 * through the instances vrc_launch_raycast picks (preint = 0), so that the two can be compared bit for bit.
 *
 * With -DPREINT_HARNESS_MAIN the file is a stand-alone program for the address and undefined-behaviour sanitizers: tiny
 * scenes whose atlases are allocated to the exact element count, a table of exactly 256 x 256 entries on the heap, rays
 * along faces, edges and diagonals, every sampler form and voxel width.
 */
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

void classified( const float* tf, const vrc_lut_params& lp, std::vector< vrc_f4 >& lut, std::vector< vrc_f4 >& tfp )
{
    lut.resize( VRC_TFP_ENTRIES );
    tfp.resize( VRC_TFP_ENTRIES );
    for( uint32_t d = 0; d < 256; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    lut[256] = lut[257] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
    }
}

/* the table as vrc_k_build_preint fills it: exactly 256 x 256 entries */
void build_table( const float* tf, const vrc_f4* lut, const vrc_lut_params& lp, int kind, std::vector< vrc_f4 >& table )
{
    std::vector< vrc_preint_sum > prefix( VRC_PREINT_DIM );
    vrc_preint_prefix( tf, prefix.data() );
    table.resize( VRC_PREINT_ENTRIES );
    for( uint32_t row = 0; row < VRC_PREINT_DIM; ++row )
        for( uint32_t col = 0; col < VRC_PREINT_DIM; ++col )
            table[row * VRC_PREINT_DIM + col] = vrc_preint_table_entry( tf, lut, prefix.data(), lp, kind, row, col );
}

/* one pixel: the instance the launchers pick (vrc_launch_raycast / vrc_launch_raycast_preint) */
template < typename T >
void pixel( const vrc_frame& f, const vrc_host_tables& t, const T* atlas, const vrc_f4* table, const vrc_classifier& cls,
            vrc_f4* pb, uint32_t px, uint32_t py, uint32_t& n, bool grid, bool fixed, bool linear, bool preint )
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
    constexpr int PLAIN_POINT = sizeof( T ) == 1 ? VRC_MODE_TABLE : VRC_MODE_POINT;
    if( preint )
    {
        if( linear ) FORMS( VRC_MODE_PREINT_TRILINEAR, false )
        else if( fixed ) FORMS( VRC_MODE_PREINT, true )
        else FORMS( VRC_MODE_PREINT, false )
    }
    else
    {
        if( linear ) FORMS( VRC_MODE_TRILINEAR, false )
        else if( fixed ) FORMS( PLAIN_POINT, true )
        else FORMS( PLAIN_POINT, false )
    }
#undef FORMS
#undef ARGS_DDA
#undef ARGS_REF
}
} // namespace

/* the host builder's table of `kind` (0 value-indexed, 1 texel-indexed): out[256 * 256 * 4] */
extern "C" int preint_harness_table( const float* tf, float r0, float r1, float k, int fracBits, int kind, float* out )
{
    if( kind != VRC_PREINT_VALUE && kind != VRC_PREINT_TEXEL )
        return 1;
    vrc_lut_params lp;
    lp.rangeMin = r0;
    lp.rangeMax = r1;
    lp.alphaCorrection = k;
    lp.fracBits = fracBits;
    std::vector< vrc_f4 > lut, tfp, table;
    classified( tf, lp, lut, tfp );
    build_table( tf, lut.data(), lp, kind, table );
    std::memcpy( out, table.data(), table.size() * sizeof( vrc_f4 ) );
    return 0;
}

/* the classified table (256 entries of 4 floats) the value-indexed diagonal copies */
extern "C" int preint_harness_lut( const float* tf, float r0, float r1, float k, int fracBits, float* out )
{
    vrc_lut_params lp;
    lp.rangeMin = r0;
    lp.rangeMax = r1;
    lp.alphaCorrection = k;
    lp.fracBits = fracBits;
    for( uint32_t d = 0; d < 256; ++d )
    {
        const vrc_f4 e = vrc_lut_entry( tf, d, lp );
        out[d * 4] = e.x, out[d * 4 + 1] = e.y, out[d * 4 + 2] = e.z, out[d * 4 + 3] = e.w;
    }
    return 0;
}

/* form: bit 0 = grid walk (else reference order), bit 1 = fixed-point stepping, bit 3 = trilinear samples, bit 5 =
 * uniform bricks.  voxelBytes: 1, 2 or 4 (float).  first != 0: the frame's first pass (the pixel buffer is not read).
 * preint: VRC_OPT_PREINTEGRATION.  perPixel: W x H counts of this call, or null. */
extern "C" int preint_harness_render( const void* atlasRowMajor, uint32_t voxelBytes, const uint32_t atlasDim[3],
                                      const uint32_t slotDim[3], const uint32_t brickDim[3], float* pixelBuffer, uint32_t W,
                                      uint32_t H, const float* planes, uint32_t nPlanes, const float* tf,
                                      const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                                      const vrc_render_data* render, int form, int fracBits, int first, int preint,
                                      uint64_t* samplesOut, uint32_t* perPixel )
{
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
    std::vector< vrc_f4 > lut, tfp, pre;
    classified( tf, lp, lut, tfp );
    vrc_host_tables t;
    vrc_build_tables( geom, nodes, nNodes, t );
    const bool grid = ( form & 1 ) != 0, linear = ( form & 8 ) != 0;
    if( grid && !t.gridOk )
        return 2;
    const bool fixed = ( form & 2 ) != 0 && !linear && !t.clamp && slotDim[0] <= 248u && slotDim[1] <= 248u && slotDim[2] <= 248u;
    const bool classify = linear || voxelBytes != 1;
    const vrc_f4* const table = classify ? tfp.data() : lut.data();
    if( preint )
        build_table( tf, lut.data(), lp, classify ? VRC_PREINT_TEXEL : VRC_PREINT_VALUE, pre );
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
    f.preintTable = preint ? pre.data() : nullptr;

    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
            if( voxelBytes == 4 )
                pixel< float >( f, t, reinterpret_cast< const float* >( atlas32.data() ), table, cls, pb, px, py, n, grid, fixed, linear, preint != 0 );
            else if( voxelBytes == 2 )
                pixel< uint16_t >( f, t, atlas16.data(), table, cls, pb, px, py, n, grid, fixed, linear, preint != 0 );
            else
                pixel< uint8_t >( f, t, atlas8.data(), table, cls, pb, px, py, n, grid, fixed, linear, preint != 0 );
            total += n;
            if( perPixel )
                perPixel[(size_t)py * W + px] = n;
        }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}

/* ---- tiny scenes: the march against a one-sample-at-a-time loop, and the stand-alone program ---------------------------- */
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

void ramp_tf( float* tf, float alpha )
{
    for( int i = 0; i < 256; ++i )
    {
        const float v = (float)i / 255.0f;
        tf[i * 4 + 0] = v, tf[i * 4 + 1] = 1.0f - v, tf[i * 4 + 2] = 0.5f * v, tf[i * 4 + 3] = alpha * v;
    }
}

/* a segment of `count` samples inside brick 0 (the box [-0.5, 0]^3), oblique, as vrc_segment_complete leaves one */
vrc_segment oblique_segment( float stepSize, uint32_t count )
{
    const float d[3] = { 0.8f, 0.5f, 0.33166248f }; /* unit length to float precision */
    vrc_segment s;
    s.pos = vrc_f3{ -0.49f, -0.47f, -0.45f };
    s.step = vrc_f3{ d[0] * stepSize, d[1] * stepSize, d[2] * stepSize };
    s.dist = ( (float)count - 0.5f ) * stepSize;
    s.tNear = 1.0f;
    return s;
}

/* the march one sample at a time, over the same table, written here: positions as the float chain makes them */
template < typename T, bool TRILINEAR >
bool march_one_by_one( const tiny< T >& sc, const vrc_segment& s, const vrc_f4* table, const vrc_classifier& cls, vrc_f4& color,
                       uint32_t& n )
{
    const vrc_sampler sm = vrc_make_sampler( sc.t.nodes[0], sc.f );
    float travel = s.dist;
    vrc_f3 pos = s.pos;
    bool have = false;
    float before = 0.0f;
    while( travel > 0.0f )
    {
        float value;
        if( TRILINEAR )
        {
            const float lx = ( pos.x - sm.minx ) * sm.kx + sm.ox, ly = ( pos.y - sm.miny ) * sm.ky + sm.oy,
                        lz = ( pos.z - sm.minz ) * sm.kz + sm.oz;
            const vrc_taps t = vrc_trilinear_taps< false >( sm, lx, ly, lz );
            float v[8];
            for( int c = 0; c < 8; ++c )
                v[c] = (float)sc.atlas[t.ax[c & 1] + t.ay[( c >> 1 ) & 1] + t.az[c >> 2]];
            value = vrc_trilerp( v, t.wx, t.wy, t.wz );
            pos.x += s.step.x, pos.y += s.step.y, pos.z += s.step.z;
        }
        else
        {
            uint32_t idx;
            vrc_group_indices< false, 1 >( sm, pos, s.step, &idx );
            value = (float)sc.atlas[idx];
        }
        vrc_f4 e;
        if( !TRILINEAR && sizeof( T ) == 1 )
        {
            const uint32_t d = (uint32_t)value, p = have ? (uint32_t)before : d;
            e = table[p * VRC_PREINT_DIM + d];
            before = value;
        }
        else
        {
            const float x = vrc_preint_coord( value, cls );
            e = vrc_preint_read( table, have ? before : x, x );
            before = x;
        }
        have = true;
        vrc_composite( color, e );
        ++n;
        if( color.w > VRC_EARLY_EXIT )
            return true;
        travel -= sc.f.stepSize;
    }
    return false;
}

template < typename T, bool TRILINEAR >
int compare_marches( float alpha, float k, uint32_t maxCount, uint32_t* exits )
{
    float tf[256 * 4];
    ramp_tf( tf, alpha );
    vrc_lut_params lp;
    lp.rangeMin = 0.0f;
    lp.rangeMax = 255.0f;
    lp.alphaCorrection = k;
    lp.fracBits = 8;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > lut, tfp, table;
    classified( tf, lp, lut, tfp );
    constexpr bool VALUE = !TRILINEAR && sizeof( T ) == 1;
    build_table( tf, lut.data(), lp, VALUE ? VRC_PREINT_VALUE : VRC_PREINT_TEXEL, table );
    const float stepSize = 1.0f / 96.0f;
    tiny< T > sc;
    build( sc, 1u, stepSize );
    sc.f.preintTable = table.data();
    constexpr int MODE = TRILINEAR ? VRC_MODE_PREINT_TRILINEAR : VRC_MODE_PREINT;
    for( uint32_t count = 1; count <= maxCount; ++count )
    {
        const vrc_segment s = oblique_segment( stepSize, count );
        const vrc_segment_ready src = { s };
        vrc_f4 a = { 0.f, 0.f, 0.f, 0.f }, b = a;
        uint32_t na = 0, nb = 0;
        const bool da = vrc_preint_brick< false, true, false, MODE, T, false, vrc_segment_ready >(
            sc.f, sc.t.nodes[0], src, sc.atlas.data(), VALUE ? lut.data() : tfp.data(), cls, a, na );
        const bool db = march_one_by_one< T, TRILINEAR >( sc, s, table.data(), cls, b, nb );
        if( da != db || na != nb || std::memcmp( &a, &b, sizeof( a ) ) != 0 )
            return (int)count;
        if( da && exits )
            exits[na < 64u ? na : 63u] += 1u; /* the sample at which the ray left, counted from 1 */
    }
    return 0;
}
} // namespace

/* The grouped march against the one-sample-at-a-time loop, bit for bit, on segments of 1 ... maxCount samples of brick 0 of
 * a tiny scene (float chain; point samples of 8- and 16-bit voxels, and trilinear samples).  alpha: the ramp's largest
 * opacity, k: the opacity exponent -- high values end rays early; exits[64] (may be null) counts, per sample number, the rays that left at it.
 * Returns 0, or the first count at which the two differ */
extern "C" int preint_harness_march( int voxelBytes, int linear, float alpha, float k, uint32_t maxCount, uint32_t* exits )
{
    if( voxelBytes == 1 )
        return linear ? compare_marches< uint8_t, true >( alpha, k, maxCount, exits )
                      : compare_marches< uint8_t, false >( alpha, k, maxCount, exits );
    if( voxelBytes == 2 )
        return linear ? compare_marches< uint16_t, true >( alpha, k, maxCount, exits )
                      : compare_marches< uint16_t, false >( alpha, k, maxCount, exits );
    return -1;
}

extern "C" int preint_harness_groups( int* value, int* texel )
{
    *value = VRC_PREINT_GROUP;
    *texel = VRC_PREINT_GROUP_TEXEL;
    return 0;
}

#if defined( PREINT_HARNESS_MAIN )
/* ---- the stand-alone program ------------------------------------------------------------------------------------------- */
namespace
{
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
uint64_t march( const tiny< T >& sc, const vrc_ray& r, const vrc_f4* lut, const vrc_f4* tfp, const vrc_f4* value,
                const vrc_f4* texel, const vrc_classifier& cls, double* sum )
{
    uint64_t total = 0;
    if( !r.hit )
        return 0;
    for( int form = 0; form < ( CLAMP ? 2 : 3 ); ++form ) /* 0: point, float chain; 1: trilinear; 2: point, fixed-point stepping */
    {
        vrc_f4 color = { 0.f, 0.f, 0.f, 0.f };
        uint32_t n = 0;
        vrc_frame f = sc.f;
        f.preintTable = ( form != 1 && sizeof( T ) == 1 ) ? value : texel;
        for( uint32_t i = 0; i < f.nodeCount; ++i )
        {
            vrc_segment s;
            bool stop;
            if( !vrc_brick_segment( f, r, sc.t.nodes[i], f.stepSize, &s, &stop ) )
            {
                if( stop )
                    break;
                continue;
            }
            const vrc_segment_ready src = { s };
            bool done;
            const vrc_f4* const table = sizeof( T ) == 1 ? lut : tfp;
            if( form == 1 )
                done = vrc_preint_brick< CLAMP, true, false, VRC_MODE_PREINT_TRILINEAR, T, false, vrc_segment_ready >(
                    f, sc.t.nodes[i], src, sc.atlas.data(), tfp, cls, color, n );
            else if( form == 2 )
                done = vrc_preint_brick< false, true, !CLAMP, VRC_MODE_PREINT, T, false, vrc_segment_ready >(
                    f, sc.t.nodes[i], src, sc.atlas.data(), table, cls, color, n );
            else
                done = vrc_preint_brick< CLAMP, true, false, VRC_MODE_PREINT, T, false, vrc_segment_ready >(
                    f, sc.t.nodes[i], src, sc.atlas.data(), table, cls, color, n );
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
    ramp_tf( tf, 0.05f );
    tf[100 * 4 + 3] = 1.0f; /* a spike that crosses 255/256 inside two texel intervals */
    vrc_lut_params lp;
    lp.rangeMin = 0.0f;
    lp.rangeMax = 255.0f;
    lp.alphaCorrection = 1.0f;
    lp.fracBits = 8;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > lut, tfp, value, texel;
    classified( tf, lp, lut, tfp );
    build_table( tf, lut.data(), lp, VRC_PREINT_VALUE, value );
    build_table( tf, lut.data(), lp, VRC_PREINT_TEXEL, texel );
    uint64_t total = 0;
    static const float steps[2] = { 1.0f / 32.0f, (float)( 1.0 / 37.0 ) };
    for( uint32_t overlap = 0; overlap < 2u; ++overlap )
        for( float step : steps )
        {
            tiny< T > sc;
            build( sc, overlap, step );
            if( sc.t.clamp != ( overlap == 0u ) )
                return ~0ull;
#define MARCH( R ) ( overlap ? march< T, false >( sc, R, lut.data(), tfp.data(), value.data(), texel.data(), cls, sum ) \
                             : march< T, true >( sc, R, lut.data(), tfp.data(), value.data(), texel.data(), cls, sum ) )
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
                            total += MARCH( r );
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
                    total += MARCH( r );
                    ++*rays;
                }
            /* from inside, towards every corner */
            for( int c = 0; c < 8; ++c )
            {
                const float o[3] = { 0.01f, -0.02f, 0.03f };
                const float to[3] = { ( c & 1 ) ? 0.5f : -0.5f, ( c & 2 ) ? 0.5f : -0.5f, ( c & 4 ) ? 0.5f : -0.5f };
                const vrc_ray r = make_ray( o, to );
                total += MARCH( r );
                ++*rays;
            }
#undef MARCH
        }
    return total;
}
} // namespace

int main()
{
    double sum = 0.0;
    uint64_t rays = 0;
    const uint64_t a = run_type< uint8_t >( &sum, &rays );
    const uint64_t b = run_type< uint16_t >( &sum, &rays );
    const uint64_t c = run_type< float >( &sum, &rays );
    if( a == ~0ull || b == ~0ull || c == ~0ull )
        return 2;
    /* the grouped march against the one-sample loop, once more under the sanitizers */
    const int m = preint_harness_march( 1, 0, 0.9f, 1.0f, 3u * VRC_PREINT_GROUP + 2u, nullptr ) |
                  preint_harness_march( 2, 1, 0.9f, 1.0f, 3u * VRC_PREINT_GROUP + 2u, nullptr );
    std::printf( "rays %llu samples %llu checksum %.6f marches %d\n", (unsigned long long)rays, (unsigned long long)( a + b + c ),
                 sum, m );
    return ( a + b + c ) > 0 && m == 0 && std::isfinite( sum ) ? 0 : 1;
}
#endif
