/*
 * walk_cache_harness.cpp -- the walk cache on the host build of the per-ray code (libre_amd/csrc/vrc_core.h), for
 * tests/test_walk_cache_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * Generated rays over small brick grids (1x1x1, 4x4x4, 4x3x2 bricks of 8^3 voxels with an overlap of 4, every third
 * brick constant -- overlap included -- and marked so in the uniformity words).  For every ray:
 *   - the walk (vrc_pixel_grid_dda, rays loaded from a ray cache) under a table that cannot end a ray, with a hook on
 *     every visit it hands to a march (vrc_core.h: VRC_WALK_VISIT_HOOK): the sequence (node, tNear, tFar);
 *   - the count pass and the record pass (vrc_pixel_walk_record): the count must be the sequence's length, the planes
 *     its nodes, the bits of tNear and tFar, and the bits of vrc_segment_dist -- and no word outside the ray's own
 *     column, or beyond walkK visits, may be written;
 *   - under four tables (alpha 0.05 and 1.0, grey and coloured) the walk and the replay from the list recorded ONCE
 *     (vrc_pixel_walk_replay): the same pixel bits and sample count; the walk's visits under an opaque table must be a
 *     prefix of the list (early termination truncates the walk, never the list); the coloured tables also onto a
 *     pixel that is not cleared first.
 * Built as a shared library (walk_cache_run) and, with -DWALK_CACHE_MAIN, as a stand-alone program for the sanitizers.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

struct vrc_dev_node;
struct vrc_ray;
struct vrc_interval;
static void walk_visit_hook( const vrc_dev_node& n, const vrc_ray& r, const vrc_interval& iv );
#define VRC_WALK_VISIT_HOOK( n, r, iv ) walk_visit_hook( n, r, iv )
#include "../../libre_amd/csrc/vrc_tables.h"

struct visit
{
    uint32_t node, dist, tNear, tFar; /* bits */
};
static std::vector< visit > g_seen;
static const std::vector< vrc_dev_node >* g_nodes = nullptr;

static void walk_visit_hook( const vrc_dev_node& n, const vrc_ray& r, const vrc_interval& iv )
{
    uint32_t node = 0xFFFFFFFFu;
    for( size_t i = 0; i < g_nodes->size(); ++i ) /* (a brick is its box: the bricks of a grid do not share one) */
        if( std::memcmp( ( *g_nodes )[i].aabbMin, n.aabbMin, sizeof( n.aabbMin ) ) == 0 )
            node = (uint32_t)i;
    const visit v = { node, vrc_float_bits( vrc_segment_dist( r, iv ) ), vrc_float_bits( iv.tNear ), vrc_float_bits( iv.tFar ) };
    g_seen.push_back( v );
}

struct rng
{
    uint64_t s;
    uint32_t next()
    {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)( s >> 16 );
    }
    float unit() { return (float)( next() & 0xFFFFFFu ) / 16777216.0f; }
    float in( float a, float b ) { return a + ( b - a ) * unit(); }
    uint32_t below( uint32_t n ) { return next() % n; }
};

enum
{
    KIND_AXIS_FACE,   /* axis-parallel, through a brick face plane exactly */
    KIND_AXIS_EDGE,   /* axis-parallel, along a brick edge exactly */
    KIND_AXIS_CORNER, /* oblique in a plane, through a brick corner exactly */
    KIND_OBLIQUE,
    KIND_EYE_INSIDE,
    KIND_NEAR_INSIDE, /* the near plane inside a brick */
    KIND_CLIPPED,     /* clip planes: the ray's global interval cut (both variants), per-brick planes (GL variant) */
    KINDS
};
/* per kind: [0] cases, [1] rays with a list, [2] visits, [3] rays an opaque table ended before the list's end,
 * [4] visits of uniform bricks, [5] mismatches */
#define TALLY 6

struct scene
{
    int dims[3];
    vrc_atlas_geom geom;
    std::vector< uint8_t > atlas;
    std::vector< uint32_t > info;
    vrc_host_tables t;
    float boxMin[3], boxMax[3], cell;
};

static void build_scene( scene& sc, int bx, int by, int bz )
{
    sc.dims[0] = bx;
    sc.dims[1] = by;
    sc.dims[2] = bz;
    const uint32_t n = (uint32_t)( bx * by * bz );
    const int longest = bx > by ? ( bx > bz ? bx : bz ) : ( by > bz ? by : bz );
    sc.cell = 1.0f / (float)longest;
    for( int a = 0; a < 3; ++a )
    {
        sc.geom.slotDim[a] = 16u;
        sc.geom.slots[a] = a == 0 ? n : 1u;
        sc.geom.atlasDim[a] = sc.geom.slots[a] * 16u;
        sc.boxMin[a] = -0.5f;
        sc.boxMax[a] = -0.5f + sc.cell * (float)sc.dims[a];
    }
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        lay.slots[a] = sc.geom.slots[a];
        lay.slotDim[a] = 16u;
    }
    sc.atlas.assign( (size_t)n * 4096u, 0 );
    sc.info.assign( n, 0u );
    std::vector< vrc_node_data > nodes( n );
    uint32_t i = 0;
    for( int z = 0; z < bz; ++z )
        for( int y = 0; y < by; ++y )
            for( int x = 0; x < bx; ++x, ++i )
            {
                const int c[3] = { x, y, z };
                vrc_node_data& nd = nodes[i];
                for( int a = 0; a < 3; ++a )
                {
                    nd.aabbMin[a] = -0.5f + sc.cell * (float)c[a];
                    nd.aabbSize[a] = sc.cell;
                    nd.textureMin[a] = (float)( ( a == 0 ? i * 16u : 0u ) + 4u ) / (float)sc.geom.atlasDim[a];
                    nd.textureSize[a] = 8.0f / (float)sc.geom.atlasDim[a];
                }
                const bool uniform = i % 3u == 1u;
                const uint8_t first = (uint8_t)( 40u + 23u * i );
                for( uint32_t vz = 0; vz < 16u; ++vz )
                    for( uint32_t vy = 0; vy < 16u; ++vy )
                        for( uint32_t vx = 0; vx < 16u; ++vx )
                        {
                            uint32_t h = ( i * 4096u + ( vz * 16u + vy ) * 16u + vx ) * 2654435761u;
                            h ^= h >> 15;
                            sc.atlas[vrc_atlas_index( lay, i * 16u + vx, vy, vz )] = uniform ? first : (uint8_t)( 30u + ( h >> 8 ) % 200u );
                        }
                const uint8_t v0 = sc.atlas[vrc_slot_base( lay, i, 0, 0 )];
                bool mixed = false;
                for( uint32_t e = 0; e < 4096u; ++e )
                    mixed = mixed || sc.atlas[vrc_slot_base( lay, i, 0, 0 ) + e] != v0;
                sc.info[i] = (uint32_t)v0 | VRC_SLOT_KNOWN | ( mixed ? VRC_SLOT_MIXED : 0u );
            }
    vrc_build_tables( sc.geom, nodes.data(), n, sc.t );
}

static void make_tables( float alpha, bool coloured, float alphaCorrection, std::vector< vrc_f4 >& lut, std::vector< vrc_f2 >& lut2 )
{
    float tf[256 * 4];
    for( int i = 0; i < 256; ++i )
    {
        const float v = (float)i / 255.0f;
        tf[i * 4 + 0] = v;
        tf[i * 4 + 1] = coloured ? 1.0f - v : v;
        tf[i * 4 + 2] = coloured ? 0.5f * v : v;
        tf[i * 4 + 3] = alpha * v;
    }
    vrc_lut_params lp;
    lp.rangeMin = 0.0f;
    lp.rangeMax = 255.0f;
    lp.alphaCorrection = alphaCorrection;
    lp.fracBits = 8;
    lut.resize( VRC_LUT_ENTRIES );
    lut2.resize( VRC_LUT_ENTRIES );
    for( uint32_t d = 0; d < 256u; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    lut[256] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    for( uint32_t d = 0; d < VRC_LUT_ENTRIES; ++d )
        lut2[d] = vrc_f2{ lut[d].x, lut[d].w };
}

/* a ray's own column of every plane: P words per plane, the ray at word AT; every other word holds GUARD */
static const uint32_t P = 7u, AT = 3u, GUARD = 0xA5A5A5A5u;

static bool one_ray( const scene& sc, rng& g, int kind, uint32_t variant, uint64_t* tally )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = variant;
    f.stepSize = ( g.next() & 1u ) ? 1.0f / 64.0f : (float)( 1.0 / 75.0 ); /* the counted uniform march, and its float chain */
    f.width = f.height = 1u;
    f.nodeCount = (uint32_t)sc.t.nodes.size();
    f.sbx = f.sby = 2u;
    f.samplesPerPixel = 1u;
    for( int a = 0; a < 3; ++a )
    {
        f.aabbMin[a] = sc.boxMin[a];
        f.aabbMax[a] = sc.boxMax[a];
        f.slotDim[a] = 16u;
        f.gridMin[a] = sc.t.g.gridMin[a];
        f.cellSize[a] = sc.t.g.cellSize[a];
        f.invCellSize[a] = sc.t.g.invCellSize[a];
        f.gridDim[a] = sc.t.g.gridDim[a];
    }
    f.slotInfo = sc.info.data();

    /* the ray */
    float origin[3], target[3];
    const uint32_t ax = g.below( 3 ), a1 = ( ax + 1u ) % 3u, a2 = ( ax + 2u ) % 3u;
    for( int a = 0; a < 3; ++a )
    {
        origin[a] = g.in( -0.3f, 0.3f );
        target[a] = g.in( sc.boxMin[a], sc.boxMax[a] );
    }
    origin[ax] = ( g.next() & 1u ) ? 1.5f : -1.5f;
    const auto facePlane = [&]( uint32_t a ) { return -0.5f + sc.cell * (float)g.below( (uint32_t)sc.dims[a] + 1u ); };
    if( kind == KIND_AXIS_FACE || kind == KIND_AXIS_EDGE )
    {
        origin[a1] = target[a1] = facePlane( a1 );
        origin[a2] = target[a2] = kind == KIND_AXIS_EDGE ? facePlane( a2 ) : target[a2];
    }
    else if( kind == KIND_AXIS_CORNER )
    {
        for( uint32_t a = 0; a < 3u; ++a )
            target[a] = facePlane( a );
        if( g.next() & 1u )
            origin[a1] = target[a1]; /* in a face plane, through the corner */
    }
    else if( kind == KIND_EYE_INSIDE )
        for( int a = 0; a < 3; ++a )
            origin[a] = g.in( sc.boxMin[a], sc.boxMax[a] );
    vrc_ray r;
    std::memset( &r, 0, sizeof( r ) );
    r.origin.x = f.eye[0] = origin[0];
    r.origin.y = f.eye[1] = origin[1];
    r.origin.z = f.eye[2] = origin[2];
    {
        /* as vrc_setup_ray_at: normalised, zero components replaced, reciprocal by division */
        const vrc_f3 d0 = { target[0] - origin[0], target[1] - origin[1], target[2] - origin[2] };
        r.dir = vrc_normalize( d0 );
        if( !( r.dir.x == r.dir.x ) ) /* the eye on the target */
            r.dir = vrc_f3{ 0.0f, 0.0f, -1.0f };
        if( r.dir.x == 0.0f ) r.dir.x = VRC_EPSILON;
        if( r.dir.y == 0.0f ) r.dir.y = VRC_EPSILON;
        if( r.dir.z == 0.0f ) r.dir.z = VRC_EPSILON;
        r.invDir.x = 1.0f / r.dir.x;
        r.invDir.y = 1.0f / r.dir.y;
        r.invDir.z = 1.0f / r.dir.z;
    }
    const vrc_f3 gmin = { f.aabbMin[0], f.aabbMin[1], f.aabbMin[2] };
    const vrc_f3 gmax = { f.aabbMax[0], f.aabbMax[1], f.aabbMax[2] };
    r.hit = vrc_intersect_box( r.origin, r.invDir, gmin, gmax, &r.tNearGlobal, &r.tFarGlobal );
    r.tNearPlane = g.in( 0.05f, 0.2f );
    if( kind == KIND_NEAR_INSIDE && r.hit )
        r.tNearPlane = r.tNearGlobal + ( r.tFarGlobal - r.tNearGlobal ) * g.in( 0.05f, 0.9f );
    if( kind == KIND_CLIPPED && r.hit )
    {
        /* what vrc_setup_ray_at's clip planes do to the cudaRaycaster ray: its global interval shrinks; the GLSL twin
         * clips every brick's interval by the planes themselves */
        const float len = r.tFarGlobal - r.tNearGlobal;
        if( variant == VRC_VARIANT_CUDA )
        {
            r.tNearGlobal += len * g.in( 0.0f, 0.4f );
            r.tFarGlobal -= len * g.in( 0.0f, 0.4f );
        }
        else
        {
            f.nPlanes = 1u + g.below( 2 );
            for( uint32_t i = 0; i < f.nPlanes; ++i )
            {
                f.planes[i][0] = g.in( -1.f, 1.f );
                f.planes[i][1] = g.in( -1.f, 1.f );
                f.planes[i][2] = g.in( -1.f, 1.f );
                f.planes[i][3] = g.in( 0.0f, 0.5f );
            }
        }
    }

    /* the ray cache, loaded */
    std::vector< uint32_t > rayPlanes( VRC_RAY_CACHE_PLANES * P, GUARD );
    {
        const float c[10] = { r.dir.x, r.dir.y, r.dir.z, r.invDir.x, r.invDir.y, r.invDir.z, r.tNearGlobal, r.tFarGlobal,
                              r.tNearPlane, vrc_bits_float( r.hit ? 1u : 0u ) };
        for( uint32_t k = 0; k < 10u; ++k )
            rayPlanes[k * P + AT] = vrc_float_bits( c[k] );
    }
    f.rayCache = reinterpret_cast< float* >( rayPlanes.data() );
    f.rayCachePlane = P;
    f.rayMode = VRC_RAY_LOAD;

    const vrc_dev_node* const nodes = sc.t.nodes.data();
    const int32_t* const grid = sc.t.grid.data();
    const vrc_classifier cls = {};
    g_nodes = &sc.t.nodes;
    bool bad = false;

    /* the list the walk makes under a table that ends no ray */
    std::vector< vrc_f4 > lut;
    std::vector< vrc_f2 > lut2;
    make_tables( 0.0f, false, 1.0f, lut, lut2 );
    f.clearFirst = 1u;
    vrc_f4 px = { 0.f, 0.f, 0.f, 0.f };
    uint32_t ns = 0;
    g_seen.clear();
    vrc_pixel_grid_dda< false, true, true, VRC_MODE_TABLE, uint8_t >( f, nodes, grid, sc.atlas.data(), lut.data(), cls, &px, 0u, 0u, ns, AT );
    const std::vector< visit > want = g_seen;
    for( const visit& v : want )
        bad = bad || v.node >= f.nodeCount;

    /* count pass, record pass (once) */
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    const uint32_t counted = vrc_pixel_walk_record( f, nodes, grid, AT );
    bad = bad || counted != want.size();
    const uint32_t K = counted > 0u ? counted : 1u;
    std::vector< uint32_t > planes( ( 1u + 4u * K ) * P, GUARD );
    f.walkCache = planes.data();
    f.walkK = K;
    planes[AT] = vrc_pixel_walk_record( f, nodes, grid, AT );
    bad = bad || planes[AT] != counted;
    for( size_t w = 0; w < planes.size(); ++w )
    {
        const size_t plane = w / P;
        uint32_t expect = GUARD;
        if( w % P == AT && plane >= 1u && ( plane - 1u ) / 4u < want.size() )
        {
            const visit& v = want[( plane - 1u ) / 4u];
            const uint32_t c[4] = { v.node, v.dist, v.tNear, v.tFar };
            expect = c[( plane - 1u ) % 4u];
        }
        if( w != AT )
            bad = bad || planes[w] != expect;
    }
    if( counted > 1u )
    {
        /* planes one visit short: the pass still counts every visit and writes nothing beyond the planes it was given */
        std::vector< uint32_t > shortPlanes( ( 1u + 4u * ( counted - 1u ) ) * P + P, GUARD );
        vrc_frame fs = f;
        fs.walkCache = shortPlanes.data();
        fs.walkK = counted - 1u;
        bad = bad || vrc_pixel_walk_record( fs, nodes, grid, AT ) != counted;
        for( uint32_t w = 0; w < P; ++w )
            bad = bad || shortPlanes[shortPlanes.size() - P + w] != GUARD;
        bad = bad || shortPlanes[( 1u + 4u * ( counted - 2u ) ) * P + AT] != want[counted - 2u].node;
    }

    /* walk against replay, from the one list */
    bool endedEarly = false;
    for( int tab = 0; tab < 6 && !bad; ++tab )
    {
        const float alpha = ( tab & 1 ) ? 1.0f : 0.05f;
        const bool coloured = tab >= 2, onto = tab >= 4;
        make_tables( alpha, coloured, 4.0f, lut, lut2 );
        f.clearFirst = onto ? 0u : 1u;
        const vrc_f4 start = onto ? vrc_f4{ 0.125f, 0.25f, 0.0625f, ( tab & 1 ) ? 0.9995f : 0.5f } : vrc_f4{ 9.f, 9.f, 9.f, 9.f };
        vrc_f4 a = start, b = start;
        uint32_t na = 0, nb = 0;
        g_seen.clear();
        vrc_frame fw = f; /* the walking frame knows nothing of the lists */
        fw.walkCache = nullptr;
        fw.walkPlane = fw.walkK = 0u;
        if( coloured )
        {
            vrc_pixel_grid_dda< false, true, true, VRC_MODE_TABLE, uint8_t, VRC_GROUP >( fw, nodes, grid, sc.atlas.data(), lut.data(), cls, &a, 0u, 0u, na, AT );
            vrc_pixel_walk_replay< true, VRC_MODE_TABLE, VRC_GROUP >( f, nodes, sc.atlas.data(), lut.data(), cls, &b, 0u, 0u, nb, AT );
        }
        else
        {
            const vrc_f4* const t2 = reinterpret_cast< const vrc_f4* >( lut2.data() );
            vrc_pixel_grid_dda< false, true, true, VRC_MODE_GREY, uint8_t, 14 >( fw, nodes, grid, sc.atlas.data(), t2, cls, &a, 0u, 0u, na, AT );
            vrc_pixel_walk_replay< true, VRC_MODE_GREY, 14 >( f, nodes, sc.atlas.data(), t2, cls, &b, 0u, 0u, nb, AT );
        }
        bad = bad || std::memcmp( &a, &b, sizeof( a ) ) != 0 || na != nb;
        /* the walk's visits under this table: a prefix of the list */
        bad = bad || g_seen.size() > want.size();
        for( size_t k = 0; k < g_seen.size() && !bad; ++k )
            bad = std::memcmp( &g_seen[k], &want[k], sizeof( visit ) ) != 0;
        endedEarly = endedEarly || ( !onto && g_seen.size() < want.size() );
    }

    ++tally[kind * TALLY + 0];
    tally[kind * TALLY + 1] += want.empty() ? 0u : 1u;
    tally[kind * TALLY + 2] += want.size();
    tally[kind * TALLY + 3] += endedEarly ? 1u : 0u;
    for( const visit& v : want )
        tally[kind * TALLY + 4] += ( v.node < sc.info.size() && !( sc.info[v.node] & VRC_SLOT_MIXED ) ) ? 1u : 0u;
    tally[kind * TALLY + 5] += bad ? 1u : 0u;
    return !bad;
}

/* `count` rays per (grid, variant, kind): 3 x 2 x KINDS combinations.  out: KINDS x TALLY.  Returns the mismatches. */
extern "C" uint64_t walk_cache_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * KINDS * TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int s = 0; s < 3; ++s )
    {
        scene sc;
        build_scene( sc, grids[s][0], grids[s][1], grids[s][2] );
        if( !sc.t.gridOk || sc.t.clamp )
            return ~0ull;
        for( uint32_t variant = 0; variant < 2u; ++variant )
            for( int kind = 0; kind < KINDS; ++kind )
                for( uint32_t i = 0; i < count; ++i )
                    (void)one_ray( sc, g, kind, variant, out );
    }
    uint64_t bad = 0;
    for( int kind = 0; kind < KINDS; ++kind )
        bad += out[kind * TALLY + 5];
    return bad;
}

extern "C" int walk_cache_kinds() { return KINDS; }

#if defined( WALK_CACHE_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 20u;
    uint64_t out[KINDS * TALLY];
    const uint64_t bad = walk_cache_run( 12345u, count, out );
    uint64_t cases = 0;
    for( int kind = 0; kind < KINDS; ++kind )
    {
        std::printf( "kind %d: cases %llu lists %llu visits %llu early %llu uniform %llu mismatches %llu\n", kind,
                     (unsigned long long)out[kind * TALLY], (unsigned long long)out[kind * TALLY + 1],
                     (unsigned long long)out[kind * TALLY + 2], (unsigned long long)out[kind * TALLY + 3],
                     (unsigned long long)out[kind * TALLY + 4], (unsigned long long)out[kind * TALLY + 5] );
        cases += out[kind * TALLY];
    }
    std::printf( "cases %llu mismatches %llu\n", (unsigned long long)cases, (unsigned long long)bad );
    return bad == 0 ? 0 : 1;
}
#endif
