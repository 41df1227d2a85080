/*
 * walk_lean_harness.cpp -- the lean form of the walk cache's lists (vrc_core.h: vrc_frame::walkLean) on the host build
 * of the per-ray code, for tests/test_walk_lean_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * The scenes, tables and random numbers are those of walk_cache_harness.cpp (included: the same grids of 1x1x1, 4x4x4
 * and 4x3x2 bricks, every third brick uniform), and so are the kinds of rays.  For every ray, with a step of 1/64 or
 * 1/128 (lean-able) or 1/75 (not):
 *   - the list is recorded in both forms.  Count, node, tNear and tFar are the same words; the second plane of the lean
 *     form unpacks to the node's own slotInfoIndex and to an n that equals the trips of
 *     `for( ; travel > 0; travel -= stepSize )` over the dist the other form recorded; the count pass asked with
 *     walkLean says "every visit packs" for the lean-able steps and "not" for 1/75 (where a visit has travel at all);
 *   - under six table set-ups (alpha 0.05 and 1.0, grey and coloured, the coloured ones also onto a pixel that is not
 *     cleared) vrc_pixel_walk_replay_lean from the lean list leaves the pixel bits and the sample count that
 *     vrc_pixel_walk_replay leaves from the other list.
 * Once per run, not per ray:
 *   - vrc_march_uniform_lean against vrc_march_segment_as<..., UNIFORM> for n = 0 .. 70 (no group, one and two groups
 *     of 32, every remainder) and 4095, entries from
 *     transparent to opaque and starting alphas on both sides of the early-exit threshold, in two and in four floats:
 *     the same colour bits, the same count, the same return value;
 *   - the limits of vrc_walk_lean_word: 4095 / 4096 steps, index 2^20 - 1 / 2^20, a step that is no power of two, a
 *     segment without travel.
 * Built as a shared library (walk_lean_run) and, with -DWALK_LEAN_MAIN, as a stand-alone program for the sanitizers.
 */
#include "walk_cache_harness.cpp"

/* [0] rays, [1] rays with a list, [2] visits checked word for word, [3] visits of uniform bricks, [4] rays the count
 * pass found not lean-able (step 1/75), [5] uniform marches compared, [6] mismatches */
#define LEAN_TALLY 7

static uint32_t float_chain_trips( float travel, float stepSize )
{
    uint32_t n = 0u;
    for( ; travel > 0.0f; travel -= stepSize )
        ++n;
    return n;
}

/* the ray kinds of walk_cache_harness.cpp's one_ray, written into f (eye, clip planes) and the loaded ray cache */
static void lean_make_ray( const scene& sc, rng& g, int kind, vrc_frame& f, std::vector< uint32_t >& rayPlanes )
{
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
            origin[a1] = target[a1];
    }
    else if( kind == KIND_EYE_INSIDE )
        for( int a = 0; a < 3; ++a )
            origin[a] = g.in( sc.boxMin[a], sc.boxMax[a] );
    vrc_ray r;
    std::memset( &r, 0, sizeof( r ) );
    r.origin.x = f.eye[0] = origin[0];
    r.origin.y = f.eye[1] = origin[1];
    r.origin.z = f.eye[2] = origin[2];
    const vrc_f3 d0 = { target[0] - origin[0], target[1] - origin[1], target[2] - origin[2] };
    r.dir = vrc_normalize( d0 );
    if( !( r.dir.x == r.dir.x ) )
        r.dir = vrc_f3{ 0.0f, 0.0f, -1.0f };
    if( r.dir.x == 0.0f ) r.dir.x = VRC_EPSILON;
    if( r.dir.y == 0.0f ) r.dir.y = VRC_EPSILON;
    if( r.dir.z == 0.0f ) r.dir.z = VRC_EPSILON;
    r.invDir.x = 1.0f / r.dir.x;
    r.invDir.y = 1.0f / r.dir.y;
    r.invDir.z = 1.0f / r.dir.z;
    const vrc_f3 gmin = { f.aabbMin[0], f.aabbMin[1], f.aabbMin[2] };
    const vrc_f3 gmax = { f.aabbMax[0], f.aabbMax[1], f.aabbMax[2] };
    r.hit = vrc_intersect_box( r.origin, r.invDir, gmin, gmax, &r.tNearGlobal, &r.tFarGlobal );
    r.tNearPlane = g.in( 0.05f, 0.2f );
    if( kind == KIND_NEAR_INSIDE && r.hit )
        r.tNearPlane = r.tNearGlobal + ( r.tFarGlobal - r.tNearGlobal ) * g.in( 0.05f, 0.9f );
    if( kind == KIND_CLIPPED && r.hit )
    {
        const float len = r.tFarGlobal - r.tNearGlobal;
        if( f.variant == VRC_VARIANT_CUDA )
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
    rayPlanes.assign( VRC_RAY_CACHE_PLANES * P, GUARD );
    const float c[10] = { r.dir.x, r.dir.y, r.dir.z, r.invDir.x, r.invDir.y, r.invDir.z, r.tNearGlobal, r.tFarGlobal,
                          r.tNearPlane, vrc_bits_float( r.hit ? 1u : 0u ) };
    for( uint32_t k = 0; k < 10u; ++k )
        rayPlanes[k * P + AT] = vrc_float_bits( c[k] );
    f.rayCache = reinterpret_cast< float* >( rayPlanes.data() );
    f.rayCachePlane = P;
    f.rayMode = VRC_RAY_LOAD;
}

static bool lean_one_ray( const scene& sc, rng& g, int kind, uint32_t variant, uint64_t* tally )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = variant;
    const uint32_t pick = g.below( 3 );
    f.stepSize = pick == 0u ? 1.0f / 64.0f : ( pick == 1u ? 1.0f / 128.0f : (float)( 1.0 / 75.0 ) );
    const bool pow2 = pick != 2u;
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
    f.clearFirst = 1u;
    std::vector< uint32_t > rayPlanes;
    lean_make_ray( sc, g, kind, f, rayPlanes );

    const vrc_dev_node* const nodes = sc.t.nodes.data();
    const int32_t* const grid = sc.t.grid.data();
    const vrc_classifier cls = {};
    bool bad = false;

    /* count pass: as it is today, and asked whether every visit packs */
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    uint32_t gathers = 0u, notLean = 7u;
    const uint32_t counted = vrc_pixel_walk_record( f, nodes, grid, AT, &gathers, &notLean );
    bad = bad || notLean != 0u; /* (not asked) */
    vrc_frame fl = f;
    fl.walkLean = 1u;
    fl.walkSlots = (uint32_t)sc.info.size();
    uint32_t gathersLean = 0u;
    bad = bad || vrc_pixel_walk_record( fl, nodes, grid, AT, &gathersLean, &notLean ) != counted || gathersLean != gathers;

    /* the two records */
    const uint32_t K = counted > 0u ? counted : 1u;
    std::vector< uint32_t > plain( ( 1u + 4u * K ) * P, GUARD ), lean( ( 1u + 4u * K ) * P, GUARD );
    f.walkCache = plain.data();
    fl.walkCache = lean.data();
    f.walkK = fl.walkK = K;
    plain[AT] = vrc_pixel_walk_record( f, nodes, grid, AT );
    lean[AT] = vrc_pixel_walk_record( fl, nodes, grid, AT );
    bad = bad || plain[AT] != counted || lean[AT] != counted;
    bool travels = false;
    for( size_t w = 0; w < plain.size(); ++w )
    {
        const size_t plane = w / P;
        const bool second = w % P == AT && plane >= 1u && ( plane - 1u ) % 4u == 1u && ( plane - 1u ) / 4u < counted;
        if( !second )
        {
            bad = bad || plain[w] != lean[w]; /* count, node, tNear, tFar and every guard word */
            continue;
        }
        const uint32_t node = plain[w - P];
        const float dist = vrc_bits_float( plain[w] );
        travels = travels || dist > 0.0f;
        bad = bad || node >= f.nodeCount;
        if( pow2 && !bad )
        {
            bad = bad || ( lean[w] & 0xFFFFFu ) != nodes[node].slotInfoIndex;
            bad = bad || ( lean[w] >> 20 ) != float_chain_trips( dist, f.stepSize );
            ++tally[2];
            tally[3] += ( sc.info[node] & VRC_SLOT_MIXED ) ? 0u : 1u;
        }
    }
    bad = bad || notLean != ( ( !pow2 && travels ) ? 1u : 0u );
    tally[4] += notLean;

    /* replay against replay, each from its own list */
    std::vector< vrc_f4 > lut;
    std::vector< vrc_f2 > lut2;
    for( int tab = 0; tab < 6 && pow2 && !bad; ++tab )
    {
        const float alpha = ( tab & 1 ) ? 1.0f : 0.05f;
        const bool coloured = tab >= 2, onto = tab >= 4;
        make_tables( alpha, coloured, 4.0f, lut, lut2 );
        f.clearFirst = fl.clearFirst = onto ? 0u : 1u;
        const vrc_f4 start = onto ? vrc_f4{ 0.125f, 0.25f, 0.0625f, ( tab & 1 ) ? 0.9995f : 0.5f } : vrc_f4{ 9.f, 9.f, 9.f, 9.f };
        vrc_f4 a = start, b = start;
        uint32_t na = 0, nb = 0;
        if( coloured )
        {
            vrc_pixel_walk_replay< true, VRC_MODE_TABLE, VRC_GROUP >( f, nodes, sc.atlas.data(), lut.data(), cls, &a, 0u, 0u, na, AT );
            vrc_pixel_walk_replay_lean< true, VRC_MODE_TABLE, VRC_GROUP >( fl, nodes, sc.atlas.data(), lut.data(), cls, &b, 0u, 0u, nb, AT );
        }
        else
        {
            const vrc_f4* const t2 = reinterpret_cast< const vrc_f4* >( lut2.data() );
            vrc_pixel_walk_replay< true, VRC_MODE_GREY, 14 >( f, nodes, sc.atlas.data(), t2, cls, &a, 0u, 0u, na, AT );
            vrc_pixel_walk_replay_lean< true, VRC_MODE_GREY, 14 >( fl, nodes, sc.atlas.data(), t2, cls, &b, 0u, 0u, nb, AT );
        }
        bad = bad || std::memcmp( &a, &b, sizeof( a ) ) != 0 || na != nb;
    }

    ++tally[0];
    tally[1] += counted > 0u ? 1u : 0u;
    tally[6] += bad ? 1u : 0u;
    return !bad;
}

/* vrc_march_uniform_lean against the uniform form of the segment march, n samples of entry `ue` from colour `start` */
template < typename E >
static bool lean_march_equals( const scene& sc, uint32_t n, const E ue, const E start )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.stepSize = 1.0f / 64.0f;
    for( int a = 0; a < 3; ++a )
        f.slotDim[a] = 16u;
    f.sbx = f.sby = 2u;
    const vrc_f3 zero = { 0.0f, 0.0f, 0.0f };
    const vrc_segment s = { zero, zero, (float)n * f.stepSize, 0.0f }; /* (exact: n < 2^24, a power-of-two step) */
    uint32_t nn = 0u;
    if( n > 0u && ( !vrc_exact_step_count( s.dist, f.stepSize, &nn ) || nn != n ) )
        return false;
    E a = start, b = start;
    uint32_t na = 0u, nb = 0u;
    const bool da = vrc_march_segment_as< false, true, true, uint8_t, 14, E, false, true >(
        f, sc.t.nodes[0], s, sc.atlas.data(), (const E*)nullptr, a, na, 0.0f, nullptr, ue );
    const bool db = vrc_march_uniform_lean< true, E >( b, ue, n, nb );
    /* and without the counter: the same colour */
    E c = start;
    uint32_t nc = 0u;
    const bool dc = vrc_march_uniform_lean< false, E >( c, ue, n, nc );
    return da == db && db == dc && na == nb && nc == 0u && std::memcmp( &a, &b, sizeof( E ) ) == 0 &&
           std::memcmp( &a, &c, sizeof( E ) ) == 0;
}

static uint64_t lean_marches( const scene& sc, uint64_t* tally )
{
    static const float alphas[] = { 0.0f, 1e-4f, 0.004f, 0.05f, 0.3f, 0.75f, 0.9991f, 1.0f };
    static const float starts[] = { 0.0f, 0.5f, 0.99f, 0.9989f, 0.999f, 0.9991f }; /* (0.9991: a pixel composited onto) */
    uint64_t bad = 0;
    for( uint32_t n = 0u; n <= 71u; ++n )
        for( float ea : alphas )
            for( float sa : starts )
            {
                const uint32_t steps = n == 71u ? 4095u : n;
                const vrc_f2 e2 = { 0.6f * ea, ea }, s2 = { 0.25f * sa, sa };
                const vrc_f4 e4 = { 0.6f * ea, 0.3f * ea, ea, ea }, s4 = { 0.25f * sa, 0.5f * sa, 0.125f * sa, sa };
                bad += lean_march_equals< vrc_f2 >( sc, steps, e2, s2 ) ? 0u : 1u;
                bad += lean_march_equals< vrc_f4 >( sc, steps, e4, s4 ) ? 0u : 1u;
                tally[5] += 2u;
            }
    return bad;
}

static uint64_t lean_limits()
{
    const float step = 1.0f / 1024.0f;
    uint64_t bad = 0;
    uint32_t w = 0u;
    bad += vrc_walk_lean_word( 4095.0f * step, step, 5u, &w ) && w == ( ( 4095u << 20 ) | 5u ) ? 0u : 1u;
    bad += vrc_walk_lean_word( 4094.5f * step, step, 5u, &w ) && w == ( ( 4095u << 20 ) | 5u ) ? 0u : 1u; /* rounds up */
    bad += !vrc_walk_lean_word( 4096.0f * step, step, 5u, &w ) ? 0u : 1u;
    bad += !vrc_walk_lean_word( 4095.5f * step, step, 5u, &w ) ? 0u : 1u;
    bad += vrc_walk_lean_word( step, step, ( 1u << 20 ) - 1u, &w ) && w == ( ( 1u << 20 ) | 0xFFFFFu ) ? 0u : 1u;
    bad += !vrc_walk_lean_word( step, step, 1u << 20, &w ) ? 0u : 1u;
    bad += vrc_walk_lean_word( step, step, 0u, &w ) && w == ( 1u << 20 ) ? 0u : 1u; /* a node without a slot word */
    /* no travel: no samples, whatever the step */
    bad += vrc_walk_lean_word( 0.0f, step, 9u, &w ) && w == 9u ? 0u : 1u;
    bad += vrc_walk_lean_word( -1.0f, 1.0f / 75.0f, 9u, &w ) && w == 9u ? 0u : 1u;
    bad += vrc_walk_lean_word( std::nanf( "" ), step, 9u, &w ) && w == 9u ? 0u : 1u; /* (!(dist > 0): the march returns) */
    /* a step the exact count refuses */
    bad += !vrc_walk_lean_word( 0.5f, 1.0f / 75.0f, 9u, &w ) ? 0u : 1u;
    bad += !vrc_walk_lean_word( 0.5f, -step, 9u, &w ) ? 0u : 1u;
    return bad;
}

/* `count` rays per (grid, variant, kind).  out: LEAN_TALLY numbers.  Returns the mismatches. */
extern "C" uint64_t walk_lean_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * LEAN_TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int s = 0; s < 3; ++s )
    {
        scene sc;
        build_scene( sc, grids[s][0], grids[s][1], grids[s][2] );
        if( !sc.t.gridOk || sc.t.clamp )
            return ~0ull;
        g_nodes = &sc.t.nodes; /* (the included harness's visit hook; the walk is not run here) */
        for( uint32_t variant = 0; variant < 2u; ++variant )
            for( int kind = 0; kind < KINDS; ++kind )
                for( uint32_t i = 0; i < count; ++i )
                    (void)lean_one_ray( sc, g, kind, variant, out );
        if( s == 1 )
            out[6] += lean_marches( sc, out );
    }
    out[6] += lean_limits();
    return out[6];
}

#if defined( WALK_LEAN_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 20u;
    uint64_t out[LEAN_TALLY];
    const uint64_t bad = walk_lean_run( 12345u, count, out );
    std::printf( "rays %llu lists %llu visits %llu uniform %llu notlean %llu marches %llu mismatches %llu\n",
                 (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                 (unsigned long long)out[3], (unsigned long long)out[4], (unsigned long long)out[5],
                 (unsigned long long)bad );
    return bad == 0 ? 0 : 1;
}
#endif
