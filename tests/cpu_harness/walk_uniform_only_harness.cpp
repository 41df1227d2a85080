/*
 * walk_uniform_only_harness.cpp -- the uniform-only form of the lean replay (vrc_core.h: vrc_pixel_walk_replay_lean<
 * ..., true >) on the host build of the per-ray code, for tests/test_walk_uniform_only_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * The grids, tables, random numbers and kinds of rays are those of walk_lean_harness.cpp (included), on scenes whose
 * every brick is made uniform: the voxels of a brick all hold its first value and its slot word says so.  For every ray,
 * with a step of 1/64 or 1/128:
 *   - the count pass reports no visit that gathers (what the host asks before it takes the form);
 *   - under the six table set-ups of the lean harness (alpha 0.05 and 1.0, grey and coloured, the coloured ones also
 *     onto a pixel that is not cleared) the uniform-only function leaves the pixel bits and the sample count of
 *     vrc_pixel_walk_replay_lean from the same list.  It is handed no node table and no atlas: it may read neither;
 *   - the same from planes that hold one visit per ray where the ray has more (the clamp by walkK);
 *   - a mixed word planted on visit j of the list (and, in turn, a word about which nothing is known) ends the list
 *     there: the pixel and the count are those of the lean replay of the first j visits.  slotInfo is an allocation of
 *     exactly walkSlots words, so under the address sanitizer a read past it is a failure;
 *   - a list word whose slot index lies past slotInfo (2^20 - 1) is clamped as the lean form clamps it: the same pixel.
 * Built as a shared library (walk_uniform_only_run) and, with -DWALK_UNIFORM_ONLY_MAIN, as a stand-alone program for
 * the sanitizers.
 */
#include "walk_lean_harness.cpp"

/* [0] rays, [1] lists of no visit, [2] of one visit, [3] of more, [4] replays compared, [5] planted words that ended a
 * list, [6] mismatches */
#define UNIFORM_ONLY_TALLY 7

static void make_every_brick_uniform( scene& sc )
{
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        lay.slots[a] = sc.geom.slots[a];
        lay.slotDim[a] = 16u;
    }
    for( uint32_t i = 0; i < (uint32_t)sc.info.size(); ++i )
    {
        const size_t base = vrc_slot_base( lay, i, 0, 0 );
        const uint8_t v0 = sc.atlas[base];
        for( uint32_t e = 0; e < 4096u; ++e )
            sc.atlas[base + e] = v0;
        sc.info[i] = (uint32_t)v0 | VRC_SLOT_KNOWN;
    }
}

struct replay_result
{
    vrc_f4 pixel;
    uint32_t samples;
};

/* one replay of the list in fl's planes under table set-up `tab` (those of lean_one_ray) */
template < bool UNIFORM_ONLY >
static replay_result uo_replay( vrc_frame fl, const scene& sc, int tab )
{
    std::vector< vrc_f4 > lut;
    std::vector< vrc_f2 > lut2;
    const float alpha = ( tab & 1 ) ? 1.0f : 0.05f;
    const bool coloured = tab >= 2, onto = tab >= 4;
    make_tables( alpha, coloured, 4.0f, lut, lut2 );
    fl.clearFirst = onto ? 0u : 1u;
    fl.walkLean = UNIFORM_ONLY ? VRC_WALK_LEAN_UNIFORM : 1u;
    const vrc_classifier cls = {};
    /* (the uniform-only form has nothing to read a node or a voxel for) */
    const vrc_dev_node* const nodes = UNIFORM_ONLY ? nullptr : sc.t.nodes.data();
    const uint8_t* const atlas = UNIFORM_ONLY ? nullptr : sc.atlas.data();
    replay_result r = { onto ? vrc_f4{ 0.125f, 0.25f, 0.0625f, ( tab & 1 ) ? 0.9995f : 0.5f } : vrc_f4{ 9.f, 9.f, 9.f, 9.f }, 0u };
    if( coloured )
        vrc_pixel_walk_replay_lean< true, VRC_MODE_TABLE, VRC_GROUP, UNIFORM_ONLY >( fl, nodes, atlas, lut.data(), cls, &r.pixel,
                                                                                     0u, 0u, r.samples, AT );
    else
        vrc_pixel_walk_replay_lean< true, VRC_MODE_GREY, 14, UNIFORM_ONLY >(
            fl, nodes, atlas, reinterpret_cast< const vrc_f4* >( lut2.data() ), cls, &r.pixel, 0u, 0u, r.samples, AT );
    return r;
}

static bool uo_same( const replay_result& a, const replay_result& b )
{
    return std::memcmp( &a.pixel, &b.pixel, sizeof( a.pixel ) ) == 0 && a.samples == b.samples;
}

static bool uo_one_ray( const scene& sc, rng& g, int kind, uint32_t variant, uint64_t* tally )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = variant;
    f.stepSize = ( g.next() & 1u ) ? 1.0f / 64.0f : 1.0f / 128.0f;
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
    /* slotInfo: a copy in an allocation of its own, exactly walkSlots words */
    std::vector< uint32_t > info( sc.info );
    f.slotInfo = info.data();
    f.clearFirst = 1u;
    f.walkLean = 1u;
    f.walkSlots = (uint32_t)info.size();
    std::vector< uint32_t > rayPlanes;
    lean_make_ray( sc, g, kind, f, rayPlanes );

    const vrc_dev_node* const nodes = sc.t.nodes.data();
    const int32_t* const grid = sc.t.grid.data();
    bool bad = false;

    /* count pass: every visit packs, none gathers */
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    uint32_t gathers = 7u, notLean = 7u;
    const uint32_t counted = vrc_pixel_walk_record( f, nodes, grid, AT, &gathers, &notLean );
    bad = bad || gathers != 0u || notLean != 0u;

    /* the lists: all `counted` visits, and planes of one visit */
    const uint32_t K = counted > 0u ? counted : 1u;
    std::vector< uint32_t > full( ( 1u + 4u * K ) * P, GUARD ), one( ( 1u + 4u * 1u ) * P, GUARD );
    vrc_frame ff = f, f1 = f;
    ff.walkCache = full.data();
    ff.walkK = K;
    f1.walkCache = one.data();
    f1.walkK = 1u;
    full[AT] = vrc_pixel_walk_record( ff, nodes, grid, AT );
    one[AT] = vrc_pixel_walk_record( f1, nodes, grid, AT );
    bad = bad || full[AT] != counted || one[AT] != counted;
    tally[counted == 0u ? 1 : ( counted == 1u ? 2 : 3 )] += 1u;

    const uint32_t j = counted > 0u ? g.below( counted ) : 0u; /* the visit a word is planted on */
    const uint32_t far = g.next() & 1u;
    for( int tab = 0; tab < 6 && !bad; ++tab )
    {
        bad = bad || !uo_same( uo_replay< true >( ff, sc, tab ), uo_replay< false >( ff, sc, tab ) );
        bad = bad || !uo_same( uo_replay< true >( f1, sc, tab ), uo_replay< false >( f1, sc, tab ) );
        tally[4] += 2u;
        if( counted == 0u )
            continue;
        /* a word that does not hold one value on visit j: the list ends there */
        const size_t at = (size_t)AT + ( 2u + 4u * (size_t)j ) * P;
        const uint32_t idx = full[at] & 0xFFFFFu;
        bad = bad || idx == 0u || idx > info.size();
        if( bad )
            break;
        const uint32_t kept = info[idx - 1u];
        std::vector< uint32_t > cut( full );
        cut[AT] = j;
        const replay_result want = uo_replay< false >( [&] { vrc_frame c = ff; c.walkCache = cut.data(); return c; }(), sc, tab );
        info[idx - 1u] = ( tab & 1 ) ? 0u : ( kept | VRC_SLOT_MIXED );
        bad = bad || !uo_same( uo_replay< true >( ff, sc, tab ), want );
        info[idx - 1u] = kept;
        tally[5] += 1u;
        /* an index past slotInfo: clamped to its last word, as the lean form clamps it */
        const uint32_t keptWord = full[at];
        full[at] = ( keptWord & ~0xFFFFFu ) | ( far ? 0xFFFFFu : (uint32_t)info.size() + 1u );
        bad = bad || !uo_same( uo_replay< true >( ff, sc, tab ), uo_replay< false >( ff, sc, tab ) );
        full[at] = keptWord;
        tally[4] += 1u;
    }

    ++tally[0];
    tally[6] += bad ? 1u : 0u;
    return !bad;
}

/* `count` rays per (grid, variant, kind).  out: UNIFORM_ONLY_TALLY numbers.  Returns the mismatches. */
extern "C" uint64_t walk_uniform_only_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * UNIFORM_ONLY_TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int s = 0; s < 3; ++s )
    {
        scene sc;
        build_scene( sc, grids[s][0], grids[s][1], grids[s][2] );
        if( !sc.t.gridOk || sc.t.clamp )
            return ~0ull;
        make_every_brick_uniform( sc );
        g_nodes = &sc.t.nodes; /* (the included harness's visit hook; the walk is not run here) */
        for( uint32_t variant = 0; variant < 2u; ++variant )
            for( int kind = 0; kind < KINDS; ++kind )
                for( uint32_t i = 0; i < count; ++i )
                    (void)uo_one_ray( sc, g, kind, variant, out );
    }
    return out[6];
}

#if defined( WALK_UNIFORM_ONLY_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 20u;
    uint64_t out[UNIFORM_ONLY_TALLY];
    const uint64_t bad = walk_uniform_only_run( 12345u, count, out );
    std::printf( "rays %llu none %llu one %llu more %llu replays %llu planted %llu mismatches %llu\n",
                 (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                 (unsigned long long)out[3], (unsigned long long)out[4], (unsigned long long)out[5],
                 (unsigned long long)bad );
    return bad == 0 ? 0 : 1;
}
#endif
