/*
 * walk_resolved_harness.cpp -- the resolved visit words of the uniform-only replay (vrc_core.h: vrc_walk_resolved_word,
 * vrc_pixel_walk_replay_resolved, vrc_frame::walkResolved), the decision behind VRC_OPT_WALK_RESOLVED (vrc_plan.h:
 * vrc_plan_walk_resolved) and the replay's tile decode (vrc_replay_tile_origin, vrc_replay_lane_pixel), on the host
 * build, for tests/test_walk_resolved_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * walk_resolved_words( tally ): vrc_walk_resolved_word against vrc_lean_slot_word + vrc_slot_holds_one_value restated
 * here over one word of slotInfo -- every known/mixed bit pattern x 256 values, a list word whose index is 0 (none), 1,
 * the last word and past walkSlots (just past, and 2^20 - 1), with slotInfo and without, step counts 0, 1, 151 and 4095,
 * the visit below, at and above the ray's count.  slotInfo is an allocation of exactly walkSlots words.
 *
 * walk_resolved_run( seed, count, out ): the generated rays of walk_uniform_only_harness.cpp (included).  For every ray
 * the planes of all its visits and planes of one visit are resolved (every column of them, the GUARD columns too: any
 * word is a list word), and vrc_pixel_walk_replay_lean< false, ..., true > with the resolved planes must leave the pixel
 * bytes it leaves without them -- grey and four-float tables, alpha 0.05 and 1.0, onto a pixel that is not cleared, with
 * the first-visit table and the free march on and off; and again with a word that does not hold one value planted on one
 * visit before the planes are resolved.
 *
 * Built as a shared library and, with -DWALK_RESOLVED_MAIN, as a stand-alone program for the sanitizers.
 */
#include "walk_uniform_only_harness.cpp"
#include "../../libre_amd/csrc/vrc_plan.h"

/* [0] words compared, [1] words with the bit set, [2] mismatches */
#define RESOLVED_WORDS_TALLY 3
/* [0] rays, [1] lists of no visit, [2] of one visit, [3] of more, [4] replays compared, [5] planted words, [6] mismatches */
#define RESOLVED_RUN_TALLY 7

extern "C" uint64_t walk_resolved_words( uint64_t* tally )
{
    std::memset( tally, 0, sizeof( uint64_t ) * RESOLVED_WORDS_TALLY );
    const uint32_t S = 5u, K = 3u, v = 1u;
    static const uint32_t patterns[4] = { 0u, VRC_SLOT_KNOWN, VRC_SLOT_MIXED, VRC_SLOT_KNOWN | VRC_SLOT_MIXED };
    static const uint32_t indices[5] = { 0u, 1u, S, S + 1u, 0xFFFFFu };
    static const uint32_t steps[4] = { 0u, 1u, 151u, 4095u };
    std::vector< uint32_t > info( S ), planes( ( 1u + 4u * K ) * P, GUARD );
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.walkCache = planes.data();
    f.walkPlane = P;
    f.walkK = K;
    f.walkLean = VRC_WALK_LEAN_UNIFORM;
    f.walkSlots = S;
    for( int have = 0; have < 2; ++have )
        for( uint32_t pat = 0; pat < 4u; ++pat )
            for( uint32_t value = 0; value < 256u; ++value )
                for( uint32_t ix = 0; ix < 5u; ++ix )
                    for( uint32_t st = 0; st < 4u; ++st )
                        for( uint32_t listed = 0; listed <= K; ++listed )
                        {
                            const uint32_t idx = indices[ix], n = steps[st];
                            /* the word the index reaches holds the pattern, every other word something else */
                            const uint32_t at = idx == 0u ? 0u : ( idx - 1u < S - 1u ? idx - 1u : S - 1u );
                            for( uint32_t s = 0; s < S; ++s )
                                info[s] = VRC_SLOT_KNOWN | ( ( value + 1u + s ) & 0xFFu );
                            info[at] = patterns[pat] | value;
                            f.slotInfo = have ? info.data() : nullptr;
                            const uint32_t packed = ( n << VRC_WALK_LEAN_INDEX_BITS ) | idx;
                            planes[AT] = listed;
                            planes[( 2u + 4u * v ) * P + AT] = packed;
                            const uint32_t word = vrc_lean_slot_word( f, packed, info[at] );
                            const bool one = v < listed && vrc_slot_holds_one_value( word );
                            const uint32_t want = ( n << VRC_WALK_LEAN_INDEX_BITS ) | ( one ? VRC_WALK_RESOLVED_ONE : 0u ) | ( word & 0xFFu );
                            const uint32_t got = vrc_walk_resolved_word( f, AT, v );
                            ++tally[0];
                            tally[1] += one ? 1u : 0u;
                            if( got != want || ( ( !have || idx == 0u ) && ( got & ( VRC_WALK_RESOLVED_ONE | 0xFFu ) ) != 0u ) )
                            {
                                if( tally[2]++ < 8u )
                                    std::fprintf( stderr, "walk_resolved: have %d pattern %x value %u index %u n %u listed %u: %08x, want %08x\n",
                                                  have, patterns[pat], value, idx, n, listed, got, want );
                            }
                        }
    return tally[2];
}

/* the resolved planes of the lists in fl's planes: every column, as the kernel fills them */
static std::vector< uint32_t > rs_resolve( const vrc_frame& fl )
{
    std::vector< uint32_t > out( (size_t)fl.walkK * fl.walkPlane );
    for( uint32_t ray = 0; ray < fl.walkPlane; ++ray )
        for( uint32_t v = 0; v < fl.walkK; ++v )
            out[(size_t)v * fl.walkPlane + ray] = vrc_walk_resolved_word( fl, ray, v );
    return out;
}

/* the first-visit table of table set-up `tab`, in the form the set-up marches */
template < typename E >
static const std::vector< E >& rs_first( int tab, const std::vector< vrc_f4 >& lut )
{
    static std::vector< E > built[6];
    std::vector< E >& t = built[tab];
    if( t.empty() )
    {
        t.resize( (size_t)VRC_FIRST_VISIT_ENTRIES * VRC_FIRST_VISIT_ROWS );
        volatile float zero = 0.0f;
        const vrc_f4 start = { zero, zero, zero, zero };
        for( uint32_t e = 0; e < VRC_FIRST_VISIT_ENTRIES; ++e )
            vrc_first_visit_row< E >( t.data() + (size_t)e * VRC_FIRST_VISIT_ROWS, vrc_lean_narrow( lut[e], (const E*)nullptr ),
                                      vrc_lean_narrow( start, (const E*)nullptr ) );
    }
    return t;
}

/* one uncounted uniform-only replay of fl's lists under table set-up `tab` (those of lean_one_ray); resolved: the planes
 * or NULL; how: bit 0 the first-visit table, bit 1 the free march */
static vrc_f4 rs_replay( vrc_frame fl, int tab, const uint32_t* resolved, int how )
{
    static std::vector< vrc_f4 > luts[6]; /* (made once per set-up: the rays are many) */
    static std::vector< vrc_f2 > luts2[6];
    const float alpha = ( tab & 1 ) ? 1.0f : 0.05f;
    const bool coloured = tab >= 2, onto = tab >= 4;
    if( luts[tab].empty() )
        make_tables( alpha, coloured, 4.0f, luts[tab], luts2[tab] );
    const std::vector< vrc_f4 >& lut = luts[tab];
    const std::vector< vrc_f2 >& lut2 = luts2[tab];
    fl.clearFirst = onto ? 0u : 1u;
    fl.walkLean = VRC_WALK_LEAN_UNIFORM;
    fl.walkResolved = resolved;
    fl.leanFree = ( how & 2 ) ? 1u : 0u;
    const vrc_classifier cls = {};
    vrc_f4 pixel = onto ? vrc_f4{ 0.125f, 0.25f, 0.0625f, ( tab & 1 ) ? 0.9995f : 0.5f } : vrc_f4{ 9.f, 9.f, 9.f, 9.f };
    uint32_t samples = 0u;
    if( coloured )
    {
        fl.firstVisit = ( how & 1 ) ? rs_first< vrc_f4 >( tab, lut ).data() : nullptr;
        vrc_pixel_walk_replay_lean< false, VRC_MODE_TABLE, VRC_GROUP, true >( fl, nullptr, nullptr, lut.data(), cls, &pixel, 0u, 0u,
                                                                              samples, AT );
    }
    else
    {
        fl.firstVisit = ( how & 1 ) ? rs_first< vrc_f2 >( tab, lut ).data() : nullptr;
        vrc_pixel_walk_replay_lean< false, VRC_MODE_GREY, 14, true >( fl, nullptr, nullptr, reinterpret_cast< const vrc_f4* >( lut2.data() ),
                                                                      cls, &pixel, 0u, 0u, samples, AT );
    }
    return pixel;
}

/* with the planes against without, under every table set-up and both switches */
static bool rs_same( const vrc_frame& fl, uint64_t* tally )
{
    const std::vector< uint32_t > planes = rs_resolve( fl );
    bool same = true;
    for( int tab = 0; tab < 6; ++tab )
        for( int how = 0; how < 4; ++how )
        {
            const vrc_f4 with = rs_replay( fl, tab, planes.data(), how ), without = rs_replay( fl, tab, nullptr, how );
            same = same && std::memcmp( &with, &without, sizeof( with ) ) == 0;
            ++tally[4];
        }
    return same;
}

static bool rs_one_ray( const scene& sc, rng& g, int kind, uint32_t variant, uint64_t* tally )
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
    std::vector< uint32_t > info( sc.info ); /* (an allocation of exactly walkSlots words) */
    f.slotInfo = info.data();
    f.clearFirst = 1u;
    f.walkLean = 1u;
    f.walkSlots = (uint32_t)info.size();
    std::vector< uint32_t > rayPlanes;
    lean_make_ray( sc, g, kind, f, rayPlanes );

    const vrc_dev_node* const nodes = sc.t.nodes.data();
    const int32_t* const grid = sc.t.grid.data();
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    const uint32_t counted = vrc_pixel_walk_record( f, nodes, grid, AT );
    const uint32_t K = counted > 0u ? counted : 1u;
    std::vector< uint32_t > full( ( 1u + 4u * K ) * P, GUARD ), one( ( 1u + 4u * 1u ) * P, GUARD );
    vrc_frame ff = f, f1 = f;
    ff.walkCache = full.data();
    ff.walkK = K;
    f1.walkCache = one.data();
    f1.walkK = 1u;
    full[AT] = vrc_pixel_walk_record( ff, nodes, grid, AT );
    one[AT] = vrc_pixel_walk_record( f1, nodes, grid, AT );
    bool bad = full[AT] != counted || one[AT] != counted;
    tally[counted == 0u ? 1 : ( counted == 1u ? 2 : 3 )] += 1u;

    /* counts 0, 1 and walkK; a count above walkK (the planes of one visit) */
    bad = bad || !rs_same( ff, tally ) || !rs_same( f1, tally );
    if( counted > 0u && !bad )
    {
        /* a word that does not hold one value on visit j: both replays end the list there */
        const uint32_t j = g.below( counted );
        const uint32_t idx = full[(size_t)AT + ( 2u + 4u * (size_t)j ) * P] & 0xFFFFFu;
        bad = bad || idx == 0u || idx > info.size();
        if( !bad )
        {
            const uint32_t kept = info[idx - 1u];
            info[idx - 1u] = ( g.next() & 1u ) ? 0u : ( kept | VRC_SLOT_MIXED );
            bad = bad || !rs_same( ff, tally );
            bad = bad || ( rs_resolve( ff )[(size_t)j * P + AT] & VRC_WALK_RESOLVED_ONE ) != 0u;
            info[idx - 1u] = kept;
            tally[5] += 1u;
        }
    }
    ++tally[0];
    tally[6] += bad ? 1u : 0u;
    return !bad;
}

/* `count` rays per (grid, variant, kind).  out: RESOLVED_RUN_TALLY numbers.  Returns the mismatches. */
extern "C" uint64_t walk_resolved_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * RESOLVED_RUN_TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int s = 0; s < 3; ++s )
    {
        scene sc;
        build_scene( sc, grids[s][0], grids[s][1], grids[s][2] );
        if( !sc.t.gridOk || sc.t.clamp )
            return ~0ull;
        make_every_brick_uniform( sc );
        g_nodes = &sc.t.nodes;
        for( uint32_t variant = 0; variant < 2u; ++variant )
            for( int kind = 0; kind < KINDS; ++kind )
                for( uint32_t i = 0; i < count; ++i )
                    (void)rs_one_ray( sc, g, kind, variant, out );
    }
    return out[6];
}

extern "C" int64_t walk_resolved_default() { return vrc_options().walkResolved; }

extern "C" int walk_resolved_plan( int64_t option, int64_t count, int uniformOnly, int fits )
{
    vrc_options o;
    o.walkResolved = option;
    o.count = count;
    return vrc_plan_walk_resolved( o, uniformOnly != 0, fits != 0 ) ? 1 : 0;
}

/* the replay's tile decode against the one it replaced (tile % tilesX, tile / tilesX and the lane's Morton bits in one
 * step): every lane of every tile of 1 x 1 up to 9 x 7 tiles.  tally: [0] pixels compared.  Returns the mismatches */
extern "C" uint64_t walk_resolved_tiles( uint64_t* tally )
{
    uint64_t bad = 0;
    tally[0] = 0;
    for( uint32_t tilesX = 1; tilesX <= 9u; ++tilesX )
        for( uint32_t tilesY = 1; tilesY <= 7u; ++tilesY )
            for( uint32_t tile = 0; tile < tilesX * tilesY; ++tile )
                for( uint32_t lane = 0; lane < 64u; ++lane )
                {
                    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
                    const uint32_t lx = ( lane & 1u ) | ( ( lane >> 1 ) & 2u ) | ( ( lane >> 2 ) & 4u );
                    const uint32_t ly = ( ( lane >> 1 ) & 1u ) | ( ( lane >> 2 ) & 2u ) | ( ( lane >> 3 ) & 4u );
                    uint32_t x0, y0, px, py;
                    vrc_replay_tile_origin( tile, tilesX, x0, y0 );
                    vrc_replay_lane_pixel( x0, y0, lane, px, py );
                    bad += ( px != tx * 8u + lx || py != ty * 8u + ly ) ? 1u : 0u;
                    ++tally[0];
                }
    return bad;
}

#if defined( WALK_RESOLVED_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 10u;
    uint64_t w[RESOLVED_WORDS_TALLY], out[RESOLVED_RUN_TALLY], t[1];
    uint64_t bad = walk_resolved_words( w );
    std::printf( "words %llu set %llu mismatches %llu\n", (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2] );
    bad += walk_resolved_run( 12345u, count, out );
    std::printf( "rays %llu none %llu one %llu more %llu replays %llu planted %llu mismatches %llu\n", (unsigned long long)out[0],
                 (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[4],
                 (unsigned long long)out[5], (unsigned long long)out[6] );
    const uint64_t tiles = walk_resolved_tiles( t );
    std::printf( "pixels %llu mismatches %llu\n", (unsigned long long)t[0], (unsigned long long)tiles );
    int wrong = 0;
    for( int64_t option = 0; option < 2; ++option )
        for( int64_t counting = 0; counting < 2; ++counting )
            for( int uniform = 0; uniform < 2; ++uniform )
                for( int fits = 0; fits < 2; ++fits )
                    wrong += walk_resolved_plan( option, counting, uniform, fits ) != ( option && !counting && uniform && fits );
    std::printf( "plan mismatches %d\n", wrong );
    return ( bad == 0 && tiles == 0 && wrong == 0 ) ? 0 : 1;
}
#endif
