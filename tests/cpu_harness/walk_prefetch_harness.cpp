/*
 * walk_prefetch_harness.cpp -- the unconditional reads of the lean replay (vrc_core.h: vrc_lean_list_word,
 * vrc_lean_slot_load) on the host build of the per-ray code, for tests/test_walk_prefetch_cpu.py.
 * TEST INFRASTRUCTURE ONLY.
 *
 * vrc_pixel_walk_replay_lean reads the list word of visit min(k + 2, walkK - 1) and the slot word of visit k + 1 in
 * every visit k, whatever the ray's count says, and the words of its first two visits before it has looked at the
 * count.  What that rests on is checked here with allocations that are EXACTLY as large as the kernel's contract says:
 * lists of (1 + 4 K) P words and a slotInfo of walkSlots words, each an array of its own from the heap, so that under
 * the address sanitizer a read one word past either is an error.
 *
 * The scenes, tables, rays and random numbers are those of walk_lean_harness.cpp (included).  A ray is recorded once in
 * both forms; then for K = 1, 2, 3 and every count c from 0 to min( K, the ray's visits ) the first c visits are copied
 * into fresh lists of K visits per ray -- so c = K occurs for every K, and where c < K the planes past the count hold
 * words of all ones (a step count of 4095 and an index of 2^20 - 1: never marched, and as an index far beyond
 * walkSlots).  Each is replayed with five set-ups of the slot index:
 *   recorded  the node's own index, slotInfo of one word per slot;
 *   none      the first visit's index is 0 in the list and in the node (no slot word: the visit gathers);
 *   last      slotInfo ends with the word of the largest index the list holds;
 *   beyond    as `last`, and the first visit's index in the list lies past walkSlots: clamped, it reads the last word,
 *             which is what the other form reads through a node whose index is walkSlots;
 *   no info   slotInfo is NULL in both forms (every visit gathers; the lean form loads word 0 of its own lists).
 * and three tables (grey at alpha 0.05 and 1.0, coloured at 0.05).  Expected in every case: the pixel bits and the
 * sample count of vrc_pixel_walk_replay from the other form of the same list, which tests/test_walk_cache_cpu.py holds
 * to the walk.
 * Built as a shared library (walk_prefetch_run) and, with -DWALK_PREFETCH_MAIN, as a stand-alone program for the
 * sanitizers.
 */
#include <memory>

#include "walk_lean_harness.cpp"

/* [0] rays with a list, [1] replays compared, [2] of them with count == K, [3] with count == 0, [4] with the largest
 * index on slotInfo's last word, [5] with an index beyond walkSlots, [6] mismatches */
#define PREFETCH_TALLY 7

enum
{
    SLOT_RECORDED,
    SLOT_NONE,
    SLOT_LAST,
    SLOT_BEYOND,
    SLOT_NO_INFO,
    SLOT_CASES
};

/* the three tables: grey at alpha 0.05 and 1.0, coloured at 0.05 (made once per run) */
static std::vector< vrc_f4 > g_lut[3];
static std::vector< vrc_f2 > g_lut2[3];

static const uint32_t INDEX_MASK = ( 1u << VRC_WALK_LEAN_INDEX_BITS ) - 1u;

static bool prefetch_one_ray( const scene& sc, rng& g, int kind, uint32_t variant, uint64_t* tally )
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
    f.slotInfo = sc.info.data();
    f.clearFirst = 1u;
    std::vector< uint32_t > rayPlanes;
    lean_make_ray( sc, g, kind, f, rayPlanes );

    const int32_t* const grid = sc.t.grid.data();
    const vrc_classifier cls = {};

    /* the ray's whole list, once in each form */
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    const uint32_t counted = vrc_pixel_walk_record( f, sc.t.nodes.data(), grid, AT );
    if( counted == 0u )
        return true;
    vrc_frame fl = f;
    fl.walkLean = 1u;
    fl.walkSlots = (uint32_t)sc.info.size();
    std::vector< uint32_t > plain( ( 1u + 4u * counted ) * P, GUARD ), lean( ( 1u + 4u * counted ) * P, GUARD );
    f.walkCache = plain.data();
    fl.walkCache = lean.data();
    f.walkK = fl.walkK = counted;
    bool bad = vrc_pixel_walk_record( f, sc.t.nodes.data(), grid, AT ) != counted ||
               vrc_pixel_walk_record( fl, sc.t.nodes.data(), grid, AT ) != counted;
    ++tally[0];

    for( uint32_t K = 1u; K <= 3u && !bad; ++K )
        for( uint32_t c = 0u; c <= K && c <= counted && !bad; ++c )
            for( int slotCase = 0; slotCase < SLOT_CASES && !bad; ++slotCase )
            {
                if( c == 0u && slotCase != SLOT_RECORDED && slotCase != SLOT_NO_INFO )
                    continue; /* (no visit whose index could be set) */
                /* lists of exactly (1 + 4 K) P words: the first c visits of the ray, all ones behind them */
                const size_t words = ( 1u + 4u * (size_t)K ) * P;
                std::unique_ptr< uint32_t[] > a( new uint32_t[words] ), b( new uint32_t[words] );
                for( size_t w = 0; w < words; ++w )
                    a[w] = b[w] = GUARD;
                a[AT] = b[AT] = c;
                uint32_t largest = 1u;
                for( uint32_t v = 0u; v < K; ++v )
                    for( uint32_t p = 1u; p <= 4u; ++p )
                    {
                        const size_t w = ( p + 4u * (size_t)v ) * P + AT;
                        a[w] = v < c ? plain[w] : 0xFFFFFFFFu;
                        b[w] = v < c ? lean[w] : 0xFFFFFFFFu;
                        if( p == 2u && v < c && ( lean[w] & INDEX_MASK ) > largest )
                            largest = lean[w] & INDEX_MASK;
                    }
                std::vector< vrc_dev_node > nodes = sc.t.nodes; /* (the case may give the first visit's node another index) */
                uint32_t nSlots = (uint32_t)sc.info.size();
                const size_t first = 2u * P + AT; /* the first visit's word; its node lies a plane in front of it */
                if( slotCase == SLOT_NONE )
                {
                    b[first] &= ~INDEX_MASK;
                    nodes[a[first - P]].slotInfoIndex = 0u;
                }
                if( slotCase == SLOT_LAST || slotCase == SLOT_BEYOND )
                    nSlots = largest;
                if( slotCase == SLOT_BEYOND )
                {
                    b[first] = ( b[first] & ~INDEX_MASK ) | ( ( g.next() & 1u ) ? INDEX_MASK : nSlots + 1u + g.below( 9 ) );
                    nodes[a[first - P]].slotInfoIndex = nSlots;
                }
                /* slotInfo of exactly nSlots words */
                std::unique_ptr< uint32_t[] > info( new uint32_t[nSlots] );
                for( uint32_t i = 0; i < nSlots; ++i )
                    info[i] = sc.info[i];
                vrc_frame fa = f, fb = fl;
                fa.walkCache = a.get();
                fb.walkCache = b.get();
                fa.walkK = fb.walkK = K;
                fa.slotInfo = fb.slotInfo = slotCase == SLOT_NO_INFO ? nullptr : info.get();
                fb.walkSlots = nSlots;
                for( int tab = 0; tab < 3 && !bad; ++tab )
                {
                    const std::vector< vrc_f4 >& lut = g_lut[tab];
                    const std::vector< vrc_f2 >& lut2 = g_lut2[tab];
                    const vrc_f4 start = { 9.f, 9.f, 9.f, 9.f };
                    vrc_f4 pa = start, pb = start;
                    uint32_t na = 0, nb = 0;
                    if( tab == 2 )
                    {
                        vrc_pixel_walk_replay< true, VRC_MODE_TABLE, VRC_GROUP >( fa, nodes.data(), sc.atlas.data(), lut.data(), cls, &pa, 0u, 0u, na, AT );
                        vrc_pixel_walk_replay_lean< true, VRC_MODE_TABLE, VRC_GROUP >( fb, nodes.data(), sc.atlas.data(), lut.data(), cls, &pb, 0u, 0u, nb, AT );
                    }
                    else
                    {
                        const vrc_f4* const t2 = reinterpret_cast< const vrc_f4* >( lut2.data() );
                        vrc_pixel_walk_replay< true, VRC_MODE_GREY, 14 >( fa, nodes.data(), sc.atlas.data(), t2, cls, &pa, 0u, 0u, na, AT );
                        vrc_pixel_walk_replay_lean< true, VRC_MODE_GREY, 14 >( fb, nodes.data(), sc.atlas.data(), t2, cls, &pb, 0u, 0u, nb, AT );
                    }
                    bad = bad || std::memcmp( &pa, &pb, sizeof( pa ) ) != 0 || na != nb;
                    /* a list of no visits clears the pixel and samples nothing */
                    bad = bad || ( c == 0u && ( nb != 0u || pb.x != 0.0f || pb.w != 0.0f ) );
                    ++tally[1];
                    tally[2] += c == K ? 1u : 0u;
                    tally[3] += c == 0u ? 1u : 0u;
                    tally[4] += slotCase == SLOT_LAST ? 1u : 0u;
                    tally[5] += slotCase == SLOT_BEYOND ? 1u : 0u;
                }
            }
    tally[6] += bad ? 1u : 0u;
    return !bad;
}

/* `count` rays per (grid, variant, kind).  out: PREFETCH_TALLY numbers.  Returns the mismatches. */
extern "C" uint64_t walk_prefetch_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * PREFETCH_TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int tab = 0; tab < 3; ++tab )
        make_tables( tab == 1 ? 1.0f : 0.05f, tab == 2, 4.0f, g_lut[tab], g_lut2[tab] );
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
                    (void)prefetch_one_ray( sc, g, kind, variant, out );
    }
    return out[6];
}

#if defined( WALK_PREFETCH_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 5u;
    uint64_t out[PREFETCH_TALLY];
    const uint64_t bad = walk_prefetch_run( 12345u, count, out );
    std::printf( "lists %llu replays %llu full %llu empty %llu last %llu beyond %llu mismatches %llu\n",
                 (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                 (unsigned long long)out[3], (unsigned long long)out[4], (unsigned long long)out[5],
                 (unsigned long long)bad );
    return bad == 0 ? 0 : 1;
}
#endif
