/*
 * first_visit_harness.cpp -- the first-visit table of the lean replay (vrc_core.h: vrc_first_visit_row,
 * vrc_frame::firstVisit) and the decisions behind VRC_OPT_FIRST_VISIT_TABLE (vrc_plan.h: vrc_plan_first_visit,
 * vrc_plan_first_visit_build), on the host build, for tests/test_first_visit_table_cpu.py.
 *
 * first_visit_run( alpha, correction, grey, tally ): a classified table from vrc_lut_entry over a coloured ramp whose
 * opacity rises to `alpha` (the grey form: the x and w of its entries, as the grey instances stage them), with entry
 * 255 replaced by one whose w is exactly 1 when alpha is 1 -- it crosses at its first sample.  For every entry e and
 * every n in 0 .. VRC_FIRST_VISIT_ROWS - 1: the row builder's T[e][n] against vrc_march_uniform_lean< false > and
 * < true > of n samples of e from zero -- the colour with memcmp, T[e][n].w > VRC_EARLY_EXIT against the march's return
 * value, and the counted march's samples against min( n, the row's crossing ).  The start colour reaches the builder
 * through a volatile, as it reaches the kernel through an argument.
 * tally: [0] cells compared, [1] cells whose march ended early, [2] entries that cross inside the rows, [3] mismatches.
 *
 * first_visit_replay( grey, tally ): vrc_pixel_walk_replay_lean< false, ..., uniform-only and not > over a list of two
 * uniform visits, with the table against without it: the same pixel bytes for every entry and n in the called-out set
 * and at n = ROWS, ROWS + 1 (marched, not looked up); with clearFirst = 0 the table is not read (it is handed a table of
 * NaNs and must leave the pixel of the run without one).
 *
 * Built as a shared library and, with -DFIRST_VISIT_MAIN, as a stand-alone program for the sanitizers.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "../../libre_amd/csrc/vrc_core.h"
#include "../../libre_amd/csrc/vrc_plan.h"

static void fv_table( float alpha, float correction, std::vector< vrc_f4 >& lut )
{
    float tf[256 * 4];
    for( int i = 0; i < 256; ++i )
    {
        const float u = (float)i / 255.0f;
        tf[4 * i + 0] = u;
        tf[4 * i + 1] = 1.0f - u;
        tf[4 * i + 2] = 0.25f + 0.5f * u;
        tf[4 * i + 3] = alpha * u;
    }
    const vrc_lut_params lp = { 0.0f, 256.0f, correction, 8 };
    lut.assign( VRC_LUT_ENTRIES + 1u, vrc_f4{ 0.f, 0.f, 0.f, 0.f } );
    for( uint32_t d = 0; d < 256u; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    if( alpha == 1.0f )
        lut[255] = vrc_f4{ 0.5f, 0.25f, 0.125f, 1.0f }; /* opaque at once: crosses at sample 1 */
    lut[1] = vrc_f4{ -0.0f, -0.0f, -0.0f, 0.0f };        /* the sign of a zero product (vrc_first_visit_row) */
}

template < typename E >
static uint64_t fv_run( const std::vector< vrc_f4 >& lut, uint64_t* tally )
{
    const uint32_t ROWS = VRC_FIRST_VISIT_ROWS;
    std::vector< E > table( (size_t)VRC_FIRST_VISIT_ENTRIES * ROWS );
    volatile float zero = 0.0f;
    uint64_t bad = 0;
    for( uint32_t e = 0; e < VRC_FIRST_VISIT_ENTRIES; ++e )
    {
        const E ue = vrc_lean_narrow( lut[e], (const E*)nullptr );
        const vrc_f4 start4 = { zero, zero, zero, zero };
        vrc_first_visit_row< E >( table.data() + (size_t)e * ROWS, ue, vrc_lean_narrow( start4, (const E*)nullptr ) );
        /* the row's crossing: the first j whose colour is past the threshold (ROWS: none inside the rows) */
        uint32_t cross = ROWS;
        for( uint32_t j = 0; j < ROWS && cross == ROWS; ++j )
            if( table[(size_t)e * ROWS + j].w > VRC_EARLY_EXIT )
                cross = j;
        if( cross < ROWS )
            ++tally[2];
        for( uint32_t n = 0; n < ROWS; ++n )
        {
            const E& t = table[(size_t)e * ROWS + n];
            E a = vrc_lean_narrow( vrc_f4{ 0.f, 0.f, 0.f, 0.f }, (const E*)nullptr ), b = a;
            uint32_t na = 0u, nb = 0u;
            const bool da = vrc_march_uniform_lean< false, E >( a, ue, n, na );
            const bool db = vrc_march_uniform_lean< true, E >( b, ue, n, nb );
            const bool done = t.w > VRC_EARLY_EXIT;
            const bool ok = std::memcmp( &t, &a, sizeof( E ) ) == 0 && std::memcmp( &t, &b, sizeof( E ) ) == 0 && done == da &&
                            done == db && na == 0u && nb == ( n < cross ? n : cross );
            ++tally[0];
            if( da )
                ++tally[1];
            if( !ok )
            {
                if( bad < 8 )
                    std::fprintf( stderr, "first_visit: entry %u n %u: table w %.9g done %d, march w %.9g done %d samples %u (cross %u)\n",
                                  e, n, (double)t.w, (int)done, (double)a.w, (int)da, nb, cross );
                ++bad;
            }
        }
    }
    tally[3] += bad;
    return bad;
}

extern "C" uint64_t first_visit_run( float alpha, float correction, int grey, uint64_t* tally )
{
    std::vector< vrc_f4 > lut;
    fv_table( alpha, correction, lut );
    std::memset( tally, 0, 4 * sizeof( uint64_t ) );
    return grey ? fv_run< vrc_f2 >( lut, tally ) : fv_run< vrc_f4 >( lut, tally );
}

/* the kernel's function on a list of two uniform visits ( e0, n0 ), ( e1, 37 ) of one ray */
template < int MODE, int GROUP, bool UNIFORM_ONLY >
static vrc_f4 fv_replay_one( const std::vector< vrc_f4 >& lut, const void* table, uint32_t clearFirst, uint32_t e0, uint32_t n0,
                             uint32_t firstWord, vrc_f4 before )
{
    typedef typename vrc_lean_colour< MODE >::type E;
    std::vector< E > tab( VRC_LUT_ENTRIES + 1u );
    for( size_t i = 0; i < tab.size(); ++i )
        tab[i] = vrc_lean_narrow( lut[i], (const E*)nullptr );
    /* planes: count | visit 0: node, word, tNear, tFar | visit 1: ... ; one ray per plane */
    uint32_t lists[9] = { 2u, 0u, ( n0 << VRC_WALK_LEAN_INDEX_BITS ) | 1u, 0u, 0u, 0u, ( 37u << VRC_WALK_LEAN_INDEX_BITS ) | 2u, 0u, 0u };
    const uint32_t slotInfo[2] = { firstWord | e0, VRC_SLOT_KNOWN | 200u };
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.width = f.height = 1u;
    f.nodeCount = 1u;
    f.clearFirst = clearFirst;
    f.walkCache = lists;
    f.walkPlane = 1u;
    f.walkK = 2u;
    f.walkLean = UNIFORM_ONLY ? VRC_WALK_LEAN_UNIFORM : 1u;
    f.walkSlots = 2u;
    f.slotInfo = slotInfo;
    f.firstVisit = table;
    vrc_classifier cls;
    std::memset( &cls, 0, sizeof( cls ) );
    vrc_f4 px = before;
    uint32_t samples = 0u;
    vrc_pixel_walk_replay_lean< false, MODE, GROUP, UNIFORM_ONLY >( f, nullptr, nullptr, reinterpret_cast< const vrc_f4* >( tab.data() ),
                                                                    cls, &px, 0u, 0u, samples, 0u );
    return px;
}

template < int MODE, int GROUP, bool UNIFORM_ONLY >
static uint64_t fv_replay( const std::vector< vrc_f4 >& lut, uint64_t* tally )
{
    typedef typename vrc_lean_colour< MODE >::type E;
    const uint32_t ROWS = VRC_FIRST_VISIT_ROWS;
    std::vector< E > table( (size_t)VRC_FIRST_VISIT_ENTRIES * ROWS ), nans( table.size() );
    std::memset( nans.data(), 0xFF, nans.size() * sizeof( E ) );
    for( uint32_t e = 0; e < VRC_FIRST_VISIT_ENTRIES; ++e )
        vrc_first_visit_row< E >( table.data() + (size_t)e * ROWS, vrc_lean_narrow( lut[e], (const E*)nullptr ),
                                  vrc_lean_narrow( vrc_f4{ 0.f, 0.f, 0.f, 0.f }, (const E*)nullptr ) );
    const uint32_t ns[] = { 0u, 1u, 31u, 32u, 33u, 63u, 64u, 150u, ROWS - 1u, ROWS, ROWS + 1u };
    const vrc_f4 before = { 0.125f, 0.125f, 0.125f, 0.25f }; /* (grey: what a grey frame could have left) */
    uint64_t bad = 0;
    for( uint32_t e = 0; e < VRC_FIRST_VISIT_ENTRIES; ++e )
        for( uint32_t n : ns )
        {
            /* a frame that clears: the table against the march */
            const vrc_f4 a = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nullptr, 1u, e, n, VRC_SLOT_KNOWN, before );
            const vrc_f4 b = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, table.data(), 1u, e, n, VRC_SLOT_KNOWN, before );
            /* rows past the table are marched: a table of NaNs changes nothing there */
            const vrc_f4 c = n >= ROWS ? fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nans.data(), 1u, e, n, VRC_SLOT_KNOWN, before ) : a;
            /* a pass that does not clear never reads the table (a grey frame always clears: vrc_render) */
            vrc_f4 d0 = a, d1 = a;
            if( MODE != VRC_MODE_GREY )
            {
                d0 = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nullptr, 0u, e, n, VRC_SLOT_KNOWN, before );
                d1 = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nans.data(), 0u, e, n, VRC_SLOT_KNOWN, before );
            }
            /* a first visit whose word does not hold one value is not looked up (uniform-only: it ends the list) */
            vrc_f4 g0 = a, g1 = a;
            if( UNIFORM_ONLY )
            {
                g0 = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nullptr, 1u, e, n, VRC_SLOT_KNOWN | VRC_SLOT_MIXED, before );
                g1 = fv_replay_one< MODE, GROUP, UNIFORM_ONLY >( lut, nans.data(), 1u, e, n, VRC_SLOT_KNOWN | VRC_SLOT_MIXED, before );
            }
            tally[0] += 4u;
            if( std::memcmp( &a, &b, sizeof( a ) ) != 0 || std::memcmp( &a, &c, sizeof( a ) ) != 0 ||
                std::memcmp( &d0, &d1, sizeof( a ) ) != 0 || std::memcmp( &g0, &g1, sizeof( a ) ) != 0 )
            {
                if( bad < 8 )
                    std::fprintf( stderr, "first_visit: replay entry %u n %u: %.9g %.9g | %.9g | %.9g %.9g | %.9g %.9g\n", e, n,
                                  (double)a.w, (double)b.w, (double)c.w, (double)d0.w, (double)d1.w, (double)g0.w, (double)g1.w );
                ++bad;
            }
        }
    tally[3] += bad;
    return bad;
}

extern "C" uint64_t first_visit_replay( float alpha, int grey, int uniformOnly, uint64_t* tally )
{
    std::vector< vrc_f4 > lut;
    fv_table( alpha, 1.0f, lut );
    std::memset( tally, 0, 4 * sizeof( uint64_t ) );
    if( grey )
        return uniformOnly ? fv_replay< VRC_MODE_GREY, 14, true >( lut, tally ) : fv_replay< VRC_MODE_GREY, 14, false >( lut, tally );
    return uniformOnly ? fv_replay< VRC_MODE_TABLE, VRC_GROUP, true >( lut, tally ) : fv_replay< VRC_MODE_TABLE, VRC_GROUP, false >( lut, tally );
}

extern "C" uint32_t first_visit_rows() { return VRC_FIRST_VISIT_ROWS; }
extern "C" int64_t first_visit_default() { return vrc_options().firstVisitTable; }

/* the two decisions over an options struct at its defaults but for the option and the sample counter.
 * bit 0: vrc_plan_first_visit, bit 1: vrc_plan_first_visit_build */
extern "C" int first_visit_plan( int64_t option, int64_t count, int64_t walkUsed, uint32_t walkLean, int clearFirst, int classify,
                                 int current, int prevSame )
{
    vrc_options o;
    o.firstVisitTable = option;
    o.count = count;
    const vrc_first_visit_facts k = { walkUsed, walkLean, clearFirst != 0, classify != 0, current != 0 };
    return ( vrc_plan_first_visit( o, k ) ? 1 : 0 ) | ( vrc_plan_first_visit_build( o, k, prevSame != 0 ) ? 2 : 0 );
}

#if defined( FIRST_VISIT_MAIN )
int main()
{
    uint64_t bad = 0, t[4], cells = 0, replays = 0;
    const float alphas[3] = { 0.05f, 0.3f, 1.0f };
    for( float alpha : alphas )
        for( int grey = 0; grey < 2; ++grey )
        {
            bad += first_visit_run( alpha, 1.0f, grey, t );
            cells += t[0];
            for( int u = 0; u < 2; ++u )
            {
                bad += first_visit_replay( alpha, grey, u, t );
                replays += t[0];
            }
        }
    bad += first_visit_run( 1.0f, 8.0f, 0, t );
    cells += t[0];
    int plans = 0, wrong = 0;
    for( int m = 0; m < 2 * 2 * 5 * 3 * 2 * 2 * 2 * 2; ++m )
    {
        int r = m;
        const int option = r % 2; r /= 2;
        const int count = r % 2; r /= 2;
        const int used = r % 5; r /= 5;
        const int lean = r % 3; r /= 3;
        const int clear = r % 2; r /= 2;
        const int classify = r % 2; r /= 2;
        const int current = r % 2; r /= 2;
        const int prev = r % 2;
        const bool wanted = option && !count && used == 4 && lean != 0 && clear && !classify;
        const int want = ( wanted && current ? 1 : 0 ) | ( wanted && !current && prev ? 2 : 0 );
        wrong += first_visit_plan( option, count, used, (uint32_t)lean, clear, classify, current, prev ) != want;
        ++plans;
    }
    std::printf( "cells %llu replays %llu plans %d mismatches %llu plan %d\n", (unsigned long long)cells, (unsigned long long)replays,
                 plans, (unsigned long long)bad, wrong );
    return ( bad || wrong ) ? 1 : 0;
}
#endif
