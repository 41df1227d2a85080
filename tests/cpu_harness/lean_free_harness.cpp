/*
 * lean_free_harness.cpp -- the free body of the lean march (vrc_core.h: vrc_march_uniform_free, vrc_lean_free_visit,
 * vrc_frame::leanFree) and the decision behind VRC_OPT_LEAN_FREE_MARCH (vrc_plan.h: vrc_plan_lean_free_march), on the
 * host build, for tests/test_lean_free_march_cpu.py.
 *
 * lean_free_run( grey, tally ): every case of
 *     n        0 .. 300 and 4095 (the largest count a list word holds)
 *     entry    alpha over lf_entry_alphas: 0, -0, denormals, a grid up to 1.0, a negative value, NaN
 *     start    alpha 0 .. 0.9 in tenths, 0.9995, a negative value, NaN, and where t = 0.99 - n * e.w lies in [0, 1):
 *              t and its neighbours one ulp below and above -- the pre-test's own edge
 * through
 *     P   the lean march as it stood before the free body (lf_parent_march: that text, over vrc_uniform_groups)
 *     F1  vrc_march_uniform_lean< false > with the frame's word set,  F0  with it clear
 *     C   vrc_march_uniform_counted< true >,  K1  vrc_march_uniform_lean< true > with the word set
 * and holds: the colours of all five equal with memcmp, the return values equal, the uncounted marches leave the count
 * alone, the counted ones agree on it; the free body is taken (the hook's counter) by F1 exactly where the pre-test
 * passes, never by F0 or K1; and the bound's premise: where the pre-test passes, P returns false.
 * tally: [0] cases, [1] cases that pass the pre-test, [2] cases whose march ended early, [3] mismatches, [4] marches the
 * hook saw in the free body, [5] premise violations, [6] free bodies taken with the word clear or counted.
 *
 * Built as a shared library and, with -DLEAN_FREE_MAIN, as a stand-alone program for the sanitizers.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#define VRC_LEAN_FREE_HOOK
#include "../../libre_amd/csrc/vrc_core.h"
#include "../../libre_amd/csrc/vrc_plan.h"

uint64_t vrc_lean_free_taken[2] = { 0u, 0u };

/* the lean march before the free body: its text, unchanged */
template < bool COUNT, typename E >
static bool lf_parent_march( E& color, const E ue, uint32_t nLeft, uint32_t& nSamples )
{
    const bool crossed = vrc_uniform_groups< COUNT, VRC_LEAN_GROUP, E >( color, ue, nLeft, nSamples );
    if( !crossed )
    {
        const E saved = color;
        for( int body = VRC_LEAN_GROUP / 2; body > 0; body >>= 1 )
            if( nLeft & (uint32_t)body )
            {
                for( int k = 0; k < body; ++k )
                    vrc_composite( color, ue );
            }
        if( !( color.w > VRC_EARLY_EXIT ) )
        {
            if( COUNT )
                nSamples += nLeft;
            return false;
        }
        color = saved;
    }
    for( ; nLeft > 0u; --nLeft )
    {
        vrc_composite( color, ue );
        if( COUNT )
            nSamples += 1u;
        if( color.w > VRC_EARLY_EXIT )
            return true;
    }
    return false;
}

static std::vector< float > lf_entry_alphas()
{
    const float nan = std::numeric_limits< float >::quiet_NaN();
    const float denorm = std::numeric_limits< float >::denorm_min();
    return { 0.0f,  -0.0f,  denorm, 1.0e-40f, 1.1754942e-38f, 1.0e-8f, 1.0e-4f, 0.001f, 0.0024f, 0.0033f, 0.005f,
             0.01f, 0.02f,  0.05f,  0.0995f,  0.1f,           0.2f,    0.33f,   0.5f,   0.59f,   0.9f,    0.98f,
             0.99f, 0.999f, 1.0f,   -0.1f,    nan };
}

static void lf_make( float x, float w, vrc_f2& e ) { e = vrc_f2{ x, w }; }
static void lf_make( float x, float w, vrc_f4& e ) { e = vrc_f4{ x, 0.5f * x, 1.0f - x, w }; }

template < typename E >
static uint64_t lf_run( uint64_t* tally )
{
    const float nan = std::numeric_limits< float >::quiet_NaN();
    const std::vector< float > alphas = lf_entry_alphas();
    uint64_t bad = 0;
    for( uint32_t i = 0; i <= 301u; ++i )
    {
        const uint32_t n = i <= 300u ? i : 4095u;
        for( float ew : alphas )
        {
            E ue;
            lf_make( 0.25f + 0.5f * ( ew == ew ? ew : 0.0f ), ew, ue );
            std::vector< float > starts = { 0.0f, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f, 0.9995f, -0.0f, -0.25f, nan };
            const float t = 0.99f - (float)n * ew;
            if( t >= 0.0f && t < 1.0f )
            {
                starts.push_back( t );
                starts.push_back( std::nextafterf( t, -1.0f ) );
                starts.push_back( std::nextafterf( t, 2.0f ) );
            }
            for( float w0 : starts )
            {
                E start;
                lf_make( 0.125f, w0, start );
                const bool pass = vrc_lean_free_visit( start, ue, n );
                E p = start, f1 = start, f0 = start, c = start, k1 = start;
                uint32_t np = 7u, nf1 = 7u, nf0 = 7u, nc = 7u, nk1 = 7u;
                const bool rp = lf_parent_march< false, E >( p, ue, n, np );
                const uint64_t t0 = vrc_lean_free_taken[1];
                const bool rf1 = vrc_march_uniform_lean< false, E >( f1, ue, n, nf1, true );
                const uint64_t t1 = vrc_lean_free_taken[1];
                const bool rf0 = vrc_march_uniform_lean< false, E >( f0, ue, n, nf0, false );
                const bool rc = vrc_march_uniform_counted< true, E >( c, ue, n, nc );
                const bool rk1 = vrc_march_uniform_lean< true, E >( k1, ue, n, nk1, true );
                const uint64_t t2 = vrc_lean_free_taken[1];
                ++tally[0];
                tally[1] += pass ? 1u : 0u;
                tally[2] += rp ? 1u : 0u;
                tally[4] += t1 - t0;
                tally[6] += t2 - t1;
                if( pass && rp )
                    ++tally[5];
                /* (a negative entry lets alpha fall, which neither tested form is written for: the counted march and the
                 * lean one already part there, before this body -- groups of 16 and of 32 test at different samples --
                 * so C is held to the others for every entry that is not negative, and P, F1, F0, K1 for all) */
                const bool monotone = !( ew < 0.0f );
                const bool ok = std::memcmp( &p, &f1, sizeof( E ) ) == 0 && std::memcmp( &p, &f0, sizeof( E ) ) == 0 &&
                                ( !monotone || std::memcmp( &p, &c, sizeof( E ) ) == 0 ) && std::memcmp( &p, &k1, sizeof( E ) ) == 0 &&
                                rp == rf1 && rp == rf0 && ( !monotone || rp == rc ) && rp == rk1 && np == 7u && nf1 == 7u &&
                                nf0 == 7u && ( !monotone || nc == nk1 ) &&
                                t1 - t0 == ( pass ? 1u : 0u ) && t2 == t1 && !( pass && rp );
                if( !ok )
                {
                    if( bad < 8 )
                        std::fprintf( stderr, "lean_free: n %u e.w %.9g w0 %.9g pass %d: w %.9g %.9g %.9g %.9g %.9g  done %d %d %d %d %d  "
                                              "count %u %u  free taken %llu %llu\n",
                                      n, (double)ew, (double)w0, (int)pass, (double)p.w, (double)f1.w, (double)f0.w, (double)c.w,
                                      (double)k1.w, (int)rp, (int)rf1, (int)rf0, (int)rc, (int)rk1, nc, nk1,
                                      (unsigned long long)( t1 - t0 ), (unsigned long long)( t2 - t1 ) );
                    ++bad;
                }
            }
        }
    }
    tally[3] += bad;
    return bad;
}

extern "C" uint64_t lean_free_run( int grey, uint64_t* tally )
{
    std::memset( tally, 0, 7 * sizeof( uint64_t ) );
    return grey ? lf_run< vrc_f2 >( tally ) : lf_run< vrc_f4 >( tally );
}

extern "C" uint32_t lean_free_group() { return VRC_LEAN_FREE_GROUP; }
extern "C" int64_t lean_free_default() { return vrc_options().leanFreeMarch; }

/* the decision over an options struct at its defaults but for the option and the sample counter */
extern "C" int lean_free_plan( int64_t option, int64_t count, int64_t walkUsed, uint32_t walkLean, int classify )
{
    vrc_options o;
    o.leanFreeMarch = option;
    o.count = count;
    return vrc_plan_lean_free_march( o, walkUsed, walkLean, classify != 0 ) ? 1 : 0;
}

#if defined( LEAN_FREE_MAIN )
int main()
{
    uint64_t bad = 0, t[7], cases = 0, passed = 0, early = 0, freed = 0, premise = 0, stray = 0;
    for( int grey = 0; grey < 2; ++grey )
    {
        bad += lean_free_run( grey, t );
        cases += t[0];
        passed += t[1];
        early += t[2];
        freed += t[4];
        premise += t[5];
        stray += t[6];
    }
    int plans = 0, wrong = 0;
    for( int m = 0; m < 2 * 2 * 5 * 3 * 2; ++m )
    {
        int r = m;
        const int option = r % 2; r /= 2;
        const int count = r % 2; r /= 2;
        const int used = r % 5; r /= 5;
        const int lean = r % 3; r /= 3;
        const int classify = r % 2;
        const int want = ( option && !count && used == 4 && lean != 0 && !classify ) ? 1 : 0;
        wrong += lean_free_plan( option, count, used, (uint32_t)lean, classify ) != want;
        ++plans;
    }
    std::printf( "cases %llu passed %llu early %llu freed %llu premise %llu stray %llu plans %d mismatches %llu plan %d\n",
                 (unsigned long long)cases, (unsigned long long)passed, (unsigned long long)early, (unsigned long long)freed,
                 (unsigned long long)premise, (unsigned long long)stray, plans, (unsigned long long)bad, wrong );
    return ( bad || wrong || premise || stray || freed != passed ) ? 1 : 0;
}
#endif
