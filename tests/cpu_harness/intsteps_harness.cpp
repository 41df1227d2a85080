/*
 * intsteps_harness.cpp -- uniform_harness.cpp built with the host-side hook of the uniform march's two forms
 * (vrc_core.h: VRC_UNIFORM_FORM_HOOK), for tests/test_uniform_intsteps_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * The render entry point is uniform_harness_render itself; on top of it: a switch that keeps every uniform segment on
 * the float chain, the tally of segments per form, and the counting identity on its own (vrc_exact_step_count against
 * the trips of the float chain it replaces).
 */
#define VRC_UNIFORM_FORM_HOOK
#include "uniform_harness.cpp"

int vrc_uniform_form_hook = 0;
uint64_t vrc_uniform_form_taken[2] = { 0, 0 };

/* 0 = as the product decides, 1 = the float chain for every uniform segment */
extern "C" void intsteps_set_form( int form )
{
    vrc_uniform_form_hook = form;
}

/* segments marched by the float chain / the counted form since the last call */
extern "C" void intsteps_taken( uint64_t out[2] )
{
    out[0] = vrc_uniform_form_taken[0];
    out[1] = vrc_uniform_form_taken[1];
    vrc_uniform_form_taken[0] = vrc_uniform_form_taken[1] = 0;
}

/* per value: whether the count is exact (exactOut), the count (nOut), and -- where trips[i] != 0 on entry -- the trips
 * of the reference's loop, counted by running it */
extern "C" void intsteps_count( const float* travel, uint32_t count, float stepSize, uint8_t* exactOut, uint32_t* nOut,
                                uint32_t* trips )
{
    for( uint32_t i = 0; i < count; ++i )
    {
        uint32_t n = 0;
        exactOut[i] = vrc_exact_step_count( travel[i], stepSize, &n ) ? 1 : 0;
        nOut[i] = n;
        if( trips[i] != 0u )
        {
            uint32_t k = 0;
            volatile float t = travel[i]; /* every subtraction rounded to float, as on the GPU */
            while( t > 0.0f )
            {
                t = t - stepSize;
                ++k;
            }
            trips[i] = k;
        }
    }
}

/* one uniform segment of `travel` through both forms from the same colour: 0 = same colour bits, same count, same
 * return value */
extern "C" int intsteps_segment( float travel, float stepSize, float eGrey, float eAlpha, float startGrey,
                                 float startAlpha, float* out, uint32_t* samplesOut )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.stepSize = stepSize;
    vrc_dev_node n;
    std::memset( &n, 0, sizeof( n ) );
    vrc_segment s;
    std::memset( &s, 0, sizeof( s ) );
    s.dist = travel;
    const vrc_f2 ue = { eGrey, eAlpha };
    vrc_f2 c[2];
    uint32_t cnt[2] = { 0, 0 };
    bool done[2];
    const int keep = vrc_uniform_form_hook;
    for( int form = 0; form < 2; ++form )
    {
        vrc_uniform_form_hook = form;
        c[form] = vrc_f2{ startGrey, startAlpha };
        done[form] = vrc_march_segment_as< false, true, true, uint8_t, 14, vrc_f2, false, true >(
            f, n, s, (const uint8_t*)nullptr, (const vrc_f2*)nullptr, c[form], cnt[form], 0.0f, nullptr, ue );
    }
    vrc_uniform_form_hook = keep;
    out[0] = c[0].x;
    out[1] = c[0].w;
    *samplesOut = cnt[0];
    return ( std::memcmp( &c[0], &c[1], sizeof( vrc_f2 ) ) == 0 && cnt[0] == cnt[1] && done[0] == done[1] ) ? 0 : 1;
}
