/*
 * store_through_harness.cpp -- the pixel store of the replay (vrc_core.h: vrc_store_pixel, vrc_frame::storeThrough) on
 * the host build of the per-ray code, and the decision that sets the word (vrc_plan.h: vrc_plan_store_through), for
 * tests/test_store_through_cpu.py.  TEST INFRASTRUCTURE ONLY.
 *
 * On the host the helper is the assignment it replaced, whatever the frame's word says.  What is held to that: the
 * walk (vrc_pixel_grid_dda), whose own stores are still plain assignments, renders the same ray into a buffer of its
 * own.  The grids, tables, random numbers and kinds of rays are those of walk_lean_harness.cpp, as they are (every third
 * brick uniform) and with every brick made uniform (walk_uniform_only_harness.cpp); steps of 1/64 and 1/128.  For every
 * ray, under the six table set-ups (alpha 0.05 and 1.0, grey and coloured, the coloured ones also onto a pixel that is
 * not cleared), with storeThrough 0 and 1:
 *   - vrc_pixel_walk_replay from the plain list, vrc_pixel_walk_replay_lean from the lean list and, on the uniform
 *     scenes, its uniform-only form leave the bytes of the walk's pixel and its sample count;
 *   - the pixel is number 4 of a buffer of 3 x 2 (px = 1, py = 1) whose other five hold a sentinel before and after, so
 *     a store that took another index, or more than 16 bytes, shows;
 *   - a ray without visits leaves zeros where the frame clears and the buffer's own bytes where it does not.
 * The buffer is an allocation of exactly six pixels: under the address sanitizer a store past it is a failure.
 * Built as a shared library (store_through_run, store_through_plan) and, with -DSTORE_THROUGH_MAIN, as a stand-alone
 * program for the sanitizers.
 */
#include "walk_uniform_only_harness.cpp"

#include "../../libre_amd/csrc/vrc_plan.h"

/* [0] rays, [1] rays without visits, [2] with, [3] replays compared, [4] replays of the uniform-only form among them,
 * [5] cleared pixels checked to be zero, [6] mismatches */
#define STORE_TALLY 7

static const uint32_t ST_W = 3u, ST_H = 2u, ST_PX = 1u, ST_PY = 1u, ST_POS = ST_PY * ST_W + ST_PX;

struct st_buffer
{
    std::vector< vrc_f4 > px;
    uint32_t samples = 0u;
};

static vrc_f4 st_sentinel( uint32_t i ) { return vrc_f4{ 100.0f + (float)i, -7.0f, 0.5f, 3.0f }; }

static st_buffer st_fresh( bool onto, int tab )
{
    st_buffer b;
    b.px.resize( (size_t)ST_W * ST_H );
    for( uint32_t i = 0; i < ST_W * ST_H; ++i )
        b.px[i] = st_sentinel( i );
    b.px[ST_POS] = onto ? vrc_f4{ 0.125f, 0.25f, 0.0625f, ( tab & 1 ) ? 0.9995f : 0.5f } : vrc_f4{ 9.f, 9.f, 9.f, 9.f };
    return b;
}

static bool st_same( const st_buffer& a, const st_buffer& b )
{
    return a.samples == b.samples && std::memcmp( a.px.data(), b.px.data(), a.px.size() * sizeof( vrc_f4 ) ) == 0;
}

static bool st_one_ray( const scene& sc, bool uniformScene, rng& g, int kind, uint32_t variant, uint64_t* tally )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = variant;
    f.stepSize = ( g.next() & 1u ) ? 1.0f / 64.0f : 1.0f / 128.0f;
    f.width = ST_W;
    f.height = ST_H;
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

    /* the two lists */
    f.walkCache = nullptr;
    f.walkPlane = P;
    f.walkK = 0u;
    const uint32_t counted = vrc_pixel_walk_record( f, nodes, grid, AT );
    const uint32_t K = counted > 0u ? counted : 1u;
    std::vector< uint32_t > plain( ( 1u + 4u * K ) * P, GUARD ), lean( ( 1u + 4u * K ) * P, GUARD );
    vrc_frame fl = f;
    fl.walkLean = 1u;
    fl.walkSlots = (uint32_t)sc.info.size();
    f.walkCache = plain.data();
    fl.walkCache = lean.data();
    f.walkK = fl.walkK = K;
    plain[AT] = vrc_pixel_walk_record( f, nodes, grid, AT );
    lean[AT] = vrc_pixel_walk_record( fl, nodes, grid, AT );
    bad = bad || plain[AT] != counted || lean[AT] != counted;

    std::vector< vrc_f4 > lut;
    std::vector< vrc_f2 > lut2;
    for( int tab = 0; tab < 6 && !bad; ++tab )
    {
        const float alpha = ( tab & 1 ) ? 1.0f : 0.05f;
        const bool coloured = tab >= 2, onto = tab >= 4;
        make_tables( alpha, coloured, 4.0f, lut, lut2 );
        const vrc_f4* const t4 = coloured ? lut.data() : reinterpret_cast< const vrc_f4* >( lut2.data() );
        const uint8_t* const atlas = sc.atlas.data();
        /* the walk: plain assignments */
        st_buffer want = st_fresh( onto, tab );
        vrc_frame fw = f;
        fw.clearFirst = onto ? 0u : 1u;
        fw.walkCache = nullptr;
        fw.walkPlane = fw.walkK = 0u;
        if( coloured )
            vrc_pixel_grid_dda< false, true, true, VRC_MODE_TABLE, uint8_t, VRC_GROUP >( fw, nodes, grid, atlas, t4, cls, want.px.data(),
                                                                                         ST_PX, ST_PY, want.samples, AT );
        else
            vrc_pixel_grid_dda< false, true, true, VRC_MODE_GREY, uint8_t, 14 >( fw, nodes, grid, atlas, t4, cls, want.px.data(), ST_PX,
                                                                                 ST_PY, want.samples, AT );
        /* what the walk itself must have left: nothing but pixel ST_POS touched; a ray without visits cleared or kept */
        const st_buffer before = st_fresh( onto, tab );
        for( uint32_t i = 0; i < ST_W * ST_H; ++i )
            bad = bad || ( i != ST_POS && std::memcmp( &want.px[i], &before.px[i], sizeof( vrc_f4 ) ) != 0 );
        if( counted == 0u )
        {
            const vrc_f4 zero = { 0.f, 0.f, 0.f, 0.f };
            bad = bad || std::memcmp( &want.px[ST_POS], onto ? &before.px[ST_POS] : &zero, sizeof( vrc_f4 ) ) != 0;
            tally[5] += onto ? 0u : 1u;
        }
        for( uint32_t through = 0u; through < 2u && !bad; ++through )
        {
            vrc_frame a = f, b = fl, u = fl;
            a.clearFirst = b.clearFirst = u.clearFirst = onto ? 0u : 1u;
            a.storeThrough = b.storeThrough = u.storeThrough = through;
            u.walkLean = VRC_WALK_LEAN_UNIFORM;
            st_buffer ra = st_fresh( onto, tab ), rb = st_fresh( onto, tab ), ru = st_fresh( onto, tab );
            if( coloured )
            {
                vrc_pixel_walk_replay< true, VRC_MODE_TABLE, VRC_GROUP >( a, nodes, atlas, t4, cls, ra.px.data(), ST_PX, ST_PY, ra.samples, AT );
                vrc_pixel_walk_replay_lean< true, VRC_MODE_TABLE, VRC_GROUP >( b, nodes, atlas, t4, cls, rb.px.data(), ST_PX, ST_PY,
                                                                                rb.samples, AT );
                if( uniformScene )
                    vrc_pixel_walk_replay_lean< true, VRC_MODE_TABLE, VRC_GROUP, true >( u, nullptr, nullptr, t4, cls, ru.px.data(), ST_PX,
                                                                                          ST_PY, ru.samples, AT );
            }
            else
            {
                vrc_pixel_walk_replay< true, VRC_MODE_GREY, 14 >( a, nodes, atlas, t4, cls, ra.px.data(), ST_PX, ST_PY, ra.samples, AT );
                vrc_pixel_walk_replay_lean< true, VRC_MODE_GREY, 14 >( b, nodes, atlas, t4, cls, rb.px.data(), ST_PX, ST_PY, rb.samples, AT );
                if( uniformScene )
                    vrc_pixel_walk_replay_lean< true, VRC_MODE_GREY, 14, true >( u, nullptr, nullptr, t4, cls, ru.px.data(), ST_PX, ST_PY,
                                                                                  ru.samples, AT );
            }
            bad = bad || !st_same( ra, want ) || !st_same( rb, want ) || ( uniformScene && !st_same( ru, want ) );
            tally[3] += uniformScene ? 3u : 2u;
            tally[4] += uniformScene ? 1u : 0u;
        }
    }
    ++tally[0];
    tally[counted == 0u ? 1 : 2] += 1u;
    tally[6] += bad ? 1u : 0u;
    return !bad;
}

/* `count` rays per (grid, scene form, variant, kind).  out: STORE_TALLY numbers.  Returns the mismatches. */
extern "C" uint64_t store_through_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const int grids[3][3] = { { 1, 1, 1 }, { 4, 4, 4 }, { 4, 3, 2 } };
    std::memset( out, 0, sizeof( uint64_t ) * STORE_TALLY );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int s = 0; s < 3; ++s )
        for( int uniformScene = 0; uniformScene < 2; ++uniformScene )
        {
            scene sc;
            build_scene( sc, grids[s][0], grids[s][1], grids[s][2] );
            if( !sc.t.gridOk || sc.t.clamp )
                return ~0ull;
            if( uniformScene )
                make_every_brick_uniform( sc );
            g_nodes = &sc.t.nodes; /* (the included harness's visit hook) */
            for( uint32_t variant = 0; variant < 2u; ++variant )
                for( int kind = 0; kind < KINDS; ++kind )
                    for( uint32_t i = 0; i < count; ++i )
                        (void)st_one_ray( sc, uniformScene != 0, g, kind, variant, out );
        }
    return out[6];
}

/* vrc_plan_store_through over an options struct at its defaults but for the option itself */
extern "C" int store_through_plan( int64_t option, int64_t walkUsed, uint32_t width, uint32_t height )
{
    vrc_options o;
    o.storeThrough = option;
    return vrc_plan_store_through( o, walkUsed, width, height ) ? 1 : 0;
}
extern "C" int64_t store_through_default() { return vrc_options().storeThrough; }

#if defined( STORE_THROUGH_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 10u;
    uint64_t out[STORE_TALLY];
    const uint64_t bad = store_through_run( 12345u, count, out );
    /* the decision's edges, once */
    const int plan = store_through_plan( 1, 4, 16384u, 16383u ) == 1 && store_through_plan( 1, 4, 16384u, 16384u ) == 0 &&
                             store_through_plan( 0, 4, 8u, 8u ) == 0 && store_through_plan( 1, 3, 8u, 8u ) == 0
                         ? 0
                         : 1;
    std::printf( "rays %llu none %llu lists %llu replays %llu uniform %llu cleared %llu mismatches %llu plan %d\n",
                 (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
                 (unsigned long long)out[3], (unsigned long long)out[4], (unsigned long long)out[5],
                 (unsigned long long)bad, plan );
    return bad == 0 && plan == 0 ? 0 : 1;
}
#endif
