/*
 * segment_split_harness.cpp -- vrc_brick_segment in two parts (vrc_core.h: vrc_brick_interval + vrc_segment_complete,
 * and vrc_segment_dist for the uniform march) against the one function it was, for tests/test_segment_split_cpu.py.
 * TEST INFRASTRUCTURE ONLY.
 *
 * brick_segment_before is a verbatim copy of vrc_brick_segment as it stood before the split (the developer switch of
 * the biased negative control left out: this harness is built without it).  Generated cases go through both; what must
 * agree: the returned bool, `stop`, and -- where a segment is returned -- the bits of pos, step, dist and tNear; the
 * distance-only completion must return the bits of dist.
 *
 * Built as a shared library (segment_split_run) and, with -DSEGMENT_SPLIT_MAIN, as a stand-alone program for the
 * sanitizer run.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

#include "../../libre_amd/csrc/vrc_core.h"

static bool brick_segment_before( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node& n,
                                  float stepSize, vrc_segment* s, bool* stop )
{
    VRC_STRICT_FP
    const vrc_f3 boxMin = { n.aabbMin[0], n.aabbMin[1], n.aabbMin[2] };
    const vrc_f3 boxMax = { boxMin.x + n.aabbSize[0], boxMin.y + n.aabbSize[1],
                            boxMin.z + n.aabbSize[2] };
    float tNear = 0.0f, tFar = 0.0f;
    *stop = false;
    if( f.variant == VRC_VARIANT_GL )
    {
        /* fragRaycast.glsl:142-177: hit test t0 <= t1; tnear raised to the near plane only;
         * first sample snapped to the lattice tnearGlobal + k*stepSize; clip planes move this
         * brick's interval, after the snap */
        (void)vrc_intersect_box( r.origin, r.invDir, boxMin, boxMax, &tNear, &tFar );
        if( !( tNear <= tFar ) )
            return false;
        if( tNear < r.tNearPlane )
            tNear = r.tNearPlane;
        const float a = tNear - r.tNearGlobal;
        const float residu = a - stepSize * floorf( a / stepSize );
        if( residu > 0.0f )
            tNear += stepSize - residu;
        if( tNear > tFar )
            return false;
        for( uint32_t i = 0; i < f.nPlanes; ++i )
        {
            const vrc_f3 pn = { f.planes[i][0], f.planes[i][1], f.planes[i][2] };
            float rn = vrc_dot( r.dir, pn );
            if( rn == 0.0f )
                rn = VRC_EPSILON;
            const float t = -( vrc_dot( pn, r.origin ) + f.planes[i][3] ) / rn;
            if( rn > 0.0f )
                tNear = fmaxf( tNear, t );
            else
                tFar = fminf( tFar, t );
        }
        if( tNear > tFar )
            return false;
    }
    else
    {
        if( !vrc_intersect_box( r.origin, r.invDir, boxMin, boxMax, &tNear, &tFar ) )
            return false;
        if( tNear > r.tFarGlobal )
        {
            *stop = true;
            return false;
        }
        if( tFar < r.tNearGlobal )
            return false;
        tNear = fmaxf( fmaxf( r.tNearPlane, tNear ), r.tNearGlobal );
        tFar = fminf( tFar, r.tFarGlobal );
        if( tNear > tFar )
            return false;
    }

    const vrc_f3 rayStart = { r.origin.x + r.dir.x * tNear, r.origin.y + r.dir.y * tNear,
                              r.origin.z + r.dir.z * tNear };
    const vrc_f3 rayStop = { r.origin.x + r.dir.x * tFar, r.origin.y + r.dir.y * tFar,
                             r.origin.z + r.dir.z * tFar };
    const vrc_f3 diff = { rayStop.x - rayStart.x, rayStop.y - rayStart.y,
                          rayStop.z - rayStart.z };
    const float d2 = vrc_dot( diff, diff );
    const float invLen = 1.0f / sqrtf( d2 );
    s->pos = rayStart;
    s->step.x = diff.x * invLen * stepSize;
    s->step.y = diff.y * invLen * stepSize;
    s->step.z = diff.z * invLen * stepSize;
    s->dist = sqrtf( d2 );
    s->tNear = tNear;
    return true;
}

/* ---- generated cases ------------------------------------------------------------------------------------------- */
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
    float unit() { return (float)( next() & 0xFFFFFFu ) / 16777216.0f; } /* [0, 1) */
    float in( float a, float b ) { return a + ( b - a ) * unit(); }
    uint32_t below( uint32_t n ) { return next() % n; }
};

static float ulps( float v, int k )
{
    for( int i = 0; i < ( k < 0 ? -k : k ); ++i )
        v = nextafterf( v, k < 0 ? -INFINITY : INFINITY );
    return v;
}

enum
{
    KIND_RANDOM,
    KIND_AXIS,
    KIND_ONE_ULP,
    KIND_CORNER,
    KIND_BEHIND,
    KIND_PAST_FAR,
    KINDS
};

/* tally per kind: [0] cases, [1] segments returned, [2] stop set, [3] intervals of at most one ulp (tFar <= the float
 * after tNear) among the segments returned, [4] mismatches */
struct tally
{
    uint64_t v[KINDS][5];
};

static int same_bits( const void* a, const void* b, size_t n ) { return std::memcmp( a, b, n ) == 0; }

static void one_case( rng& g, int kind, uint32_t variant, uint32_t nPlanes, tally& t )
{
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    f.variant = variant;
    f.nPlanes = nPlanes;
    f.stepSize = ( g.next() & 1u ) ? 1.0f / 256.0f : (float)( 1.0 / 300.0 );
    for( int a = 0; a < 3; ++a )
    {
        f.aabbMin[a] = -0.5f;
        f.aabbMax[a] = 0.5f;
    }
    for( uint32_t i = 0; i < nPlanes; ++i )
    {
        float nrm[3] = { g.in( -1.f, 1.f ), g.in( -1.f, 1.f ), g.in( -1.f, 1.f ) };
        if( g.below( 8 ) == 0 ) /* a plane normal along an axis: its dot product with an axis-parallel ray can be 0 */
        {
            const uint32_t ax = g.below( 3 );
            nrm[ax] = 1.0f;
            nrm[( ax + 1 ) % 3] = nrm[( ax + 2 ) % 3] = 0.0f;
        }
        f.planes[i][0] = nrm[0];
        f.planes[i][1] = nrm[1];
        f.planes[i][2] = nrm[2];
        f.planes[i][3] = g.in( -0.1f, 0.6f );
    }

    /* a brick of a 4^3 grid over the volume (or, one-ulp: a sliver) */
    vrc_dev_node n;
    std::memset( &n, 0, sizeof( n ) );
    int cell[3];
    for( int a = 0; a < 3; ++a )
    {
        cell[a] = (int)g.below( 4 );
        n.aabbMin[a] = -0.5f + 0.25f * (float)cell[a];
        n.aabbSize[a] = 0.25f;
    }

    vrc_ray r;
    std::memset( &r, 0, sizeof( r ) );
    const float eye[3] = { g.in( -0.3f, 0.3f ), g.in( -0.3f, 0.3f ), g.in( 1.2f, 1.8f ) };
    float target[3];
    for( int a = 0; a < 3; ++a )
        target[a] = n.aabbMin[a] + n.aabbSize[a] * g.in( -0.2f, 1.2f ); /* through the brick, or just past it */
    float origin[3] = { eye[0], eye[1], eye[2] };
    if( kind == KIND_AXIS )
    {
        /* the eye straight in front of the target along one axis: two direction components are exactly 0 */
        const uint32_t ax = g.below( 3 );
        for( int a = 0; a < 3; ++a )
            origin[a] = target[a];
        origin[ax] = ( g.next() & 1u ) ? 1.5f : -1.5f;
        if( g.next() & 1u ) /* ... in a face plane of the brick */
            origin[( ax + 1 ) % 3] = target[( ax + 1 ) % 3] = n.aabbMin[( ax + 1 ) % 3];
    }
    else if( kind == KIND_CORNER || kind == KIND_ONE_ULP )
    {
        /* at a corner of the brick, to within a few ulps */
        for( int a = 0; a < 3; ++a )
            target[a] = ulps( n.aabbMin[a] + ( ( g.next() & 1u ) ? n.aabbSize[a] : 0.0f ), (int)g.below( 5 ) - 2 );
        if( kind == KIND_ONE_ULP && ( g.next() & 1u ) )
        {
            /* a sliver of a brick a few ulps thick around the target, across the ray's main axis */
            n.aabbMin[2] = target[2];
            n.aabbSize[2] = ulps( target[2], 1 + (int)g.below( 3 ) ) - target[2];
            for( int a = 0; a < 2; ++a )
                target[a] = n.aabbMin[a] + n.aabbSize[a] * g.unit();
        }
    }
    else if( kind == KIND_BEHIND )
    {
        /* the brick lies behind the eye: the ray points away from it */
        for( int a = 0; a < 3; ++a )
            target[a] = origin[a] + ( origin[a] - target[a] );
    }
    r.origin.x = origin[0];
    r.origin.y = origin[1];
    r.origin.z = origin[2];
    {
        /* as vrc_setup_ray_at: normalised, zero components replaced, reciprocal by division */
        const vrc_f3 d0 = { target[0] - origin[0], target[1] - origin[1], target[2] - origin[2] };
        r.dir = vrc_normalize( d0 );
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
    if( g.below( 16 ) == 0 )
        r.tNearPlane = g.in( 0.9f, 1.6f ); /* a near plane inside the volume */
    if( kind == KIND_PAST_FAR )
    {
        /* the ray's interval ends (a clip plane of vrc_setup_ray_at) in front of, inside or just at the brick */
        float tn = 0.f, tf = 0.f;
        const vrc_f3 bmin = { n.aabbMin[0], n.aabbMin[1], n.aabbMin[2] };
        const vrc_f3 bmax = { bmin.x + n.aabbSize[0], bmin.y + n.aabbSize[1], bmin.z + n.aabbSize[2] };
        (void)vrc_intersect_box( r.origin, r.invDir, bmin, bmax, &tn, &tf );
        const uint32_t how = g.below( 4 );
        r.tFarGlobal = how == 0 ? tn : how == 1 ? ulps( tn, -1 - (int)g.below( 3 ) ) : how == 2 ? tn - g.in( 0.f, 0.3f )
                                                                                                : tn + g.in( 0.f, 0.1f );
    }
    else if( kind == KIND_ONE_ULP && ( g.next() & 1u ) )
    {
        /* the global interval leaves one ulp (or none) of the brick */
        float tn = 0.f, tf = 0.f;
        const vrc_f3 bmin = { n.aabbMin[0], n.aabbMin[1], n.aabbMin[2] };
        const vrc_f3 bmax = { bmin.x + n.aabbSize[0], bmin.y + n.aabbSize[1], bmin.z + n.aabbSize[2] };
        if( vrc_intersect_box( r.origin, r.invDir, bmin, bmax, &tn, &tf ) )
            r.tFarGlobal = ulps( tn, (int)g.below( 3 ) );
    }

    vrc_segment want, got;
    std::memset( &want, 0, sizeof( want ) );
    std::memset( &got, 0, sizeof( got ) );
    bool stopWant = false, stopGot = false, stopIv = false;
    const bool okWant = brick_segment_before( f, r, n, f.stepSize, &want, &stopWant );
    const bool okGot = vrc_brick_segment( f, r, n, f.stepSize, &got, &stopGot );
    vrc_interval iv = { 0.0f, 0.0f };
    const bool okIv = vrc_brick_interval( f, r, n, f.stepSize, &iv, &stopIv );
    bool bad = okWant != okGot || okWant != okIv || stopWant != stopGot || stopWant != stopIv;
    if( okWant && !bad )
    {
        vrc_segment full;
        std::memset( &full, 0, sizeof( full ) );
        vrc_segment_complete( r, iv, f.stepSize, &full );
        const float dist = vrc_segment_dist( r, iv );
        const vrc_segment_from_interval src = { r, iv, f.stepSize };
        const vrc_segment lazyFull = src.full(), lazyDist = src.distOnly();
        bad = !same_bits( &want.pos, &got.pos, sizeof( vrc_f3 ) ) || !same_bits( &want.step, &got.step, sizeof( vrc_f3 ) ) ||
              !same_bits( &want.dist, &got.dist, 4 ) || !same_bits( &want.tNear, &got.tNear, 4 ) ||
              !same_bits( &want.pos, &full.pos, sizeof( vrc_f3 ) ) || !same_bits( &want.step, &full.step, sizeof( vrc_f3 ) ) ||
              !same_bits( &want.dist, &full.dist, 4 ) || !same_bits( &want.tNear, &full.tNear, 4 ) ||
              !same_bits( &want.tNear, &iv.tNear, 4 ) || !same_bits( &want.dist, &dist, 4 ) ||
              !same_bits( &want.pos, &lazyFull.pos, sizeof( vrc_f3 ) ) ||
              !same_bits( &want.step, &lazyFull.step, sizeof( vrc_f3 ) ) || !same_bits( &want.dist, &lazyFull.dist, 4 ) ||
              !same_bits( &want.tNear, &lazyFull.tNear, 4 ) || !same_bits( &want.dist, &lazyDist.dist, 4 ) ||
              !same_bits( &want.tNear, &lazyDist.tNear, 4 );
        if( iv.tFar <= nextafterf( iv.tNear, INFINITY ) )
            ++t.v[kind][3];
    }
    ++t.v[kind][0];
    t.v[kind][1] += okWant ? 1u : 0u;
    t.v[kind][2] += stopWant ? 1u : 0u;
    t.v[kind][4] += bad ? 1u : 0u;
}

/* `count` cases per (kind, variant, plane count): 6 x 2 x 3 combinations.  out: KINDS x 5 tallies.  Returns the
 * number of mismatches. */
extern "C" uint64_t segment_split_run( uint64_t seed, uint32_t count, uint64_t* out )
{
    static const uint32_t planeCounts[3] = { 0u, 1u, 3u };
    tally t;
    std::memset( &t, 0, sizeof( t ) );
    rng g = { seed ? seed : 0x9E3779B97F4A7C15ull };
    for( int kind = 0; kind < KINDS; ++kind )
        for( uint32_t variant = 0; variant < 2; ++variant )
            for( int p = 0; p < 3; ++p )
                for( uint32_t i = 0; i < count; ++i )
                    one_case( g, kind, variant, planeCounts[p], t );
    uint64_t bad = 0;
    for( int kind = 0; kind < KINDS; ++kind )
    {
        for( int k = 0; k < 5; ++k )
            out[kind * 5 + k] = t.v[kind][k];
        bad += t.v[kind][4];
    }
    return bad;
}

extern "C" int segment_split_kinds() { return KINDS; }

#if defined( SEGMENT_SPLIT_MAIN )
int main( int argc, char** argv )
{
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul( argv[1], nullptr, 10 ) : 1000u;
    uint64_t out[KINDS * 5];
    const uint64_t bad = segment_split_run( 12345u, count, out );
    uint64_t cases = 0;
    for( int kind = 0; kind < KINDS; ++kind )
    {
        std::printf( "kind %d: cases %llu segments %llu stop %llu one-ulp %llu mismatches %llu\n", kind,
                     (unsigned long long)out[kind * 5], (unsigned long long)out[kind * 5 + 1],
                     (unsigned long long)out[kind * 5 + 2], (unsigned long long)out[kind * 5 + 3],
                     (unsigned long long)out[kind * 5 + 4] );
        cases += out[kind * 5];
    }
    std::printf( "cases %llu mismatches %llu\n", (unsigned long long)cases, (unsigned long long)bad );
    return bad == 0 ? 0 : 1;
}
#endif
