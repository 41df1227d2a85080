/*
 * walk_plan_harness.cpp -- the host logic of the walk cache and the ray cache in libre_amd/csrc/vrc_plan.h (vrc_walk_open,
 * vrc_walk_decide, vrc_walk_commit, vrc_walk_launched, vrc_walk_forget; vrc_plan_ray_cache, vrc_ray_stored,
 * vrc_ray_forget) against the text of vrc_api.hip they replaced, for tests/test_walk_plan_cpu.py.
 * TEST INFRASTRUCTURE ONLY.
 *
 * namespace before holds verbatim copies (between BEGIN / END markers: the test counts their lines) of render_ray_cache
 * and render_walk_cache as they stood before the rules moved, of the three transitions of render_march with the line
 * that makes the ray cache valid, and of the outside resets.  namespace after holds the callers as vrc_api.hip has them
 * now (between BEGIN NEW / END NEW markers: the test holds them to vrc_api.hip's own text).  Both run over stand-in
 * structs with the field names the context has on their side.  A stand-in frame carries an id for the constants
 * ray_constants_equal compares and one for those walk_constants_equal adds, and the copies of the two compare the ids.  ctx_grow, hipEventQuery and the launches are inputs --
 * succeed or fail, ready or not -- and every call of theirs is counted.
 *
 * The subject is the state machine: both sides go through the same generated SEQUENCES of renders, with option changes
 * and outside resets between them.  After every step they must agree on the return code, the read-backs, the calls made
 * (polls, allocations and their words, launches), and the whole remembered state; after every step that returned VRC_OK
 * also on every frame field either side writes (the frame of a refused vrc_render is a local that nothing reads).
 * The tallies say what the sequences reached; the test asserts each is nonzero.
 *
 * Built as a shared library and, with -DWALK_PLAN_MAIN, as a stand-alone program for the sanitizer run.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../libre_amd/csrc/vrc_plan.h"

namespace
{
/* ---- stand-ins both sides share ---- */
enum hipError_t
{
    hipSuccess = 0,
    hipErrorNotReady = 600,
    hipErrorLaunchFailure = 719
};
typedef void* hipStream_t;
typedef void* hipEvent_t;
enum
{
    hipEventDisableTiming = 2,
    hipMemcpyDeviceToHost = 2
};
#define VRC_WALK_LEAN_INDEX_BITS 20u
#define VRC_TILE_W 8u
#define VRC_TILE_H 8u
#define VRC_RAY_CACHE_PLANES 10u
#define VRC_FIRST_VISIT_ENTRIES 256u
#define VRC_FIRST_VISIT_ROWS 64u
struct vrc_f4
{
    float x, y, z, w;
};
struct vrc_walk_count
{
    uint32_t longest, notLean;
    unsigned long long visits, gathers;
};

/* the fields of vrc_frame the text reads and writes, and two ids for all the constants it compares: of the ray's, and
 * of what the walk reads beside the ray */
struct vrc_frame
{
    int id, walkId;
    uint32_t width, height, nodeCount, clearFirst;
    float stepSize;
    const uint32_t* slotInfo;
    uint32_t rayMode, rayCachePlane;
    const float* rayCache;
    const uint32_t* walkCache;
    uint32_t walkPlane, walkK, walkLean, walkSlots, storeThrough, leanFree;
    const void* firstVisit;
    const uint32_t* walkResolved;
};
bool ray_constants_equal( const vrc_frame& a, const vrc_frame& b ) { return a.id == b.id; }
bool walk_constants_equal( const vrc_frame& a, const vrc_frame& b ) { return ray_constants_equal( a, b ) && a.walkId == b.walkId; }

struct vrc_raycast_args
{
    vrc_frame frame;
    bool greyTable, replayEligible;
    int depthSplit, ertParts;
};
bool vrc_walk_replay_eligible( const vrc_raycast_args& a ) { return a.replayEligible; }
/* (a step of one half is "one vrc_exact_step_count counts") */
bool vrc_exact_step_count( float step, float, uint32_t* ) { return step == 0.5f; }
struct vrc_pool
{
    struct
    {
        size_t n;
        size_t size() const { return n; }
    } resident;
    uint64_t uploadGen;
};
struct pass_base
{
    vrc_pool* pool;
    vrc_mode mode;
    vrc_form form;
    bool sameNodes;
    size_t plane;
    vrc_raycast_args a;
};

/* what a step's calls find, and what they leave */
enum
{
    SITE_RAY = 0,
    SITE_LISTS,
    SITE_RESOLVED,
    SITES
};
enum
{
    LAUNCH_COUNT = 0,
    LAUNCH_RECORD,
    LAUNCH_RESOLVE,
    LAUNCH_TABLE,
    LAUNCH_MARCH,
    LAUNCHES
};
struct call_log
{
    uint32_t polls, mallocs, eventRecords;
    uint32_t growCalls[SITES], growMade[SITES], growFailed[SITES];
    uint64_t growWords[SITES];
    uint32_t launches[LAUNCHES];
    uint32_t launchK[LAUNCHES], launchLean[LAUNCHES], launchPlane[LAUNCHES]; /* vrc_frame::walkK, walkLean, walkPlane as a launch found them */
};
struct side_io
{
    call_log log;
    void** site[SITES];   /* where the three grown pointers live on this side */
    vrc_walk_count hMax;  /* the pinned copy of the count's answer */
};
side_io* g_io;
bool g_eventReady, g_allocFails;
int g_launchFails; /* LAUNCH_*, or -1 */
char g_device[16]; /* what the device pointers point to */

int fail( int code, const char* ) { return code; }
#define VRC_HIP_CHECK( expr )              \
    do                                     \
    {                                      \
        const hipError_t _e = ( expr );    \
        if( _e != hipSuccess )             \
            return fail( VRC_EHIP, #expr ); \
    } while( 0 )
#define VRC_TRY( call ) \
    do { const int _rc = ( call ); if( _rc != VRC_OK ) return _rc; } while( 0 )

template< class T > hipError_t hipMalloc( T** p, size_t )
{
    ++g_io->log.mallocs;
    *p = reinterpret_cast< T* >( g_device );
    return hipSuccess;
}
hipError_t hipHostMalloc( vrc_walk_count** p, size_t )
{
    ++g_io->log.mallocs;
    *p = &g_io->hMax;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags( hipEvent_t* e, int )
{
    ++g_io->log.mallocs;
    *e = g_device;
    return hipSuccess;
}
hipError_t hipEventQuery( hipEvent_t )
{
    ++g_io->log.polls;
    return g_eventReady ? hipSuccess : hipErrorNotReady;
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipEventRecord( hipEvent_t, hipStream_t )
{
    ++g_io->log.eventRecords;
    return hipSuccess;
}
hipError_t hipMemsetAsync( void*, int, size_t, hipStream_t ) { return hipSuccess; }
hipError_t hipMemcpyAsync( void*, const void*, size_t, int, hipStream_t ) { return hipSuccess; }
hipError_t launched( int which, const vrc_frame* f = nullptr )
{
    ++g_io->log.launches[which];
    if( f )
    {
        g_io->log.launchK[which] = f->walkK;
        g_io->log.launchLean[which] = f->walkLean;
        g_io->log.launchPlane[which] = f->walkPlane;
    }
    return g_launchFails == which ? hipErrorLaunchFailure : hipSuccess;
}
hipError_t vrc_launch_walk_record( const vrc_raycast_args& a, vrc_walk_count* result, hipStream_t )
{
    return launched( result ? LAUNCH_COUNT : LAUNCH_RECORD, &a.frame );
}
hipError_t vrc_launch_walk_resolve( const vrc_frame& f, uint32_t*, hipStream_t ) { return launched( LAUNCH_RESOLVE, &f ); }
hipError_t vrc_launch_build_first_visit( const vrc_f4*, void*, bool, hipStream_t ) { return launched( LAUNCH_TABLE ); }
hipError_t launch_march() { return launched( LAUNCH_MARCH ); }

/* ctx_grow as the context's: nothing to do where the capacity suffices; else everything is freed and allocated anew,
 * and after a failure the pointers are NULL and the capacity is 0 */
struct vrc_grown
{
    void** p;
    size_t elemBytes;
    template< class T > vrc_grown( T*& q, size_t elem = sizeof( T ) ) : p( reinterpret_cast< void** >( &q ) ), elemBytes( elem ) {}
};
template< class Ctx > int ctx_grow( Ctx*, size_t& cap, size_t n, size_t want, std::initializer_list< vrc_grown > bufs )
{
    const vrc_grown& b = *bufs.begin();
    int site = 0;
    while( site < SITES - 1 && g_io->site[site] != b.p )
        ++site;
    ++g_io->log.growCalls[site];
    g_io->log.growWords[site] = n;
    if( n <= cap )
        return VRC_OK;
    *b.p = nullptr;
    cap = 0;
    if( g_allocFails )
    {
        ++g_io->log.growFailed[site];
        return fail( VRC_EHIP, "hipMalloc" );
    }
    ++g_io->log.growMade[site];
    *b.p = g_device;
    cap = want;
    return VRC_OK;
}

/* ---------------------------------------------------------------------------------------- */
namespace before
{
/* BEGIN STRUCTS BLOCK */
struct vrc_walk_cache
{
    enum { IDLE = 0, COUNTING = 1, VALID = 2 };
    int state = IDLE;
    uint32_t* dLists = nullptr;
    size_t words = 0;               /* allocated */
    uint32_t k = 0;                 /* visits per ray the planes hold */
    vrc_walk_count* dMax = nullptr; /* the count pass's result, and its pinned copy */
    vrc_walk_count* hMax = nullptr;
    hipEvent_t ev = nullptr;
    vrc_frame frame;
    vrc_frame prevFrame;
    bool prevSet = false;
    uint64_t prevGen = 0, gen = 0;
    const uint32_t* slotInfo = nullptr;
    int64_t used = 0; /* VRC_OPT_WALK_CACHE_USED */
    /* the form of the lists (vrc_core.h: vrc_frame::walkLean).  leanAsked: what the host saw when the count pass went
     * out -- a step that vrc_exact_step_count counts, a pool whose slot indices fit the word -- and so what that pass was
     * asked to check; part of what the lists are valid for.  lean: the form the record pass wrote.  leanUsed:
     * VRC_OPT_WALK_LEAN_USED */
    bool leanAsked = false, lean = false;
    int64_t leanUsed = 0;
    /* the uniform-only replay (VRC_OPT_WALK_UNIFORM_ONLY).  gathers: what the count pass of the lists in the planes
     * said of the slot words it read, those of gen and slotInfo -- compared for this whatever VRC_OPT_WALK_CACHE
     * says, because at VRC_WALK_CACHE_ALWAYS the lists outlive an upload and that answer does not.  uniformUsed:
     * VRC_OPT_WALK_UNIFORM_ONLY_USED */
    unsigned long long gathers = 0;
    int64_t uniformUsed = 0;
    int64_t throughUsed = 0; /* VRC_OPT_STORE_THROUGH_USED */
    int64_t freeUsed = 0;    /* VRC_OPT_LEAN_FREE_MARCH_USED */
    /* the resolved visit words of the uniform-only replay (VRC_OPT_WALK_RESOLVED; vrc_core.h: vrc_walk_resolved_word): k
     * planes beside the lists, built from them and from the slot words by the first frame that is handed the
     * uniform-only instance without them.  resolvedValid: the planes hold the words of the lists in dLists as recorded
     * (a record pass ends it) under the uploads resolvedGen and the array resolvedSlotInfo; a frame that finds another
     * of the three takes the list words and drops the planes.  resolvedUsed: VRC_OPT_WALK_RESOLVED_USED */
    uint32_t* dResolved = nullptr;
    size_t resolvedWords = 0; /* allocated */
    bool resolvedValid = false;
    uint64_t resolvedGen = 0;
    const uint32_t* resolvedSlotInfo = nullptr;
    int64_t resolvedUsed = 0;
};

/* the first-visit table of the lean replay (VRC_OPT_FIRST_VISIT_TABLE; vrc_core.h: vrc_first_visit_row).  It depends on
 * the classified table alone -- transfer function, opacity correction -- and on the form the frame marches, not on the
 * view, the volume or the lists.  dTable: allocated by the first build, for the four-float form.  gen, grey: the
 * generation (vrc_ctx::lutGen) and form it was built for (gen 0: never).  prevGen: the generation the vrc_render before
 * rendered with (0: none).  used: VRC_OPT_FIRST_VISIT_TABLE_USED */
struct vrc_first_visit
{
    void* dTable = nullptr;
    uint64_t gen = 0, prevGen = 0;
    bool grey = false;
    int64_t used = 0;
};
/* END STRUCTS BLOCK */

/* the fields of the context the text reads and writes, under their names */
struct vrc_ctx
{
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    vrc_options opt;
    vrc_f4* dLut = nullptr;
    uint64_t lutGen = 0;
    vrc_first_visit first;
    float* dRayCache = nullptr;
    size_t dRayCacheCap = 0;
    bool rayCacheValid = false;
    bool rayPrevSet = false;
    vrc_frame rayPrevFrame;
    int64_t rayCacheUsed = 0;
    vrc_walk_cache walk;
    bool rayLod = false;
    uint64_t waitedPoolUid = 0, waitedGen = 0;
    bool tileOrderValid = false;
};
struct render_pass : pass_base
{
    bool walkCount, walkRecord;
    bool walkResolve;
};

/* BEGIN RAY BLOCK */
static int render_ray_cache( vrc_ctx* c, render_pass& p )
{
    vrc_frame& f = p.a.frame;
    const size_t plane = p.plane;
    c->rayCacheUsed = 0;
    const bool eligible = c->opt.rayCache && p.form.useDda && !p.form.useLds && !c->rayLod && !p.mode.mip && !p.form.glSuper &&
                          !p.a.depthSplit && p.a.ertParts <= 1 && VRC_TILE_W * VRC_TILE_H == 64u &&
                          plane * VRC_RAY_CACHE_PLANES <= 0xFFFFFFFFull; /* (32-bit word offsets in the kernel) */
    if( !eligible )
        c->rayCacheValid = c->rayPrevSet = false;
    else
    {
        const bool same = c->rayPrevSet && ray_constants_equal( c->rayPrevFrame, f );
        if( !same )
            c->rayCacheValid = false;
        else if( !c->rayCacheValid )
        {
            VRC_TRY( ctx_grow( c, c->dRayCacheCap, plane, plane, { { c->dRayCache, VRC_RAY_CACHE_PLANES * sizeof( float ) } } ) );
            c->rayCacheUsed = VRC_RAY_STORE; /* (valid once the march is on the stream: render_march) */
        }
        else
            c->rayCacheUsed = VRC_RAY_LOAD;
        std::memcpy( &c->rayPrevFrame, &f, sizeof( f ) );
        c->rayPrevSet = true;
    }
    f.rayMode = (uint32_t)c->rayCacheUsed;
    f.rayCache = c->rayCacheUsed ? c->dRayCache : nullptr;
    f.rayCachePlane = c->rayCacheUsed ? (uint32_t)plane : 0u;
    return VRC_OK;
}
/* END RAY BLOCK */

/* BEGIN WALK BLOCK */
static int render_walk_cache( vrc_ctx* c, render_pass& p )
{
    vrc_walk_cache& w = c->walk;
    vrc_frame& f = p.a.frame;
    const size_t plane = p.plane;
    w.used = 0;
    w.leanUsed = 0;
    w.uniformUsed = 0;
    w.throughUsed = 0;
    w.freeUsed = 0;
    f.walkCache = nullptr;
    f.walkPlane = f.walkK = 0u;
    f.walkLean = f.walkSlots = 0u;
    p.walkCount = p.walkRecord = false;
    /* the form of the lists.  A lean list (vrc_core.h: vrc_frame::walkLean) holds every visit's step count and slot
     * index in one word of 12 + 20 bits.  What the host can see of that: the step is one vrc_exact_step_count counts
     * (its own test, asked here with a travel that passes it), and the pool's slot indices fit.  The rest -- no
     * visit whose count is inexact or takes more than 12 bits -- the count pass reports with the count */
    uint32_t one = 0u;
    const size_t nSlots = p.pool->resident.size();
    const bool leanAsked = vrc_exact_step_count( f.stepSize, f.stepSize, &one ) && nSlots >= 1u &&
                           nSlots < ( (size_t)1u << VRC_WALK_LEAN_INDEX_BITS );
    const auto fits = [&]( uint32_t k ) { /* the planes of k visits: 32-bit word offsets in the kernels, and the budget */
        const unsigned long long words = ( 1ull + 4ull * k ) * plane;
        return words <= 0xFFFFFFFFull && words * sizeof( uint32_t ) <= (unsigned long long)c->opt.walkBudget;
    };
    const bool eligible = c->opt.walkCache && c->rayCacheUsed == VRC_RAY_LOAD && vrc_walk_replay_eligible( p.a ) &&
                          f.nodeCount > 0u && plane > 0u && fits( 1u );
    const bool byContent = c->opt.walkCache != VRC_WALK_CACHE_ALWAYS;
    const uint64_t gen = p.pool->uploadGen; /* (compared only where the choice goes by the bricks' content) */
    if( !eligible || ( w.state != vrc_walk_cache::IDLE &&
                       ( !walk_constants_equal( w.frame, f ) || leanAsked != w.leanAsked ||
                         ( byContent && ( w.gen != gen || w.slotInfo != f.slotInfo ) ) ) ) )
        w.state = vrc_walk_cache::IDLE;
    const bool repeats = p.sameNodes && w.prevSet && ( !byContent || w.prevGen == gen ) && walk_constants_equal( w.prevFrame, f );
    std::memcpy( &w.prevFrame, &f, sizeof( f ) );
    w.prevSet = true;
    w.prevGen = gen;
    if( eligible && w.state == vrc_walk_cache::IDLE && repeats )
    {
        if( !w.dMax )
        {
            VRC_HIP_CHECK( hipMalloc( &w.dMax, sizeof( vrc_walk_count ) ) );
            VRC_HIP_CHECK( hipHostMalloc( &w.hMax, sizeof( vrc_walk_count ) ) );
            VRC_HIP_CHECK( hipEventCreateWithFlags( &w.ev, hipEventDisableTiming ) );
        }
        p.walkCount = true;
        w.leanAsked = leanAsked;
        w.gen = gen;
        w.slotInfo = f.slotInfo;
        w.used = 1;
    }
    else if( eligible && w.state == vrc_walk_cache::COUNTING )
    {
        w.used = 2;
        const hipError_t q = hipEventQuery( w.ev );
        if( q == hipErrorNotReady )
            (void)hipGetLastError(); /* (not an error: nothing later may find it there) */
        else if( q != hipSuccess )
            VRC_HIP_CHECK( q );
        if( q == hipSuccess )
        {
            const uint32_t k = w.hMax->longest > 0u ? w.hMax->longest : 1u;
            if( !fits( k ) )
                w.used = 0; /* over the budget or the offset limit: this view stays on the walk */
            else if( byContent && 2u * w.hMax->gathers > w.hMax->visits )
                w.used = 0; /* most visits gather: so does this one */
            else
            {
                const size_t words = ( 1u + 4u * (size_t)k ) * plane;
                VRC_TRY( ctx_grow( c, w.words, words, words, { w.dLists } ) );
                w.k = k;
                w.lean = w.leanAsked && w.hMax->notLean == 0u;
                w.gathers = w.hMax->gathers;
                p.walkRecord = true;
                w.used = 3;
            }
        }
    }
    else if( eligible && w.state == vrc_walk_cache::VALID )
        w.used = 4;
    /* (eligible, IDLE and not a repeat: mode 0 -- the next call counts if it is this one again) */
    if( p.walkRecord || w.used == 4 )
    {
        f.walkCache = w.dLists;
        f.walkPlane = (uint32_t)plane;
        f.walkK = w.k;
        f.walkLean = w.lean ? 1u : 0u;
        f.walkSlots = (uint32_t)nSlots;
        w.leanUsed = ( w.lean && w.used == 4 ) ? 1 : 0;
        /* the uniform-only instance (vrc_kernels_walk.hip): a replayed lean frame none of whose visits gathers --
         * by the count pass of these lists, which is still the answer while the pool has taken no upload and the
         * words are the ones it read.  Where the lists outlive that (VRC_WALK_CACHE_ALWAYS) the frame goes back to
         * the lean instance and keeps them */
        if( w.leanUsed && c->opt.walkUniformOnly && w.gathers == 0ull && w.gen == gen && w.slotInfo == f.slotInfo )
        {
            f.walkLean = VRC_WALK_LEAN_UNIFORM;
            w.uniformUsed = 1;
        }
    }
    else if( p.walkCount )
        f.walkLean = leanAsked ? 1u : 0u; /* (the count pass: check every visit) */
    /* how the replay stores its pixels (vrc_core.h: vrc_store_pixel): set behind prevFrame's copy, and not among what
     * walk_constants_equal compares -- the lists do not depend on it */
    w.throughUsed = vrc_plan_store_through( c->opt, w.used, f.width, f.height ) ? 1 : 0;
    f.storeThrough = (uint32_t)w.throughUsed;
    /* ... and whether it takes first visits from the table (vrc_core.h: vrc_first_visit_row), set behind the same
     * copies for the same reason.  The table is built here, on the stream behind the classified table it reads and in
     * front of the march's timing pair: no march, not timed, not counted as a launch */
    vrc_first_visit& fv = c->first;
    const bool grey = p.a.greyTable;
    vrc_first_visit_facts k = { w.used, f.walkLean, f.clearFirst != 0u, p.mode.classify,
                                fv.gen != 0u && fv.gen == c->lutGen && fv.grey == grey };
    if( vrc_plan_first_visit_build( c->opt, k, fv.prevGen == c->lutGen ) )
    {
        if( !fv.dTable )
            VRC_HIP_CHECK( hipMalloc( &fv.dTable, (size_t)VRC_FIRST_VISIT_ENTRIES * VRC_FIRST_VISIT_ROWS * sizeof( vrc_f4 ) ) );
        VRC_HIP_CHECK( vrc_launch_build_first_visit( c->dLut, fv.dTable, grey, c->stream ) );
        fv.gen = c->lutGen;
        fv.grey = grey;
        k.current = true;
    }
    fv.prevGen = c->lutGen;
    fv.used = vrc_plan_first_visit( c->opt, k ) ? 1 : 0;
    f.firstVisit = fv.used ? fv.dTable : nullptr;
    /* ... and whether a visit that cannot reach the exit threshold marches without the test (vrc_core.h:
     * vrc_march_uniform_free): behind the same copies, for the same reason */
    w.freeUsed = vrc_plan_lean_free_march( c->opt, w.used, f.walkLean, p.mode.classify ) ? 1 : 0;
    f.leanFree = (uint32_t)w.freeUsed;
    /* ... and whether the uniform-only instance reads resolved visit words (vrc_core.h: vrc_walk_resolved_word): behind
     * the same copies, for the same reason.  The planes are the lists' as recorded, under the uploads and the slotInfo
     * the frame renders with -- what a frame must find unchanged to be handed VRC_WALK_LEAN_UNIFORM at all -- and count
     * against the budget beside the lists.  The first such frame without them builds them (render_march, behind the
     * pool's uploads and in front of the timing pair: no march); planes of anything else are dropped, and so are they
     * where the frame is not handed that instance because the triple moved */
    p.walkResolve = false;
    const bool uniformOnly = f.walkLean == VRC_WALK_LEAN_UNIFORM;
    if( w.resolvedValid && ( p.walkRecord || ( w.used == 4 && ( w.resolvedGen != gen || w.resolvedSlotInfo != f.slotInfo ) ) ) )
        w.resolvedValid = false;
    const unsigned long long resolvedBytes = ( 1ull + 5ull * w.k ) * plane * sizeof( uint32_t );
    w.resolvedUsed = vrc_plan_walk_resolved( c->opt, uniformOnly, resolvedBytes <= (unsigned long long)c->opt.walkBudget ) ? 1 : 0;
    if( w.resolvedUsed && !w.resolvedValid )
    {
        const size_t words = (size_t)w.k * plane;
        VRC_TRY( ctx_grow( c, w.resolvedWords, words, words, { w.dResolved } ) );
        p.walkResolve = true; /* (valid once render_march has launched the build) */
        w.resolvedGen = gen;
        w.resolvedSlotInfo = f.slotInfo;
    }
    f.walkResolved = w.resolvedUsed ? w.dResolved : nullptr;
    return VRC_OK;
}
/* END WALK BLOCK */

static int render_march( vrc_ctx* c, render_pass& p )
{
    vrc_raycast_args& a = p.a;
    vrc_frame& f = a.frame;
    /* BEGIN MARCH BLOCK */
    if( p.walkCount )
    {
        VRC_HIP_CHECK( hipMemsetAsync( c->walk.dMax, 0, sizeof( vrc_walk_count ), c->stream ) );
        VRC_HIP_CHECK( vrc_launch_walk_record( a, c->walk.dMax, c->stream ) );
        VRC_HIP_CHECK( hipMemcpyAsync( c->walk.hMax, c->walk.dMax, sizeof( vrc_walk_count ), hipMemcpyDeviceToHost, c->stream ) );
        VRC_HIP_CHECK( hipEventRecord( c->walk.ev, c->stream ) );
        std::memcpy( &c->walk.frame, &f, sizeof( f ) );
        c->walk.state = vrc_walk_cache::COUNTING;
        f.walkLean = 0u; /* (asked of the count pass alone) */
    }
    if( p.walkRecord )
    {
        VRC_HIP_CHECK( vrc_launch_walk_record( a, nullptr, c->stream ) );
        c->walk.state = vrc_walk_cache::VALID;
        /* this frame still walks: the march below reads none of the planes */
        f.walkCache = nullptr;
        f.walkPlane = f.walkK = 0u;
        f.walkLean = f.walkSlots = 0u;
    }
    if( p.walkResolve )
    {
        VRC_HIP_CHECK( vrc_launch_walk_resolve( f, c->walk.dResolved, c->stream ) );
        c->walk.resolvedValid = true;
    }
    /* END MARCH BLOCK */
    VRC_HIP_CHECK( launch_march() );
    /* BEGIN STORED BLOCK */
    if( c->rayCacheUsed == VRC_RAY_STORE )
        c->rayCacheValid = true;
    /* END STORED BLOCK */
    return VRC_OK;
}

static void set_stream( vrc_ctx* c, void* s )
{
    /* BEGIN STREAM BLOCK */
    c->stream = s ? (hipStream_t)s : c->ownStream;
    c->waitedPoolUid = c->waitedGen = 0; /* the new stream has waited for no upload */
    c->rayCacheValid = c->rayPrevSet = false; /* (the planes were written on the stream before) */
    c->walk.state = vrc_walk_cache::IDLE;        /* (and so were the lists; a count pass in flight has ended above) */
    /* END STREAM BLOCK */
}

static int set_option( vrc_ctx* c, int option, int64_t value )
{
    switch( option )
    {
    /* BEGIN OPTION BLOCK */
    case VRC_OPT_RAY_CACHE:
        if( c->opt.rayCache != ( value ? 1 : 0 ) )
            c->rayCacheValid = c->rayPrevSet = false;
        c->opt.rayCache = value ? 1 : 0;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE:
        if( value < 0 || value > VRC_WALK_CACHE_ALWAYS )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE is 0 (off), 1 (on) or 2 (on for every view)" );
        if( c->opt.walkCache != value )
            c->walk.state = vrc_walk_cache::IDLE;
        c->opt.walkCache = value;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET:
        if( value < 0 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE_BUDGET is a number of bytes" );
        if( c->opt.walkBudget != value )
            c->walk.state = vrc_walk_cache::IDLE;
        c->opt.walkBudget = value;
        return VRC_OK;
    /* END OPTION BLOCK */
    default: return fail( VRC_EINVAL, "vrc_set_option: unknown option" );
    }
}

static void set_row_map( vrc_ctx* c )
{
    /* BEGIN ROWMAP BLOCK */
    c->tileOrderValid = false;
    c->rayCacheValid = c->rayPrevSet = false;
    c->walk.state = vrc_walk_cache::IDLE; /* (the stream was synchronised above) */
    /* END ROWMAP BLOCK */
}

static void render_nodes( vrc_ctx* c, render_pass& p )
{
    if( p.sameNodes )
        return;
    /* BEGIN NODES BLOCK */
    c->walk.state = vrc_walk_cache::IDLE; /* the walk cache's lists index the node table that is replaced here */
    /* END NODES BLOCK */
}
} // namespace before

/* ---------------------------------------------------------------------------------------- */
namespace after
{
struct vrc_walk_cache
{
    vrc_walk_state s;
    uint32_t* dLists = nullptr;
    size_t words = 0;
    vrc_walk_count* dMax = nullptr;
    vrc_walk_count* hMax = nullptr;
    hipEvent_t ev = nullptr;
    vrc_frame frame;
    vrc_frame prevFrame;
    uint32_t* dResolved = nullptr;
    size_t resolvedWords = 0;
    void* dFirstVisit = nullptr;
};
struct vrc_ctx
{
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    vrc_options opt;
    vrc_f4* dLut = nullptr;
    uint64_t lutGen = 0;
    float* dRayCache = nullptr;
    size_t dRayCacheCap = 0;
    vrc_ray_state ray;
    vrc_frame rayPrevFrame;
    int64_t rayCacheUsed = 0;
    vrc_walk_cache walk;
    vrc_walk_plan walkPlan;
    bool rayLod = false;
};
struct render_pass : pass_base
{
};

/* BEGIN NEW render_ray_cache */
static int render_ray_cache( vrc_ctx* c, render_pass& p )
{
    vrc_frame& f = p.a.frame;
    const size_t plane = p.plane;
    c->rayCacheUsed = 0;
    const bool eligible = c->opt.rayCache && p.form.useDda && !p.form.useLds && !c->rayLod && !p.mode.mip && !p.form.glSuper &&
                          !p.a.depthSplit && p.a.ertParts <= 1 && VRC_TILE_W * VRC_TILE_H == 64u &&
                          plane * VRC_RAY_CACHE_PLANES <= 0xFFFFFFFFull; /* (32-bit word offsets in the kernel) */
    const bool same = eligible && c->ray.prevSet && ray_constants_equal( c->rayPrevFrame, f );
    const uint32_t mode = vrc_plan_ray_cache( c->ray, eligible, same );
    if( mode == VRC_RAY_STORE ) /* (valid once the march is on the stream: render_march) */
        VRC_TRY( ctx_grow( c, c->dRayCacheCap, plane, plane, { { c->dRayCache, VRC_RAY_CACHE_PLANES * sizeof( float ) } } ) );
    c->rayCacheUsed = mode;
    if( eligible )
        std::memcpy( &c->rayPrevFrame, &f, sizeof( f ) );
    f.rayMode = mode;
    f.rayCache = mode ? c->dRayCache : nullptr;
    f.rayCachePlane = mode ? (uint32_t)plane : 0u;
    return VRC_OK;
}
/* END NEW render_ray_cache */

/* BEGIN NEW walk_poll */
static int walk_poll( vrc_walk_cache& w, vrc_walk_counted& n )
{
    const hipError_t q = hipEventQuery( w.ev );
    if( q == hipErrorNotReady )
        (void)hipGetLastError(); /* (not an error: nothing later may find it there) */
    else if( q != hipSuccess )
        VRC_HIP_CHECK( q );
    if( q == hipSuccess )
        n = { true, w.hMax->longest, w.hMax->notLean, w.hMax->visits, w.hMax->gathers };
    return VRC_OK;
}
/* END NEW walk_poll */

/* BEGIN NEW walk_allocate */
static int walk_allocate( vrc_ctx* c, const vrc_walk_plan& pl, bool grey, vrc_walk_reached& reached )
{
    vrc_walk_cache& w = c->walk;
    reached = VRC_WALK_REACHED_NOTHING;
    if( pl.count && !w.dMax )
    {
        VRC_HIP_CHECK( hipMalloc( &w.dMax, sizeof( vrc_walk_count ) ) );
        VRC_HIP_CHECK( hipHostMalloc( &w.hMax, sizeof( vrc_walk_count ) ) );
        VRC_HIP_CHECK( hipEventCreateWithFlags( &w.ev, hipEventDisableTiming ) );
    }
    if( pl.record )
        VRC_TRY( ctx_grow( c, w.words, pl.listWords, pl.listWords, { w.dLists } ) );
    reached = VRC_WALK_REACHED_LISTS;
    if( pl.firstVisitBuild )
    {
        if( !w.dFirstVisit )
            VRC_HIP_CHECK( hipMalloc( &w.dFirstVisit, (size_t)VRC_FIRST_VISIT_ENTRIES * VRC_FIRST_VISIT_ROWS * sizeof( vrc_f4 ) ) );
        VRC_HIP_CHECK( vrc_launch_build_first_visit( c->dLut, w.dFirstVisit, grey, c->stream ) );
    }
    reached = VRC_WALK_REACHED_TABLE;
    if( pl.resolveBuild )
        VRC_TRY( ctx_grow( c, w.resolvedWords, pl.resolvedWords, pl.resolvedWords, { w.dResolved } ) );
    reached = VRC_WALK_REACHED_ALL;
    return VRC_OK;
}
/* END NEW walk_allocate */

/* BEGIN NEW render_walk_cache */
static int render_walk_cache( vrc_ctx* c, render_pass& p )
{
    vrc_walk_cache& w = c->walk;
    vrc_frame& f = p.a.frame;
    uint32_t one = 0u;
    const size_t nSlots = p.pool->resident.size();
    vrc_walk_facts k;
    k.eligibleSoFar = c->opt.walkCache && c->rayCacheUsed == VRC_RAY_LOAD && vrc_walk_replay_eligible( p.a ) &&
                      f.nodeCount > 0u && p.plane > 0u;
    k.leanAsked = vrc_exact_step_count( f.stepSize, f.stepSize, &one ) && nSlots >= 1u &&
                  nSlots < ( (size_t)1u << VRC_WALK_LEAN_INDEX_BITS );
    k.sameAsListed = w.s.state != VRC_WALK_IDLE && walk_constants_equal( w.frame, f );
    k.sameAsPrev = w.s.prevSet && walk_constants_equal( w.prevFrame, f );
    k.sameNodes = p.sameNodes;
    k.uploadGen = p.pool->uploadGen;
    k.slotInfo = f.slotInfo;
    k.plane = p.plane;
    k.nSlots = nSlots;
    k.width = f.width;
    k.height = f.height;
    k.clearFirst = f.clearFirst != 0u;
    k.classify = p.mode.classify;
    k.greyTable = p.a.greyTable;
    k.lutGen = c->lutGen;
    vrc_walk_plan pl;
    vrc_walk_counted n;
    int rc = VRC_OK;
    if( vrc_walk_open( c->opt, w.s, k, pl ) )
        rc = walk_poll( w, n );
    std::memcpy( &w.prevFrame, &f, sizeof( f ) );
    vrc_walk_decide( c->opt, w.s, k, n, pl );
    vrc_walk_reached reached = VRC_WALK_REACHED_NOTHING;
    if( rc == VRC_OK )
        rc = walk_allocate( c, pl, k.greyTable, reached );
    vrc_walk_commit( w.s, k, pl, reached, c->walkPlan );
    VRC_TRY( rc );
    f.walkCache = pl.lists() ? w.dLists : nullptr;
    f.walkPlane = pl.lists() ? (uint32_t)p.plane : 0u;
    f.walkK = pl.walkK;
    f.walkLean = pl.walkLean;
    f.walkSlots = pl.walkSlots;
    /* (the riders' fields: behind prevFrame's copy, and not among what walk_constants_equal compares) */
    f.storeThrough = (uint32_t)pl.storeThrough;
    f.firstVisit = pl.firstVisit ? w.dFirstVisit : nullptr;
    f.leanFree = (uint32_t)pl.leanFree;
    f.walkResolved = pl.resolved ? w.dResolved : nullptr;
    return VRC_OK;
}
/* END NEW render_walk_cache */

static int render_march( vrc_ctx* c, render_pass& p )
{
    vrc_raycast_args& a = p.a;
    vrc_frame& f = a.frame;
    /* BEGIN NEW march */
    const vrc_walk_plan& pl = c->walkPlan;
    if( pl.count )
    {
        VRC_HIP_CHECK( hipMemsetAsync( c->walk.dMax, 0, sizeof( vrc_walk_count ), c->stream ) );
        VRC_HIP_CHECK( vrc_launch_walk_record( a, c->walk.dMax, c->stream ) );
        VRC_HIP_CHECK( hipMemcpyAsync( c->walk.hMax, c->walk.dMax, sizeof( vrc_walk_count ), hipMemcpyDeviceToHost, c->stream ) );
        VRC_HIP_CHECK( hipEventRecord( c->walk.ev, c->stream ) );
        std::memcpy( &c->walk.frame, &f, sizeof( f ) );
        vrc_walk_launched( c->walk.s, VRC_WALK_LAUNCHED_COUNT );
        f.walkLean = 0u; /* (asked of the count pass alone) */
    }
    if( pl.record )
    {
        VRC_HIP_CHECK( vrc_launch_walk_record( a, nullptr, c->stream ) );
        vrc_walk_launched( c->walk.s, VRC_WALK_LAUNCHED_RECORD );
        /* this frame still walks: the march below reads none of the planes */
        f.walkCache = nullptr;
        f.walkPlane = f.walkK = 0u;
        f.walkLean = f.walkSlots = 0u;
    }
    if( pl.resolveBuild )
    {
        VRC_HIP_CHECK( vrc_launch_walk_resolve( f, c->walk.dResolved, c->stream ) );
        vrc_walk_launched( c->walk.s, VRC_WALK_LAUNCHED_RESOLVE );
    }
    /* END NEW march */
    VRC_HIP_CHECK( launch_march() );
    /* BEGIN NEW stored */
    if( c->rayCacheUsed == VRC_RAY_STORE )
        vrc_ray_stored( c->ray );
    /* END NEW stored */
    return VRC_OK;
}

/* the outside resets, as vrc_ctx_set_stream, vrc_set_option, vrc_set_row_map and render_nodes make them now */
static void set_stream( vrc_ctx* c, void* s )
{
    c->stream = s ? (hipStream_t)s : c->ownStream;
    vrc_ray_forget( c->ray );
    vrc_walk_forget( c->walk.s );
}
static int set_option( vrc_ctx* c, int option, int64_t value )
{
    switch( option )
    {
    case VRC_OPT_RAY_CACHE:
        if( c->opt.rayCache != ( value ? 1 : 0 ) )
            vrc_ray_forget( c->ray );
        c->opt.rayCache = value ? 1 : 0;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE:
        if( value < 0 || value > VRC_WALK_CACHE_ALWAYS )
            return fail( VRC_EINVAL, "" );
        if( c->opt.walkCache != value )
            vrc_walk_forget( c->walk.s );
        c->opt.walkCache = value;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET:
        if( value < 0 )
            return fail( VRC_EINVAL, "" );
        if( c->opt.walkBudget != value )
            vrc_walk_forget( c->walk.s );
        c->opt.walkBudget = value;
        return VRC_OK;
    default: return fail( VRC_EINVAL, "" );
    }
}
static void set_row_map( vrc_ctx* c )
{
    vrc_ray_forget( c->ray );
    vrc_walk_forget( c->walk.s );
}
static void render_nodes( vrc_ctx* c, render_pass& p )
{
    if( p.sameNodes )
        return;
    vrc_walk_forget( c->walk.s );
}
} // namespace after

/* ---------------------------------------------------------------------------------------- */
/* what both sides must agree on after a step */
struct seen
{
    int rc;
    int64_t used[8]; /* walk cache, lean, uniform-only, store-through, first-visit, free march, resolved; ray cache */
    call_log log;
    /* the remembered state */
    int state;
    uint32_t k;
    bool leanAsked, lean, prevSet, resolvedValid, tableGrey, rayValid, rayPrevSet;
    unsigned long long gathers;
    uint64_t gen, prevGen, resolvedGen, tableGen, tablePrevGen;
    const void *slotInfo, *resolvedSlotInfo;
    int listedId, prevId, rayPrevId; /* the frames kept (-1: none yet) */
    size_t words, resolvedWords, rayCap;
    bool dLists, dMax, hMax, ev, dResolved, dTable, dRay;
    /* the frame (steps that returned VRC_OK) */
    vrc_frame f;
};

void frame_seen( const vrc_frame& f, seen& s )
{
    s.f = vrc_frame();
    s.f.rayMode = f.rayMode;
    s.f.rayCachePlane = f.rayCachePlane;
    s.f.rayCache = f.rayCache ? reinterpret_cast< const float* >( g_device ) : nullptr;
    s.f.walkCache = f.walkCache ? reinterpret_cast< const uint32_t* >( g_device ) : nullptr;
    s.f.walkPlane = f.walkPlane;
    s.f.walkK = f.walkK;
    s.f.walkLean = f.walkLean;
    s.f.walkSlots = f.walkSlots;
    s.f.storeThrough = f.storeThrough;
    s.f.leanFree = f.leanFree;
    s.f.firstVisit = f.firstVisit ? g_device : nullptr;
    s.f.walkResolved = f.walkResolved ? reinterpret_cast< const uint32_t* >( g_device ) : nullptr;
}

struct world_before
{
    before::vrc_ctx c;
    side_io io;
    world_before()
    {
        std::memset( &io, 0, sizeof( io ) );
        io.site[SITE_RAY] = reinterpret_cast< void** >( &c.dRayCache );
        io.site[SITE_LISTS] = reinterpret_cast< void** >( &c.walk.dLists );
        io.site[SITE_RESOLVED] = reinterpret_cast< void** >( &c.walk.dResolved );
        c.walk.frame = vrc_frame();
        c.walk.prevFrame = vrc_frame();
        c.rayPrevFrame = vrc_frame();
        c.walk.frame.id = c.walk.prevFrame.id = c.rayPrevFrame.id = -1;
    }
    void see( seen& s ) const
    {
        const before::vrc_walk_cache& w = c.walk;
        const int64_t u[8] = { w.used, w.leanUsed, w.uniformUsed, w.throughUsed, c.first.used, w.freeUsed, w.resolvedUsed, c.rayCacheUsed };
        std::memcpy( s.used, u, sizeof( u ) );
        s.log = io.log;
        s.state = w.state;
        s.k = w.k;
        s.leanAsked = w.leanAsked;
        s.lean = w.lean;
        s.prevSet = w.prevSet;
        s.resolvedValid = w.resolvedValid;
        s.tableGrey = c.first.grey;
        s.rayValid = c.rayCacheValid;
        s.rayPrevSet = c.rayPrevSet;
        s.gathers = w.gathers;
        s.gen = w.gen;
        s.prevGen = w.prevGen;
        s.resolvedGen = w.resolvedGen;
        s.tableGen = c.first.gen;
        s.tablePrevGen = c.first.prevGen;
        s.slotInfo = w.slotInfo;
        s.resolvedSlotInfo = w.resolvedSlotInfo;
        s.listedId = w.frame.id * 16 + w.frame.walkId;
        s.prevId = w.prevFrame.id * 16 + w.prevFrame.walkId;
        s.rayPrevId = c.rayPrevFrame.id;
        s.words = w.words;
        s.resolvedWords = w.resolvedWords;
        s.rayCap = c.dRayCacheCap;
        s.dLists = w.dLists != nullptr;
        s.dMax = w.dMax != nullptr;
        s.hMax = w.hMax != nullptr;
        s.ev = w.ev != nullptr;
        s.dResolved = w.dResolved != nullptr;
        s.dTable = c.first.dTable != nullptr;
        s.dRay = c.dRayCache != nullptr;
    }
};

struct world_after
{
    after::vrc_ctx c;
    side_io io;
    world_after()
    {
        std::memset( &io, 0, sizeof( io ) );
        io.site[SITE_RAY] = reinterpret_cast< void** >( &c.dRayCache );
        io.site[SITE_LISTS] = reinterpret_cast< void** >( &c.walk.dLists );
        io.site[SITE_RESOLVED] = reinterpret_cast< void** >( &c.walk.dResolved );
        c.walk.frame = vrc_frame();
        c.walk.prevFrame = vrc_frame();
        c.rayPrevFrame = vrc_frame();
        c.walk.frame.id = c.walk.prevFrame.id = c.rayPrevFrame.id = -1;
    }
    void see( seen& s ) const
    {
        const after::vrc_walk_cache& w = c.walk;
        const vrc_walk_plan& pl = c.walkPlan;
        const int64_t u[8] = { pl.used, pl.leanUsed, pl.uniformUsed, pl.storeThrough, pl.firstVisit, pl.leanFree, pl.resolved, c.rayCacheUsed };
        std::memcpy( s.used, u, sizeof( u ) );
        s.log = io.log;
        s.state = w.s.state;
        s.k = w.s.k;
        s.leanAsked = w.s.leanAsked;
        s.lean = w.s.lean;
        s.prevSet = w.s.prevSet;
        s.resolvedValid = w.s.resolvedValid;
        s.tableGrey = w.s.tableGrey;
        s.rayValid = c.ray.valid;
        s.rayPrevSet = c.ray.prevSet;
        s.gathers = w.s.gathers;
        s.gen = w.s.gen;
        s.prevGen = w.s.prevGen;
        s.resolvedGen = w.s.resolvedGen;
        s.tableGen = w.s.tableGen;
        s.tablePrevGen = w.s.tablePrevGen;
        s.slotInfo = w.s.slotInfo;
        s.resolvedSlotInfo = w.s.resolvedSlotInfo;
        s.listedId = w.frame.id * 16 + w.frame.walkId;
        s.prevId = w.prevFrame.id * 16 + w.prevFrame.walkId;
        s.rayPrevId = c.rayPrevFrame.id;
        s.words = w.words;
        s.resolvedWords = w.resolvedWords;
        s.rayCap = c.dRayCacheCap;
        s.dLists = w.dLists != nullptr;
        s.dMax = w.dMax != nullptr;
        s.hMax = w.hMax != nullptr;
        s.ev = w.ev != nullptr;
        s.dResolved = w.dResolved != nullptr;
        s.dTable = w.dFirstVisit != nullptr;
        s.dRay = c.dRayCache != nullptr;
    }
};

bool same_seen( const seen& a, const seen& b )
{
    return a.rc == b.rc && std::memcmp( a.used, b.used, sizeof( a.used ) ) == 0 && std::memcmp( &a.log, &b.log, sizeof( a.log ) ) == 0 &&
           a.state == b.state && a.k == b.k && a.leanAsked == b.leanAsked && a.lean == b.lean && a.prevSet == b.prevSet &&
           a.resolvedValid == b.resolvedValid && a.tableGrey == b.tableGrey && a.rayValid == b.rayValid &&
           a.rayPrevSet == b.rayPrevSet && a.gathers == b.gathers && a.gen == b.gen && a.prevGen == b.prevGen &&
           a.resolvedGen == b.resolvedGen && a.tableGen == b.tableGen && a.tablePrevGen == b.tablePrevGen &&
           a.slotInfo == b.slotInfo && a.resolvedSlotInfo == b.resolvedSlotInfo && a.listedId == b.listedId &&
           a.prevId == b.prevId && a.rayPrevId == b.rayPrevId && a.words == b.words && a.resolvedWords == b.resolvedWords &&
           a.rayCap == b.rayCap && a.dLists == b.dLists && a.dMax == b.dMax && a.hMax == b.hMax && a.ev == b.ev &&
           a.dResolved == b.dResolved && a.dTable == b.dTable && a.dRay == b.dRay &&
           ( a.rc != VRC_OK ||
             ( a.f.rayMode == b.f.rayMode && a.f.rayCachePlane == b.f.rayCachePlane && a.f.rayCache == b.f.rayCache &&
               a.f.walkCache == b.f.walkCache && a.f.walkPlane == b.f.walkPlane && a.f.walkK == b.f.walkK &&
               a.f.walkLean == b.f.walkLean && a.f.walkSlots == b.f.walkSlots && a.f.storeThrough == b.f.storeThrough &&
               a.f.leanFree == b.f.leanFree && a.f.firstVisit == b.f.firstVisit && a.f.walkResolved == b.f.walkResolved ) );
}

/* ---- the tallies: what the sequences reached, by the side of the copied text ---- */
enum
{
    T_STEPS = 0,
    T_BAD,
    T_REFUSED,             /* steps that returned an error */
    T_USED0,               /* VRC_OPT_WALK_CACHE_USED at 0 .. 4 (steps that returned VRC_OK) */
    T_RAY0 = T_USED0 + 5,  /* VRC_OPT_RAY_CACHE_USED at compute, store, load */
    T_ONE = T_RAY0 + 3,    /* lean, uniform-only, store-through, first-visit, free march, resolved: read back 1 */
    T_ZERO = T_ONE + 6,    /* ... and 0 in a replayed frame */
    T_DROP_INELIGIBLE = T_ZERO + 6, /* VALID lists dropped by one cause alone */
    T_DROP_FRAME,
    T_DROP_LEAN_ASKED,
    T_DROP_GEN,
    T_DROP_SLOT_INFO,
    T_KEPT_ALWAYS,         /* VALID lists kept across an upload under VRC_WALK_CACHE_ALWAYS, the uniform-only instance withdrawn */
    T_OVER_BUDGET,         /* a counted view stays on the walk: over the budget or the offset limit */
    T_MOST_GATHER,         /* ... most of its visits gather */
    T_TABLE_DEFERRED,      /* the first-visit build is put off by a frame, and made by the next */
    T_TABLE_OTHER_FORM,    /* the table is rebuilt for the other form under the same generation */
    T_RESOLVED_DROP_RECORD, /* resolved planes dropped by a record pass, the generation alone, slotInfo alone */
    T_RESOLVED_DROP_GEN,
    T_RESOLVED_DROP_SLOT_INFO,
    T_RESOLVED_BUDGET,     /* resolved words refused for the budget alone */
    T_FAIL_LISTS,          /* the lists could not grow, and the next step grew them */
    T_FAIL_RESOLVED,       /* ... the resolved planes */
    T_FAIL_RAY,            /* ... the ray cache's planes */
    T_FAIL_LAUNCH,         /* a launch failed: count, record, resolve, table, march */
    T_RESET_STREAM = T_FAIL_LAUNCH + LAUNCHES, /* each outside reset over IDLE, COUNTING, VALID */
    T_RESET_WALK_OPTION = T_RESET_STREAM + 3,
    T_RESET_BUDGET = T_RESET_WALK_OPTION + 3,
    T_RESET_ROW_MAP = T_RESET_BUDGET + 3,
    T_RESET_NODES = T_RESET_ROW_MAP + 3,
    T_RAY_FORGOT_STREAM = T_RESET_NODES + 3, /* valid ray planes forgotten by each path */
    T_RAY_FORGOT_OPTION,
    T_RAY_FORGOT_ROW_MAP,
    T_RAY_FORGOT_INELIGIBLE,
    T_RAY_FORGOT_FRAME,
    T_COUNT
};
const char* const kTallyNames[T_COUNT] = {
    "steps", "bad", "refused", "used0", "used1", "used2", "used3", "used4", "ray_compute", "ray_store", "ray_load",
    "lean_one", "uniform_one", "through_one", "first_visit_one", "free_one", "resolved_one",
    "lean_zero", "uniform_zero", "through_zero", "first_visit_zero", "free_zero", "resolved_zero",
    "drop_ineligible", "drop_frame", "drop_lean_asked", "drop_gen", "drop_slot_info", "kept_always", "over_budget",
    "most_gather", "table_deferred", "table_other_form", "resolved_drop_record", "resolved_drop_gen",
    "resolved_drop_slot_info", "resolved_budget", "fail_lists", "fail_resolved", "fail_ray",
    "fail_launch_count", "fail_launch_record", "fail_launch_resolve", "fail_launch_table", "fail_launch_march",
    "reset_stream_idle", "reset_stream_counting", "reset_stream_valid",
    "reset_walk_option_idle", "reset_walk_option_counting", "reset_walk_option_valid",
    "reset_budget_idle", "reset_budget_counting", "reset_budget_valid",
    "reset_row_map_idle", "reset_row_map_counting", "reset_row_map_valid",
    "reset_nodes_idle", "reset_nodes_counting", "reset_nodes_valid",
    "ray_forgot_stream", "ray_forgot_option", "ray_forgot_row_map", "ray_forgot_ineligible", "ray_forgot_frame" };

uint64_t g_rng;
uint32_t rnd( uint32_t n ) /* splitmix64 */
{
    uint64_t z = ( g_rng += 0x9E3779B97F4A7C15ull );
    z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
    z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull;
    return (uint32_t)( ( ( z ^ ( z >> 31 ) ) >> 33 ) % n );
}
bool one_in( uint32_t n ) { return rnd( n ) == 0u; }

const uint32_t kSlotInfoA[1] = { 0 }, kSlotInfoB[1] = { 0 };
const uint32_t* const kSlotInfo[3] = { kSlotInfoA, kSlotInfoB, nullptr };
const size_t kSlots[4] = { 0u, 1u, ( 1u << 20 ) - 1u, 1u << 20 };
const size_t kPlanes[4] = { 0u, 64u, 1000u, 1u << 20 };
const uint32_t kLongest[4] = { 0u, 1u, 3u, 5000u };
const unsigned long long kGathers[4] = { 0ull, 50ull, 51ull, 100ull }; /* of 100 visits: none, one half, just over, all */
const uint32_t kSize[3][2] = { { 64u, 64u }, { 1u << 14, ( 1u << 14 ) - 1u }, { 1u << 14, 1u << 14 } }; /* below, below, at 2^28 */

/* what a view keeps from step to step unless something moves it */
struct scene
{
    int frameId = 0, walkId = 0;
    size_t plane = 64u, nSlots = 1u;
    uint64_t uploadGen = 1, lutGen = 1;
    int slotInfo = 0, size = 0;
    bool exact = true, classify = false, grey = false;
    int budgetKind = 3;
};

/* the budget kinds: fits nothing; the planes of one visit; the lists of three visits but not the resolved planes beside
 * them; everything */
int64_t budget_of( int kind, size_t plane )
{
    const int64_t p = (int64_t)( plane ? plane : 64u ) * (int64_t)sizeof( uint32_t );
    return kind == 0 ? 0 : kind == 1 ? 5 * p : kind == 2 ? 13 * p : (int64_t)1 << 40;
}

bool fits_restated( int64_t budget, size_t plane, uint64_t k )
{
    const uint64_t words = ( 1u + 4u * k ) * (uint64_t)plane;
    return words <= 0xFFFFFFFFull && words * 4u <= (uint64_t)budget;
}

template< class World, class Pass > void fill_pass( const scene& sc, World& w, Pass& p, vrc_pool& pool, bool sameNodes,
                                                    bool replayEligible, bool nodes, bool rayBit, bool clearFirst )
{
    std::memset( &p.a, 0, sizeof( p.a ) );
    pool.resident.n = sc.nSlots;
    pool.uploadGen = sc.uploadGen;
    p.pool = &pool;
    p.mode = vrc_mode();
    p.mode.classify = sc.classify;
    p.form = vrc_form();
    p.form.useDda = rayBit;
    p.sameNodes = sameNodes;
    p.plane = sc.plane;
    p.a.greyTable = sc.grey;
    p.a.replayEligible = replayEligible;
    vrc_frame& f = p.a.frame;
    f.id = sc.frameId;
    f.walkId = sc.walkId;
    f.width = kSize[sc.size][0];
    f.height = kSize[sc.size][1];
    f.nodeCount = nodes ? 7u : 0u;
    f.clearFirst = clearFirst ? 1u : 0u;
    f.stepSize = sc.exact ? 0.5f : 0.3f;
    f.slotInfo = kSlotInfo[sc.slotInfo];
    w.c.lutGen = sc.lutGen;
}

/* one sequence of `steps` renders through both sides.  Returns the steps at which they differed */
uint64_t run_sequence( uint32_t steps, uint64_t* t )
{
    world_before B;
    world_after A;
    scene sc;
    uint64_t bad = 0;
    /* a sequence starts from any setting of the options the text reads */
    vrc_options o;
    o.walkCache = one_in( 4 ) ? VRC_WALK_CACHE_ALWAYS : 1;
    sc.budgetKind = one_in( 4 ) ? (int)rnd( 4 ) : 3;
    o.walkBudget = budget_of( sc.budgetKind, sc.plane );
    o.walkUniformOnly = one_in( 4 ) ? 0 : 1;
    o.storeThrough = one_in( 4 ) ? 0 : 1;
    o.firstVisitTable = one_in( 4 ) ? 0 : 1;
    o.leanFreeMarch = one_in( 4 ) ? 0 : 1;
    o.walkResolved = one_in( 4 ) ? 0 : 1;
    o.count = one_in( 8 ) ? 1 : 0;
    o.rayCache = 1;
    B.c.opt = o;
    A.c.opt = o;
    int failedSite = -1;     /* the allocation that failed in the step before */
    bool deferred = false;   /* the step before put the first-visit build off */
    for( uint32_t step = 0; step < steps; ++step )
    {
        /* -- between renders: an outside reset, an option -- */
        const int stateNow = B.c.walk.state;
        const bool rayValidNow = B.c.rayCacheValid;
        if( one_in( 24 ) )
        {
            if( one_in( 2 ) )
            {
                before::set_stream( &B.c, nullptr );
                after::set_stream( &A.c, nullptr );
                ++t[T_RESET_STREAM + stateNow];
                t[T_RAY_FORGOT_STREAM] += rayValidNow;
            }
            else
            {
                before::set_row_map( &B.c );
                after::set_row_map( &A.c );
                ++t[T_RESET_ROW_MAP + stateNow];
                t[T_RAY_FORGOT_ROW_MAP] += rayValidNow;
            }
        }
        else if( one_in( 12 ) )
        {
            int option = 0;
            int64_t value = 0;
            switch( rnd( 9 ) )
            {
            case 0:
                option = VRC_OPT_WALK_CACHE;
                value = (int64_t)rnd( 4 ) - 1 + (int64_t)rnd( 2 ); /* -1 .. 3: the refused values too */
                if( value >= 0 && value <= VRC_WALK_CACHE_ALWAYS && value != B.c.opt.walkCache )
                    ++t[T_RESET_WALK_OPTION + stateNow];
                break;
            case 1:
                option = VRC_OPT_WALK_CACHE_BUDGET;
                sc.budgetKind = (int)rnd( 4 );
                value = one_in( 16 ) ? -1 : budget_of( sc.budgetKind, sc.plane );
                if( value >= 0 && value != B.c.opt.walkBudget )
                    ++t[T_RESET_BUDGET + stateNow];
                break;
            case 2:
                option = VRC_OPT_RAY_CACHE;
                value = B.c.opt.rayCache ? 0 : 7;
                t[T_RAY_FORGOT_OPTION] += rayValidNow;
                break;
            case 3: B.c.opt.walkUniformOnly = A.c.opt.walkUniformOnly = 1 - B.c.opt.walkUniformOnly; break;
            case 4: B.c.opt.storeThrough = A.c.opt.storeThrough = 1 - B.c.opt.storeThrough; break;
            case 5: B.c.opt.firstVisitTable = A.c.opt.firstVisitTable = 1 - B.c.opt.firstVisitTable; break;
            case 6: B.c.opt.leanFreeMarch = A.c.opt.leanFreeMarch = 1 - B.c.opt.leanFreeMarch; break;
            case 7: B.c.opt.walkResolved = A.c.opt.walkResolved = 1 - B.c.opt.walkResolved; break;
            default: B.c.opt.count = A.c.opt.count = 1 - B.c.opt.count; break;
            }
            if( option && before::set_option( &B.c, option, value ) != after::set_option( &A.c, option, value ) )
                ++bad;
        }
        else if( !B.c.opt.rayCache && one_in( 2 ) ) /* (a view without the ray cache goes nowhere: not for long) */
        {
            before::set_option( &B.c, VRC_OPT_RAY_CACHE, 1 );
            after::set_option( &A.c, VRC_OPT_RAY_CACHE, 1 );
        }
        /* -- what moves in the view -- */
        if( one_in( 16 ) )
            sc.frameId = (int)rnd( 3 );
        if( one_in( 24 ) )
            sc.walkId = (int)rnd( 3 );
        if( one_in( 32 ) )
            sc.plane = kPlanes[rnd( 4 )];
        if( one_in( 12 ) )
            ++sc.uploadGen;
        if( one_in( 24 ) )
            sc.slotInfo = (int)rnd( 3 );
        if( one_in( 32 ) )
            sc.nSlots = kSlots[rnd( 4 )];
        if( one_in( 32 ) )
            sc.exact = !sc.exact;
        if( one_in( 32 ) )
            sc.classify = !sc.classify;
        if( one_in( 16 ) )
            sc.grey = !sc.grey;
        if( one_in( 10 ) )
            ++sc.lutGen;
        if( one_in( 16 ) )
            sc.size = (int)rnd( 3 );
        const bool sameNodes = !one_in( 24 ), replayEligible = !one_in( 32 ), nodes = !one_in( 48 ), rayBit = !one_in( 32 );
        const bool clearFirst = !one_in( 8 );
        g_eventReady = !one_in( 4 );
        g_allocFails = one_in( 16 );
        g_launchFails = !one_in( 24 ) ? -1 : one_in( 2 ) ? LAUNCH_TABLE : (int)rnd( LAUNCHES ); /* (a build is rare: more of those) */
        vrc_walk_count answer;
        answer.longest = kLongest[one_in( 3 ) ? rnd( 4 ) : 1u + rnd( 2 )];
        answer.notLean = one_in( 4 ) ? 1u : 0u;
        answer.visits = 100ull;
        answer.gathers = one_in( 2 ) ? 0ull : kGathers[rnd( 4 )];

        /* -- the render, the side of the copied text: with what the tallies need noted on the way -- */
        seen sb, sa;
        std::memset( &sb, 0, sizeof( sb ) );
        std::memset( &sa, 0, sizeof( sa ) );
        vrc_pool poolB, poolA;
        before::render_pass pb;
        after::render_pass pa;
        fill_pass( sc, B, pb, poolB, sameNodes, replayEligible, nodes, rayBit, clearFirst );
        fill_pass( sc, A, pa, poolA, sameNodes, replayEligible, nodes, rayBit, clearFirst );
        std::memset( &B.io.log, 0, sizeof( call_log ) );
        std::memset( &A.io.log, 0, sizeof( call_log ) );
        B.io.hMax = answer;
        A.io.hMax = answer;
        g_io = &B.io;
        const before::vrc_walk_cache& w = B.c.walk;
        if( !sameNodes )
            ++t[T_RESET_NODES + w.state];
        before::render_nodes( &B.c, pb );
        const bool rayWasValid = B.c.rayCacheValid;
        const int rayPrevId = B.c.rayPrevSet ? B.c.rayPrevFrame.id : -1;
        sb.rc = before::render_ray_cache( &B.c, pb );
        if( rayWasValid && !B.c.rayCacheValid )
            ++t[B.c.rayPrevSet && rayPrevId != sc.frameId ? T_RAY_FORGOT_FRAME : T_RAY_FORGOT_INELIGIBLE];
        /* (restated from the inputs, not read from either side) */
        const int64_t budget = B.c.opt.walkBudget;
        const bool eligible = B.c.opt.walkCache && B.c.rayCacheUsed == VRC_RAY_LOAD && replayEligible && nodes && sc.plane > 0u &&
                              fits_restated( budget, sc.plane, 1u );
        const bool leanAsked = sc.exact && sc.nSlots >= 1u && sc.nSlots < ( 1u << 20 );
        const int pre = w.state;
        const bool byContent = B.c.opt.walkCache == 1;
        const bool movedFrame = w.frame.id != sc.frameId || w.frame.walkId != sc.walkId, movedLean = leanAsked != w.leanAsked;
        const bool movedGen = w.gen != sc.uploadGen, movedSlotInfo = w.slotInfo != kSlotInfo[sc.slotInfo];
        const bool resolvedWas = w.resolvedValid;
        const bool resolvedGenMoved = w.resolvedGen != sc.uploadGen, resolvedSlotInfoMoved = w.resolvedSlotInfo != kSlotInfo[sc.slotInfo];
        const before::vrc_first_visit fvWas = B.c.first;
        const bool walkRan = sb.rc == VRC_OK;
        if( walkRan )
            sb.rc = before::render_walk_cache( &B.c, pb );
        if( walkRan && pre == before::vrc_walk_cache::VALID )
        {
            const int causes = !eligible + ( eligible && movedFrame ) + ( eligible && movedLean ) +
                               ( eligible && byContent && movedGen ) + ( eligible && byContent && movedSlotInfo );
            if( causes == 1 )
            {
                ++t[!eligible ? T_DROP_INELIGIBLE : movedFrame ? T_DROP_FRAME : movedLean ? T_DROP_LEAN_ASKED : movedGen ? T_DROP_GEN : T_DROP_SLOT_INFO];
                if( w.used == 4 )
                    ++bad; /* (the restatement and the text disagree) */
            }
            if( causes == 0 && !byContent && movedGen && w.used == 4 && w.lean && w.gathers == 0ull && B.c.opt.walkUniformOnly &&
                w.leanUsed == 1 && w.uniformUsed == 0 )
                ++t[T_KEPT_ALWAYS];
            if( causes == 0 && w.used != 4 )
                ++bad;
        }
        if( walkRan && pre == before::vrc_walk_cache::COUNTING && w.state == before::vrc_walk_cache::COUNTING && g_eventReady &&
            w.used == 0 )
        {
            const uint64_t k = answer.longest ? answer.longest : 1u;
            ++t[!fits_restated( budget, sc.plane, k ) ? T_OVER_BUDGET : T_MOST_GATHER];
            if( fits_restated( budget, sc.plane, k ) && !( byContent && 2u * answer.gathers > answer.visits ) )
                ++bad;
        }
        if( walkRan && sb.rc == VRC_OK )
        {
            const bool built = B.io.log.launches[LAUNCH_TABLE] != 0u;
            t[T_TABLE_DEFERRED] += deferred && built;
            t[T_TABLE_OTHER_FORM] += built && fvWas.gen == sc.lutGen && fvWas.grey != sc.grey;
            /* put off: a pass that would take the table, finds it stale, and follows a render of another generation */
            deferred = !built && !B.c.first.used && B.c.opt.firstVisitTable && w.used == 4 && pb.a.frame.walkLean != 0u && clearFirst &&
                       !sc.classify && !B.c.opt.count && fvWas.prevGen != sc.lutGen;
            if( resolvedWas && !w.resolvedValid )
            {
                if( pb.walkRecord )
                    ++t[T_RESOLVED_DROP_RECORD];
                else if( resolvedGenMoved != resolvedSlotInfoMoved )
                    ++t[resolvedGenMoved ? T_RESOLVED_DROP_GEN : T_RESOLVED_DROP_SLOT_INFO];
            }
            if( pb.a.frame.walkLean == VRC_WALK_LEAN_UNIFORM && B.c.opt.walkResolved && !B.c.opt.count && !w.resolvedUsed )
                ++t[T_RESOLVED_BUDGET];
        }
        else
            deferred = false;
        /* an allocation that failed, and the step that makes it good */
        if( failedSite >= 0 && B.io.log.growMade[failedSite] != 0u )
            ++t[failedSite == SITE_LISTS ? T_FAIL_LISTS : failedSite == SITE_RESOLVED ? T_FAIL_RESOLVED : T_FAIL_RAY];
        failedSite = -1;
        for( int s = 0; s < SITES; ++s )
            if( B.io.log.growFailed[s] != 0u )
                failedSite = s;
        if( sb.rc == VRC_OK )
            sb.rc = before::render_march( &B.c, pb );
        if( sb.rc != VRC_OK && failedSite < 0 ) /* (what else fails is a launch) */
            ++t[T_FAIL_LAUNCH + g_launchFails];
        B.see( sb );
        frame_seen( pb.a.frame, sb );

        /* -- the same render through vrc_plan.h -- */
        g_io = &A.io;
        after::render_nodes( &A.c, pa );
        sa.rc = after::render_ray_cache( &A.c, pa );
        if( sa.rc == VRC_OK )
            sa.rc = after::render_walk_cache( &A.c, pa );
        if( sa.rc == VRC_OK )
            sa.rc = after::render_march( &A.c, pa );
        A.see( sa );
        frame_seen( pa.a.frame, sa );

        ++t[T_STEPS];
        if( sb.rc != VRC_OK )
            ++t[T_REFUSED];
        else
        {
            ++t[T_USED0 + sb.used[0]];
            ++t[T_RAY0 + sb.used[7]];
            for( int i = 0; i < 6; ++i )
            {
                t[T_ONE + i] += sb.used[1 + i] == 1;
                t[T_ZERO + i] += sb.used[0] == 4 && sb.used[1 + i] == 0;
            }
        }
        if( !same_seen( sb, sa ) )
        {
            if( t[T_BAD] + bad < 5u )
                std::fprintf( stderr, "step %u: rc %d / %d, used %lld%lld%lld%lld%lld%lld%lld %lld / %lld%lld%lld%lld%lld%lld%lld %lld, state %d / %d\n",
                              step, sb.rc, sa.rc, (long long)sb.used[0], (long long)sb.used[1], (long long)sb.used[2],
                              (long long)sb.used[3], (long long)sb.used[4], (long long)sb.used[5], (long long)sb.used[6],
                              (long long)sb.used[7], (long long)sa.used[0], (long long)sa.used[1], (long long)sa.used[2],
                              (long long)sa.used[3], (long long)sa.used[4], (long long)sa.used[5], (long long)sa.used[6],
                              (long long)sa.used[7], sb.state, sa.state );
            ++bad;
        }
    }
    t[T_BAD] += bad;
    return bad;
}
} // namespace

extern "C" {

int walk_plan_tallies( void ) { return T_COUNT; }
const char* walk_plan_tally_name( int i ) { return i >= 0 && i < T_COUNT ? kTallyNames[i] : ""; }

/* `sequences` sequences of `steps` renders each, seeded; out: T_COUNT tallies.  Returns the steps that differed */
uint64_t walk_plan_run( uint64_t seed, uint64_t sequences, uint32_t steps, uint64_t* out )
{
    for( int i = 0; i < T_COUNT; ++i )
        out[i] = 0;
    g_rng = seed;
    uint64_t bad = 0;
    for( uint64_t s = 0; s < sequences; ++s )
        bad += run_sequence( steps, out );
    return bad;
}
}

#ifdef WALK_PLAN_MAIN
int main( int argc, char** argv )
{
    const uint64_t sequences = argc > 1 ? std::strtoull( argv[1], nullptr, 10 ) : 1000ull;
    const uint32_t steps = argc > 2 ? (uint32_t)std::strtoul( argv[2], nullptr, 10 ) : 64u;
    uint64_t t[T_COUNT];
    const uint64_t bad = walk_plan_run( 2024, sequences, steps, t );
    for( int i = 0; i < T_COUNT; ++i )
        std::printf( "%s %llu\n", kTallyNames[i], (unsigned long long)t[i] );
    return bad ? 1 : 0;
}
#endif
