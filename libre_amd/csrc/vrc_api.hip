/*
 * vrc_api.hip -- implementation of the C ABI declared in include/vrc_hip.h.
 *
 * Host-side logic of the device layer: context + stream, brick atlas (slot grid, free list,
 * pinned staging ring, upload stream + event ordering), classified-table cache, node table
 * and brick-grid construction, kernel selection, timing.  Replaces the host halves of
 * cuda::Renderer::Impl (cuda/Renderer.cu:232-333) and cuda::TexturePool (cuda/TexturePool.cu).
 */
#include "../../include/vrc_hip.h"
#include "vrc_internal.h"
#include "vrc_plan.h"
#include "vrc_tables.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace
{
thread_local std::string g_lastError;

int fail( int code, const std::string& msg )
{
    g_lastError = msg;
    return code;
}

#define VRC_HIP_CHECK( expr )                                                              \
    do                                                                                     \
    {                                                                                      \
        const hipError_t _e = ( expr );                                                    \
        if( _e != hipSuccess )                                                             \
            return fail( VRC_EHIP, std::string( #expr ) + ": " + hipGetErrorString( _e ) ); \
    } while( 0 )

constexpr int kStagingSlots = 8;
constexpr int kNodeStages = 4;
} // namespace

/* the timing events of a context: one pair per raycast launch since the last vrc_get_stats (ring, grows on demand).
 * Shared with the render fences of the pools the context marched from (vrc_pool::RenderFence::keep) */
struct vrc_event_ring
{
    std::vector< std::pair< hipEvent_t, hipEvent_t > > pairs;
    ~vrc_event_ring()
    {
        for( auto& pr : pairs )
        {
            (void)hipEventDestroy( pr.first );
            (void)hipEventDestroy( pr.second );
        }
    }
};

struct vrc_pool
{
    vrc_ctx* ctx = nullptr; /* creating context (device identification only) */
    int device = 0;
    uint64_t uid = 0;       /* unique per process, keys the node-table caches of contexts */
    uint32_t elemBytes = 1; /* of an atlas element = of a voxel as uploaded: 1, 2 or 4 (the float atlas) */
    int voxelType = VRC_VOXEL_UINT8;
    uint32_t xform = VRC_XF_NONE; /* what the upload does to a voxel (vrc_core.h: VRC_XF_*) */
    float rangeShift = 0.0f;      /* signed 8/16-bit voxels are stored offset-binary: + 128 / + 32768 on dataSourceRange */
    uint32_t maxBlock[3] = { 0, 0, 0 };
    uint32_t slotDim[3] = { 0, 0, 0 }; /* maxBlock rounded up to the micro-block size */
    uint32_t slots[3] = { 1, 1, 1 };
    uint32_t atlasDim[3] = { 0, 0, 0 };
    size_t slotBytes = 0, atlasBytes = 0;
    void* dAtlas = nullptr;
    bool bigAtlas = false; /* more than 2^32 voxels */
    /* one uniformity word per slot (vrc_core.h: VRC_SLOT_*), indexed by pool_slot_index.  Device memory only, written
     * on uploadStream alone: cleared with the atlas, zeroed and refilled by every upload next to the voxels it describes,
     * so a march ordered behind lastUpload sees the word of exactly the voxels it would fetch.  No host copy. */
    uint32_t* dSlotInfo = nullptr;
    /* the largest value every slot's last upload stored (vrc_core.h: vrc_frame::slotMax; the MIP march skips bricks by
     * it): the second half of dSlotInfo's allocation, so the same lifetime; zeroed and refilled by every upload with the
     * uniformity word -- same stream, same fences, same lastUpload */
    uint32_t* dSlotMax = nullptr;
    /* ... and the smallest, as a complemented key (vrc_frame::slotMin; the minimum fold skips by it): the third part */
    uint32_t* dSlotMin = nullptr;
    /* tap-packed atlas of the trilinear filter (vrc_core.h): same slots, a texel of twice the voxel's bytes per voxel in
     * blocks of 64 rows of 9.
     * Allocated and filled from the byte atlas the first time a render asks for it (pool_enable_packed); from then
     * on every upload packs its slot too.  Guarded by `mutex`. */
    void* dPacked = nullptr;
    bool packedOn = false;
    bool packedFailed = false; /* the allocation was refused once: not tried again */

    std::mutex mutex; /* free list + staging ring index + upload event + render fences */
    /* slot position + "was in use before" flag: a released slot may still be read by a march
     * that is in flight; the upload that reuses it waits for the render fences first */
    std::vector< std::array< float, 4 > > freeList;
    struct RenderFence
    {
        const vrc_ctx* ctx;
        hipEvent_t event; /* the pool's own, recorded behind a march or a frame histogram, or a march's stop event */
        /* what an upload waits for: `event`, or the stop event of the context's last march where the dispatch carried
         * one of the context's timing events (VRC_OPT_STREAM_MARKERS = 0); `keep` holds those events alive for as long
         * as this entry names one, whatever becomes of the context */
        hipEvent_t last;
        std::shared_ptr< vrc_event_ring > keep;
    };
    std::vector< RenderFence > renderFences; /* last march of every context that used this pool */

    hipStream_t uploadStream = nullptr; /* every write to the atlas (the repack kernels), in issue order */
    /* the host-to-device copies into the staging buffers alternate between two streams of their own: the DMA of
     * one brick runs while the repack kernel of the brick before it writes the atlas */
    hipStream_t copyStream[2] = { nullptr, nullptr };
    hipEvent_t lastUpload = nullptr;
    bool hasUpload = false;
    uint64_t uploadGen = 0; /* counts the records of lastUpload: a stream that has waited for this one need not again */

    struct Staging
    {
        std::mutex mutex;
        void* pinned = nullptr;
        void* device = nullptr;
        hipEvent_t copied = nullptr; /* the brick is in `device` */
        hipEvent_t done = nullptr;   /* ... and has been repacked into the atlas: both buffers are free */
        bool used = false;
    };
    Staging staging[kStagingSlots];
    uint32_t nextStaging = 0;

    /* per-slot histograms (vrc_pool_enable_histograms), guarded by `mutex`: binCount uint32 per slot, a row is
     * valid while its slot holds a binned brick.  slotSize: the brick size of every slot's last upload */
    uint32_t histBins = 0;
    uint32_t histOverlap[3] = { 0, 0, 0 };
    uint32_t* dHist = nullptr;
    std::vector< uint8_t > histValid;
    std::vector< uint8_t > resident;
    std::vector< std::array< uint32_t, 3 > > slotSize;
};

/* walk cache (VRC_OPT_WALK_CACHE; vrc_core.h: vrc_frame::walkCache): the device memory, the event and the frames.  What it
 * remembers and decides is vrc_plan.h's (s: vrc_walk_state); nothing here exists before the first count pass */
struct vrc_walk_cache
{
    vrc_walk_state s;
    uint32_t* dLists = nullptr;
    size_t words = 0;               /* allocated */
    vrc_walk_count* dMax = nullptr; /* the count pass's result, and its pinned copy */
    vrc_walk_count* hMax = nullptr;
    hipEvent_t ev = nullptr;
    vrc_frame frame;     /* the frame the lists were counted for */
    vrc_frame prevFrame; /* the frame of the vrc_render before */
    uint32_t* dResolved = nullptr; /* the resolved visit words (VRC_OPT_WALK_RESOLVED) */
    size_t resolvedWords = 0;      /* allocated */
    void* dFirstVisit = nullptr;   /* the first-visit table (VRC_OPT_FIRST_VISIT_TABLE): allocated by the first build, for
                                    * the four-float form */
};

struct vrc_ctx
{
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    vrc_options opt;   /* vrc_plan.h: every VRC_OPT_* that can be set */
    vrc_latches latch; /* ... and what the frame's first pass read of those its later passes must not change */

    /* cuda::ColorMap + cuda::ClipPlanes state */
    float* dTf = nullptr;
    float* hTf = nullptr; /* pinned copy of the last uploaded TF: skips identical re-uploads */
    uint64_t tfVersion = 0;
    float planes[6][4];
    uint32_t nPlanes = 0;

    /* classified table */
    vrc_f4* dLut = nullptr;
    bool lutValid = false;
    uint64_t lutTfVersion = 0;
    vrc_lut_params lutParams = { 0, 0, 0, 0 };
    float lutMaxAlpha = 1.0f; /* largest opacity in the classified table (1: unknown) */
    bool tfGrey = false;      /* red == green == blue in every entry of the transfer function (bitwise) */
    bool lutLinear = false;
    uint32_t lutLevels = 1;
    uint64_t lutGen = 0; /* bumped wherever render_tables rebuilds the classified table (0: never built) */

    /* pixel buffer (cuda::PixelBufferObject) */
    vrc_f4* fbOwn = nullptr;
    size_t fbOwnPixels = 0;
    vrc_f4* fbExt = nullptr;
    uint32_t fbW = 0, fbH = 0;
    bool clearPending = false; /* pre_render's clear, folded into the first march or done lazily */

    /* node table + brick grid */
    vrc_dev_node* dNodes = nullptr;
    size_t dNodesCap = 0;
    int32_t* dGrid = nullptr;
    size_t dGridCap = 0;
    /* pinned staging for nodes + grid: a ring of kNodeStages areas of hStageCap bytes, each with
     * the event of the copies last issued from it, so a changed node list (a moving camera
     * re-sorts the bricks) does not have to wait for the frames still in the stream */
    void* hStage = nullptr;
    size_t hStageCap = 0;
    hipEvent_t stageEvent[4] = { nullptr, nullptr, nullptr, nullptr };
    bool stageUsed[4] = { false, false, false, false };
    uint32_t stageNext = 0;
    std::vector< vrc_node_data > cachedNodes;
    uint64_t cachedPoolUid = 0;
    bool cachedGridOk = false;
    bool cachedOneCell = false; /* every brick = one grid cell (vrc_host_tables::oneCellPerBrick) */
    bool cachedRayLod = false; /* tables are per-level (vrc_build_lod_tables) */
    bool cachedLodOk = false;
    uint32_t cachedLodLevels = 0;
    double cachedFinestVoxel = 0.0;
    bool cachedClamp = false;
    vrc_frame cachedGridFrame = {}; /* only grid* / lod* fields are meaningful */

    /* sort-first row map */
    uint32_t* dRowMap = nullptr;
    size_t dRowMapCap = 0;
    std::vector< uint32_t > rowMap;

    /* tile schedule */
    uint32_t* dTileOrder = nullptr;
    size_t dTileOrderCap = 0;
    bool tileOrderValid = false;
    uint32_t tileOrderReused = 0; /* frames in a row that kept the schedule of a nearby view */
    vrc_frame tileOrderFrame;
    /* ray cache (VRC_OPT_RAY_CACHE; vrc_core.h: vrc_frame::rayCache): the planes, regrown like dTileOrder; what it
     * remembers (vrc_plan.h) and the frame constants of the vrc_render before; the mode the last vrc_render used
     * (VRC_OPT_RAY_CACHE_USED) */
    float* dRayCache = nullptr;
    size_t dRayCacheCap = 0; /* words per plane */
    vrc_ray_state ray;
    vrc_frame rayPrevFrame;
    /* ... of which kind of frame: slice frames keep their rays in the same planes, and a frame of the other kind
     * forgets the state first (render_ray_kind).  To the frames of another projection a slice frame is thereby what a
     * MIP frame is -- behind it they compute, store and load, and count, record and replay their walk, as they would
     * without it -- and the other way round */
    bool rayOfSlice = false;
    int64_t rayCacheUsed = 0;
    vrc_walk_cache walk;
    vrc_walk_plan walkPlan; /* what the last vrc_render did about the walk cache (vrc_plan.h; VRC_OPT_*_USED) */
    bool rayLod = false; /* vrc_set_ray_lod */
    float rayLodSse = 1.0f, rayLodWorldPerPixel = 0.0f;

    unsigned long long* dCounter = nullptr;
    unsigned long long* hCounter = nullptr; /* pinned */

    /* one event pair per raycast launch since the last vrc_get_stats (ring, grows on demand) */
    std::shared_ptr< vrc_event_ring > evRing = std::make_shared< vrc_event_ring >();
    /* the upload this context's stream has waited for: pool and its vrc_pool::uploadGen (0 = none) */
    uint64_t waitedPoolUid = 0, waitedGen = 0;
    size_t evUsed = 0;
    double evFoldedMs = 0.0;      /* pairs taken out of a full ring before anyone asked for the statistics */
    uint32_t evFoldedLaunches = 0;
    bool timed = false;

    /* MIP: one running maximum per pixel of the pixel buffer (vrc_core.h: vrc_frame::mipMax), whichever buffer that
     * is; vrc_pre_render invalidates it (mipFirst: the next MIP pass does not read it) and forgets the latches of
     * the frame before */
    uint32_t* dMipMax = nullptr;
    size_t dMipMaxPixels = 0;
    bool mipFirst = true;
    /* the mean fold's running (sum, count) per pixel (vrc_frame::meanSum, meanCount): allocated, invalidated and grown
     * where dMipMax is */
    unsigned long long* dMeanSum = nullptr;
    uint32_t* dMeanCount = nullptr;
    size_t dMeanPixels = 0;
    /* what vrc_get_projection_values reads: the state the frame's last MIP pass left (pixels = 0: none -- no MIP pass
     * since vrc_pre_render), and the device buffer its kernel writes (values | counts) */
    vrc_projection_state projState = { nullptr, nullptr, nullptr, 0u, 0u, 0u, 0.0f };
    float* dProjOut = nullptr;
    size_t dProjOutPixels = 0;
    /* the depth of the projected sample (include/vrc_hip.h, "The depth of a MIP frame"): one running D per pixel beside
     * dMipMax (vrc_frame::mipDepth): allocated by the first frame that tracks depth, grown and invalidated where dMipMax
     * is.  A composite frame's depth (VRC_OPT_COMPOSITE_DEPTH) keeps its pair per pixel in the same two buffers */
    float* dMipDepth = nullptr;
    size_t dMipDepthPixels = 0;
    /* what vrc_get_projection_depths reads: did the frame's last MIP pass track depth, the frame it marched (camera,
     * pixel buffer geometry) with the row map it had, and the device buffer of the read-back (t | xyz | rows) */
    bool depthValid = false;
    vrc_frame depthFrame = {};
    std::vector< uint32_t > depthRows;
    float* dDepthOut = nullptr;
    size_t dDepthOutWords = 0;
    /* an isosurface frame (include/vrc_hip.h, "An isosurface frame"): vrc_set_isosurface's two values (isoSet: called at
     * all), the running G per pixel beside dMipMax and dMipDepth (vrc_frame::isoGrad, three floats a pixel: grown and
     * invalidated where they are), and whether the frame's last pass left one (vrc_get_projection_gradients) */
    bool isoSet = false;
    float isoValue = 0.0f;
    float isoAmbient = 0.0f;
    float* dIsoGrad = nullptr;
    size_t dIsoGradPixels = 0;
    bool gradValid = false;
    /* a slice frame (include/vrc_hip.h, "A slice frame"): vrc_set_slice's plane (sliceSet: called at all).  Its (V, D) per
     * pixel are dMipMax and dMipDepth; sliceFrame: the read-backs' messages speak of the frame the state is of */
    bool sliceSet = false;
    float slicePlane[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    bool sliceFrame = false;
    /* a pre-integrated composite frame (include/vrc_hip.h, "A pre-integrated composite frame"): the one table, allocated
     * by the first frame that needs it, rebuilt when the kind or one of the classified table's inputs changed */
    vrc_f4* dPreint = nullptr;
    int preintKind = -1; /* of the table in dPreint; -1: none built yet */
    uint64_t preintTfVersion = 0;
    vrc_lut_params preintParams;
    int64_t preintBuilds = 0; /* VRC_OPT_PREINT_BUILDS */
    uint32_t* dRayList = nullptr; /* counts | two ray lists (vrc_internal.h) */
    size_t dRayListCap = 0;       /* pixels */
    int lastErtParts = 0;         /* of the last vrc_render */
    int64_t gridWalkUsed = 0;     /* VRC_OPT_GRID_WALK_USED: did the last vrc_render find its bricks through the grid? */

    vrc_stats stats = {};

    /* frame histogram (vrc_frame_histogram): uint64 bins on the device, the refs of the last calls staged through a
     * pinned ring (an area is rewritten only after the copy that read it has run) */
    unsigned long long* dFrameHist = nullptr;
    unsigned long long* hFrameHist = nullptr; /* pinned */
    size_t frameHistCap = 0;
    uint32_t frameHistBins = 0;
    vrc_hist_ref* dHistRefs = nullptr;
    vrc_hist_ref* hHistRefs = nullptr; /* pinned, kNodeStages areas of histRefsCap */
    size_t histRefsCap = 0;
    hipEvent_t histRefsEvent[kNodeStages] = { nullptr, nullptr, nullptr, nullptr };
    bool histRefsUsed[kNodeStages] = { false, false, false, false };
    uint32_t histRefsNext = 0;
};

#define VRC_TRY( call ) /* a step that has already said why it failed */ \
    do { const int _rc = ( call ); if( _rc != VRC_OK ) return _rc; } while( 0 )

/* one allocation of a growth group: where its pointer lives, its bytes per element of the group's capacity plus a fixed
 * tail, device or pinned memory */
struct vrc_grown
{
    enum { DEVICE = 0, PINNED = 1 };
    void** p;
    size_t elemBytes, tailBytes;
    int where;
    template< class T > vrc_grown( T*& q, size_t elem = sizeof( T ), size_t tail = 0, int w = DEVICE )
        : p( reinterpret_cast< void** >( &q ) ), elemBytes( elem ), tailBytes( tail ), where( w ) {}
};

/* Where the capacity `cap` the allocations share is below n elements, make it `want` (>= n): behind a synchronisation of
 * the context's stream -- whatever reads the old ones has run -- all are freed, then all allocated anew; nothing is
 * carried over.  After a failed allocation what was not reallocated is NULL and the capacity is 0.  grew: it happened,
 * and the contents are the caller's to fill */
static int ctx_grow( vrc_ctx* c, size_t& cap, size_t n, size_t want, std::initializer_list< vrc_grown > bufs, bool* grew = nullptr )
{
    if( grew )
        *grew = n > cap;
    if( n <= cap )
        return VRC_OK;
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    for( const vrc_grown& b : bufs )
        if( *b.p )
            VRC_HIP_CHECK( b.where == vrc_grown::PINNED ? hipHostFree( *b.p ) : hipFree( *b.p ) );
    for( const vrc_grown& b : bufs )
        *b.p = nullptr;
    cap = 0;
    for( const vrc_grown& b : bufs )
    {
        const size_t bytes = want * b.elemBytes + b.tailBytes;
        VRC_HIP_CHECK( b.where == vrc_grown::PINNED ? hipHostMalloc( b.p, bytes ) : hipMalloc( b.p, bytes ) );
    }
    cap = want;
    return VRC_OK;
}

int vrc_internal_fail( int code, const std::string& msg ) { return fail( code, msg ); }
static thread_local char tlsKernel[160] = "";
void vrc_internal_note_kernel( const char* fmt, ... )
{
    va_list ap;
    va_start( ap, fmt );
    vsnprintf( tlsKernel, sizeof( tlsKernel ), fmt, ap );
    va_end( ap );
}
static thread_local const void* tlsKernelFn = nullptr;
static thread_local int tlsKernelThreads = 0;
static thread_local size_t tlsKernelLds = 0;
void vrc_internal_note_kernel_fn( const void* fn, int threads, size_t dynamicLds )
{
    tlsKernelFn = fn;
    tlsKernelThreads = threads;
    tlsKernelLds = dynamicLds;
}
hipStream_t vrc_internal_ctx_stream( vrc_ctx* c, int* deviceOut )
{
    if( deviceOut )
        *deviceOut = c->device;
    return c->stream;
}

extern "C" {

const char* vrc_last_error( void ) { return g_lastError.c_str(); }
const char* vrc_last_kernel( void ) { return tlsKernel; }
int vrc_last_kernel_occupancy( int* workgroupsPerCu, int* threadsPerWorkgroup )
{
    if( !workgroupsPerCu )
        return fail( VRC_EINVAL, "vrc_last_kernel_occupancy: NULL argument" );
    *workgroupsPerCu = 0;
    if( threadsPerWorkgroup )
        *threadsPerWorkgroup = tlsKernelThreads;
    if( !tlsKernelFn )
        return fail( VRC_EINVAL, "vrc_last_kernel_occupancy: the calling thread's last vrc_render did not launch vrc_k_raycast" );
    int n = 0;
    VRC_HIP_CHECK( hipOccupancyMaxActiveBlocksPerMultiprocessor( &n, tlsKernelFn, tlsKernelThreads, tlsKernelLds ) );
    *workgroupsPerCu = n;
    return VRC_OK;
}
#if defined( VRC_DEV_BUILD )
int vrc_abi_version( void ) { return -VRC_ABI_VERSION; }
int vrc_is_dev_build( void ) { return 1; }
#else
int vrc_abi_version( void ) { return VRC_ABI_VERSION; }
int vrc_is_dev_build( void ) { return 0; }
#endif

/* ---------------------------------------------------------------------------------------- */
int vrc_ctx_create( int device, vrc_ctx** out )
{
    if( !out )
        return fail( VRC_EINVAL, "vrc_ctx_create: out is NULL" );
    *out = nullptr;
    int count = 0;
    VRC_HIP_CHECK( hipGetDeviceCount( &count ) );
    if( device < 0 || device >= count )
        return fail( VRC_EINVAL, "vrc_ctx_create: no such device" );
    VRC_HIP_CHECK( hipSetDevice( device ) );
    vrc_ctx* c = new vrc_ctx();
    c->device = device;
    std::memset( c->planes, 0, sizeof( c->planes ) );
    /* default transfer function: linear grey ramp (the reference uploads lexis' default
     * colour map in cuda::ColorMap::ColorMap, cuda/ColorMap.cu:32; that map lives in the
     * un-vendored Lexis library, so the default here is documented and explicit) */
    float tf[256 * 4];
    for( int i = 0; i < 256; ++i )
        tf[i * 4 + 0] = tf[i * 4 + 1] = tf[i * 4 + 2] = tf[i * 4 + 3] = (float)i / 255.0f;
    hipError_t e = hipStreamCreateWithFlags( &c->ownStream, hipStreamNonBlocking );
    if( e == hipSuccess ) e = hipMalloc( &c->dTf, 256 * 4 * sizeof( float ) );
    if( e == hipSuccess ) e = hipMalloc( &c->dLut, ( VRC_MAX_LOD_LEVELS * VRC_LUT_ENTRIES + 1u ) * sizeof( vrc_f4 ) );
    if( e == hipSuccess ) e = hipHostMalloc( &c->hTf, 256 * 4 * sizeof( float ) );
    if( e == hipSuccess ) e = hipMalloc( &c->dCounter, sizeof( unsigned long long ) );
    if( e == hipSuccess ) e = hipHostMalloc( &c->hCounter, sizeof( unsigned long long ) );
    if( e == hipSuccess ) e = hipMemcpy( c->dTf, tf, sizeof( tf ), hipMemcpyHostToDevice );
    if( e != hipSuccess )
    {
        const std::string msg = std::string( "vrc_ctx_create: " ) + hipGetErrorString( e );
        vrc_ctx_destroy( c );
        return fail( VRC_EHIP, msg );
    }
    c->stream = c->ownStream;
    *c->hCounter = 0;
    std::memcpy( c->hTf, tf, sizeof( tf ) );
    c->tfGrey = true;
    if( const char* g = std::getenv( "VRC_GREY_TABLE" ) ) /* default of VRC_OPT_GREY_TABLE for this process */
        c->opt.greyTable = g[0] != '0';
    c->tfVersion = 1;
    *out = c;
    return VRC_OK;
}

void vrc_ctx_destroy( vrc_ctx* c )
{
    if( !c )
        return;
    (void)hipSetDevice( c->device );
    if( c->stream ) (void)hipStreamSynchronize( c->stream );
    const std::initializer_list< void* > device = {
        c->dTf,      c->dLut,     c->dPreint,  c->fbOwn,     c->dNodes,    c->dGrid,    c->dTileOrder, c->dRayCache,
        c->walk.dLists, c->walk.dMax, c->dRayList, c->dMipMax, c->dMeanSum, c->dMeanCount, c->dProjOut, c->dMipDepth,
        c->dIsoGrad, c->dDepthOut, c->dRowMap, c->dCounter,  c->dFrameHist, c->dHistRefs, c->walk.dFirstVisit,
        c->walk.dResolved };
    const std::initializer_list< void* > pinned = { c->hTf, c->hStage, c->walk.hMax, c->hCounter, c->hFrameHist, c->hHistRefs };
    for( void* d : device )
        if( d ) (void)hipFree( d );
    for( void* h : pinned )
        if( h ) (void)hipHostFree( h );
    for( hipEvent_t e : c->stageEvent )
        if( e ) (void)hipEventDestroy( e );
    for( hipEvent_t e : c->histRefsEvent )
        if( e ) (void)hipEventDestroy( e );
    if( c->walk.ev ) (void)hipEventDestroy( c->walk.ev );
    c->evRing.reset(); /* (the events live on while a pool's render fence names one) */
    if( c->ownStream ) (void)hipStreamDestroy( c->ownStream );
    delete c;
}

int vrc_ctx_set_stream( vrc_ctx* c, void* s )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_ctx_set_stream: ctx is NULL" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    c->stream = s ? (hipStream_t)s : c->ownStream;
    c->waitedPoolUid = c->waitedGen = 0; /* the new stream has waited for no upload */
    vrc_ray_forget( c->ray );         /* (the planes were written on the stream before) */
    vrc_walk_forget( c->walk.s ); /* (and so were the lists; a count pass in flight has ended above) */
    return VRC_OK;
}

int vrc_set_option( vrc_ctx* c, int option, int64_t value )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_set_option: ctx is NULL" );
    switch( option )
    {
    case VRC_OPT_KERNEL:
        if( value < VRC_KERNEL_AUTO || ( value > VRC_KERNEL_LDS && value != VRC_KERNEL_PACKED ) )
            return fail( VRC_EINVAL, "vrc_set_option: bad kernel variant" );
        c->opt.kernel = value;
        return VRC_OK;
    case VRC_OPT_FILTER:
        if( value != VRC_FILTER_NEAREST && value != VRC_FILTER_TRILINEAR )
            return fail( VRC_EINVAL, "vrc_set_option: filter is 0 (nearest) or 1 (trilinear)" );
        c->opt.filter = value;
        return VRC_OK;
    case VRC_OPT_TF_FRAC_BITS:
        if( value < 0 || value > 16 )
            return fail( VRC_EINVAL, "vrc_set_option: tf frac bits out of range" );
        c->opt.tfFracBits = value;
        return VRC_OK;
    case VRC_OPT_COUNT_SAMPLES: c->opt.count = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_TILE_ORDER: c->opt.tileOrder = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_STEPPING: c->opt.stepping = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_KERNEL_TIMING: c->opt.timing = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_DEPTH_SPLIT: c->opt.depthSplit = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_GREY_TABLE: c->opt.greyTable = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_PACKED_ATLAS: c->opt.packedAtlas = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_UNIFORM_BRICKS: c->opt.uniformBricks = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_STREAM_MARKERS: c->opt.streamMarkers = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_RAY_CACHE:
        if( c->opt.rayCache != ( value ? 1 : 0 ) )
            vrc_ray_forget( c->ray );
        c->opt.rayCache = value ? 1 : 0;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE:
        if( value < 0 || value > VRC_WALK_CACHE_ALWAYS )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE is 0 (off), 1 (on) or 2 (on for every view)" );
        if( c->opt.walkCache != value )
            vrc_walk_forget( c->walk.s );
        c->opt.walkCache = value;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET:
        if( value < 0 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE_BUDGET is a number of bytes" );
        if( c->opt.walkBudget != value )
            vrc_walk_forget( c->walk.s );
        c->opt.walkBudget = value;
        return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_UNIFORM_ONLY is 0 (off) or 1 (on)" );
        c->opt.walkUniformOnly = value; /* (which instance replays the lists: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_UNIFORM_ONLY_USED is read-only" );
    case VRC_OPT_STORE_THROUGH:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_STORE_THROUGH is 0 (plain stores) or 1 (write-through)" );
        c->opt.storeThrough = value; /* (how the replay stores its pixels: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_STORE_THROUGH_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_STORE_THROUGH_USED is read-only" );
    case VRC_OPT_FIRST_VISIT_TABLE:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_FIRST_VISIT_TABLE is 0 (march every visit) or 1 (first visits from the table)" );
        c->opt.firstVisitTable = value; /* (how the replay takes a first visit: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_FIRST_VISIT_TABLE_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_FIRST_VISIT_TABLE_USED is read-only" );
    case VRC_OPT_LEAN_FREE_MARCH:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_LEAN_FREE_MARCH is 0 (every visit tests for the exit) or 1 (not where it is out of reach)" );
        c->opt.leanFreeMarch = value; /* (how the replay marches a visit: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_LEAN_FREE_MARCH_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_LEAN_FREE_MARCH_USED is read-only" );
    case VRC_OPT_WALK_RESOLVED:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_RESOLVED is 0 (list and slot words) or 1 (resolved visit words)" );
        c->opt.walkResolved = value; /* (what the uniform-only replay reads of a visit: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_WALK_RESOLVED_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_RESOLVED_USED is read-only" );
    case VRC_OPT_PROJECTION:
        if( value != VRC_PROJECTION_COMPOSITE && value != VRC_PROJECTION_MIP && value != VRC_PROJECTION_ISO &&
            value != VRC_PROJECTION_SLICE )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PROJECTION is 0 (composite), 1 (maximum intensity), 2 (isosurface) "
                                     "or 4 (slice)" );
        /* ... and one that never called vrc_set_slice what it had before the slice projection existed */
        if( value == VRC_PROJECTION_SLICE && !c->sliceSet )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE needs vrc_set_slice first" );
        /* a context that never called vrc_set_isosurface keeps what it had before the isosurface projection existed: the
         * value is refused, here and not only by the render it could not serve */
        if( value == VRC_PROJECTION_ISO && !c->isoSet )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PROJECTION = VRC_PROJECTION_ISO needs vrc_set_isosurface first" );
        c->opt.projection = value;
        return VRC_OK;
    case VRC_OPT_MIP_SKIP: c->opt.mipSkip = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_MIP_FOLD:
        if( value != VRC_MIP_FOLD_MAX && value != VRC_MIP_FOLD_MIN && value != VRC_MIP_FOLD_MEAN )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_FOLD is 0 (maximum), 1 (minimum) or 2 (mean)" );
        c->opt.mipFold = value;
        return VRC_OK;
    case VRC_OPT_MIP_DEPTH:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_DEPTH is 0 (off) or 1 (keep the depth of the projected sample)" );
        c->opt.mipDepth = value;
        return VRC_OK;
    case VRC_OPT_MIP_DEPTH_CUE:
        if( value < 0 || value > 1000 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_DEPTH_CUE is the cue strength in thousandths, 0 (off) to 1000" );
        c->opt.mipDepthCue = value;
        return VRC_OK;
    case VRC_OPT_SHADING:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_SHADING is 0 (off) or 1 (light every sample of a composite frame by its gradient)" );
        c->opt.shading = value;
        return VRC_OK;
    case VRC_OPT_SHADING_AMBIENT:
        if( value < 0 || value > 1000 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_SHADING_AMBIENT is the ambient share in thousandths, 0 to 1000" );
        c->opt.shadingAmbient = value;
        return VRC_OK;
    case VRC_OPT_COMPOSITE_DEPTH:
        if( value < 0 || value > 999 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_COMPOSITE_DEPTH is 0 (off) or the opacity threshold in thousandths, 1 to 999" );
        c->opt.compositeDepth = value;
        return VRC_OK;
    case VRC_OPT_PREINTEGRATION:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PREINTEGRATION is 0 (off) or 1 (classify every step of a composite frame from the pre-integrated table)" );
        c->opt.preint = value;
        return VRC_OK;
    case VRC_OPT_PREINT_BUILDS:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PREINT_BUILDS is read-only" );
    case VRC_OPT_ERT_COMPACTION:
        if( value < 0 || value > VRC_MAX_ERT_PARTS )
            return fail( VRC_EINVAL, "VRC_OPT_ERT_COMPACTION: 0 (off) or 2.." + std::to_string( VRC_MAX_ERT_PARTS ) +
                                         " launches per frame" );
        c->opt.ertParts = value < 2 ? 0 : value;
        return VRC_OK;
    case VRC_OPT_VARIANT:
        if( value != VRC_VARIANT_CUDARAYCASTER && value != VRC_VARIANT_GLRAYCASTER )
            return fail( VRC_EINVAL, "vrc_set_option: variant is 0 (cudaRaycaster) or 1 (glRaycaster)" );
        c->opt.variant = value;
        return VRC_OK;
    default: return fail( VRC_EINVAL, "vrc_set_option: unknown option" );
    }
}

int vrc_get_option( vrc_ctx* c, int option, int64_t* value )
{
    if( !c || !value )
        return fail( VRC_EINVAL, "vrc_get_option: NULL argument" );
    switch( option )
    {
    case VRC_OPT_KERNEL: *value = c->opt.kernel; return VRC_OK;
    case VRC_OPT_FILTER: *value = c->opt.filter; return VRC_OK;
    case VRC_OPT_TF_FRAC_BITS: *value = c->opt.tfFracBits; return VRC_OK;
    case VRC_OPT_COUNT_SAMPLES: *value = c->opt.count; return VRC_OK;
    case VRC_OPT_TILE_ORDER: *value = c->opt.tileOrder; return VRC_OK;
    case VRC_OPT_STEPPING: *value = c->opt.stepping; return VRC_OK;
    case VRC_OPT_KERNEL_TIMING: *value = c->opt.timing; return VRC_OK;
    case VRC_OPT_DEPTH_SPLIT: *value = c->opt.depthSplit; return VRC_OK;
    case VRC_OPT_ERT_COMPACTION: *value = c->opt.ertParts; return VRC_OK;
    case VRC_OPT_GREY_TABLE: *value = c->opt.greyTable; return VRC_OK;
    case VRC_OPT_PACKED_ATLAS: *value = c->opt.packedAtlas; return VRC_OK;
    case VRC_OPT_UNIFORM_BRICKS: *value = c->opt.uniformBricks; return VRC_OK;
    case VRC_OPT_STREAM_MARKERS: *value = c->opt.streamMarkers; return VRC_OK;
    case VRC_OPT_RAY_CACHE: *value = c->opt.rayCache; return VRC_OK;
    case VRC_OPT_RAY_CACHE_USED: *value = c->rayCacheUsed; return VRC_OK;
    case VRC_OPT_WALK_CACHE: *value = c->opt.walkCache; return VRC_OK;
    case VRC_OPT_WALK_CACHE_USED: *value = c->walkPlan.used; return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET: *value = c->opt.walkBudget; return VRC_OK;
    case VRC_OPT_WALK_CACHE_BYTES: *value = (int64_t)( c->walk.words * sizeof( uint32_t ) ); return VRC_OK;
    case VRC_OPT_WALK_LEAN_USED: *value = c->walkPlan.leanUsed; return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY: *value = c->opt.walkUniformOnly; return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY_USED: *value = c->walkPlan.uniformUsed; return VRC_OK;
    case VRC_OPT_STORE_THROUGH: *value = c->opt.storeThrough; return VRC_OK;
    case VRC_OPT_STORE_THROUGH_USED: *value = c->walkPlan.storeThrough; return VRC_OK;
    case VRC_OPT_FIRST_VISIT_TABLE: *value = c->opt.firstVisitTable; return VRC_OK;
    case VRC_OPT_FIRST_VISIT_TABLE_USED: *value = c->walkPlan.firstVisit; return VRC_OK;
    case VRC_OPT_LEAN_FREE_MARCH: *value = c->opt.leanFreeMarch; return VRC_OK;
    case VRC_OPT_LEAN_FREE_MARCH_USED: *value = c->walkPlan.leanFree; return VRC_OK;
    case VRC_OPT_WALK_RESOLVED: *value = c->opt.walkResolved; return VRC_OK;
    case VRC_OPT_WALK_RESOLVED_USED: *value = c->walkPlan.resolved; return VRC_OK;
    case VRC_OPT_PROJECTION: *value = c->opt.projection; return VRC_OK;
    case VRC_OPT_MIP_SKIP: *value = c->opt.mipSkip; return VRC_OK;
    case VRC_OPT_MIP_FOLD: *value = c->opt.mipFold; return VRC_OK;
    case VRC_OPT_MIP_DEPTH: *value = c->opt.mipDepth; return VRC_OK;
    case VRC_OPT_MIP_DEPTH_CUE: *value = c->opt.mipDepthCue; return VRC_OK;
    case VRC_OPT_VARIANT: *value = c->opt.variant; return VRC_OK;
    case VRC_OPT_SHADING: *value = c->opt.shading; return VRC_OK;
    case VRC_OPT_SHADING_AMBIENT: *value = c->opt.shadingAmbient; return VRC_OK;
    case VRC_OPT_COMPOSITE_DEPTH: *value = c->opt.compositeDepth; return VRC_OK;
    case VRC_OPT_PREINTEGRATION: *value = c->opt.preint; return VRC_OK;
    case VRC_OPT_PREINT_BUILDS: *value = c->preintBuilds; return VRC_OK;
    case VRC_OPT_KERNEL_USED: *value = c->stats.kernel_variant; return VRC_OK;
    case VRC_OPT_GRID_WALK_USED: *value = c->gridWalkUsed; return VRC_OK;
    default: return fail( VRC_EINVAL, "vrc_get_option: unknown option" );
    }
}

/* per-ray adaptive LOD (extension): see include/vrc_hip.h */
int vrc_set_ray_lod( vrc_ctx* c, int enable, float screenSpaceError, float worldSpacePerPixel )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_set_ray_lod: ctx is NULL" );
    if( enable && ( !( screenSpaceError > 0.0f ) || !( worldSpacePerPixel > 0.0f ) ) )
        return fail( VRC_EINVAL, "vrc_set_ray_lod: screen-space error and world space per pixel must be > 0" );
    c->rayLod = enable != 0;
    if( enable )
    {
        c->rayLodSse = screenSpaceError;
        c->rayLodWorldPerPixel = worldSpacePerPixel;
    }
    return VRC_OK;
}

/* ---------------------------------------------------------------------------------------- */
static int pool_create( vrc_ctx* c, int voxelType, const uint32_t maxBlock[3], size_t maxBytes, vrc_pool** out );

int vrc_pool_create( vrc_ctx* c, size_t bytesPerVoxel, int isSigned, int isFloat,
                     size_t nComponents, const uint32_t maxBlock[3], size_t maxBytes,
                     vrc_pool** out )
{
    if( !c || !out || !maxBlock )
        return fail( VRC_EINVAL, "vrc_pool_create: NULL argument" );
    *out = nullptr;
    /* cuda/TexturePool.cu:66-67 */
    if( nComponents == 0 || nComponents > 4 )
        return fail( VRC_EUNSUPPORTED, "Channel number cannot be 0 or larger than 4" );
    /* the reference kernel only ever fetches unsigned char (Renderer.cu:211, quirk Q2); this entry point
     * makes pools of unsigned 8-bit (the reference path) and, as an extension, unsigned 16-bit
     * single-channel volumes, and says so for the rest: signed, 32-bit and float volumes have
     * vrc_pool_create_typed */
    if( ( bytesPerVoxel != 1 && bytesPerVoxel != 2 ) || nComponents != 1 || isFloat || isSigned )
        return fail( VRC_EUNSUPPORTED,
                     "vrc_pool_create: only unsigned 8/16-bit single-channel volumes are implemented "
                     "(signed, 32-bit and float: vrc_pool_create_typed)" );
    return pool_create( c, bytesPerVoxel == 1 ? VRC_VOXEL_UINT8 : VRC_VOXEL_UINT16, maxBlock, maxBytes, out );
}

int vrc_pool_create_typed( vrc_ctx* c, int voxelType, const uint32_t maxBlock[3], size_t maxBytes, vrc_pool** out )
{
    if( !c || !out || !maxBlock )
        return fail( VRC_EINVAL, "vrc_pool_create_typed: NULL argument" );
    *out = nullptr;
    if( voxelType < VRC_VOXEL_UINT8 || voxelType > VRC_VOXEL_FLOAT32 )
        return fail( VRC_EINVAL, "vrc_pool_create_typed: unknown voxel type " + std::to_string( voxelType ) );
    return pool_create( c, voxelType, maxBlock, maxBytes, out );
}

int vrc_pool_voxel_type( const vrc_pool* p, int* voxelType )
{
    if( !p || !voxelType )
        return fail( VRC_EINVAL, "vrc_pool_voxel_type: NULL argument" );
    *voxelType = p->voxelType;
    return VRC_OK;
}

static int pool_create( vrc_ctx* c, int voxelType, const uint32_t maxBlock[3], size_t maxBytes, vrc_pool** out )
{
    size_t bytesPerVoxel = 1;
    const size_t nComponents = 1;
    uint32_t xform = VRC_XF_NONE;
    float rangeShift = 0.0f;
    switch( voxelType )
    {
    case VRC_VOXEL_UINT8: break;
    case VRC_VOXEL_UINT16: bytesPerVoxel = 2; break;
    case VRC_VOXEL_INT8: xform = VRC_XF_FLIP; rangeShift = 128.0f; break;
    case VRC_VOXEL_INT16: bytesPerVoxel = 2; xform = VRC_XF_FLIP; rangeShift = 32768.0f; break;
    case VRC_VOXEL_UINT32: bytesPerVoxel = 4; xform = VRC_XF_U32F; break;
    case VRC_VOXEL_INT32: bytesPerVoxel = 4; xform = VRC_XF_I32F; break;
    default: bytesPerVoxel = 4; break; /* VRC_VOXEL_FLOAT32: copied as it is */
    }
    if( maxBlock[0] == 0 || maxBlock[1] == 0 || maxBlock[2] == 0 )
        return fail( VRC_EINVAL, "vrc_pool_create: zero block size" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );

    static std::mutex uidMutex;
    static uint64_t nextUid = 1;
    vrc_pool* p = new vrc_pool();
    p->ctx = c;
    p->device = c->device;
    {
        std::lock_guard< std::mutex > lock( uidMutex );
        p->uid = nextUid++;
    }
    p->elemBytes = (uint32_t)( bytesPerVoxel * nComponents );
    p->voxelType = voxelType;
    p->xform = xform;
    p->rangeShift = rangeShift;
    for( int a = 0; a < 3; ++a )
    {
        p->maxBlock[a] = maxBlock[a];
        p->slotDim[a] = ( maxBlock[a] + VRC_MB - 1 ) / VRC_MB * VRC_MB;
        if( p->slotDim[a] > VRC_MAX_TEXTURE_3D )
        {
            delete p;
            return fail( VRC_EINVAL, "vrc_pool_create: block larger than VRC_MAX_TEXTURE_3D" );
        }
    }
    p->slotBytes = (size_t)p->slotDim[0] * p->slotDim[1] * p->slotDim[2] * p->elemBytes;
    if( (size_t)p->slotDim[0] * p->slotDim[1] * p->slotDim[2] >= ( 1u << 24 ) )
    {
        delete p;
        return fail( VRC_EINVAL, "vrc_pool_create: block of 2^24 voxels or more (max 248^3)" );
    }

    /* cuda/TexturePool.cu:119-135, with 64-bit arithmetic (fixes quirk Q12) */
    size_t freeMem = 0, totalMem = 0;
    hipError_t e = hipMemGetInfo( &freeMem, &totalMem );
    if( e != hipSuccess )
    {
        delete p;
        return fail( VRC_EHIP, std::string( "hipMemGetInfo: " ) + hipGetErrorString( e ) );
    }
    const size_t maxMemory = std::min( freeMem, maxBytes );
    const uint64_t maxBlocks64 = maxMemory / p->slotBytes;
    const uint32_t maxBlocks = (uint32_t)std::min< uint64_t >( maxBlocks64, 0xFFFFFFFFull );
    p->slots[0] = std::min( VRC_MAX_TEXTURE_3D / p->slotDim[0], std::max( maxBlocks, 1u ) );
    p->slots[1] = std::min( VRC_MAX_TEXTURE_3D / p->slotDim[1],
                            std::max( maxBlocks / p->slots[0], 1u ) );
    p->slots[2] = std::min( VRC_MAX_TEXTURE_3D / p->slotDim[2],
                            std::max( maxBlocks / ( p->slots[0] * p->slots[1] ), 1u ) );
    for( int a = 0; a < 3; ++a )
        p->atlasDim[a] = p->slots[a] * p->slotDim[a];
    p->atlasBytes = (size_t)p->slots[0] * p->slots[1] * p->slots[2] *
                    vrc_slot_elems( p->slotDim[0], p->slotDim[1], p->slotDim[2] ) * p->elemBytes;
    /* more than 2^32 voxels: slot bases become 64-bit (BIG kernel instances; the LDS-staged and the
     * per-ray LOD kernels, whose slot bases are 32-bit, are not offered for such a pool) */
    p->bigAtlas = p->atlasBytes / p->elemBytes >= 0xFFFFFFFFull;

    const size_t nSlots = (size_t)p->slots[0] * p->slots[1] * p->slots[2];
    p->resident.assign( nSlots, 0 );
    p->slotSize.assign( nSlots, { 0u, 0u, 0u } );

    /* cuda/TexturePool.cu:137-144: i,j,k descending, k innermost; slots are popped from the back */
    for( int i = (int)p->slots[0] - 1; i >= 0; --i )
        for( int j = (int)p->slots[1] - 1; j >= 0; --j )
            for( int k = (int)p->slots[2] - 1; k >= 0; --k )
                p->freeList.push_back( { (float)i / (float)p->slots[0],
                                         (float)j / (float)p->slots[1],
                                         (float)k / (float)p->slots[2], 0.0f } );

    e = hipMalloc( &p->dAtlas, p->atlasBytes );
    if( e == hipSuccess ) e = hipStreamCreateWithFlags( &p->uploadStream, hipStreamNonBlocking );
    /* the clear goes on the upload stream, where every write to the atlas is queued: a hipMemset on the null stream is
     * not ordered with a non-blocking stream, and the first uploads of a large pool could be overtaken by it (seen once:
     * a 6 GB pool of 16-bit voxels, round 4) */
    if( e == hipSuccess ) e = hipMemsetAsync( p->dAtlas, 0, p->atlasBytes, p->uploadStream );
    if( e == hipSuccess ) e = hipMalloc( &p->dSlotInfo, 3 * nSlots * sizeof( uint32_t ) );
    if( e == hipSuccess ) e = hipMemsetAsync( p->dSlotInfo, 0, 3 * nSlots * sizeof( uint32_t ), p->uploadStream );
    if( e == hipSuccess ) p->dSlotMax = p->dSlotInfo + nSlots;
    if( e == hipSuccess ) p->dSlotMin = p->dSlotInfo + 2 * nSlots;
    if( e == hipSuccess ) e = hipEventCreateWithFlags( &p->lastUpload, hipEventDisableTiming );
    if( e == hipSuccess )
    {
        e = hipEventRecord( p->lastUpload, p->uploadStream ); /* a render before any upload waits for the clear too */
        p->hasUpload = true;
        ++p->uploadGen;
    }
    for( int k = 0; k < 2 && e == hipSuccess; ++k )
        e = hipStreamCreateWithFlags( &p->copyStream[k], hipStreamNonBlocking );
    for( int s = 0; s < kStagingSlots && e == hipSuccess; ++s )
    {
        e = hipHostMalloc( &p->staging[s].pinned, p->slotBytes );
        if( e == hipSuccess ) e = hipMalloc( &p->staging[s].device, p->slotBytes );
        if( e == hipSuccess )
            e = hipEventCreateWithFlags( &p->staging[s].copied, hipEventDisableTiming );
        if( e == hipSuccess )
            e = hipEventCreateWithFlags( &p->staging[s].done, hipEventDisableTiming );
    }
    if( e != hipSuccess )
    {
        const std::string msg = std::string( "vrc_pool_create: " ) + hipGetErrorString( e );
        vrc_pool_destroy( p );
        return fail( e == hipErrorOutOfMemory ? VRC_ENOMEM : VRC_EHIP, msg );
    }
    *out = p;
    return VRC_OK;
}

void vrc_pool_destroy( vrc_pool* p )
{
    if( !p )
        return;
    /* the caller guarantees no context is still rendering from this pool */
    (void)hipSetDevice( p->device );
    (void)hipDeviceSynchronize();
    for( int s = 0; s < kStagingSlots; ++s )
    {
        if( p->staging[s].pinned ) (void)hipHostFree( p->staging[s].pinned );
        if( p->staging[s].device ) (void)hipFree( p->staging[s].device );
        if( p->staging[s].copied ) (void)hipEventDestroy( p->staging[s].copied );
        if( p->staging[s].done ) (void)hipEventDestroy( p->staging[s].done );
    }
    for( int k = 0; k < 2; ++k )
        if( p->copyStream[k] ) (void)hipStreamDestroy( p->copyStream[k] );
    if( p->lastUpload ) (void)hipEventDestroy( p->lastUpload );
    for( auto& f : p->renderFences )
        (void)hipEventDestroy( f.event );
    if( p->uploadStream ) (void)hipStreamDestroy( p->uploadStream );
    if( p->dPacked ) (void)hipFree( p->dPacked );
    if( p->dHist ) (void)hipFree( p->dHist );
    if( p->dSlotInfo ) (void)hipFree( p->dSlotInfo );
    if( p->dAtlas ) (void)hipFree( p->dAtlas );
    delete p;
}

/* fences: the render events a reused slot's upload has to wait for (empty for a fresh slot) */
static int pool_take_slot( vrc_pool* p, float slot[3], std::vector< hipEvent_t >& fences )
{
    std::lock_guard< std::mutex > lock( p->mutex );
    if( p->freeList.empty() )
    {
        slot[0] = slot[1] = slot[2] = -1.0f; /* INVALID_SLOT_POSITION, TexturePool.cu:98 */
        return fail( VRC_EFULL, "vrc_pool_copy_to_slot: no free slot" );
    }
    const auto s = p->freeList.back();
    p->freeList.pop_back();
    slot[0] = s[0];
    slot[1] = s[1];
    slot[2] = s[2];
    if( s[3] != 0.0f )
        for( const auto& f : p->renderFences )
            fences.push_back( f.last );
    return VRC_OK;
}

/* the render fence of context c on the pool, made on first use (caller holds the mutex); NULL: vrc_last_error is set */
static vrc_pool::RenderFence* pool_render_fence( vrc_pool* p, const vrc_ctx* c )
{
    for( auto& f : p->renderFences )
        if( f.ctx == c )
            return &f;
    hipEvent_t e = nullptr;
    const hipError_t err = hipEventCreateWithFlags( &e, hipEventDisableTiming );
    if( err != hipSuccess )
    {
        (void)fail( VRC_EHIP, std::string( "render fence: " ) + hipGetErrorString( err ) );
        return nullptr;
    }
    p->renderFences.push_back( { c, e, e, nullptr } );
    return &p->renderFences.back();
}

/* order the context's stream behind every upload the pool has issued so far.  The stream waits once for each record of
 * lastUpload (uploadGen): a wait it has made already orders everything it runs later.  VRC_OPT_STREAM_MARKERS = 1 waits
 * before every march, as the library always did */
static int ctx_wait_uploads( vrc_ctx* c, vrc_pool* p )
{
    std::lock_guard< std::mutex > lock( p->mutex );
    if( !p->hasUpload )
        return VRC_OK;
    if( !c->opt.streamMarkers && c->waitedPoolUid == p->uid && c->waitedGen == p->uploadGen )
        return VRC_OK;
    VRC_HIP_CHECK( hipStreamWaitEvent( c->stream, p->lastUpload, 0 ) );
    c->waitedPoolUid = p->uid;
    c->waitedGen = p->uploadGen;
    return VRC_OK;
}

/* the context's render fence on the pool (pool_upload waits for it before it overwrites a recycled slot) now stands
 * behind the context's last work on its stream: `done`, one of the context's timing events that already does (the
 * pool keeps the context's events alive while it names one), or NULL = record the pool's own event there */
static int pool_fence_behind( vrc_pool* p, vrc_ctx* c, hipEvent_t done )
{
    std::lock_guard< std::mutex > lock( p->mutex );
    vrc_pool::RenderFence* const f = pool_render_fence( p, c );
    if( !f )
        return VRC_EHIP;
    if( !done )
    {
        VRC_HIP_CHECK( hipEventRecord( f->event, c->stream ) );
        f->last = f->event;
        f->keep.reset();
    }
    else
    {
        f->last = done;
        f->keep = c->evRing;
    }
    return VRC_OK;
}

static void pool_slot_voxel( const vrc_pool* p, const float slot[3], uint32_t o[3] )
{
    /* cuda/TexturePool.cu:193-197 */
    for( int a = 0; a < 3; ++a )
        o[a] = (uint32_t)std::lround( slot[a] * (float)p->atlasDim[a] );
}

/* linear index of the slot at atlas voxel o (the row of its histogram) */
static uint32_t pool_slot_index( const vrc_pool* p, const uint32_t o[3] )
{
    return ( ( o[2] / p->slotDim[2] ) * p->slots[1] + o[1] / p->slotDim[1] ) * p->slots[0] + o[0] / p->slotDim[0];
}
static vrc_layout pool_layout( const vrc_pool* p )
{
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        lay.slots[a] = p->slots[a];
        lay.slotDim[a] = p->slotDim[a];
    }
    return lay;
}
/* the histogram entry of slot `index` holding a brick of `size` voxels: its interior [overlap, size - overlap)
 * (HistogramObject.cpp:94-97); false if the interior is empty (the row stays zero) */
static bool pool_hist_entry( const vrc_pool* p, uint32_t index, const uint32_t size[3], vrc_hist_entry& en )
{
    const uint32_t i = index % p->slots[0], j = ( index / p->slots[0] ) % p->slots[1],
                   k = index / ( p->slots[0] * p->slots[1] );
    en = vrc_hist_entry{};
    en.base = vrc_slot_base( pool_layout( p ), i, j, k );
    en.row = index;
    for( int a = 0; a < 3; ++a )
    {
        if( size[a] <= 2u * p->histOverlap[a] )
            return false;
        en.origin[a] = p->histOverlap[a];
        en.size[a] = size[a] - 2u * p->histOverlap[a];
    }
    return true;
}
/* zero the row of slot `index` and bin the brick of `size` voxels into it, on the upload stream (caller holds mutex) */
static hipError_t pool_bin_slot( vrc_pool* p, uint32_t index, const uint32_t size[3] )
{
    hipError_t e = hipMemsetAsync( p->dHist + (size_t)index * p->histBins, 0, p->histBins * sizeof( uint32_t ),
                                   p->uploadStream );
    vrc_hist_entry en;
    if( e == hipSuccess && pool_hist_entry( p, index, size, en ) )
        e = vrc_launch_bin_bricks( p->dAtlas, p->elemBytes, p->slotDim, nullptr, 0, &en, 0, p->histBins, p->dHist,
                                   p->uploadStream );
    if( e == hipSuccess )
        p->histValid[index] = 1;
    return e;
}

static int pool_check_size( const vrc_pool* p, const uint32_t size[3] )
{
    for( int a = 0; a < 3; ++a )
        if( size[a] == 0 || size[a] > p->slotDim[a] )
            return fail( VRC_EINVAL, "vrc_pool_copy_to_slot: brick does not fit a slot" );
    return VRC_OK;
}

static int pool_upload( vrc_pool* p, const void* src, bool srcIsDevice, const uint32_t size[3],
                        float slotOut[3] )
{
    if( !p || !src || !size || !slotOut )
        return fail( VRC_EINVAL, "vrc_pool_copy_to_slot: NULL argument" );
    slotOut[0] = slotOut[1] = slotOut[2] = -1.0f;
    int rc = pool_check_size( p, size );
    if( rc != VRC_OK )
        return rc;
    VRC_HIP_CHECK( hipSetDevice( p->device ) );
    float slot[3];
    std::vector< hipEvent_t > fences;
    rc = pool_take_slot( p, slot, fences );
    if( rc != VRC_OK )
        return rc;
    uint32_t o[3];
    pool_slot_voxel( p, slot, o );
    const size_t bytes = (size_t)size[0] * size[1] * size[2] * p->elemBytes;

    uint32_t si;
    {
        std::lock_guard< std::mutex > lock( p->mutex );
        si = p->nextStaging++ % kStagingSlots;
    }
    vrc_pool::Staging& st = p->staging[si];
    hipError_t e = hipSuccess;
    {
        std::lock_guard< std::mutex > slock( st.mutex );
        if( st.used )
            e = hipEventSynchronize( st.done ); /* staging buffers free again */
        /* a slot that was released may still be read by a march in flight (the texture cache
         * drops an object as soon as the host is done with it): order the overwrite after the
         * last march of every context that rendered from this pool */
        for( size_t i = 0; i < fences.size() && e == hipSuccess; ++i )
            e = hipStreamWaitEvent( p->uploadStream, fences[i], 0 );
        const void* devSrc = src;
        if( e == hipSuccess && !srcIsDevice )
        {
            std::memcpy( st.pinned, src, bytes ); /* the host pointer is only borrowed */
            hipStream_t const cs = p->copyStream[si & 1u];
            e = hipMemcpyAsync( st.device, st.pinned, bytes, hipMemcpyHostToDevice, cs );
            if( e == hipSuccess ) e = hipEventRecord( st.copied, cs );
            if( e == hipSuccess ) e = hipStreamWaitEvent( p->uploadStream, st.copied, 0 );
            devSrc = st.device;
        }
        if( e == hipSuccess )
        {
            vrc_layout lay;
            for( int a = 0; a < 3; ++a )
            {
                lay.slots[a] = p->slots[a];
                lay.slotDim[a] = p->slotDim[a];
            }
            const uint64_t base = vrc_slot_base( lay, o[0] / p->slotDim[0], o[1] / p->slotDim[1],
                                                 o[2] / p->slotDim[2] );
            uint8_t* const slotPtr = (uint8_t*)p->dAtlas + (size_t)base * p->elemBytes;
            /* the writes of one upload are queued as a unit (pool_enable_packed packs every slot written before it
             * was called; every upload after it packs its own) */
            std::lock_guard< std::mutex > lock( p->mutex );
            const uint32_t index = pool_slot_index( p, o );
            /* the slot's uniformity word: back to "nothing known" before the new voxels land, then whatever the
             * repack finds in them -- same stream, same fences, same lastUpload as the voxels */
            uint32_t* const info = p->dSlotInfo + index;
            uint32_t* const top = p->dSlotMax + index; /* ... and the slot's largest stored value */
            uint32_t* const low = p->dSlotMin + index; /* ... and its smallest */
            e = hipMemsetAsync( info, 0, sizeof( uint32_t ), p->uploadStream );
            if( e == hipSuccess )
                e = hipMemsetAsync( top, 0, sizeof( uint32_t ), p->uploadStream );
            if( e == hipSuccess )
                e = hipMemsetAsync( low, 0, sizeof( uint32_t ), p->uploadStream );
            if( e == hipSuccess )
                e = vrc_launch_repack_brick( devSrc, slotPtr, p->elemBytes, size, p->slotDim, p->uploadStream, info,
                                             p->xform, top, low );
            if( e == hipSuccess && p->packedOn )
                e = vrc_launch_pack_slots( p->dAtlas, p->dPacked, base,
                                           (uint64_t)p->slotDim[0] * p->slotDim[1] * p->slotDim[2], p->slotDim,
                                           p->elemBytes, p->uploadStream );
            p->resident[index] = 1;
            p->slotSize[index] = { size[0], size[1], size[2] };
            /* the slot's histogram row, behind the repack and before lastUpload (vrc_pool_enable_histograms) */
            if( e == hipSuccess && p->histBins )
                e = pool_bin_slot( p, index, size );
            if( e == hipSuccess )
                e = hipEventRecord( st.done, p->uploadStream );
            if( e == hipSuccess )
            {
                e = hipEventRecord( p->lastUpload, p->uploadStream );
                p->hasUpload = true;
                ++p->uploadGen;
            }
        }
        st.used = true;
    }
    if( e != hipSuccess )
    {
        vrc_pool_release_slot( p, slot );
        return fail( VRC_EHIP, std::string( "vrc_pool_copy_to_slot: " ) + hipGetErrorString( e ) );
    }
    if( srcIsDevice )
    {
        /* the caller's device buffer must stay valid until the repack has run */
        e = hipStreamSynchronize( p->uploadStream );
        if( e != hipSuccess )
            return fail( VRC_EHIP, std::string( "vrc_pool_copy_to_slot_device: " ) +
                                       hipGetErrorString( e ) );
    }
    slotOut[0] = slot[0];
    slotOut[1] = slot[1];
    slotOut[2] = slot[2];
    return VRC_OK;
}

/* The tap-packed atlas of the trilinear filter, on first use: 2.25 times the atlas's bytes, filled from it on the upload
 * stream behind every upload queued so far.  false (and no error) when the pool cannot have one: voxels of more than
 * 16 bits, or not enough device memory (tried once). */
static bool pool_packed_possible( const vrc_pool* p )
{
    return p->elemBytes == 1 || p->elemBytes == 2;
}
/* bytes of the pool's packed atlas (+ 8: a pair is read as 4 / 8 bytes at the last texel) */
static uint64_t pool_packed_bytes( const vrc_pool* p )
{
    return vrc_packed_elems( p->atlasBytes / p->elemBytes ) * VRC_PK_TEXEL( p->elemBytes ) + 8u;
}
static bool pool_enable_packed( vrc_pool* p )
{
    std::lock_guard< std::mutex > lock( p->mutex );
    if( p->packedOn )
        return true;
    if( p->packedFailed || !pool_packed_possible( p ) )
        return false;
    const size_t bytes = (size_t)pool_packed_bytes( p );
    size_t freeMem = 0, totalMem = 0;
    hipError_t e = hipMemGetInfo( &freeMem, &totalMem );
    /* leave a margin for the caller's frame buffers and staging */
    if( e == hipSuccess && bytes + ( 256u << 20 ) > freeMem )
        e = hipErrorOutOfMemory;
    if( e == hipSuccess )
        e = hipMalloc( &p->dPacked, bytes );
    if( e == hipSuccess )
        e = vrc_launch_pack_slots( p->dAtlas, p->dPacked, 0u, p->atlasBytes / p->elemBytes, p->slotDim, p->elemBytes,
                                   p->uploadStream );
    if( e == hipSuccess )
    {
        e = hipEventRecord( p->lastUpload, p->uploadStream );
        p->hasUpload = true;
        ++p->uploadGen;
    }
    if( e != hipSuccess )
    {
        (void)hipGetLastError();
        if( p->dPacked )
        {
            (void)hipStreamSynchronize( p->uploadStream );
            (void)hipFree( p->dPacked );
        }
        p->dPacked = nullptr;
        p->packedFailed = true;
        return false;
    }
    p->packedOn = true;
    return true;
}

int vrc_pool_copy_to_slot( vrc_pool* p, const void* hostBrick, const uint32_t size[3],
                           float slotOut[3] )
{
    return pool_upload( p, hostBrick, false, size, slotOut );
}

int vrc_pool_copy_to_slot_device( vrc_pool* p, const void* deviceBrick, const uint32_t size[3],
                                  float slotOut[3] )
{
    return pool_upload( p, deviceBrick, true, size, slotOut );
}

int vrc_pool_release_slot( vrc_pool* p, const float slot[3] )
{
    if( !p || !slot )
        return fail( VRC_EINVAL, "vrc_pool_release_slot: NULL argument" );
    if( slot[0] < 0.f || slot[1] < 0.f || slot[2] < 0.f )
        return fail( VRC_EINVAL, "vrc_pool_release_slot: invalid slot" );
    uint32_t o[3];
    pool_slot_voxel( p, slot, o );
    std::lock_guard< std::mutex > lock( p->mutex );
    const uint32_t index = pool_slot_index( p, o );
    if( index < p->resident.size() )
    {
        p->resident[index] = 0;
        if( index < p->histValid.size() )
            p->histValid[index] = 0;
    }
    p->freeList.push_back( { slot[0], slot[1], slot[2], 1.0f } );
    return VRC_OK;
}

int vrc_pool_info( const vrc_pool* p, size_t* slotBytes, uint32_t atlasDim[3], size_t* atlasBytes,
                   uint32_t slots[3], uint32_t* freeSlots )
{
    if( !p )
        return fail( VRC_EINVAL, "vrc_pool_info: pool is NULL" );
    if( slotBytes ) *slotBytes = p->slotBytes;
    if( atlasBytes ) *atlasBytes = p->atlasBytes;
    for( int a = 0; a < 3; ++a )
    {
        if( atlasDim ) atlasDim[a] = p->atlasDim[a];
        if( slots ) slots[a] = p->slots[a];
    }
    if( freeSlots )
    {
        std::lock_guard< std::mutex > lock( const_cast< vrc_pool* >( p )->mutex );
        *freeSlots = (uint32_t)p->freeList.size();
    }
    return VRC_OK;
}

int vrc_pool_synchronize( vrc_pool* p )
{
    if( !p )
        return fail( VRC_EINVAL, "vrc_pool_synchronize: pool is NULL" );
    VRC_HIP_CHECK( hipSetDevice( p->device ) );
    VRC_HIP_CHECK( hipStreamSynchronize( p->uploadStream ) );
    return VRC_OK;
}

int vrc_pool_read_region( vrc_pool* p, const uint32_t origin[3], const uint32_t size[3],
                          void* hostOut )
{
    if( !p || !origin || !size || !hostOut )
        return fail( VRC_EINVAL, "vrc_pool_read_region: NULL argument" );
    for( int a = 0; a < 3; ++a )
        if( (uint64_t)origin[a] + size[a] > p->atlasDim[a] )
            return fail( VRC_EINVAL, "vrc_pool_read_region: region outside the atlas" );
    VRC_HIP_CHECK( hipSetDevice( p->device ) );
    const size_t bytes = (size_t)size[0] * size[1] * size[2] * p->elemBytes;
    if( bytes == 0 )
        return VRC_OK;
    void* tmp = nullptr;
    VRC_HIP_CHECK( hipMalloc( &tmp, bytes ) );
    hipError_t e = hipStreamSynchronize( p->uploadStream );
    if( e == hipSuccess )
    {
        vrc_layout lay;
        for( int a = 0; a < 3; ++a )
        {
            lay.slots[a] = p->slots[a];
            lay.slotDim[a] = p->slotDim[a];
        }
        /* offset-binary voxels come back signed; a 4-byte atlas comes back as what it holds, float32 */
        e = vrc_launch_read_region( p->dAtlas, tmp, p->elemBytes, origin, size, lay,
                                    p->uploadStream, p->xform == VRC_XF_FLIP ? VRC_XF_FLIP : VRC_XF_NONE );
    }
    if( e == hipSuccess ) e = hipStreamSynchronize( p->uploadStream );
    if( e == hipSuccess ) e = hipMemcpy( hostOut, tmp, bytes, hipMemcpyDeviceToHost );
    (void)hipFree( tmp );
    if( e != hipSuccess )
        return fail( VRC_EHIP, std::string( "vrc_pool_read_region: " ) + hipGetErrorString( e ) );
    return VRC_OK;
}

/* brick histograms bin unsigned 8/16-bit voxels over the type's range */
static bool pool_has_histograms( const vrc_pool* p )
{
    return p->voxelType == VRC_VOXEL_UINT8 || p->voxelType == VRC_VOXEL_UINT16;
}

int vrc_pool_histogram( vrc_pool* p, const float slot[3], const uint32_t origin[3],
                        const uint32_t size[3], uint32_t binCount, uint64_t scaleFactor,
                        uint64_t* hostBins )
{
    if( !p || !slot || !origin || !size || !hostBins )
        return fail( VRC_EINVAL, "vrc_pool_histogram: NULL argument" );
    if( slot[0] < 0.f || slot[1] < 0.f || slot[2] < 0.f )
        return fail( VRC_EINVAL, "vrc_pool_histogram: invalid slot" );
    if( !pool_has_histograms( p ) )
        return fail( VRC_EUNSUPPORTED, "vrc_pool_histogram: histograms of signed, 32-bit and float voxels are not implemented" );
    const uint32_t typeRange = p->elemBytes == 1 ? 256u : 65536u;
    if( binCount == 0 || binCount > 4096 || typeRange % binCount != 0 )
        return fail( VRC_EINVAL, "vrc_pool_histogram: bin count must divide the voxel type's range (max 4096)" );
    for( int a = 0; a < 3; ++a )
        if( (uint64_t)origin[a] + size[a] > p->slotDim[a] )
            return fail( VRC_EINVAL, "vrc_pool_histogram: region outside the slot" );
    for( int a = 0; a < 3; ++a )
        if( size[a] == 0 )
        {
            std::fill( hostBins, hostBins + binCount, (uint64_t)0 );
            return VRC_OK;
        }
    VRC_HIP_CHECK( hipSetDevice( p->device ) );
    uint32_t o[3];
    pool_slot_voxel( p, slot, o );
    vrc_hist_entry en = {};
    en.base = vrc_slot_base( pool_layout( p ), o[0] / p->slotDim[0], o[1] / p->slotDim[1], o[2] / p->slotDim[2] );
    for( int a = 0; a < 3; ++a )
    {
        en.origin[a] = origin[a];
        en.size[a] = size[a];
    }
    /* the brick binning kernel into one row of uint32 counts (a slot holds < 2^24 voxels), scaled on the host */
    uint32_t* dRow = nullptr;
    VRC_HIP_CHECK( hipMalloc( &dRow, binCount * sizeof( uint32_t ) ) );
    std::vector< uint32_t > row( binCount );
    /* on the upload stream: ordered after the brick's own upload */
    hipError_t e = hipMemsetAsync( dRow, 0, binCount * sizeof( uint32_t ), p->uploadStream );
    if( e == hipSuccess )
        e = vrc_launch_bin_bricks( p->dAtlas, p->elemBytes, p->slotDim, nullptr, 0, &en, 0, binCount, dRow,
                                   p->uploadStream );
    if( e == hipSuccess )
        e = hipMemcpyAsync( row.data(), dRow, binCount * sizeof( uint32_t ), hipMemcpyDeviceToHost, p->uploadStream );
    if( e == hipSuccess )
        e = hipStreamSynchronize( p->uploadStream );
    (void)hipFree( dRow );
    if( e != hipSuccess )
        return fail( VRC_EHIP, std::string( "vrc_pool_histogram: " ) + hipGetErrorString( e ) );
    for( uint32_t b = 0; b < binCount; ++b )
        hostBins[b] = (uint64_t)row[b] * scaleFactor;
    return VRC_OK;
}

int vrc_pool_enable_histograms( vrc_pool* p, uint32_t binCount, const uint32_t overlap[3] )
{
    if( !p )
        return fail( VRC_EINVAL, "vrc_pool_enable_histograms: pool is NULL" );
    if( binCount != 0 && !pool_has_histograms( p ) )
        return fail( VRC_EUNSUPPORTED, "vrc_pool_enable_histograms: histograms of signed, 32-bit and float voxels are not implemented" );
    const uint32_t typeRange = p->elemBytes == 1 ? 256u : 65536u;
    if( binCount != 0 && ( !overlap || binCount > VRC_HIST_MAX_BINS || typeRange % binCount != 0 ) )
        return fail( VRC_EINVAL, "vrc_pool_enable_histograms: bin count must divide the voxel type's range (max 4096), "
                                 "overlap must be given" );
    if( binCount != 0 )
        for( int a = 0; a < 3; ++a )
            if( overlap[a] >= p->slotDim[a] )
                return fail( VRC_EINVAL, "vrc_pool_enable_histograms: overlap larger than the slot" );
    VRC_HIP_CHECK( hipSetDevice( p->device ) );
    std::lock_guard< std::mutex > lock( p->mutex );
    if( binCount == p->histBins && ( binCount == 0 || std::equal( overlap, overlap + 3, p->histOverlap ) ) )
        return VRC_OK;
    if( p->dHist )
    {
        /* a frame reduction may still read the table: wait for the device before freeing it */
        VRC_HIP_CHECK( hipDeviceSynchronize() );
        VRC_HIP_CHECK( hipFree( p->dHist ) );
        p->dHist = nullptr;
    }
    p->histBins = 0;
    p->histValid.clear();
    if( binCount == 0 )
        return VRC_OK;
    const size_t nSlots = p->resident.size();
    hipError_t e = hipMalloc( &p->dHist, nSlots * binCount * sizeof( uint32_t ) );
    if( e != hipSuccess )
    {
        p->dHist = nullptr;
        (void)hipGetLastError();
        return fail( e == hipErrorOutOfMemory ? VRC_ENOMEM : VRC_EHIP,
                     std::string( "vrc_pool_enable_histograms: " ) + hipGetErrorString( e ) );
    }
    p->histBins = binCount;
    std::copy( overlap, overlap + 3, p->histOverlap );
    p->histValid.assign( nSlots, 0 );
    /* the bricks resident now: one launch over all of them, behind every upload queued so far */
    std::vector< vrc_hist_entry > entries;
    uint64_t maxVoxels = 0;
    for( uint32_t index = 0; index < nSlots; ++index )
        if( p->resident[index] )
        {
            vrc_hist_entry en;
            if( pool_hist_entry( p, index, p->slotSize[index].data(), en ) )
            {
                entries.push_back( en );
                maxVoxels = std::max< uint64_t >( maxVoxels, (uint64_t)en.size[0] * en.size[1] * en.size[2] );
            }
            p->histValid[index] = 1;
        }
    vrc_hist_entry* dEntries = nullptr;
    e = hipMemsetAsync( p->dHist, 0, nSlots * binCount * sizeof( uint32_t ), p->uploadStream );
    if( e == hipSuccess && !entries.empty() )
        e = hipMalloc( &dEntries, entries.size() * sizeof( vrc_hist_entry ) );
    for( size_t first = 0; e == hipSuccess && first < entries.size(); first += 65535u )
    {
        const uint32_t n = (uint32_t)std::min< size_t >( 65535u, entries.size() - first );
        e = hipMemcpyAsync( dEntries + first, entries.data() + first, n * sizeof( vrc_hist_entry ),
                            hipMemcpyHostToDevice, p->uploadStream );
        if( e == hipSuccess )
            e = vrc_launch_bin_bricks( p->dAtlas, p->elemBytes, p->slotDim, dEntries + first, n, nullptr, maxVoxels,
                                       binCount, p->dHist, p->uploadStream );
    }
    if( e == hipSuccess )
        e = hipEventRecord( p->lastUpload, p->uploadStream );
    if( e == hipSuccess )
    {
        p->hasUpload = true;
        ++p->uploadGen;
    }
    if( dEntries )
    {
        const hipError_t e2 = hipStreamSynchronize( p->uploadStream ); /* the entries are read by the launch */
        (void)hipFree( dEntries );
        if( e == hipSuccess )
            e = e2;
    }
    if( e != hipSuccess )
    {
        (void)hipStreamSynchronize( p->uploadStream );
        (void)hipFree( p->dHist );
        p->dHist = nullptr;
        p->histBins = 0;
        p->histValid.clear();
        return fail( VRC_EHIP, std::string( "vrc_pool_enable_histograms: " ) + hipGetErrorString( e ) );
    }
    return VRC_OK;
}

/* ---------------------------------------------------------------------------------------- */
int vrc_update( vrc_ctx* c, const float tf[256 * 4], const float* planes, uint32_t nPlanes )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_update: ctx is NULL" );
    if( nPlanes > 6 )
        return fail( VRC_EINVAL, "vrc_update: more than 6 clip planes" );
    if( nPlanes > 0 && !planes )
        return fail( VRC_EINVAL, "vrc_update: planes is NULL" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    if( tf && std::memcmp( c->hTf, tf, 256 * 4 * sizeof( float ) ) != 0 )
    {
        /* 4 KiB, as cudaMemcpyToArray in cuda/ColorMap.cu:61-64.  The reference re-uploads every
         * frame (CudaRaycastRenderer.cpp:109-110); an unchanged map is skipped here, so the
         * per-frame call neither copies nor synchronizes.  The pinned copy may only be
         * rewritten once the previous async copy from it has been consumed. */
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        std::memcpy( c->hTf, tf, 256 * 4 * sizeof( float ) );
        c->tfGrey = true;
        for( int i = 0; i < 256 && c->tfGrey; ++i )
            c->tfGrey = std::memcmp( c->hTf + 4 * i, c->hTf + 4 * i + 1, sizeof( float ) ) == 0 &&
                        std::memcmp( c->hTf + 4 * i, c->hTf + 4 * i + 2, sizeof( float ) ) == 0;
        VRC_HIP_CHECK( hipMemcpyAsync( c->dTf, c->hTf, 256 * 4 * sizeof( float ),
                                       hipMemcpyHostToDevice, c->stream ) );
        ++c->tfVersion;
    }
    c->nPlanes = nPlanes;
    for( uint32_t i = 0; i < nPlanes; ++i )
        for( int k = 0; k < 4; ++k )
            c->planes[i][k] = planes[i * 4 + k];
    return VRC_OK;
}

static vrc_f4* ctx_fb( vrc_ctx* c ) { return c->fbExt ? c->fbExt : c->fbOwn; }

/* Do two frames cast the same rays?  Exactly the frame constants vrc_setup_ray_at reads (vrc_core.h) and the pixel
 * buffer's shape, bit for bit -- no tolerance, unlike the tile schedule's: a ray cache entry stands for the computed
 * ray.  (The contents of the row map: vrc_set_row_map forgets the frame before when they change.) */
static bool ray_constants_equal( const vrc_frame& a, const vrc_frame& b )
{
    return a.width == b.width && a.height == b.height && a.rowMap == b.rowMap && a.variant == b.variant &&
           a.nPlanes == b.nPlanes && std::memcmp( &a.vpX, &b.vpX, 4 * sizeof( float ) ) == 0 &&
           std::memcmp( &a.pixelOffX, &b.pixelOffX, 2 * sizeof( float ) ) == 0 &&
           std::memcmp( &a.nearPlane, &b.nearPlane, sizeof( float ) ) == 0 &&
           std::memcmp( a.eye, b.eye, sizeof( a.eye ) ) == 0 &&
           std::memcmp( a.invProj, b.invProj, sizeof( a.invProj ) ) == 0 &&
           std::memcmp( a.invView, b.invView, sizeof( a.invView ) ) == 0 &&
           std::memcmp( a.aabbMin, b.aabbMin, sizeof( a.aabbMin ) ) == 0 &&
           std::memcmp( a.aabbMax, b.aabbMax, sizeof( a.aabbMax ) ) == 0 &&
           std::memcmp( a.planes, b.planes, sizeof( a.planes ) ) == 0;
}

/* Do two frames of the same rays visit the same bricks over the same intervals?  What vrc_ray_grid_dda and
 * vrc_brick_interval read beside the ray, bit for bit (the node table itself: vrc_render forgets the lists when the
 * node list changes) */
static bool walk_constants_equal( const vrc_frame& a, const vrc_frame& b )
{
    return ray_constants_equal( a, b ) && a.nodeCount == b.nodeCount &&
           std::memcmp( &a.stepSize, &b.stepSize, sizeof( float ) ) == 0 &&
           std::memcmp( a.gridMin, b.gridMin, sizeof( a.gridMin ) ) == 0 &&
           std::memcmp( a.cellSize, b.cellSize, sizeof( a.cellSize ) ) == 0 &&
           std::memcmp( a.invCellSize, b.invCellSize, sizeof( a.invCellSize ) ) == 0 &&
           std::memcmp( a.gridDim, b.gridDim, sizeof( a.gridDim ) ) == 0;
}

int vrc_set_row_map( vrc_ctx* c, const uint32_t* rows, uint32_t n )
{
    if( !c || ( n && !rows ) )
        return fail( VRC_EINVAL, "vrc_set_row_map: NULL argument" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    if( n == c->rowMap.size() && ( n == 0 || std::memcmp( rows, c->rowMap.data(), n * sizeof( uint32_t ) ) == 0 ) )
        return VRC_OK;
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    VRC_TRY( ctx_grow( c, c->dRowMapCap, n, n, { c->dRowMap } ) );
    if( n )
        VRC_HIP_CHECK( hipMemcpy( c->dRowMap, rows, n * sizeof( uint32_t ), hipMemcpyHostToDevice ) );
    c->rowMap.assign( rows, rows + n );
    c->tileOrderValid = false;
    vrc_ray_forget( c->ray );
    vrc_walk_forget( c->walk.s ); /* (the stream was synchronised above) */
    return VRC_OK;
}

int vrc_pre_render( vrc_ctx* c, const vrc_view_data* view )
{
    if( !c || !view )
        return fail( VRC_EINVAL, "vrc_pre_render: NULL argument" );
    const uint32_t w = view->glViewport[2];
    const uint32_t h = c->rowMap.empty() ? view->glViewport[3] : (uint32_t)c->rowMap.size();
    if( w == 0 || h == 0 || view->glViewport[3] == 0 )
        return fail( VRC_EINVAL, "vrc_pre_render: empty viewport" );
    /* pixels are indexed in 32 bits (y * width + x) */
    if( (uint64_t)w * h > 0xFFFFFFFFull )
        return fail( VRC_EINVAL, "vrc_pre_render: a pixel buffer of 2^32 pixels or more" );
    for( uint32_t r : c->rowMap )
        if( r >= view->glViewport[3] )
            return fail( VRC_EINVAL, "vrc_pre_render: row map entry outside the frame" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    if( c->fbExt )
    {
        if( w != c->fbW || h != c->fbH )
            return fail( VRC_EINVAL, "vrc_pre_render: viewport differs from the external framebuffer" );
    }
    else
    {
        const size_t pixels = (size_t)w * h;
        VRC_TRY( ctx_grow( c, c->fbOwnPixels, pixels, pixels, { c->fbOwn } ) );
        c->fbW = w;
        c->fbH = h;
    }
    /* PixelBufferObject::mapBuffer clears the mapped buffer (cuda/PixelBufferObject.cu:80).  The
     * clear is folded into the first march of the frame (vrc_frame::clearFirst); whoever looks at
     * the buffer before a march has run gets it done then (resolve_clear). */
    c->clearPending = true;
    /* a new frame: its MIP passes start over, and it may take either projection */
    c->mipFirst = true;
    c->latch = vrc_latches();
    c->depthValid = false;
    c->gradValid = false;
    c->projState.pixels = 0u; /* vrc_get_projection_values: nothing to read until a MIP pass of this frame */
    return VRC_OK;
}

/* the pixel buffer is about to be read or re-pointed: do the clear pre_render promised */
static int resolve_clear( vrc_ctx* c )
{
    if( c->clearPending && ctx_fb( c ) && c->fbW && c->fbH )
    {
        VRC_HIP_CHECK( hipSetDevice( c->device ) );
        VRC_HIP_CHECK( hipMemsetAsync( ctx_fb( c ), 0, (size_t)c->fbW * c->fbH * sizeof( vrc_f4 ), c->stream ) );
    }
    c->clearPending = false;
    return VRC_OK;
}

int vrc_set_framebuffer( vrc_ctx* c, void* deviceRgba, uint32_t width, uint32_t height )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_set_framebuffer: ctx is NULL" );
    if( deviceRgba && ( width == 0 || height == 0 ) )
        return fail( VRC_EINVAL, "vrc_set_framebuffer: empty framebuffer" );
    if( deviceRgba && ( (uintptr_t)deviceRgba % 16u ) != 0 )
        return fail( VRC_EINVAL, "vrc_set_framebuffer: pointer must be 16-byte aligned" );
    VRC_TRY( resolve_clear( c ) );
    c->fbExt = (vrc_f4*)deviceRgba;
    if( deviceRgba )
    {
        c->fbW = width;
        c->fbH = height;
    }
    else
    {
        c->fbW = c->fbH = 0;
        if( c->fbOwn )
        {
            (void)hipSetDevice( c->device );
            (void)hipStreamSynchronize( c->stream );
            (void)hipFree( c->fbOwn );
            c->fbOwn = nullptr;
            c->fbOwnPixels = 0;
        }
    }
    return VRC_OK;
}

int vrc_get_framebuffer( vrc_ctx* c, void** deviceRgba, uint32_t* width, uint32_t* height )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_get_framebuffer: ctx is NULL" );
    VRC_TRY( resolve_clear( c ) );
    if( deviceRgba ) *deviceRgba = ctx_fb( c );
    if( width ) *width = c->fbW;
    if( height ) *height = c->fbH;
    return VRC_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* vrc_render is a sequence of phases (the render_* functions below, in the order they run); this is what they hand on.
 * The ORDER is part of the contract: the refusals of render_mode come before anything is launched or latched, those of
 * render_form after the tables are up to date; and every cached copy of the frame constants (tileOrderFrame,
 * depthFrame, rayPrevFrame, walk.prevFrame, walk.frame) is compared and taken with exactly the fields set that the
 * phases before it set -- a field set earlier makes an unchanged view compare unequal */
struct render_pass
{
    const vrc_view_data* view;
    const vrc_node_data* nodes;
    uint32_t nNodes;
    const vrc_render_data* render;
    vrc_pool* pool;
    vrc_lut_params lp;
    vrc_mode mode;        /* vrc_plan.h */
    vrc_form form;
    bool sameNodes, tableWalk; /* the node list of the vrc_render before, on the same pool; vrc_plan_table_walk */
    size_t pixels, plane; /* of the pixel buffer in use; of a plane of the ray and walk caches: its whole tiles */
    vrc_raycast_args a;
};

static int render_check_args( vrc_ctx* c, const vrc_view_data* view, const vrc_node_data* nodes, uint32_t nNodes,
                              const vrc_render_data* render, vrc_pool* pool )
{
    if( !c || !view || !render || !pool )
        return fail( VRC_EINVAL, "vrc_render: NULL argument" );
    if( nNodes > 0 && !nodes )
        return fail( VRC_EINVAL, "vrc_render: nodes is NULL" );
    if( pool->device != c->device )
        return fail( VRC_EINVAL, "vrc_render: pool lives on another device" );
    if( !ctx_fb( c ) || c->fbW == 0 )
        return fail( VRC_EINVAL, "vrc_render: vrc_pre_render has not been called" );
    if( view->glViewport[2] != c->fbW ||
        ( c->rowMap.empty() ? view->glViewport[3] : (uint32_t)c->rowMap.size() ) != c->fbH )
        return fail( VRC_EINVAL, "vrc_render: viewport differs from the pixel buffer" );
    if( render->samplesPerRay == 0 )
        return fail( VRC_EINVAL, "vrc_render: samplesPerRay is 0" );
    if( render->dataSourceRange[1] == render->dataSourceRange[0] )
        return fail( VRC_EINVAL, "vrc_render: empty data source range" );
    return VRC_OK;
}

/* which frame this pass renders, or why not: nothing has been launched or latched when it refuses */
static int render_mode( vrc_ctx* c, render_pass& p )
{
    /* signed 8/16-bit voxels are in the atlas offset-binary (v + 128 / + 32768): the range moves with them, and every
     * kernel form serves the pool as the unsigned one it then is (the trilinear filter commutes with the offset) */
    p.lp.rangeMin = p.render->dataSourceRange[0] + p.pool->rangeShift;
    p.lp.rangeMax = p.render->dataSourceRange[1] + p.pool->rangeShift;
    p.lp.alphaCorrection = (float)p.render->maxSamplesPerRay / (float)p.render->samplesPerRay;
    p.lp.fracBits = (int)c->opt.tfFracBits;
    const vrc_refusal r = vrc_plan_mode( c->opt, c->latch, c->rayLod, c->isoSet, c->isoValue, c->isoAmbient, p.pool->elemBytes, p.mode,
                                         c->sliceSet, c->slicePlane );
    return r.code == VRC_OK ? VRC_OK : fail( r.code, r.msg );
}

/* classified table, rebuilt only when one of its inputs changed; behind it the pre-integrated one */
static int render_tables( vrc_ctx* c, render_pass& p )
{
    const vrc_lut_params& lp = p.lp;
    const bool classify = p.mode.classify;
    /* per-ray LOD: one classified table per level, opacity exponent doubled per level (a level-j
     * brick is sampled with step * 2^j); always all levels, so the table does not depend on the list */
    const uint32_t lutLevels = ( c->rayLod && !classify ) ? (uint32_t)VRC_MAX_LOD_LEVELS : 1u;
    if( !c->lutValid || c->lutTfVersion != c->tfVersion || c->lutLinear != classify ||
        c->lutLevels != lutLevels || std::memcmp( &lp, &c->lutParams, sizeof( lp ) ) != 0 )
    {
        for( uint32_t j = 0; j < lutLevels; ++j )
        {
            vrc_lut_params lj = lp;
            lj.alphaCorrection = lp.alphaCorrection * (float)( 1u << j );
            VRC_HIP_CHECK( vrc_launch_build_lut( c->dTf, c->dLut + j * VRC_LUT_ENTRIES, lj, classify,
                                                 c->stream ) );
        }
        c->lutParams = lp;
        c->lutLinear = classify;
        c->lutLevels = lutLevels;
        c->lutTfVersion = c->tfVersion;
        c->lutValid = true;
        ++c->lutGen; /* (what was built from the table before -- the first-visit table -- is no longer current) */
        /* the largest classified opacity of a sample (same function as the device table, evaluated on the
         * pinned copy of the transfer function): decides whether early ray termination can occur at all */
        c->lutMaxAlpha = 1.0f;
        if( !classify )
        {
            float m = 0.0f;
            for( uint32_t d = 0; d < 256u; ++d )
                m = std::max( m, vrc_lut_entry( c->hTf, d, lp ).w );
            c->lutMaxAlpha = m;
        }
    }
    /* the pre-integrated table, behind the classified table on the stream (its value-indexed diagonal copies that one):
     * value-indexed where the frame marches stored bytes through the classified table, texel-indexed otherwise */
    if( p.mode.preint )
    {
        const int kind = classify ? VRC_PREINT_TEXEL : VRC_PREINT_VALUE;
        if( !c->dPreint )
            VRC_HIP_CHECK( hipMalloc( &c->dPreint, (size_t)VRC_PREINT_ENTRIES * sizeof( vrc_f4 ) ) );
        if( c->preintKind != kind || c->preintTfVersion != c->tfVersion ||
            std::memcmp( &lp, &c->preintParams, sizeof( lp ) ) != 0 )
        {
            VRC_HIP_CHECK( vrc_launch_build_preint( c->dTf, c->dLut, c->dPreint, lp, kind, c->stream ) );
            c->preintKind = kind;
            c->preintTfVersion = c->tfVersion;
            c->preintParams = lp;
            ++c->preintBuilds;
        }
    }
    return VRC_OK;
}

static vrc_atlas_geom pool_geom( const vrc_pool* pool )
{
    vrc_atlas_geom geom;
    for( int a = 0; a < 3; ++a )
    {
        geom.atlasDim[a] = pool->atlasDim[a];
        geom.slotDim[a] = pool->slotDim[a];
        geom.slots[a] = pool->slots[a];
    }
    return geom;
}

/* node table + brick grid (vrc_tables.h), re-derived and re-uploaded only when the node list changed
 * (the reference re-uploads synchronously every pass, Renderer.cu:259-267) */
static int render_nodes( vrc_ctx* c, render_pass& p )
{
    p.sameNodes = c->cachedPoolUid == p.pool->uid && c->cachedNodes.size() == p.nNodes && c->cachedRayLod == c->rayLod &&
                  std::memcmp( c->cachedNodes.data(), p.nodes, p.nNodes * sizeof( vrc_node_data ) ) == 0;
    if( p.sameNodes )
        return VRC_OK;
    vrc_walk_forget( c->walk.s ); /* the walk cache's lists index the node table that is replaced here */
    vrc_host_tables t;
    const vrc_atlas_geom geom = pool_geom( p.pool );
    vrc_build_tables( geom, p.nodes, p.nNodes, t );
    if( c->rayLod )
        vrc_build_lod_tables( geom, p.nodes, p.nNodes, t );
    const size_t nb = t.nodes.size() * sizeof( vrc_dev_node );
    const size_t gb = t.grid.size() * sizeof( int32_t );
    VRC_TRY( ctx_grow( c, c->dNodesCap, t.nodes.size(), std::max< size_t >( t.nodes.size(), 1024 ), { c->dNodes } ) );
    VRC_TRY( ctx_grow( c, c->dGridCap, t.grid.size(), std::max< size_t >( t.grid.size(), 4096 ), { c->dGrid } ) );
    /* pinned staging: kNodeStages areas of hStageCap bytes */
    bool grew = false;
    VRC_TRY( ctx_grow( c, c->hStageCap, nb + gb, ( std::max< size_t >( nb + gb, 1 << 18 ) + 255 ) / 256 * 256,
                       { { c->hStage, kNodeStages, 0, vrc_grown::PINNED } }, &grew ) );
    for( int i = 0; grew && i < kNodeStages; ++i )
        c->stageUsed[i] = false;
    const uint32_t stage = c->stageNext++ % kNodeStages;
    if( c->stageUsed[stage] ) /* the copies issued from this area four node lists ago */
        VRC_HIP_CHECK( hipEventSynchronize( c->stageEvent[stage] ) );
    if( !c->stageEvent[stage] )
        VRC_HIP_CHECK( hipEventCreateWithFlags( &c->stageEvent[stage], hipEventDisableTiming ) );
    uint8_t* h = (uint8_t*)c->hStage + (size_t)stage * c->hStageCap;
    std::memcpy( h, t.nodes.data(), nb );
    VRC_HIP_CHECK( hipMemcpyAsync( c->dNodes, h, nb, hipMemcpyHostToDevice, c->stream ) );
    if( gb )
    {
        std::memcpy( h + nb, t.grid.data(), gb );
        VRC_HIP_CHECK( hipMemcpyAsync( c->dGrid, h + nb, gb, hipMemcpyHostToDevice, c->stream ) );
    }
    VRC_HIP_CHECK( hipEventRecord( c->stageEvent[stage], c->stream ) );
    c->stageUsed[stage] = true;
    c->cachedNodes.assign( p.nodes, p.nodes + p.nNodes );
    c->cachedPoolUid = p.pool->uid;
    c->cachedGridOk = t.gridOk && !c->rayLod; /* the grid buffer holds the per-level tables */
    c->cachedOneCell = t.oneCellPerBrick;
    c->cachedRayLod = c->rayLod;
    c->cachedLodOk = t.lodOk;
    c->cachedLodLevels = t.lodLevels;
    c->cachedFinestVoxel = t.finestVoxelWorld;
    c->cachedClamp = t.clamp;
    c->cachedGridFrame = t.g;
    return VRC_OK;
}

/* which kernel form marches the frame (vrc_plan_form), or why none does; the pool's packed atlas where the form wants
 * it.  Refuses with the tables up to date, as it always has; VRC_ENOMEM is the last refusal of all */
static int render_form( vrc_ctx* c, render_pass& p )
{
    const vrc_pool* const pool = p.pool;
    const vrc_form_facts k = { c->rayLod, c->cachedGridOk, c->cachedOneCell, c->cachedLodOk, c->cachedClamp, p.nNodes,
                               p.render->samplesPerPixel, { pool->slotDim[0], pool->slotDim[1], pool->slotDim[2] },
                               pool->elemBytes, pool->bigAtlas, pool_packed_possible( pool ) };
    const vrc_refusal r = vrc_plan_form( c->opt, p.mode, k, p.form );
    if( r.code != VRC_OK )
        return fail( r.code, r.msg );
    p.form.usePacked = p.form.packed != VRC_PACKED_NONE && pool_enable_packed( p.pool );
    if( p.form.packed == VRC_PACKED_REQUIRED && !p.form.usePacked )
        return fail( vrc_plan_no_packed_memory.code, vrc_plan_no_packed_memory.msg );
    p.form.useLds = vrc_plan_use_lds( c->opt, p.mode, k, p.form, p.form.usePacked );
    p.tableWalk = vrc_plan_table_walk( c->opt, p.mode, k, p.form );
    return VRC_OK;
}

/* the frame constants, as far as every cached copy of them compares them */
static void render_frame( vrc_ctx* c, render_pass& p )
{
    std::memset( &p.a, 0, sizeof( p.a ) );
    p.a.shade = p.mode.shade;
    p.a.cdepth = p.mode.cdepth;
    p.a.preint = p.mode.preint;
    p.a.slice = p.mode.slice;
    vrc_frame& f = p.a.frame;
    /* the GLSL twin casts through the pixel centre (gl_FragCoord, fragRaycast.glsl:127), the
     * CUDA kernel through the pixel corner (Renderer.cu:106-112) */
    const float centre = c->opt.variant == VRC_VARIANT_GLRAYCASTER ? 0.5f : 0.0f;
    vrc_fill_frame( f, *p.view, *p.render, pool_geom( p.pool ), c->cachedGridFrame, c->planes, c->nPlanes, p.nNodes,
                    c->fbW, c->fbH, centre, centre );
    f.rowMap = c->rowMap.empty() ? nullptr : c->dRowMap;
    f.variant = c->opt.variant == VRC_VARIANT_GLRAYCASTER ? VRC_VARIANT_GL : VRC_VARIANT_CUDA;
    f.samplesPerPixel = ( f.variant == VRC_VARIANT_GL && p.render->samplesPerPixel > 1u ) ? p.render->samplesPerPixel : 1u;
    if( c->rayLod )
    {
        f.lodLevels = c->cachedLodLevels;
        f.lodBase = (float)( c->cachedFinestVoxel /
                             ( (double)c->rayLodSse * (double)c->rayLodWorldPerPixel ) );
    }
    p.pixels = (size_t)c->fbW * c->fbH;
    p.plane = (size_t)( ( c->fbW + VRC_TILE_W - 1 ) / VRC_TILE_W ) * ( ( c->fbH + VRC_TILE_H - 1 ) / VRC_TILE_H ) * 64u;
}

/* tile schedule, recomputed only when the frame constants changed */
static int render_tile_schedule( vrc_ctx* c, render_pass& p )
{
    const vrc_frame& f = p.a.frame;
    p.a.tileOrder = nullptr;
    if( !c->opt.tileOrder )
        return VRC_OK;
    /* one entry per schedule slot: four per 2x2 block of tiles (vrc_internal.h) */
    const size_t nTiles = vrc_schedule_slots( ( c->fbW + VRC_TILE_W - 1 ) / VRC_TILE_W,
                                              ( c->fbH + VRC_TILE_H - 1 ) / VRC_TILE_H );
    /* order[nTiles] | scratch[VRC_TILE_SCRATCH_WORDS] | bucket[nTiles] (bytes) */
    bool grew = false;
    VRC_TRY( ctx_grow( c, c->dTileOrderCap, nTiles, nTiles,
                       { { c->dTileOrder, sizeof( uint32_t ) + 1, VRC_TILE_SCRATCH_WORDS * sizeof( uint32_t ) } }, &grew ) );
    if( grew )
        c->tileOrderValid = false;
    /* The schedule is a heuristic (any permutation of the tiles renders the same frame): a camera
     * that moved a little keeps the last one -- same pixel buffer and volume box, eye and ray
     * matrices within 2 % -- for at most 15 frames in a row; two small kernels and a memset
     * less per frame of an orbit. */
    bool reuse = c->tileOrderValid;
    if( reuse && std::memcmp( &c->tileOrderFrame, &f, sizeof( f ) ) != 0 )
    {
        const vrc_frame& o = c->tileOrderFrame;
        reuse = c->tileOrderReused < 15u && o.width == f.width && o.height == f.height && o.vpW == f.vpW &&
                o.vpH == f.vpH && o.vpX == f.vpX && o.vpY == f.vpY && o.pixelOffX == f.pixelOffX &&
                o.pixelOffY == f.pixelOffY && o.rowMap == f.rowMap && o.nPlanes == f.nPlanes &&
                std::memcmp( o.planes, f.planes, sizeof( f.planes ) ) == 0 &&
                std::memcmp( o.aabbMin, f.aabbMin, sizeof( f.aabbMin ) ) == 0 &&
                std::memcmp( o.aabbMax, f.aabbMax, sizeof( f.aabbMax ) ) == 0 &&
                std::memcmp( o.invProj, f.invProj, sizeof( f.invProj ) ) == 0;
        for( int i = 0; reuse && i < 3; ++i )
            reuse = std::fabs( o.eye[i] - f.eye[i] ) <= 0.02f;
        for( int i = 0; reuse && i < 16; ++i )
            reuse = std::fabs( o.invView[i] - f.invView[i] ) <= 0.02f;
        if( reuse )
            ++c->tileOrderReused;
    }
    if( !reuse )
    {
        c->tileOrderReused = 0;
        VRC_HIP_CHECK( vrc_launch_tile_order( f, c->dTileOrder, c->dTileOrder + c->dTileOrderCap,
                                              (uint8_t*)( c->dTileOrder + c->dTileOrderCap + VRC_TILE_SCRATCH_WORDS ),
                                              c->stream ) );
        std::memcpy( &c->tileOrderFrame, &f, sizeof( f ) );
        c->tileOrderValid = true;
    }
    p.a.tileOrder = c->dTileOrder;
    return VRC_OK;
}

/* fold the frame's clear into this march (after the tile-schedule cache compared frames), and hand it the pool's
 * uniformity words (VRC_OPT_UNIFORM_BRICKS): NULL = every brick takes the general march */
static void render_clear_and_slot_words( vrc_ctx* c, render_pass& p )
{
    p.a.frame.clearFirst = c->clearPending ? 1u : 0u;
    c->clearPending = false;
    p.a.frame.slotInfo = c->opt.uniformBricks ? p.pool->dSlotInfo : nullptr;
}

/* The running state per pixel of the pixel buffer in use, grown with it: dMipMax (a MIP frame's M, a composite-depth
 * frame's V) and dMipDepth (the D of both).  A later pass of a frame whose pixel buffer grew (vrc_set_framebuffer), or
 * whose buffer before was large enough from an earlier frame and keeps the passes so far, fills the new one with
 * "nothing known as far as this buffer knows": all bits set for the value, +infinity for the depth (no sample equals M,
 * no pixel has crossed).  The first pass of a frame reads neither (mipFirst) */
static int grow_pixel_values( vrc_ctx* c, size_t pixels )
{
    bool grew = false;
    VRC_TRY( ctx_grow( c, c->dMipMaxPixels, pixels, pixels, { c->dMipMax }, &grew ) );
    if( grew && !c->mipFirst )
        VRC_HIP_CHECK( hipMemsetAsync( c->dMipMax, 0xFF, pixels * sizeof( uint32_t ), c->stream ) );
    return VRC_OK;
}
static int grow_pixel_depths( vrc_ctx* c, size_t pixels )
{
    bool grew = false;
    VRC_TRY( ctx_grow( c, c->dMipDepthPixels, pixels, pixels, { c->dMipDepth }, &grew ) );
    if( grew && !c->mipFirst )
        VRC_HIP_CHECK( hipMemsetD32Async( reinterpret_cast< hipDeviceptr_t >( c->dMipDepth ), 0x7F800000, pixels, c->stream ) );
    return VRC_OK;
}

/* what a pass leaves for vrc_get_projection_values and vrc_get_projection_depths */
static void leave_projection( vrc_ctx* c, render_pass& p, uint32_t fold, bool sums )
{
    c->depthValid = p.mode.mipDepth || p.mode.cdepth || p.mode.slice;
    c->sliceFrame = p.mode.slice;
    if( c->depthValid )
    {
        c->depthFrame = p.a.frame;
        c->depthRows = c->rowMap;
    }
    c->mipFirst = false;
    c->projState.mipMax = c->dMipMax;
    c->projState.meanSum = sums ? c->dMeanSum : nullptr;
    c->projState.meanCount = sums ? c->dMeanCount : nullptr;
    c->projState.pixels = (uint32_t)p.pixels;
    c->projState.fold = fold;
    c->projState.floatState = ( p.mode.linear || p.pool->elemBytes == 4 ) ? 1u : 0u;
    c->projState.shift = p.pool->rangeShift;
}

/* projection state: the per-pixel buffers of a MIP, isosurface or composite-depth frame, what the pass leaves for the
 * read-backs, and the latches -- written here and nowhere else, each by the pass that read its option */
static int render_projection( vrc_ctx* c, render_pass& p )
{
    vrc_pool* const pool = p.pool;
    const vrc_mode& m = p.mode;
    vrc_frame& f = p.a.frame;
    const size_t pixels = p.pixels;
    if( m.mip )
    {
        bool grew = false;
        VRC_TRY( grow_pixel_values( c, pixels ) );
        if( m.mean )
        {
            VRC_TRY( ctx_grow( c, c->dMeanPixels, pixels, pixels, { c->dMeanSum, c->dMeanCount }, &grew ) );
            if( grew && !c->mipFirst ) /* no sample yet, which is a sum of 0 (integer and double alike) and a count of 0 */
            {
                VRC_HIP_CHECK( hipMemsetAsync( c->dMeanSum, 0, pixels * sizeof( unsigned long long ), c->stream ) );
                VRC_HIP_CHECK( hipMemsetAsync( c->dMeanCount, 0, pixels * sizeof( uint32_t ), c->stream ) );
            }
        }
        f.mipMax = c->dMipMax;
        f.mipFirst = c->mipFirst ? 1u : 0u;
        f.slotMax = c->opt.mipSkip ? pool->dSlotMax : nullptr;
        f.slotMin = c->opt.mipSkip ? pool->dSlotMin : nullptr;
        f.meanSum = m.mean ? c->dMeanSum : nullptr;
        f.meanCount = m.mean ? c->dMeanCount : nullptr;
        if( m.mipDepth )
            VRC_TRY( grow_pixel_depths( c, pixels ) );
        f.mipDepth = m.mipDepth ? c->dMipDepth : nullptr;
        f.mipCue = ( m.mipDepth && !m.iso ) ? (float)c->opt.mipDepthCue / 1000.0f : 0.0f;
        if( m.iso )
        {
            VRC_TRY( ctx_grow( c, c->dIsoGradPixels, pixels, pixels, { { c->dIsoGrad, 3u * sizeof( float ) } }, &grew ) );
            if( grew && !c->mipFirst ) /* (as dMipDepth: no hit yet as far as this buffer knows) */
                VRC_HIP_CHECK( hipMemsetAsync( c->dIsoGrad, 0, pixels * 3u * sizeof( float ), c->stream ) );
            f.isoGrad = c->dIsoGrad;
            f.isoThreshold = vrc_iso_int_threshold( c->isoValue, pool->rangeShift, pool->elemBytes == 1 ? 255u : 65535u );
            f.isoStored = vrc_iso_float_threshold( c->isoValue, pool->rangeShift );
            f.isoClassify = c->isoValue + pool->rangeShift;
            f.isoAmbient = c->isoAmbient;
            c->latch.iso = true;
            c->latch.isoValue = c->isoValue;
            c->latch.isoAmbient = c->isoAmbient;
        }
        c->gradValid = m.iso;
        if( !m.mean && !m.iso )
        {
            c->latch.depth = c->opt.mipDepth;
            c->latch.cue = c->opt.mipDepthCue;
        }
        if( !m.iso )
            c->latch.fold = c->opt.mipFold;
        leave_projection( c, p, m.iso ? (uint32_t)VRC_FOLD_FIRST : (uint32_t)c->opt.mipFold, true );
    }
    if( m.cdepth )
    {
        /* the pair per pixel where a MIP frame's running maximum and depth are: grown, invalidated by vrc_pre_render
         * (mipFirst) and not read by the frame's first pass as those are */
        VRC_TRY( grow_pixel_values( c, pixels ) );
        VRC_TRY( grow_pixel_depths( c, pixels ) );
        f.mipMax = c->dMipMax;
        f.mipDepth = c->dMipDepth;
        f.mipFirst = c->mipFirst ? 1u : 0u;
        c->gradValid = false;
        leave_projection( c, p, (uint32_t)VRC_FOLD_FIRST, false ); /* V as a first-crossing frame leaves it */
    }
    if( m.slice )
    {
        /* (V, D) per pixel where a composite-depth frame keeps its pair, read back as that frame's are; the plane goes
         * into the frame behind the tile schedule's comparison of frames, which does not depend on it */
        VRC_TRY( grow_pixel_values( c, pixels ) );
        VRC_TRY( grow_pixel_depths( c, pixels ) );
        f.mipMax = c->dMipMax;
        f.mipDepth = c->dMipDepth;
        f.mipFirst = c->mipFirst ? 1u : 0u;
        for( int i = 0; i < 4; ++i )
            f.slicePlane[i] = c->latch.slicePlane[i] = c->slicePlane[i];
        c->latch.slice = true;
        c->gradValid = false;
        leave_projection( c, p, (uint32_t)VRC_FOLD_FIRST, false );
    }
    f.cdepthTau = m.cdepth ? (float)c->opt.compositeDepth / 1000.0f : 0.0f;
    f.preintTable = m.preint ? c->dPreint : nullptr;
    f.shadeAmbient = m.shade ? (float)c->opt.shadingAmbient / 1000.0f : 0.0f;
    c->latch.projection = c->opt.projection;
    if( !m.mip && !m.slice )
    {
        c->latch.preint = c->opt.preint;
        c->latch.compositeDepth = c->opt.compositeDepth;
        c->latch.shading = c->opt.shading;
        c->latch.shadingAmbient = c->opt.shadingAmbient;
    }
    return VRC_OK;
}

/* the launcher's arguments; the depth split and ray compaction of the table walk kernel */
static int render_split_and_compact( vrc_ctx* c, render_pass& p )
{
    vrc_pool* const pool = p.pool;
    vrc_raycast_args& a = p.a;
    const vrc_frame& f = a.frame;
    const bool gridWalk = p.form.useDda || c->rayLod;
    a.nodes = c->dNodes;
    a.gridTable = gridWalk ? c->dGrid : nullptr;
    a.atlas = p.form.usePacked ? pool->dPacked : pool->dAtlas;
    a.packed = p.form.usePacked;
    /* a packed atlas of more than 4 GiB, or of a pool of more than 2^32 voxels: 64-bit lane pointers (the BIG instances of
     * the packed modes) */
    a.packedWide = p.form.usePacked && ( pool->bigAtlas || pool_packed_bytes( pool ) > 0xFFFFFFFFull );
    a.lut = c->dLut;
    a.pixelBuffer = ctx_fb( c );
    a.sampleCounter = c->opt.count ? c->dCounter : nullptr;
    a.clamp = c->cachedClamp;
    a.gridDda = p.form.useDda;
    a.fixedStepping = c->opt.stepping != 0 && p.form.slotsFit8Bits;
    a.linear = p.mode.linear;
    a.elemBytes = pool->elemBytes;
    a.bigAtlas = pool->bigAtlas;
    a.classifier = vrc_make_classifier( p.lp );
    /* grey transfer function, frame starting from zero: two-float table entries, the same bits (VRC_MODE_GREY) */
    a.greyTable = c->opt.greyTable && c->tfGrey && f.clearFirst && !p.form.glSuper; /* (a sub-ray starts from the pixel so far) */
    /* depth split: only where it is exact.  (i) The far half cannot know the near half's opacity, so early ray
     * termination must be impossible: (1 - largest classified alpha)^(most samples a ray can take) stays above
     * 1 - 0.999 (a ray crosses at most sqrt(3) world units -- the volume's longest edge is 1 -- plus one
     * restart sample per brick).  (ii) The frame starts from zero (first pass: the clear is folded in).
     * (iii) the table-driven point-sampling walk kernel. */
    a.depthSplit = false;
    if( c->opt.depthSplit && p.tableWalk && f.clearFirst )
    {
        const double nMax = 1.7320508 * (double)p.render->samplesPerRay +
                            3.0 * ( f.gridDim[0] + f.gridDim[1] + f.gridDim[2] ) + 8.0;
        /* with a margin: the kernel accumulates the opacity in float with contracted multiply-adds and regroups the
         * far half's additions, ~1e-6 absolute after 2000 samples = 1e-3 of the 0.001 of transmittance left at
         * the threshold; the bound must clear the threshold by ten times that (0.01 in the logarithm), so that a
         * frame at the limit takes the single-wave kernel rather than a split that might meet an early exit */
        a.depthSplit = VRC_TILE_W == 8u && c->lutMaxAlpha < 1.0f &&
                       nMax * std::log1p( -(double)c->lutMaxAlpha ) > std::log( 1.0 - 0.999 ) + 0.01;
    }
    /* ray compaction: the table walk kernel; packed 16-bit pixel coordinates */
    a.ertParts = 0;
    a.rayList = nullptr;
    /* (the same predicate as the launcher's, vrc_launch_raycast: what vrc_get_ray_counts reports is what ran) */
    if( c->opt.ertParts > 1 && p.tableWalk && !a.depthSplit && c->fbW < 65536u && c->fbH < 65536u && VRC_TILE_W == 8u )
    {
        /* counts | two ray lists (vrc_internal.h) */
        VRC_TRY( ctx_grow( c, c->dRayListCap, p.pixels, p.pixels,
                           { { c->dRayList, 2 * sizeof( uint32_t ), VRC_MAX_ERT_PARTS * sizeof( uint32_t ) } } ) );
        a.ertParts = (int)c->opt.ertParts;
        a.rayList = c->dRayList;
    }
    c->lastErtParts = a.ertParts;
    return VRC_OK;
}

/* whose rays the ray cache keeps: a slice frame's or another frame's.  A change of kind forgets them (vrc_ctx::rayOfSlice) */
static void render_ray_kind( vrc_ctx* c, const render_pass& p )
{
    if( c->rayOfSlice != p.mode.slice )
    {
        vrc_ray_forget( c->ray );
        c->rayOfSlice = p.mode.slice;
    }
}

/* ray cache (VRC_OPT_RAY_CACHE): the tile-scheduled grid walk of vrc_k_raycast only (vrc_pixel_grid_dda; the
 * supersampled GL variant, whose rays are jittered, is not a grid walk).  Compute, store or load: vrc_plan_ray_cache.
 * The kernel-visible fields are set here, after the tile schedule compared frames */
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

/* has the count pass's answer arrived?  Polled, never waited for */
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

/* what the plan asks for, in the order vrc_walk_reached names: the count pass's three objects or the lists; the
 * first-visit table, built here; the resolved planes */
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

/* walk cache (VRC_OPT_WALK_CACHE) and the riders of its replay: the rules are vrc_plan.h's.  Here: the facts, the poll,
 * the memory, and the frame's fields from the plan (c->walkPlan; render_march launches what it asks for) */
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

/* the march: behind the pool's uploads, the walk cache's passes in front of it, the timing pair around it, the pool's
 * fence and the counter's read-back behind it */
static int render_march( vrc_ctx* c, render_pass& p )
{
    vrc_raycast_args& a = p.a;
    vrc_frame& f = a.frame;
    const vrc_mode& m = p.mode;
    /* order the march after every brick upload issued so far (fixes quirk Q9) */
    VRC_TRY( ctx_wait_uploads( c, p.pool ) );
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
    if( c->opt.count )
        VRC_HIP_CHECK( hipMemsetAsync( c->dCounter, 0, sizeof( unsigned long long ), c->stream ) );
    if( c->opt.timing && c->evUsed == c->evRing->pairs.size() )
    {
        if( c->evRing->pairs.size() >= 4096 )
        {
            /* nobody has read the timings for 4096 launches: fold them into running sums (waits for the
             * launches still in flight, once per 4096) so that vrc_get_stats still accounts for every one */
            VRC_HIP_CHECK( hipEventSynchronize( c->evRing->pairs[c->evUsed - 1].second ) );
            for( size_t i = 0; i < c->evUsed; ++i )
            {
                float ms = 0.f;
                VRC_HIP_CHECK( hipEventElapsedTime( &ms, c->evRing->pairs[i].first, c->evRing->pairs[i].second ) );
                c->evFoldedMs += ms;
            }
            c->evFoldedLaunches += (uint32_t)c->evUsed;
            c->evUsed = 0;
        }
        else
        {
            hipEvent_t a0 = nullptr, a1 = nullptr;
            VRC_HIP_CHECK( hipEventCreate( &a0 ) );
            VRC_HIP_CHECK( hipEventCreate( &a1 ) );
            c->evRing->pairs.push_back( { a0, a1 } );
        }
    }
    const std::pair< hipEvent_t, hipEvent_t > evp =
        c->opt.timing ? c->evRing->pairs[c->evUsed++] : std::pair< hipEvent_t, hipEvent_t >( nullptr, nullptr );
    vrc_internal_note_kernel_fn( nullptr, 0, 0 ); /* set again by the launchers that report their occupancy */
    /* VRC_OPT_STREAM_MARKERS = 0: the dispatch of a timed march that is one launch carries the pair's second event as its
     * stop event, and that event is also what an upload that recycles a slot waits for.  The pair's first event is
     * recorded in front of the dispatch: the runtime puts a marker on the queue for an attached start event all the
     * same, and a dispatch that carries one holds up a copy queued behind it (profiles/r8_frame_packets.txt).  A
     * launcher says whether it attached the event; the marches of several launches (depth split, ray compaction) do
     * not, and theirs is recorded behind the sequence.  VRC_OPT_STREAM_MARKERS = 1, and a march that is not timed,
     * record the pool's own fence behind the march */
    const bool pairFences = c->opt.timing && !c->opt.streamMarkers;
    bool attached = false;
    a.stopEvent = pairFences ? evp.second : nullptr;
    a.attached = &attached;
    if( c->opt.timing )
        VRC_HIP_CHECK( hipEventRecord( evp.first, c->stream ) );
    VRC_HIP_CHECK( m.iso        ? vrc_launch_raycast_iso( a, c->stream )
                   : m.mipDepth ? vrc_launch_raycast_mip_depth( a, (int)c->opt.mipFold, c->stream )
                   : m.mip      ? ( c->opt.mipFold == VRC_MIP_FOLD_MIN    ? vrc_launch_raycast_minip( a, c->stream )
                                    : c->opt.mipFold == VRC_MIP_FOLD_MEAN ? vrc_launch_raycast_meanip( a, c->stream )
                                                                          : vrc_launch_raycast_mip( a, c->stream ) )
                   : m.slice    ? vrc_launch_raycast_slice( a, c->stream )
                   : m.cdepth   ? vrc_launch_raycast_cdepth( a, c->stream )
                   : m.preint   ? vrc_launch_raycast_preint( a, c->stream )
                   : m.shade    ? vrc_launch_raycast_shade( a, c->stream )
                   : p.form.useLds ? vrc_launch_raycast_lds( a, c->stream ) /* (also its per-ray LOD form) */
                   : c->rayLod  ? vrc_launch_raycast_raylod( a, c->stream )
                   : pl.used == 4      ? vrc_launch_raycast_replay( a, c->stream )
                                : vrc_launch_raycast( a, c->stream ) );
    if( c->rayCacheUsed == VRC_RAY_STORE )
        vrc_ray_stored( c->ray );
    if( c->opt.timing && !attached ) /* (also a frame without tiles, which launches nothing) */
        VRC_HIP_CHECK( hipEventRecord( evp.second, c->stream ) );
    VRC_TRY( pool_fence_behind( p.pool, c, pairFences ? evp.second : nullptr ) );
    if( c->opt.count )
        VRC_HIP_CHECK( hipMemcpyAsync( c->hCounter, c->dCounter, sizeof( unsigned long long ),
                                       hipMemcpyDeviceToHost, c->stream ) );
    return VRC_OK;
}

static void render_stats( vrc_ctx* c, const render_pass& p )
{
    const bool gridWalk = p.form.useDda || c->rayLod;
    c->timed = true; /* a render has happened: vrc_get_stats has something to report */
    c->stats.kernel_variant = c->rayLod          ? VRC_KERNEL_RAY_LOD
                              : p.form.useLds    ? VRC_KERNEL_LDS
                              : p.form.usePacked ? VRC_KERNEL_PACKED
                              : p.form.useDda    ? VRC_KERNEL_GRID_DDA
                                                 : VRC_KERNEL_REFERENCE_ORDER;
    for( int i = 0; i < 3; ++i )
        c->stats.grid_dims[i] = gridWalk ? (uint32_t)p.a.frame.gridDim[i] : 0u;
    c->gridWalkUsed = gridWalk ? 1 : 0;
}

int vrc_render( vrc_ctx* c, const vrc_view_data* view, const vrc_node_data* nodes, uint32_t nNodes,
                const vrc_render_data* render, vrc_pool* pool )
{
    VRC_TRY( render_check_args( c, view, nodes, nNodes, render, pool ) );
    if( nNodes == 0 ) /* CudaRaycastRenderer.cpp:157-158 */
        return VRC_OK;
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    render_pass p;
    p.view = view;
    p.nodes = nodes;
    p.nNodes = nNodes;
    p.render = render;
    p.pool = pool;
    VRC_TRY( render_mode( c, p ) );
    VRC_TRY( render_tables( c, p ) );
    VRC_TRY( render_nodes( c, p ) );
    VRC_TRY( render_form( c, p ) );
    render_frame( c, p );
    VRC_TRY( render_tile_schedule( c, p ) );
    render_clear_and_slot_words( c, p );
    VRC_TRY( render_projection( c, p ) );
    VRC_TRY( render_split_and_compact( c, p ) );
    render_ray_kind( c, p );
    VRC_TRY( render_ray_cache( c, p ) );
    VRC_TRY( render_walk_cache( c, p ) );
    VRC_TRY( render_march( c, p ) );
    render_stats( c, p );
    return VRC_OK;
}

int vrc_post_render( vrc_ctx* c, float* hostRgba )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_post_render: ctx is NULL" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_TRY( resolve_clear( c ) ); /* a frame without a march still ends cleared */
    if( hostRgba )
    {
        if( !ctx_fb( c ) || c->fbW == 0 )
            return fail( VRC_EINVAL, "vrc_post_render: no pixel buffer" );
        VRC_HIP_CHECK( hipMemcpyAsync( hostRgba, ctx_fb( c ),
                                       (size_t)c->fbW * c->fbH * sizeof( vrc_f4 ),
                                       hipMemcpyDeviceToHost, c->stream ) );
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    }
    return VRC_OK;
}

static_assert( VRC_MIP_FOLD_MAX == VRC_FOLD_MAX && VRC_MIP_FOLD_MIN == VRC_FOLD_MIN && VRC_MIP_FOLD_MEAN == VRC_FOLD_MEAN,
               "the option's values are the march's folds" );

int vrc_get_projection_values( vrc_ctx* c, float* hostValues, uint32_t* hostCounts )
{
    if( !c || !hostValues )
        return fail( VRC_EINVAL, "vrc_get_projection_values: NULL argument" );
    if( c->projState.pixels == 0u )
        return fail( VRC_EINVAL, "vrc_get_projection_values: no VRC_OPT_PROJECTION = MIP, ISO or SLICE vrc_render since the last "
                                 "vrc_pre_render; the values exist from a frame's first such pass until the next frame" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    const size_t pixels = c->projState.pixels;
    VRC_TRY( ctx_grow( c, c->dProjOutPixels, pixels, pixels, { { c->dProjOut, sizeof( float ) + sizeof( uint32_t ) } } ) );
    uint32_t* const dCounts = reinterpret_cast< uint32_t* >( c->dProjOut + pixels );
    VRC_HIP_CHECK( vrc_launch_projection_values( c->projState, c->dProjOut, dCounts, c->stream ) );
    VRC_HIP_CHECK( hipMemcpyAsync( hostValues, c->dProjOut, pixels * sizeof( float ), hipMemcpyDeviceToHost, c->stream ) );
    if( hostCounts )
        VRC_HIP_CHECK( hipMemcpyAsync( hostCounts, dCounts, pixels * sizeof( uint32_t ), hipMemcpyDeviceToHost, c->stream ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    return VRC_OK;
}

int vrc_get_projection_depths( vrc_ctx* c, float* hostT, float* hostXyz )
{
    if( !c || !hostT )
        return fail( VRC_EINVAL, "vrc_get_projection_depths: NULL argument" );
    if( c->projState.pixels == 0u )
        return fail( VRC_EINVAL, "vrc_get_projection_depths: no VRC_OPT_PROJECTION = MIP, ISO or SLICE vrc_render since the last "
                                 "vrc_pre_render; the depths exist from a frame's first such pass until the next frame" );
    if( c->projState.fold == (uint32_t)VRC_MIP_FOLD_MEAN )
        return fail( VRC_EINVAL, "vrc_get_projection_depths: the frame's fold is VRC_MIP_FOLD_MEAN (VRC_OPT_MIP_FOLD); the mean "
                                 "has no position" );
    if( !c->depthValid )
        return fail( VRC_EINVAL, "vrc_get_projection_depths: the frame's MIP passes ran without depth tracking "
                                 "(VRC_OPT_MIP_DEPTH = 0 and VRC_OPT_MIP_DEPTH_CUE = 0)" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    const size_t pixels = c->projState.pixels;
    vrc_frame f = c->depthFrame;
    if( pixels != (size_t)f.width * f.height || ( !c->depthRows.empty() && c->depthRows.size() != f.height ) )
        return fail( VRC_EINVAL, "vrc_get_projection_depths: the frame's geometry does not match its state" );
    const size_t words = pixels * 4u + f.height;
    VRC_TRY( ctx_grow( c, c->dDepthOutWords, words, words, { c->dDepthOut } ) );
    float* const dXyz = c->dDepthOut + pixels;
    uint32_t* const dRows = reinterpret_cast< uint32_t* >( c->dDepthOut + pixels * 4u );
    f.rowMap = nullptr;
    if( !c->depthRows.empty() )
    {
        /* the rows the frame was marched with, whatever vrc_set_row_map has done since */
        VRC_HIP_CHECK( hipMemcpyAsync( dRows, c->depthRows.data(), c->depthRows.size() * sizeof( uint32_t ),
                                       hipMemcpyHostToDevice, c->stream ) );
        f.rowMap = dRows;
    }
    VRC_HIP_CHECK( vrc_launch_projection_depths( f, c->dMipDepth, (uint32_t)pixels, c->dDepthOut, hostXyz ? dXyz : nullptr,
                                                 c->stream ) );
    VRC_HIP_CHECK( hipMemcpyAsync( hostT, c->dDepthOut, pixels * sizeof( float ), hipMemcpyDeviceToHost, c->stream ) );
    if( hostXyz )
        VRC_HIP_CHECK( hipMemcpyAsync( hostXyz, dXyz, pixels * 3u * sizeof( float ), hipMemcpyDeviceToHost, c->stream ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    return VRC_OK;
}

int vrc_set_isosurface( vrc_ctx* c, float isoValue, float ambient )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_set_isosurface: ctx is NULL" );
    if( isoValue != isoValue )
        return fail( VRC_EINVAL, "vrc_set_isosurface: iso_value is not a number" );
    if( !( ambient >= 0.0f && ambient <= 1.0f ) )
        return fail( VRC_EINVAL, "vrc_set_isosurface: ambient lies in [0, 1]" );
    c->isoSet = true;
    c->isoValue = isoValue;
    c->isoAmbient = ambient;
    return VRC_OK;
}

int vrc_set_slice( vrc_ctx* c, const float plane[4] )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_set_slice: ctx is NULL" );
    if( !plane )
        return fail( VRC_EINVAL, "vrc_set_slice: plane is NULL" );
    for( int i = 0; i < 4; ++i )
        if( !std::isfinite( plane[i] ) )
            return fail( VRC_EINVAL, "vrc_set_slice: plane has an entry that is not finite" );
    if( plane[0] == 0.0f && plane[1] == 0.0f && plane[2] == 0.0f )
        return fail( VRC_EINVAL, "vrc_set_slice: plane has a zero normal" );
    c->sliceSet = true;
    for( int i = 0; i < 4; ++i )
        c->slicePlane[i] = plane[i];
    return VRC_OK;
}

int vrc_get_projection_gradients( vrc_ctx* c, float* hostG )
{
    if( !c || !hostG )
        return fail( VRC_EINVAL, "vrc_get_projection_gradients: NULL argument" );
    if( c->projState.pixels != 0u && c->sliceFrame )
        return fail( VRC_EINVAL, "vrc_get_projection_gradients: the frame is a slice frame (VRC_OPT_PROJECTION = SLICE); "
                                 "gradients exist after an isosurface frame" );
    if( c->projState.pixels == 0u || !c->gradValid )
        return fail( VRC_EINVAL, "vrc_get_projection_gradients: no VRC_OPT_PROJECTION = ISO vrc_render since the last "
                                 "vrc_pre_render; the gradients exist from a frame's first ISO pass until the next frame" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_HIP_CHECK( hipMemcpyAsync( hostG, c->dIsoGrad, (size_t)c->projState.pixels * 3u * sizeof( float ),
                                   hipMemcpyDeviceToHost, c->stream ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    return VRC_OK;
}

int vrc_get_preintegrated_table( vrc_ctx* c, float* hostRgba, int* kind )
{
    if( !c || !hostRgba )
        return fail( VRC_EINVAL, "vrc_get_preintegrated_table: NULL argument" );
    if( !c->dPreint || c->preintKind < 0 )
        return fail( VRC_EINVAL, "vrc_get_preintegrated_table: no vrc_render with VRC_OPT_PREINTEGRATION = 1 yet; the table "
                                 "is built by the first frame that needs it" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_HIP_CHECK( hipMemcpyAsync( hostRgba, c->dPreint, (size_t)VRC_PREINT_ENTRIES * sizeof( vrc_f4 ), hipMemcpyDeviceToHost,
                                   c->stream ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    if( kind )
        *kind = c->preintKind;
    return VRC_OK;
}

int vrc_synchronize( vrc_ctx* c )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_synchronize: ctx is NULL" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_TRY( resolve_clear( c ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    return VRC_OK;
}

int vrc_get_ray_counts( vrc_ctx* c, uint32_t counts[8], int* parts )
{
    if( !c || !counts || !parts )
        return fail( VRC_EINVAL, "vrc_get_ray_counts: NULL argument" );
    static_assert( VRC_MAX_ERT_PARTS == 8, "vrc_get_ray_counts reports 8 entries" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    for( int i = 0; i < 8; ++i )
        counts[i] = 0;
    *parts = c->lastErtParts;
    if( c->lastErtParts > 1 )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        VRC_HIP_CHECK( hipMemcpy( counts, c->dRayList, VRC_MAX_ERT_PARTS * sizeof( uint32_t ), hipMemcpyDeviceToHost ) );
    }
    return VRC_OK;
}

int vrc_get_stats( vrc_ctx* c, vrc_stats* out )
{
    if( !c || !out )
        return fail( VRC_EINVAL, "vrc_get_stats: NULL argument" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    c->stats.kernel_ms_sum = 0.0;
    c->stats.kernel_launches = 0;
    if( c->evUsed > 0 )
    {
        VRC_HIP_CHECK( hipEventSynchronize( c->evRing->pairs[c->evUsed - 1].second ) );
        float ms = 0.f;
        for( size_t i = 0; i < c->evUsed; ++i )
        {
            VRC_HIP_CHECK( hipEventElapsedTime( &ms, c->evRing->pairs[i].first, c->evRing->pairs[i].second ) );
            c->stats.kernel_ms_sum += ms;
        }
        c->stats.kernel_launches = (uint32_t)c->evUsed;
        c->stats.kernel_ms = ms; /* the last launch */
        c->evUsed = 0;
        c->stats.kernel_ms_sum += c->evFoldedMs;
        c->stats.kernel_launches += c->evFoldedLaunches;
        c->evFoldedMs = 0.0;
        c->evFoldedLaunches = 0;
    }
    else if( !c->opt.timing )
        c->stats.kernel_ms = 0.f;
    if( c->timed )
    {
        /* the sample counter of the last vrc_render (VRC_OPT_COUNT_SAMPLES) */
        if( c->opt.count )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            c->stats.samples = *c->hCounter;
        }
        else
            c->stats.samples = 0;
    }
    *out = c->stats;
    return VRC_OK;
}

int vrc_frame_histogram( vrc_ctx* c, vrc_pool* pool, const float* slots, const uint64_t* scales, uint32_t n,
                         int accumulate )
{
    if( !c || !pool || ( n && ( !slots || !scales ) ) )
        return fail( VRC_EINVAL, "vrc_frame_histogram: NULL argument" );
    if( pool->voxelType != VRC_VOXEL_UINT8 && pool->voxelType != VRC_VOXEL_UINT16 )
        return fail( VRC_EUNSUPPORTED, "vrc_frame_histogram: histograms of signed, 32-bit and float voxels are not implemented" );
    if( accumulate && c->frameHistBins == 0 )
        return fail( VRC_EINVAL, "vrc_frame_histogram: nothing to accumulate into" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    uint32_t bins = 0;
    const uint32_t* dRows = nullptr;
    std::vector< vrc_hist_ref > refs( n );
    {
        std::lock_guard< std::mutex > lock( pool->mutex );
        bins = pool->histBins;
        dRows = pool->dHist;
        if( bins == 0 )
            return fail( VRC_EINVAL, "vrc_frame_histogram: the pool keeps no histograms (vrc_pool_enable_histograms)" );
        for( uint32_t i = 0; i < n; ++i )
        {
            const float* s = slots + 3 * (size_t)i;
            if( !( s[0] >= 0.f && s[1] >= 0.f && s[2] >= 0.f && s[0] < 1.f && s[1] < 1.f && s[2] < 1.f ) )
                return fail( VRC_EINVAL, "vrc_frame_histogram: invalid slot" );
            uint32_t o[3];
            pool_slot_voxel( pool, s, o );
            const uint32_t index = pool_slot_index( pool, o );
            if( index >= pool->histValid.size() || !pool->histValid[index] )
                return fail( VRC_EINVAL, "vrc_frame_histogram: a slot holds no binned brick" );
            refs[i].row = index;
            refs[i].pad = 0;
            refs[i].scale = scales[i];
        }
    }
    if( accumulate && c->frameHistBins != bins )
        return fail( VRC_EINVAL, "vrc_frame_histogram: the bin count changed inside a frame" );
    VRC_TRY( ctx_grow( c, c->frameHistCap, bins, bins, { c->dFrameHist, { c->hFrameHist, sizeof( unsigned long long ), 0, vrc_grown::PINNED } } ) );
    /* the pinned ring and the device list: grown behind every copy that reads the old ones */
    bool grew = false;
    VRC_TRY( ctx_grow( c, c->histRefsCap, n, std::max< size_t >( 1024, n ),
                       { { c->hHistRefs, kNodeStages * sizeof( vrc_hist_ref ), 0, vrc_grown::PINNED }, c->dHistRefs }, &grew ) );
    for( int s = 0; grew && s < kNodeStages; ++s )
        c->histRefsUsed[s] = false;
    /* the rows are written on the pool's upload stream */
    VRC_TRY( ctx_wait_uploads( c, pool ) );
    if( n )
    {
        const uint32_t s = c->histRefsNext++ % kNodeStages;
        if( !c->histRefsEvent[s] )
            VRC_HIP_CHECK( hipEventCreateWithFlags( &c->histRefsEvent[s], hipEventDisableTiming ) );
        if( c->histRefsUsed[s] )
            VRC_HIP_CHECK( hipEventSynchronize( c->histRefsEvent[s] ) );
        vrc_hist_ref* const h = c->hHistRefs + s * c->histRefsCap;
        std::memcpy( h, refs.data(), n * sizeof( vrc_hist_ref ) );
        VRC_HIP_CHECK( hipMemcpyAsync( c->dHistRefs, h, n * sizeof( vrc_hist_ref ), hipMemcpyHostToDevice, c->stream ) );
        VRC_HIP_CHECK( hipEventRecord( c->histRefsEvent[s], c->stream ) );
        c->histRefsUsed[s] = true;
    }
    VRC_HIP_CHECK( vrc_launch_frame_histogram( dRows, bins, c->dHistRefs, n, c->dFrameHist, accumulate != 0, c->stream ) );
    c->frameHistBins = bins;
    /* the context's render fence on the pool (pool_upload) now stands behind this reduction too: an upload that
     * recycles one of these slots does not overwrite its row while the reduction reads it */
    return pool_fence_behind( pool, c, nullptr );
}

int vrc_get_frame_histogram( vrc_ctx* c, uint64_t* hostBins, uint32_t binCount )
{
    if( !c || !hostBins )
        return fail( VRC_EINVAL, "vrc_get_frame_histogram: NULL argument" );
    if( c->frameHistBins == 0 )
        return fail( VRC_EINVAL, "vrc_get_frame_histogram: no frame histogram yet (vrc_frame_histogram)" );
    if( binCount != c->frameHistBins )
        return fail( VRC_EINVAL, "vrc_get_frame_histogram: the frame histogram has " +
                                     std::to_string( c->frameHistBins ) + " bins" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    VRC_HIP_CHECK( hipMemcpyAsync( c->hFrameHist, c->dFrameHist, binCount * sizeof( unsigned long long ),
                                   hipMemcpyDeviceToHost, c->stream ) );
    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
    std::memcpy( hostBins, c->hFrameHist, binCount * sizeof( uint64_t ) );
    return VRC_OK;
}

} /* extern "C" */
