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
#include "vrc_tables.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
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

struct vrc_ctx
{
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;

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
    int64_t optGreyTable = 1; /* VRC_OPT_GREY_TABLE */
    bool lutLinear = false;
    uint32_t lutLevels = 1;

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
    int64_t optTileOrder = 1;
    /* ray cache (VRC_OPT_RAY_CACHE; vrc_core.h: vrc_frame::rayCache): the planes, regrown like dTileOrder; the frame
     * constants of the vrc_render before (rayPrevSet: there was one that could have used the cache) and whether the
     * planes hold the rays of exactly those constants; the mode the last vrc_render used (VRC_OPT_RAY_CACHE_USED) */
    float* dRayCache = nullptr;
    size_t dRayCacheCap = 0; /* words per plane */
    bool rayCacheValid = false;
    bool rayPrevSet = false;
    vrc_frame rayPrevFrame;
    int64_t optRayCache = 1;
    int64_t rayCacheUsed = 0;
    /* walk cache (VRC_OPT_WALK_CACHE; vrc_core.h: vrc_frame::walkCache).  walkState: WALK_IDLE nothing known; WALK_COUNTING
     * the count pass is on the stream, its result on the way to hWalkMax behind evWalk; WALK_VALID the planes hold the
     * lists of walkFrame's constants over the node table as it is.  Nothing here exists before the first count pass: a
     * camera that moves every frame allocates nothing.  The count pass runs only for a frame whose constants, node list
     * and (option at 1) pool uploads are those of the vrc_render before, walkPrev*: what changes every call -- passes over
     * different node subsets, bricks streaming in -- launches nothing extra.  Option at 1: a view whose visits mostly
     * gather stays on the walk (walkGen, walkSlotInfo: the uploads and uniformity words that was decided under; when they
     * change the view is counted again) */
    enum { WALK_IDLE = 0, WALK_COUNTING = 1, WALK_VALID = 2 };
    int walkState = WALK_IDLE;
    uint32_t* dWalk = nullptr;
    size_t dWalkWords = 0;        /* allocated */
    uint32_t walkK = 0;           /* visits per ray the planes hold */
    vrc_walk_count* dWalkMax = nullptr; /* the count pass's result, and its pinned copy */
    vrc_walk_count* hWalkMax = nullptr;
    hipEvent_t evWalk = nullptr;
    vrc_frame walkFrame;
    vrc_frame walkPrevFrame;
    bool walkPrevSet = false;
    uint64_t walkPrevGen = 0, walkGen = 0;
    const uint32_t* walkSlotInfo = nullptr;
    int64_t optWalkCache = 1;
    int64_t optWalkBudget = VRC_WALK_CACHE_DEFAULT_BUDGET;
    int64_t walkCacheUsed = 0;
    /* the form of the lists (vrc_core.h: vrc_frame::walkLean).  walkLeanAsked: what the host saw when the count pass went
     * out -- a step that vrc_exact_step_count counts, a pool whose slot indices fit the word -- and so what that pass was
     * asked to check; part of what the lists are valid for.  walkLean: the form the record pass wrote.  walkLeanUsed:
     * VRC_OPT_WALK_LEAN_USED */
    bool walkLeanAsked = false, walkLean = false;
    int64_t walkLeanUsed = 0;
    /* the uniform-only replay (VRC_OPT_WALK_UNIFORM_ONLY).  walkGathers: what the count pass of the lists in the planes
     * said of the slot words it read, those of walkGen and walkSlotInfo -- compared for this whatever VRC_OPT_WALK_CACHE
     * says, because at VRC_WALK_CACHE_ALWAYS the lists outlive an upload and that answer does not.  walkUniformUsed:
     * VRC_OPT_WALK_UNIFORM_ONLY_USED */
    unsigned long long walkGathers = 0;
    int64_t optWalkUniformOnly = 1;
    int64_t walkUniformUsed = 0;
    int64_t optStepping = 1;
    int64_t optVariant = VRC_VARIANT_CUDARAYCASTER;
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

    int64_t optKernel = VRC_KERNEL_AUTO;
    int64_t optFilter = 0;
    int64_t optTfFracBits = 8;
    int64_t optCount = 0;
    int64_t optTiming = 1;
    int64_t optDepthSplit = 0;
    int64_t optErtParts = 0;     /* VRC_OPT_ERT_COMPACTION */
    int64_t optPackedAtlas = 1;  /* VRC_OPT_PACKED_ATLAS */
    int64_t optUniformBricks = 1; /* VRC_OPT_UNIFORM_BRICKS */
    int64_t optStreamMarkers = 0; /* VRC_OPT_STREAM_MARKERS */
    int64_t optProjection = VRC_PROJECTION_COMPOSITE; /* VRC_OPT_PROJECTION */
    int64_t optMipSkip = 1;                           /* VRC_OPT_MIP_SKIP */
    int64_t optMipFold = VRC_MIP_FOLD_MAX;            /* VRC_OPT_MIP_FOLD */
    /* MIP: one running maximum per pixel of the pixel buffer (vrc_core.h: vrc_frame::mipMax), whichever buffer that
     * is; vrc_pre_render invalidates it (mipFirst: the next MIP pass does not read it) and forgets the projection of
     * the frame before (frameProjection: that of the frame's first vrc_render, -1 = none yet) */
    uint32_t* dMipMax = nullptr;
    size_t dMipMaxPixels = 0;
    bool mipFirst = true;
    int64_t frameProjection = -1;
    /* the mean fold's running (sum, count) per pixel (vrc_frame::meanSum, meanCount): allocated, invalidated and grown
     * where dMipMax is; frameFold: the fold of the frame's first MIP vrc_render, as frameProjection is its projection */
    unsigned long long* dMeanSum = nullptr;
    uint32_t* dMeanCount = nullptr;
    size_t dMeanPixels = 0;
    int64_t frameFold = -1;
    /* what vrc_get_projection_values reads: the state the frame's last MIP pass left (pixels = 0: none -- no MIP pass
     * since vrc_pre_render), and the device buffer its kernel writes (values | counts) */
    vrc_projection_state projState = { nullptr, nullptr, nullptr, 0u, 0u, 0u, 0.0f };
    float* dProjOut = nullptr;
    size_t dProjOutPixels = 0;
    /* the depth of the projected sample (include/vrc_hip.h, "The depth of a MIP frame") */
    int64_t optMipDepth = 0;    /* VRC_OPT_MIP_DEPTH */
    int64_t optMipDepthCue = 0; /* VRC_OPT_MIP_DEPTH_CUE, thousandths */
    /* one running D per pixel beside dMipMax (vrc_frame::mipDepth): allocated by the first frame that tracks depth, grown
     * and invalidated where dMipMax is; frameDepth / frameCue: what the frame's first MIP vrc_render read of the two
     * options (-1 = none yet), as frameFold is its fold */
    float* dMipDepth = nullptr;
    size_t dMipDepthPixels = 0;
    int64_t frameDepth = -1;
    int64_t frameCue = -1;
    /* what vrc_get_projection_depths reads: did the frame's last MIP pass track depth, the frame it marched (camera,
     * pixel buffer geometry) with the row map it had, and the device buffer of the read-back (t | xyz | rows) */
    bool depthValid = false;
    vrc_frame depthFrame = {};
    std::vector< uint32_t > depthRows;
    float* dDepthOut = nullptr;
    size_t dDepthOutWords = 0;
    /* an isosurface frame (include/vrc_hip.h, "An isosurface frame"): vrc_set_isosurface's two values (isoSet: called at
     * all), what the frame's first ISO vrc_render read of them (frameIso: did one), the running G per pixel beside
     * dMipMax and dMipDepth (vrc_frame::isoGrad, three floats a pixel: grown and invalidated where they are), and whether
     * the frame's last pass left one (vrc_get_projection_gradients) */
    bool isoSet = false;
    float isoValue = 0.0f;
    float isoAmbient = 0.0f;
    bool frameIso = false;
    float frameIsoValue = 0.0f;
    float frameIsoAmbient = 0.0f;
    float* dIsoGrad = nullptr;
    size_t dIsoGradPixels = 0;
    bool gradValid = false;
    /* a shaded composite frame (include/vrc_hip.h, "A shaded composite frame"): the two options, and what the frame's
     * first composite vrc_render read of them (-1 = none yet), as frameFold is its fold */
    int64_t optShading = 0;          /* VRC_OPT_SHADING */
    int64_t optShadingAmbient = 250; /* VRC_OPT_SHADING_AMBIENT, thousandths */
    int64_t frameShading = -1;
    int64_t frameShadingAmbient = -1;
    /* the depth of a composite frame (include/vrc_hip.h, "The depth of a composite frame"): the option, and what the
     * frame's first composite vrc_render read of it (-1 = none yet).  The pair per pixel lives in dMipMax and dMipDepth */
    int64_t optCompositeDepth = 0; /* VRC_OPT_COMPOSITE_DEPTH, thousandths */
    int64_t frameCompositeDepth = -1;
    /* a pre-integrated composite frame (include/vrc_hip.h, "A pre-integrated composite frame"): the option, what the
     * frame's first composite vrc_render read of it (-1 = none yet), and the one table: allocated by the first frame
     * that needs it, rebuilt when the kind or one of the classified table's inputs changed */
    int64_t optPreint = 0; /* VRC_OPT_PREINTEGRATION */
    int64_t framePreint = -1;
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
    uint32_t frameHistCap = 0, frameHistBins = 0;
    vrc_hist_ref* dHistRefs = nullptr;
    vrc_hist_ref* hHistRefs = nullptr; /* pinned, kNodeStages areas of histRefsCap */
    size_t histRefsCap = 0;
    hipEvent_t histRefsEvent[kNodeStages] = { nullptr, nullptr, nullptr, nullptr };
    bool histRefsUsed[kNodeStages] = { false, false, false, false };
    uint32_t histRefsNext = 0;
};

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
    hipError_t e = hipStreamCreateWithFlags( &c->ownStream, hipStreamNonBlocking );
    if( e == hipSuccess ) e = hipMalloc( &c->dTf, 256 * 4 * sizeof( float ) );
    if( e == hipSuccess ) e = hipMalloc( &c->dLut, ( VRC_MAX_LOD_LEVELS * VRC_LUT_ENTRIES + 1u ) * sizeof( vrc_f4 ) );
    if( e == hipSuccess ) e = hipHostMalloc( &c->hTf, 256 * 4 * sizeof( float ) );
    if( e == hipSuccess ) e = hipMalloc( &c->dCounter, sizeof( unsigned long long ) );
    if( e == hipSuccess ) e = hipHostMalloc( &c->hCounter, sizeof( unsigned long long ) );
    if( e != hipSuccess )
    {
        const std::string msg = std::string( "vrc_ctx_create: " ) + hipGetErrorString( e );
        vrc_ctx_destroy( c );
        return fail( VRC_EHIP, msg );
    }
    c->stream = c->ownStream;
    *c->hCounter = 0;
    /* default transfer function: linear grey ramp (the reference uploads lexis' default
     * colour map in cuda::ColorMap::ColorMap, cuda/ColorMap.cu:32; that map lives in the
     * un-vendored Lexis library, so the default here is documented and explicit) */
    float tf[256 * 4];
    for( int i = 0; i < 256; ++i )
        tf[i * 4 + 0] = tf[i * 4 + 1] = tf[i * 4 + 2] = tf[i * 4 + 3] = (float)i / 255.0f;
    std::memcpy( c->hTf, tf, sizeof( tf ) );
    c->tfGrey = true;
    if( const char* g = std::getenv( "VRC_GREY_TABLE" ) ) /* default of VRC_OPT_GREY_TABLE for this process */
        c->optGreyTable = g[0] != '0';
    e = hipMemcpy( c->dTf, tf, sizeof( tf ), hipMemcpyHostToDevice );
    if( e != hipSuccess )
    {
        const std::string msg = std::string( "vrc_ctx_create: " ) + hipGetErrorString( e );
        vrc_ctx_destroy( c );
        return fail( VRC_EHIP, msg );
    }
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
    if( c->dTf ) (void)hipFree( c->dTf );
    if( c->dLut ) (void)hipFree( c->dLut );
    if( c->dPreint ) (void)hipFree( c->dPreint );
    if( c->hTf ) (void)hipHostFree( c->hTf );
    if( c->fbOwn ) (void)hipFree( c->fbOwn );
    if( c->dNodes ) (void)hipFree( c->dNodes );
    if( c->dGrid ) (void)hipFree( c->dGrid );
    if( c->hStage ) (void)hipHostFree( c->hStage );
    for( hipEvent_t e : c->stageEvent )
        if( e ) (void)hipEventDestroy( e );
    if( c->dTileOrder ) (void)hipFree( c->dTileOrder );
    if( c->dRayCache ) (void)hipFree( c->dRayCache );
    if( c->dWalk ) (void)hipFree( c->dWalk );
    if( c->dWalkMax ) (void)hipFree( c->dWalkMax );
    if( c->hWalkMax ) (void)hipHostFree( c->hWalkMax );
    if( c->evWalk ) (void)hipEventDestroy( c->evWalk );
    if( c->dRayList ) (void)hipFree( c->dRayList );
    if( c->dMipMax ) (void)hipFree( c->dMipMax );
    if( c->dMeanSum ) (void)hipFree( c->dMeanSum );
    if( c->dMeanCount ) (void)hipFree( c->dMeanCount );
    if( c->dProjOut ) (void)hipFree( c->dProjOut );
    if( c->dMipDepth ) (void)hipFree( c->dMipDepth );
    if( c->dIsoGrad ) (void)hipFree( c->dIsoGrad );
    if( c->dDepthOut ) (void)hipFree( c->dDepthOut );
    if( c->dRowMap ) (void)hipFree( c->dRowMap );
    if( c->dCounter ) (void)hipFree( c->dCounter );
    if( c->hCounter ) (void)hipHostFree( c->hCounter );
    if( c->dFrameHist ) (void)hipFree( c->dFrameHist );
    if( c->hFrameHist ) (void)hipHostFree( c->hFrameHist );
    if( c->dHistRefs ) (void)hipFree( c->dHistRefs );
    if( c->hHistRefs ) (void)hipHostFree( c->hHistRefs );
    for( hipEvent_t e : c->histRefsEvent )
        if( e ) (void)hipEventDestroy( e );
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
    c->rayCacheValid = c->rayPrevSet = false; /* (the planes were written on the stream before) */
    c->walkState = vrc_ctx::WALK_IDLE;        /* (and so were the lists; a count pass in flight has ended above) */
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
        c->optKernel = value;
        return VRC_OK;
    case VRC_OPT_FILTER:
        if( value != VRC_FILTER_NEAREST && value != VRC_FILTER_TRILINEAR )
            return fail( VRC_EINVAL, "vrc_set_option: filter is 0 (nearest) or 1 (trilinear)" );
        c->optFilter = value;
        return VRC_OK;
    case VRC_OPT_TF_FRAC_BITS:
        if( value < 0 || value > 16 )
            return fail( VRC_EINVAL, "vrc_set_option: tf frac bits out of range" );
        c->optTfFracBits = value;
        return VRC_OK;
    case VRC_OPT_COUNT_SAMPLES: c->optCount = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_TILE_ORDER: c->optTileOrder = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_STEPPING: c->optStepping = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_KERNEL_TIMING: c->optTiming = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_DEPTH_SPLIT: c->optDepthSplit = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_GREY_TABLE: c->optGreyTable = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_PACKED_ATLAS: c->optPackedAtlas = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_UNIFORM_BRICKS: c->optUniformBricks = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_STREAM_MARKERS: c->optStreamMarkers = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_RAY_CACHE:
        if( c->optRayCache != ( value ? 1 : 0 ) )
            c->rayCacheValid = c->rayPrevSet = false;
        c->optRayCache = value ? 1 : 0;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE:
        if( value < 0 || value > VRC_WALK_CACHE_ALWAYS )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE is 0 (off), 1 (on) or 2 (on for every view)" );
        if( c->optWalkCache != value )
            c->walkState = vrc_ctx::WALK_IDLE;
        c->optWalkCache = value;
        return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET:
        if( value < 0 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_CACHE_BUDGET is a number of bytes" );
        if( c->optWalkBudget != value )
            c->walkState = vrc_ctx::WALK_IDLE;
        c->optWalkBudget = value;
        return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_UNIFORM_ONLY is 0 (off) or 1 (on)" );
        c->optWalkUniformOnly = value; /* (which instance replays the lists: nothing starts over) */
        return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY_USED:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_WALK_UNIFORM_ONLY_USED is read-only" );
    case VRC_OPT_PROJECTION:
        if( value != VRC_PROJECTION_COMPOSITE && value != VRC_PROJECTION_MIP && value != VRC_PROJECTION_ISO )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PROJECTION is 0 (composite), 1 (maximum intensity) or 2 (isosurface)" );
        /* a context that never called vrc_set_isosurface keeps what it had before the isosurface projection existed: the
         * value is refused, here and not only by the render it could not serve */
        if( value == VRC_PROJECTION_ISO && !c->isoSet )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PROJECTION = VRC_PROJECTION_ISO needs vrc_set_isosurface first" );
        c->optProjection = value;
        return VRC_OK;
    case VRC_OPT_MIP_SKIP: c->optMipSkip = value ? 1 : 0; return VRC_OK;
    case VRC_OPT_MIP_FOLD:
        if( value != VRC_MIP_FOLD_MAX && value != VRC_MIP_FOLD_MIN && value != VRC_MIP_FOLD_MEAN )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_FOLD is 0 (maximum), 1 (minimum) or 2 (mean)" );
        c->optMipFold = value;
        return VRC_OK;
    case VRC_OPT_MIP_DEPTH:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_DEPTH is 0 (off) or 1 (keep the depth of the projected sample)" );
        c->optMipDepth = value;
        return VRC_OK;
    case VRC_OPT_MIP_DEPTH_CUE:
        if( value < 0 || value > 1000 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_MIP_DEPTH_CUE is the cue strength in thousandths, 0 (off) to 1000" );
        c->optMipDepthCue = value;
        return VRC_OK;
    case VRC_OPT_SHADING:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_SHADING is 0 (off) or 1 (light every sample of a composite frame by its gradient)" );
        c->optShading = value;
        return VRC_OK;
    case VRC_OPT_SHADING_AMBIENT:
        if( value < 0 || value > 1000 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_SHADING_AMBIENT is the ambient share in thousandths, 0 to 1000" );
        c->optShadingAmbient = value;
        return VRC_OK;
    case VRC_OPT_COMPOSITE_DEPTH:
        if( value < 0 || value > 999 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_COMPOSITE_DEPTH is 0 (off) or the opacity threshold in thousandths, 1 to 999" );
        c->optCompositeDepth = value;
        return VRC_OK;
    case VRC_OPT_PREINTEGRATION:
        if( value != 0 && value != 1 )
            return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PREINTEGRATION is 0 (off) or 1 (classify every step of a composite frame from the pre-integrated table)" );
        c->optPreint = value;
        return VRC_OK;
    case VRC_OPT_PREINT_BUILDS:
        return fail( VRC_EINVAL, "vrc_set_option: VRC_OPT_PREINT_BUILDS is read-only" );
    case VRC_OPT_ERT_COMPACTION:
        if( value < 0 || value > VRC_MAX_ERT_PARTS )
            return fail( VRC_EINVAL, "VRC_OPT_ERT_COMPACTION: 0 (off) or 2.." + std::to_string( VRC_MAX_ERT_PARTS ) +
                                         " launches per frame" );
        c->optErtParts = value < 2 ? 0 : value;
        return VRC_OK;
    case VRC_OPT_VARIANT:
        if( value != VRC_VARIANT_CUDARAYCASTER && value != VRC_VARIANT_GLRAYCASTER )
            return fail( VRC_EINVAL, "vrc_set_option: variant is 0 (cudaRaycaster) or 1 (glRaycaster)" );
        c->optVariant = value;
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
    case VRC_OPT_KERNEL: *value = c->optKernel; return VRC_OK;
    case VRC_OPT_FILTER: *value = c->optFilter; return VRC_OK;
    case VRC_OPT_TF_FRAC_BITS: *value = c->optTfFracBits; return VRC_OK;
    case VRC_OPT_COUNT_SAMPLES: *value = c->optCount; return VRC_OK;
    case VRC_OPT_TILE_ORDER: *value = c->optTileOrder; return VRC_OK;
    case VRC_OPT_STEPPING: *value = c->optStepping; return VRC_OK;
    case VRC_OPT_KERNEL_TIMING: *value = c->optTiming; return VRC_OK;
    case VRC_OPT_DEPTH_SPLIT: *value = c->optDepthSplit; return VRC_OK;
    case VRC_OPT_ERT_COMPACTION: *value = c->optErtParts; return VRC_OK;
    case VRC_OPT_GREY_TABLE: *value = c->optGreyTable; return VRC_OK;
    case VRC_OPT_PACKED_ATLAS: *value = c->optPackedAtlas; return VRC_OK;
    case VRC_OPT_UNIFORM_BRICKS: *value = c->optUniformBricks; return VRC_OK;
    case VRC_OPT_STREAM_MARKERS: *value = c->optStreamMarkers; return VRC_OK;
    case VRC_OPT_RAY_CACHE: *value = c->optRayCache; return VRC_OK;
    case VRC_OPT_RAY_CACHE_USED: *value = c->rayCacheUsed; return VRC_OK;
    case VRC_OPT_WALK_CACHE: *value = c->optWalkCache; return VRC_OK;
    case VRC_OPT_WALK_CACHE_USED: *value = c->walkCacheUsed; return VRC_OK;
    case VRC_OPT_WALK_CACHE_BUDGET: *value = c->optWalkBudget; return VRC_OK;
    case VRC_OPT_WALK_CACHE_BYTES: *value = (int64_t)( c->dWalkWords * sizeof( uint32_t ) ); return VRC_OK;
    case VRC_OPT_WALK_LEAN_USED: *value = c->walkLeanUsed; return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY: *value = c->optWalkUniformOnly; return VRC_OK;
    case VRC_OPT_WALK_UNIFORM_ONLY_USED: *value = c->walkUniformUsed; return VRC_OK;
    case VRC_OPT_PROJECTION: *value = c->optProjection; return VRC_OK;
    case VRC_OPT_MIP_SKIP: *value = c->optMipSkip; return VRC_OK;
    case VRC_OPT_MIP_FOLD: *value = c->optMipFold; return VRC_OK;
    case VRC_OPT_MIP_DEPTH: *value = c->optMipDepth; return VRC_OK;
    case VRC_OPT_MIP_DEPTH_CUE: *value = c->optMipDepthCue; return VRC_OK;
    case VRC_OPT_VARIANT: *value = c->optVariant; return VRC_OK;
    case VRC_OPT_SHADING: *value = c->optShading; return VRC_OK;
    case VRC_OPT_SHADING_AMBIENT: *value = c->optShadingAmbient; return VRC_OK;
    case VRC_OPT_COMPOSITE_DEPTH: *value = c->optCompositeDepth; return VRC_OK;
    case VRC_OPT_PREINTEGRATION: *value = c->optPreint; return VRC_OK;
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
    if( !c->optStreamMarkers && c->waitedPoolUid == p->uid && c->waitedGen == p->uploadGen )
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
    if( n > c->dRowMapCap )
    {
        if( c->dRowMap ) VRC_HIP_CHECK( hipFree( c->dRowMap ) );
        c->dRowMap = nullptr;
        c->dRowMapCap = 0;
        VRC_HIP_CHECK( hipMalloc( &c->dRowMap, n * sizeof( uint32_t ) ) );
        c->dRowMapCap = n;
    }
    if( n )
        VRC_HIP_CHECK( hipMemcpy( c->dRowMap, rows, n * sizeof( uint32_t ), hipMemcpyHostToDevice ) );
    c->rowMap.assign( rows, rows + n );
    c->tileOrderValid = false;
    c->rayCacheValid = c->rayPrevSet = false;
    c->walkState = vrc_ctx::WALK_IDLE; /* (the stream was synchronised above) */
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
        if( pixels > c->fbOwnPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->fbOwn ) VRC_HIP_CHECK( hipFree( c->fbOwn ) );
            c->fbOwn = nullptr;
            c->fbOwnPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->fbOwn, pixels * sizeof( vrc_f4 ) ) );
            c->fbOwnPixels = pixels;
        }
        c->fbW = w;
        c->fbH = h;
    }
    /* PixelBufferObject::mapBuffer clears the mapped buffer (cuda/PixelBufferObject.cu:80).  The
     * clear is folded into the first march of the frame (vrc_frame::clearFirst); whoever looks at
     * the buffer before a march has run gets it done then (resolve_clear). */
    c->clearPending = true;
    /* a new frame: its MIP passes start over, and it may take either projection */
    c->mipFirst = true;
    c->frameProjection = -1;
    c->frameFold = -1;
    c->frameDepth = -1;
    c->frameCue = -1;
    c->depthValid = false;
    c->frameIso = false;
    c->gradValid = false;
    c->frameShading = c->frameShadingAmbient = -1;
    c->frameCompositeDepth = -1;
    c->framePreint = -1;
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
    {
        const int rc = resolve_clear( c );
        if( rc != VRC_OK )
            return rc;
    }
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
    {
        const int rc = resolve_clear( c );
        if( rc != VRC_OK )
            return rc;
    }
    if( deviceRgba ) *deviceRgba = ctx_fb( c );
    if( width ) *width = c->fbW;
    if( height ) *height = c->fbH;
    return VRC_OK;
}

/* node table + brick grid: vrc_tables.h */
static int ensure_capacity( vrc_ctx* c, size_t nNodes, size_t nGrid )
{
    if( nNodes > c->dNodesCap )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->dNodes ) VRC_HIP_CHECK( hipFree( c->dNodes ) );
        c->dNodes = nullptr;
        c->dNodesCap = 0;
        const size_t cap = std::max< size_t >( nNodes, 1024 ); /* sized to n (fixes Q8) */
        VRC_HIP_CHECK( hipMalloc( &c->dNodes, cap * sizeof( vrc_dev_node ) ) );
        c->dNodesCap = cap;
    }
    if( nGrid > c->dGridCap )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->dGrid ) VRC_HIP_CHECK( hipFree( c->dGrid ) );
        c->dGrid = nullptr;
        c->dGridCap = 0;
        const size_t cap = std::max< size_t >( nGrid, 4096 );
        VRC_HIP_CHECK( hipMalloc( &c->dGrid, cap * sizeof( int32_t ) ) );
        c->dGridCap = cap;
    }
    const size_t stageBytes = nNodes * sizeof( vrc_dev_node ) + nGrid * sizeof( int32_t );
    if( stageBytes > c->hStageCap )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->hStage ) VRC_HIP_CHECK( hipHostFree( c->hStage ) );
        c->hStage = nullptr;
        c->hStageCap = 0;
        const size_t cap = ( std::max< size_t >( stageBytes, 1 << 18 ) + 255 ) / 256 * 256;
        VRC_HIP_CHECK( hipHostMalloc( &c->hStage, cap * kNodeStages ) );
        c->hStageCap = cap;
        for( int i = 0; i < kNodeStages; ++i )
            c->stageUsed[i] = false;
    }
    return VRC_OK;
}

int vrc_render( vrc_ctx* c, const vrc_view_data* view, const vrc_node_data* nodes, uint32_t nNodes,
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
    if( nNodes == 0 ) /* CudaRaycastRenderer.cpp:157-158 */
        return VRC_OK;
    VRC_HIP_CHECK( hipSetDevice( c->device ) );

    /* classified table, rebuilt only when one of its inputs changed */
    vrc_lut_params lp;
    /* signed 8/16-bit voxels are in the atlas offset-binary (v + 128 / + 32768): the range moves with them, and every
     * kernel form serves the pool as the unsigned one it then is (the trilinear filter commutes with the offset) */
    lp.rangeMin = render->dataSourceRange[0] + pool->rangeShift;
    lp.rangeMax = render->dataSourceRange[1] + pool->rangeShift;
    lp.alphaCorrection = (float)render->maxSamplesPerRay / (float)render->samplesPerRay;
    lp.fracBits = (int)c->optTfFracBits;
    if( pool->elemBytes == 4 && ( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED ) )
        return fail( VRC_EINVAL, "vrc_render: 32-bit and float voxels are marched by gathers; the LDS-staged and tap-packed "
                                 "forms take 8- and 16-bit voxels (VRC_OPT_KERNEL = AUTO, REFERENCE_ORDER or GRID_DDA)" );
    /* an isosurface frame is a MIP frame with the first-crossing fold: it reads none of the MIP frame's options but
     * VRC_OPT_MIP_SKIP, and is served and refused as one */
    const bool iso = c->optProjection == VRC_PROJECTION_ISO;
    const bool mip = c->optProjection == VRC_PROJECTION_MIP || iso;
    if( c->frameProjection >= 0 && c->frameProjection != c->optProjection )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PROJECTION changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame take one projection" );
    if( iso && !c->isoSet )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PROJECTION = ISO needs vrc_set_isosurface first" );
    if( iso && c->frameIso && ( c->frameIsoValue != c->isoValue || c->frameIsoAmbient != c->isoAmbient ) )
        return fail( VRC_EINVAL, "vrc_render: vrc_set_isosurface changed iso_value or ambient between vrc_pre_render and "
                                 "vrc_post_render; the passes of one frame take one isosurface" );
    if( mip && !iso && c->frameFold >= 0 && c->frameFold != c->optMipFold )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_FOLD changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame take one fold" );
    /* depth tracking: the maximum and the minimum only; the mean reads neither option */
    const bool mipDepth = iso || ( mip && c->optMipFold != VRC_MIP_FOLD_MEAN && ( c->optMipDepth != 0 || c->optMipDepthCue > 0 ) );
    if( mip && !iso && c->optMipFold != VRC_MIP_FOLD_MEAN )
    {
        if( c->frameDepth >= 0 && c->frameDepth != c->optMipDepth )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_DEPTH changed between vrc_pre_render and vrc_post_render; the "
                                     "passes of one frame all keep the depth or none does" );
        if( c->frameCue >= 0 && c->frameCue != c->optMipDepthCue )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_MIP_DEPTH_CUE changed between vrc_pre_render and vrc_post_render; "
                                     "the passes of one frame take one cue strength" );
    }
    if( mip )
    {
        /* what the maximum-intensity projection is not defined for (include/vrc_hip.h) */
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, iso ? "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no isosurface form; "
                                           "VRC_OPT_PROJECTION = ISO is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)"
                                         : "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no maximum-intensity form; "
                                           "VRC_OPT_PROJECTION = MIP is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, iso ? "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PROJECTION = ISO renders a per-brick cut"
                                         : "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PROJECTION = MIP renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, iso ? "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PROJECTION = ISO is defined on the "
                                           "cudaRaycaster variant's sample set"
                                         : "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PROJECTION = MIP is defined on the "
                                           "cudaRaycaster variant's sample set" );
    }
    /* a shaded composite frame (include/vrc_hip.h, "A shaded composite frame"): read by composite frames only; served by
     * the gather marches of vrc_kernels_shade.hip and refused where those have no form */
    const bool shade = !mip && c->optShading != 0;
    if( !mip )
    {
        if( c->frameShading >= 0 && c->frameShading != c->optShading )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING changed between vrc_pre_render and vrc_post_render; the "
                                     "passes of one frame are all shaded or none is" );
        if( c->frameShadingAmbient >= 0 && c->frameShadingAmbient != c->optShadingAmbient )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING_AMBIENT changed between vrc_pre_render and vrc_post_render; "
                                     "the passes of one frame take one ambient share" );
    }
    /* the depth of a composite frame (include/vrc_hip.h, "The depth of a composite frame"): read by composite frames only;
     * served by the gather marches of vrc_kernels_cdepth.hip and refused where those have no form */
    const bool cdepth = !mip && c->optCompositeDepth != 0;
    if( !mip && c->frameCompositeDepth >= 0 && c->frameCompositeDepth != c->optCompositeDepth )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_COMPOSITE_DEPTH changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame cross one threshold" );
    if( cdepth )
    {
        if( shade )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_COMPOSITE_DEPTH; alpha does not "
                                     "depend on shading: render the unshaded frame to pick in a shaded picture" );
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no depth-tracking form; "
                                     "VRC_OPT_COMPOSITE_DEPTH is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_COMPOSITE_DEPTH tracks a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_COMPOSITE_DEPTH is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    /* a pre-integrated composite frame (include/vrc_hip.h, "A pre-integrated composite frame"): read by composite frames
     * only; served by the gather marches of vrc_kernels_preint.hip and refused where those have no form */
    const bool preint = !mip && c->optPreint != 0;
    if( !mip && c->framePreint >= 0 && c->framePreint != c->optPreint )
        return fail( VRC_EINVAL, "vrc_render: VRC_OPT_PREINTEGRATION changed between vrc_pre_render and vrc_post_render; the "
                                 "passes of one frame are all pre-integrated or none is" );
    if( preint )
    {
        if( shade )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_SHADING = 1 together with VRC_OPT_PREINTEGRATION; a step has no one "
                                     "gradient: the two are not combined" );
        if( cdepth )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_COMPOSITE_DEPTH together with VRC_OPT_PREINTEGRATION; the depth is "
                                     "defined on the plain frame's alpha: the two are not combined" );
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no pre-integrated form; "
                                     "VRC_OPT_PREINTEGRATION = 1 is marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_PREINTEGRATION = 1 renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_PREINTEGRATION = 1 is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    if( shade )
    {
        if( c->optKernel == VRC_KERNEL_LDS || c->optKernel == VRC_KERNEL_PACKED )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_KERNEL = LDS / PACKED has no shaded form; VRC_OPT_SHADING = 1 is "
                                     "marched by gathers (AUTO, REFERENCE_ORDER or GRID_DDA)" );
        if( c->rayLod )
            return fail( VRC_EINVAL, "vrc_render: vrc_set_ray_lod is on; VRC_OPT_SHADING = 1 renders a per-brick cut" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: VRC_OPT_VARIANT = GLRAYCASTER; VRC_OPT_SHADING = 1 is defined on the "
                                     "cudaRaycaster variant's sample set" );
    }
    const bool linear = c->optFilter == VRC_FILTER_TRILINEAR;
    /* samples classified one by one (padded transfer function in the table buffer) whenever the
     * 257-entry classified table cannot be used: continuous or 16-bit densities */
    /* (MIP: the one classification per ray reads the padded transfer function too) */
    const bool classify = linear || pool->elemBytes != 1 || mip;
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
    if( preint )
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

    /* node table + grid, re-derived and re-uploaded only when the node list changed
     * (the reference re-uploads synchronously every pass, Renderer.cu:259-267) */
    const bool sameNodes = c->cachedPoolUid == pool->uid && c->cachedNodes.size() == nNodes &&
                           c->cachedRayLod == c->rayLod &&
                           std::memcmp( c->cachedNodes.data(), nodes,
                                        nNodes * sizeof( vrc_node_data ) ) == 0;
    if( !sameNodes )
    {
        c->walkState = vrc_ctx::WALK_IDLE; /* the walk cache's lists index the node table that is replaced here */
        vrc_host_tables t;
        vrc_atlas_geom geom;
        for( int a = 0; a < 3; ++a )
        {
            geom.atlasDim[a] = pool->atlasDim[a];
            geom.slotDim[a] = pool->slotDim[a];
        }
        for( int a = 0; a < 3; ++a )
            geom.slots[a] = pool->slots[a];
        vrc_build_tables( geom, nodes, nNodes, t );
        if( c->rayLod )
            vrc_build_lod_tables( geom, nodes, nNodes, t );
        const int rc = ensure_capacity( c, t.nodes.size(), t.grid.size() );
        if( rc != VRC_OK )
            return rc;
        const uint32_t stage = c->stageNext++ % kNodeStages;
        if( c->stageUsed[stage] ) /* the copies issued from this area four node lists ago */
            VRC_HIP_CHECK( hipEventSynchronize( c->stageEvent[stage] ) );
        if( !c->stageEvent[stage] )
            VRC_HIP_CHECK( hipEventCreateWithFlags( &c->stageEvent[stage], hipEventDisableTiming ) );
        uint8_t* h = (uint8_t*)c->hStage + (size_t)stage * c->hStageCap;
        const size_t nb = t.nodes.size() * sizeof( vrc_dev_node );
        const size_t gb = t.grid.size() * sizeof( int32_t );
        std::memcpy( h, t.nodes.data(), nb );
        VRC_HIP_CHECK( hipMemcpyAsync( c->dNodes, h, nb, hipMemcpyHostToDevice, c->stream ) );
        if( gb )
        {
            std::memcpy( h + nb, t.grid.data(), gb );
            VRC_HIP_CHECK(
                hipMemcpyAsync( c->dGrid, h + nb, gb, hipMemcpyHostToDevice, c->stream ) );
        }
        VRC_HIP_CHECK( hipEventRecord( c->stageEvent[stage], c->stream ) );
        c->stageUsed[stage] = true;
        c->cachedNodes.assign( nodes, nodes + nNodes );
        c->cachedPoolUid = pool->uid;
        c->cachedGridOk = t.gridOk && !c->rayLod; /* the grid buffer holds the per-level tables */
        c->cachedOneCell = t.oneCellPerBrick;
        c->cachedRayLod = c->rayLod;
        c->cachedLodOk = t.lodOk;
        c->cachedLodLevels = t.lodLevels;
        c->cachedFinestVoxel = t.finestVoxelWorld;
        c->cachedClamp = t.clamp;
        c->cachedGridFrame = t.g;
    }

    if( c->rayLod )
    {
        if( !c->cachedLodOk )
            return fail( VRC_EHIERARCHY, "vrc_render: per-ray LOD needs a brick hierarchy (every level a regular grid of bricks, one brick per cell)" );
        if( c->optVariant != VRC_VARIANT_CUDARAYCASTER )
            return fail( VRC_EINVAL, "vrc_render: per-ray LOD is defined for the cudaRaycaster variant only" );
        /* AUTO: the LDS-staged form for the trilinear filter where it applies, else the gather form; GRID_DDA asks for
         * the gather form, LDS for the staged one */
        if( c->optKernel == VRC_KERNEL_REFERENCE_ORDER )
            return fail( VRC_EINVAL, "vrc_render: per-ray LOD walks the hierarchy; VRC_OPT_KERNEL = AUTO, GRID_DDA (gathers), LDS or PACKED" );
    }
    bool useDda = c->cachedGridOk;
    /* AUTO keeps the reference's frame: bricks of one size are met by the grid walk in the reference's
     * order; a list that mixes brick sizes (an LOD cut) is composited in the host's centre-distance order,
     * which is not a visibility order for every ray (quirk Q6) -- the literal loop reproduces that as long
     * as testing every brick per ray is affordable.  GRID_DDA can always be asked for (true visibility
     * order); the trilinear filter (extension, no reference frame to keep) stays on the grid. */
    if( c->optKernel == VRC_KERNEL_AUTO && useDda && !c->cachedOneCell && !linear &&
        nNodes <= VRC_REFERENCE_ORDER_MAX_NODES )
        useDda = false;
    /* glRaycaster with more than one sample per pixel (fragRaycast.glsl:121-129): the pixel is averaged brick by
     * brick in the host's order -- the reference-order loop is the only form that has a "brick by brick" */
    const bool glSuper = c->optVariant == VRC_VARIANT_GLRAYCASTER && render->samplesPerPixel > 1u;
    if( glSuper )
    {
        if( c->optKernel == VRC_KERNEL_GRID_DDA || c->optKernel == VRC_KERNEL_LDS )
            return fail( VRC_EINVAL, "vrc_render: the glRaycaster variant with samplesPerPixel > 1 is rendered by the "
                                     "reference-order kernel (VRC_OPT_KERNEL = AUTO or REFERENCE_ORDER)" );
        useDda = false;
    }
    if( c->optKernel == VRC_KERNEL_REFERENCE_ORDER )
        useDda = false;
    else if( c->optKernel == VRC_KERNEL_GRID_DDA && !c->cachedGridOk && !c->rayLod )
        return fail( VRC_EINVAL, "vrc_render: node set is not grid-aligned; GRID_DDA unavailable" );
    /* LDS-staged kernel: brick-grid DDA + unclamped sampler (overlap >= 1).  AUTO takes it for
     * the trilinear filter (eight taps per sample), the gather kernel for point sampling. */
    /* its trilinear form takes the transfer-function texel and CUDA's 1.8 fixed-point lerp weight out of one
     * float -> integer conversion (vrc_kernels_lds.hip: lds_classify): other weight widths use the gather form */
    /* slot-local positions in 8.24 fixed point (fixed-point stepping, the per-axis address tables, the LDS kernel's boxes)
     * need every slot dimension to fit eight bits; pool creation bounds a slot's VOLUME only (2^24 voxels), so a flat
     * or long brick can exceed it: such pools march with float positions */
    const bool slotsFit8Bits = pool->slotDim[0] <= 248u && pool->slotDim[1] <= 248u && pool->slotDim[2] <= 248u;
    /* 16-bit voxels: its trilinear form only (a 16-bit density does not index the classified table of the point form) */
    const bool ldsVoxels = slotsFit8Bits && ( pool->elemBytes == 1 || ( pool->elemBytes == 2 && linear ) );
    /* atlases of more than 2^32 voxels (64-bit slot bases): its trilinear form only */
    const bool ldsEligible = c->cachedGridOk && !c->cachedClamp && ldsVoxels && ( !pool->bigAtlas || linear ) &&
                             ( !linear || c->optTfFracBits == 8 );
    if( !c->rayLod && c->optKernel == VRC_KERNEL_LDS && !ldsEligible )
        return fail( VRC_EINVAL, "vrc_render: the LDS kernel needs a grid-aligned node set of 8-bit bricks in an atlas of at most 2^32 voxels (trilinear: 8- or 16-bit, any atlas, VRC_OPT_TF_FRAC_BITS = 8) with overlap >= 1" );
    /* per-ray LOD: the staged kernel's trilinear form only (samples classified one by one: no table per level) */
    const bool ldsLodEligible = c->rayLod && linear && !c->cachedClamp && ldsVoxels && !pool->bigAtlas &&
                                c->optTfFracBits == 8;
    if( c->rayLod && c->optKernel == VRC_KERNEL_LDS && !ldsLodEligible )
        return fail( VRC_EINVAL, "vrc_render: under per-ray LOD the LDS kernel needs the trilinear filter, 8- or 16-bit bricks with overlap >= 1 and VRC_OPT_TF_FRAC_BITS = 8" );
    /* tap-packed atlas (VRC_KERNEL_PACKED; vrc_core.h): the trilinear filter as two gathers per sample.  Needs what its
     * positions and its classifier need -- 8- or 16-bit bricks with overlap >= 1 in slots of at most 248 voxels a side,
     * VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping -- and 2.25 times the atlas in device memory; either brick
     * enumeration (grid walk where the node set is grid-aligned, else the reference-order loop) */
    const bool packedEligible = linear && !glSuper && !mip && !shade && !cdepth && !preint && !c->cachedClamp && slotsFit8Bits &&
                                pool_packed_possible( pool ) && c->optTfFracBits == 8 && c->optStepping != 0;
    bool usePacked = false;
    if( c->optKernel == VRC_KERNEL_PACKED )
    {
        if( !packedEligible )
            return fail( VRC_EINVAL, "vrc_render: the packed kernel needs the trilinear filter on 8- or 16-bit bricks with overlap >= 1 (slots of at most 248 voxels a side), VRC_OPT_TF_FRAC_BITS = 8, fixed-point stepping" );
        if( !pool_enable_packed( pool ) )
            return fail( VRC_ENOMEM, "vrc_render: no device memory for the tap-packed atlas (2.25 times the brick atlas)" );
        usePacked = true;
    }
    else if( c->optKernel == VRC_KERNEL_AUTO && packedEligible && c->optPackedAtlas )
        /* measured on C2: 1.2 against 1.7 ms along the axis, 1.5 against 2.4 at 30/20 degrees;
         * under per-ray LOD 1.4-2.1 x the staged form (profiles/r4_c5_trilinear_three_forms.txt); without the memory for
         * it the frame takes the staged form below */
        usePacked = pool_enable_packed( pool );
    const bool useLds = c->rayLod ? ( ldsLodEligible && c->optKernel != VRC_KERNEL_GRID_DDA && !usePacked )
                                  : !glSuper && !usePacked && !mip && !shade && !cdepth && !preint && ( c->optKernel == VRC_KERNEL_LDS ||
                                                  ( c->optKernel == VRC_KERNEL_AUTO && linear && ldsEligible ) );

    vrc_raycast_args a;
    std::memset( &a, 0, sizeof( a ) );
    a.shade = shade;
    a.cdepth = cdepth;
    a.preint = preint;
    vrc_frame& f = a.frame;
    {
        vrc_atlas_geom geom;
        for( int i = 0; i < 3; ++i )
        {
            geom.atlasDim[i] = pool->atlasDim[i];
            geom.slotDim[i] = pool->slotDim[i];
        }
        for( int a = 0; a < 3; ++a )
            geom.slots[a] = pool->slots[a];
        /* the GLSL twin casts through the pixel centre (gl_FragCoord, fragRaycast.glsl:127), the
         * CUDA kernel through the pixel corner (Renderer.cu:106-112) */
        const float centre = c->optVariant == VRC_VARIANT_GLRAYCASTER ? 0.5f : 0.0f;
        vrc_fill_frame( f, *view, *render, geom, c->cachedGridFrame, c->planes, c->nPlanes, nNodes,
                        c->fbW, c->fbH, centre, centre );
        f.rowMap = c->rowMap.empty() ? nullptr : c->dRowMap;
        f.variant = c->optVariant == VRC_VARIANT_GLRAYCASTER ? VRC_VARIANT_GL : VRC_VARIANT_CUDA;
        f.samplesPerPixel = ( f.variant == VRC_VARIANT_GL && render->samplesPerPixel > 1u ) ? render->samplesPerPixel : 1u;
        if( c->rayLod )
        {
            f.lodLevels = c->cachedLodLevels;
            f.lodBase = (float)( c->cachedFinestVoxel /
                                 ( (double)c->rayLodSse * (double)c->rayLodWorldPerPixel ) );
        }
    }

    /* tile schedule, recomputed only when the frame constants changed */
    a.tileOrder = nullptr;
    if( c->optTileOrder )
    {
        /* one entry per schedule slot: four per 2x2 block of tiles (vrc_internal.h) */
        const size_t nTiles = vrc_schedule_slots( ( c->fbW + VRC_TILE_W - 1 ) / VRC_TILE_W,
                                                  ( c->fbH + VRC_TILE_H - 1 ) / VRC_TILE_H );
        if( nTiles > c->dTileOrderCap )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dTileOrder ) VRC_HIP_CHECK( hipFree( c->dTileOrder ) );
            c->dTileOrder = nullptr;
            c->dTileOrderCap = 0;
            /* order[nTiles] | scratch[VRC_TILE_SCRATCH_WORDS] | bucket[nTiles] (bytes) */
            VRC_HIP_CHECK( hipMalloc( &c->dTileOrder, ( nTiles + VRC_TILE_SCRATCH_WORDS ) * sizeof( uint32_t ) + nTiles ) );
            c->dTileOrderCap = nTiles;
            c->tileOrderValid = false;
        }
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
        a.tileOrder = c->dTileOrder;
    }

    /* fold the frame's clear into this march (after the tile-schedule cache compared frames) */
    f.clearFirst = c->clearPending ? 1u : 0u;
    c->clearPending = false;
    /* the pool's uniformity words (VRC_OPT_UNIFORM_BRICKS): NULL = every brick takes the general march */
    f.slotInfo = c->optUniformBricks ? pool->dSlotInfo : nullptr;
    if( mip )
    {
        /* the running maxima: one word per pixel of the pixel buffer in use */
        const size_t pixels = (size_t)c->fbW * c->fbH;
        if( pixels > c->dMipMaxPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dMipMax ) VRC_HIP_CHECK( hipFree( c->dMipMax ) );
            c->dMipMax = nullptr;
            c->dMipMaxPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dMipMax, pixels * sizeof( uint32_t ) ) );
            c->dMipMaxPixels = pixels;
            if( !c->mipFirst ) /* a later pass of a frame whose pixel buffer grew (vrc_set_framebuffer): nothing known */
                VRC_HIP_CHECK( hipMemsetAsync( c->dMipMax, 0xFF, pixels * sizeof( uint32_t ), c->stream ) );
        }
        const bool mean = !iso && c->optMipFold == VRC_MIP_FOLD_MEAN;
        if( mean && pixels > c->dMeanPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dMeanSum ) VRC_HIP_CHECK( hipFree( c->dMeanSum ) );
            if( c->dMeanCount ) VRC_HIP_CHECK( hipFree( c->dMeanCount ) );
            c->dMeanSum = nullptr;
            c->dMeanCount = nullptr;
            c->dMeanPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dMeanSum, pixels * sizeof( unsigned long long ) ) );
            VRC_HIP_CHECK( hipMalloc( &c->dMeanCount, pixels * sizeof( uint32_t ) ) );
            c->dMeanPixels = pixels;
            if( !c->mipFirst ) /* as above: no sample yet, which is a sum of 0 (integer and double alike) and a count of 0 */
            {
                VRC_HIP_CHECK( hipMemsetAsync( c->dMeanSum, 0, pixels * sizeof( unsigned long long ), c->stream ) );
                VRC_HIP_CHECK( hipMemsetAsync( c->dMeanCount, 0, pixels * sizeof( uint32_t ), c->stream ) );
            }
        }
        f.mipMax = c->dMipMax;
        f.mipFirst = c->mipFirst ? 1u : 0u;
        f.slotMax = c->optMipSkip ? pool->dSlotMax : nullptr;
        f.slotMin = c->optMipSkip ? pool->dSlotMin : nullptr;
        f.meanSum = mean ? c->dMeanSum : nullptr;
        f.meanCount = mean ? c->dMeanCount : nullptr;
        if( mipDepth && pixels > c->dMipDepthPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dMipDepth ) VRC_HIP_CHECK( hipFree( c->dMipDepth ) );
            c->dMipDepth = nullptr;
            c->dMipDepthPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dMipDepth, pixels * sizeof( float ) ) );
            c->dMipDepthPixels = pixels;
            if( !c->mipFirst ) /* a later pass (the pixel buffer grew, or dMipMax was large enough from an earlier frame
                                * and keeps the passes so far): no sample equals M yet as far as this buffer knows */
                VRC_HIP_CHECK( hipMemsetD32Async( reinterpret_cast< hipDeviceptr_t >( c->dMipDepth ), 0x7F800000, pixels, c->stream ) );
        }
        f.mipDepth = mipDepth ? c->dMipDepth : nullptr;
        f.mipCue = ( mipDepth && !iso ) ? (float)c->optMipDepthCue / 1000.0f : 0.0f;
        if( iso )
        {
            if( pixels > c->dIsoGradPixels )
            {
                VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
                if( c->dIsoGrad ) VRC_HIP_CHECK( hipFree( c->dIsoGrad ) );
                c->dIsoGrad = nullptr;
                c->dIsoGradPixels = 0;
                VRC_HIP_CHECK( hipMalloc( &c->dIsoGrad, pixels * 3u * sizeof( float ) ) );
                c->dIsoGradPixels = pixels;
                if( !c->mipFirst ) /* (as dMipDepth above: no hit yet as far as this buffer knows) */
                    VRC_HIP_CHECK( hipMemsetAsync( c->dIsoGrad, 0, pixels * 3u * sizeof( float ), c->stream ) );
            }
            f.isoGrad = c->dIsoGrad;
            f.isoThreshold = vrc_iso_int_threshold( c->isoValue, pool->rangeShift, pool->elemBytes == 1 ? 255u : 65535u );
            f.isoStored = vrc_iso_float_threshold( c->isoValue, pool->rangeShift );
            f.isoClassify = c->isoValue + pool->rangeShift;
            f.isoAmbient = c->isoAmbient;
            c->frameIso = true;
            c->frameIsoValue = c->isoValue;
            c->frameIsoAmbient = c->isoAmbient;
        }
        c->gradValid = iso;
        if( !mean && !iso )
        {
            c->frameDepth = c->optMipDepth;
            c->frameCue = c->optMipDepthCue;
        }
        c->depthValid = mipDepth;
        if( mipDepth )
        {
            c->depthFrame = f;
            c->depthRows = c->rowMap;
        }
        c->mipFirst = false;
        if( !iso )
            c->frameFold = c->optMipFold;
        /* what this pass leaves for vrc_get_projection_values */
        c->projState.mipMax = c->dMipMax;
        c->projState.meanSum = c->dMeanSum;
        c->projState.meanCount = c->dMeanCount;
        c->projState.pixels = (uint32_t)pixels;
        c->projState.fold = iso ? (uint32_t)VRC_FOLD_FIRST : (uint32_t)c->optMipFold;
        c->projState.floatState = ( linear || pool->elemBytes == 4 ) ? 1u : 0u;
        c->projState.shift = pool->rangeShift;
    }
    if( cdepth )
    {
        /* the pair per pixel of the pixel buffer in use, where a MIP frame's running maximum and depth are: grown,
         * invalidated by vrc_pre_render (mipFirst) and not read by the frame's first pass as those are */
        const size_t pixels = (size_t)c->fbW * c->fbH;
        if( pixels > c->dMipMaxPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dMipMax ) VRC_HIP_CHECK( hipFree( c->dMipMax ) );
            c->dMipMax = nullptr;
            c->dMipMaxPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dMipMax, pixels * sizeof( uint32_t ) ) );
            c->dMipMaxPixels = pixels;
            if( !c->mipFirst ) /* a later pass of a frame whose pixel buffer grew: no pixel has crossed as far as this knows */
                VRC_HIP_CHECK( hipMemsetAsync( c->dMipMax, 0xFF, pixels * sizeof( uint32_t ), c->stream ) );
        }
        if( pixels > c->dMipDepthPixels )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dMipDepth ) VRC_HIP_CHECK( hipFree( c->dMipDepth ) );
            c->dMipDepth = nullptr;
            c->dMipDepthPixels = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dMipDepth, pixels * sizeof( float ) ) );
            c->dMipDepthPixels = pixels;
            if( !c->mipFirst )
                VRC_HIP_CHECK( hipMemsetD32Async( reinterpret_cast< hipDeviceptr_t >( c->dMipDepth ), 0x7F800000, pixels, c->stream ) );
        }
        f.mipMax = c->dMipMax;
        f.mipDepth = c->dMipDepth;
        f.mipFirst = c->mipFirst ? 1u : 0u;
        c->mipFirst = false;
        c->gradValid = false;
        c->depthValid = true;
        c->depthFrame = f;
        c->depthRows = c->rowMap;
        /* what this pass leaves for vrc_get_projection_values: V as a first-crossing frame leaves it */
        c->projState.mipMax = c->dMipMax;
        c->projState.meanSum = nullptr;
        c->projState.meanCount = nullptr;
        c->projState.pixels = (uint32_t)pixels;
        c->projState.fold = (uint32_t)VRC_FOLD_FIRST;
        c->projState.floatState = ( linear || pool->elemBytes == 4 ) ? 1u : 0u;
        c->projState.shift = pool->rangeShift;
    }
    f.cdepthTau = cdepth ? (float)c->optCompositeDepth / 1000.0f : 0.0f;
    f.preintTable = preint ? c->dPreint : nullptr;
    if( !mip )
        c->framePreint = c->optPreint;
    c->frameProjection = c->optProjection;
    if( !mip )
        c->frameCompositeDepth = c->optCompositeDepth;
    if( !mip )
    {
        c->frameShading = c->optShading;
        c->frameShadingAmbient = c->optShadingAmbient;
    }
    f.shadeAmbient = shade ? (float)c->optShadingAmbient / 1000.0f : 0.0f;

    a.nodes = c->dNodes;
    a.gridTable = ( useDda || c->rayLod ) ? c->dGrid : nullptr;
    a.atlas = usePacked ? pool->dPacked : pool->dAtlas;
    a.packed = usePacked;
    /* a packed atlas of more than 4 GiB, or of a pool of more than 2^32 voxels: 64-bit lane pointers (the BIG instances of
     * the packed modes) */
    a.packedWide = usePacked && ( pool->bigAtlas || pool_packed_bytes( pool ) > 0xFFFFFFFFull );
    a.lut = c->dLut;
    a.pixelBuffer = ctx_fb( c );
    a.sampleCounter = c->optCount ? c->dCounter : nullptr;
    a.clamp = c->cachedClamp;
    a.gridDda = useDda;
    a.fixedStepping = c->optStepping != 0 && slotsFit8Bits;
    a.linear = linear;
    a.elemBytes = pool->elemBytes;
    a.bigAtlas = pool->bigAtlas;
    /* depth split: only where it is exact.  (i) The far half cannot know the near half's opacity, so early ray
     * termination must be impossible: (1 - largest classified alpha)^(most samples a ray can take) stays above
     * 1 - 0.999 (a ray crosses at most sqrt(3) world units -- the volume's longest edge is 1 -- plus one
     * restart sample per brick).  (ii) The frame starts from zero (first pass: the clear is folded in).
     * (iii) the table-driven point-sampling walk kernel. */
    a.depthSplit = false;
    if( c->optDepthSplit && !mip && !shade && !cdepth && !preint && useDda && !useLds && !c->rayLod && !linear && pool->elemBytes == 1 && !pool->bigAtlas &&
        !c->cachedClamp && c->optStepping != 0 && slotsFit8Bits && f.clearFirst )
    {
        const double nMax = 1.7320508 * (double)render->samplesPerRay +
                            3.0 * ( f.gridDim[0] + f.gridDim[1] + f.gridDim[2] ) + 8.0;
        /* with a margin: the kernel accumulates the opacity in float with contracted multiply-adds and regroups the
         * far half's additions, ~1e-6 absolute after 2000 samples = 1e-3 of the 0.001 of transmittance left at
         * the threshold; the bound must clear the threshold by ten times that (0.01 in the logarithm), so that a
         * frame at the limit takes the single-wave kernel rather than a split that might meet an early exit */
        a.depthSplit = VRC_TILE_W == 8u && c->lutMaxAlpha < 1.0f &&
                       nMax * std::log1p( -(double)c->lutMaxAlpha ) > std::log( 1.0 - 0.999 ) + 0.01;
    }
    /* ray compaction: the table-driven point-sampling walk kernel; packed 16-bit pixel coordinates */
    a.ertParts = 0;
    a.rayList = nullptr;
    /* (the same predicate as the launcher's, vrc_launch_raycast: what vrc_get_ray_counts reports is what ran) */
    if( c->optErtParts > 1 && !mip && !shade && !cdepth && !preint && !a.depthSplit && useDda && !useLds && !c->rayLod && !linear && pool->elemBytes == 1 &&
        !pool->bigAtlas && !c->cachedClamp && c->optStepping != 0 && slotsFit8Bits && c->fbW < 65536u && c->fbH < 65536u &&
        VRC_TILE_W == 8u )
    {
        const size_t pixels = (size_t)c->fbW * c->fbH;
        if( pixels > c->dRayListCap )
        {
            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
            if( c->dRayList ) VRC_HIP_CHECK( hipFree( c->dRayList ) );
            c->dRayList = nullptr;
            c->dRayListCap = 0;
            VRC_HIP_CHECK( hipMalloc( &c->dRayList, ( VRC_MAX_ERT_PARTS + 2 * pixels ) * sizeof( uint32_t ) ) );
            c->dRayListCap = pixels;
        }
        a.ertParts = (int)c->optErtParts;
        a.rayList = c->dRayList;
    }
    c->lastErtParts = a.ertParts;
    /* ray cache (VRC_OPT_RAY_CACHE): the tile-scheduled grid walk of vrc_k_raycast only (vrc_pixel_grid_dda; the
     * supersampled GL variant, whose rays are jittered, is not a grid walk).  A frame whose ray constants differ from
     * those of the vrc_render before computes its rays (a moving camera pays nothing); the first that repeats them
     * also stores them, and the ones after that load them.  The kernel-visible fields are set here, after the tile
     * schedule compared frames */
    c->rayCacheUsed = 0;
    {
        const size_t tiles = (size_t)( ( c->fbW + VRC_TILE_W - 1 ) / VRC_TILE_W ) * ( ( c->fbH + VRC_TILE_H - 1 ) / VRC_TILE_H );
        const size_t plane = tiles * 64u; /* whole tiles */
        const bool eligible = c->optRayCache && useDda && !useLds && !c->rayLod && !mip && !glSuper && !a.depthSplit &&
                              a.ertParts <= 1 && VRC_TILE_W * VRC_TILE_H == 64u &&
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
                if( plane > c->dRayCacheCap )
                {
                    VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
                    if( c->dRayCache ) VRC_HIP_CHECK( hipFree( c->dRayCache ) );
                    c->dRayCache = nullptr;
                    c->dRayCacheCap = 0;
                    VRC_HIP_CHECK( hipMalloc( &c->dRayCache, plane * VRC_RAY_CACHE_PLANES * sizeof( float ) ) );
                    c->dRayCacheCap = plane;
                }
                c->rayCacheUsed = VRC_RAY_STORE; /* (valid once the march is on the stream, below) */
            }
            else
                c->rayCacheUsed = VRC_RAY_LOAD;
            std::memcpy( &c->rayPrevFrame, &f, sizeof( f ) );
            c->rayPrevSet = true;
        }
        f.rayMode = (uint32_t)c->rayCacheUsed;
        f.rayCache = c->rayCacheUsed ? c->dRayCache : nullptr;
        f.rayCachePlane = c->rayCacheUsed ? (uint32_t)plane : 0u;
    }
    /* grey transfer function, frame starting from zero: two-float table entries, the same bits (VRC_MODE_GREY) */
    a.greyTable = c->optGreyTable && c->tfGrey && f.clearFirst && !glSuper; /* (a sub-ray starts from the pixel so far) */
    /* walk cache (VRC_OPT_WALK_CACHE): a frame that loads its rays, of the instances the replay march exists for
     * (vrc_internal.h: vrc_walk_replay_eligible).  The first such frame also runs the count pass; the first one after
     * its result has arrived (polled, never waited for) sizes the planes and runs the record pass; the ones after that
     * replay.  Both passes go on the stream in front of the march's timing pair and are no marches: not timed, not
     * counted as launches.  Whatever the lists depend on starts over when it changes: walk_constants_equal here,
     * the node list above, the stream, the row map and the options where they are set; the transfer function, the
     * uniformity words and the pixel buffer's contents are not among them.  What the lists do not depend on may still
     * decide whether they are worth using: where every visit gathers the replay is no faster than the walk, and by 1 to
     * 3 % slower (profiles/r10_walk_cache.txt), so with the option at 1 a view more than half of whose visits gather, by
     * the count pass and the uniformity words it read, is not recorded and stays on the walk until the pool's uploads or
     * VRC_OPT_UNIFORM_BRICKS change; VRC_WALK_CACHE_ALWAYS replays whatever the bricks hold */
    c->walkCacheUsed = 0;
    c->walkLeanUsed = 0;
    c->walkUniformUsed = 0;
    f.walkCache = nullptr;
    f.walkPlane = f.walkK = 0u;
    f.walkLean = f.walkSlots = 0u;
    bool walkCount = false, walkRecord = false;
    {
        /* the form of the lists.  A lean list (vrc_core.h: vrc_frame::walkLean) holds every visit's step count and slot
         * index in one word of 12 + 20 bits.  What the host can see of that: the step is one vrc_exact_step_count counts
         * (its own test, asked here with a travel that passes it), and the pool's slot indices fit.  The rest -- no
         * visit whose count is inexact or takes more than 12 bits -- the count pass reports with the count */
        uint32_t one = 0u;
        const size_t nSlots = pool->resident.size();
        const bool leanAsked = vrc_exact_step_count( f.stepSize, f.stepSize, &one ) && nSlots >= 1u &&
                               nSlots < ( (size_t)1u << VRC_WALK_LEAN_INDEX_BITS );
        const size_t tiles = (size_t)( ( c->fbW + VRC_TILE_W - 1 ) / VRC_TILE_W ) * ( ( c->fbH + VRC_TILE_H - 1 ) / VRC_TILE_H );
        const size_t plane = tiles * 64u;
        const auto fits = [&]( uint32_t k ) { /* the planes of k visits: 32-bit word offsets in the kernels, and the budget */
            const unsigned long long words = ( 1ull + 4ull * k ) * plane;
            return words <= 0xFFFFFFFFull && words * sizeof( uint32_t ) <= (unsigned long long)c->optWalkBudget;
        };
        const bool eligible = c->optWalkCache && c->rayCacheUsed == VRC_RAY_LOAD && vrc_walk_replay_eligible( a ) &&
                              f.nodeCount > 0u && plane > 0u && fits( 1u );
        const bool byContent = c->optWalkCache != VRC_WALK_CACHE_ALWAYS;
        const uint64_t gen = pool->uploadGen; /* (compared only where the choice goes by the bricks' content) */
        if( !eligible || ( c->walkState != vrc_ctx::WALK_IDLE &&
                           ( !walk_constants_equal( c->walkFrame, f ) ||
                             leanAsked != c->walkLeanAsked ||
                             ( byContent && ( c->walkGen != gen || c->walkSlotInfo != f.slotInfo ) ) ) ) )
            c->walkState = vrc_ctx::WALK_IDLE;
        const bool repeats = sameNodes && c->walkPrevSet && ( !byContent || c->walkPrevGen == gen ) &&
                             walk_constants_equal( c->walkPrevFrame, f );
        std::memcpy( &c->walkPrevFrame, &f, sizeof( f ) );
        c->walkPrevSet = true;
        c->walkPrevGen = gen;
        if( eligible )
        {
            if( c->walkState == vrc_ctx::WALK_IDLE && !repeats )
                ; /* mode 0: the next call counts if it is this one again */
            else if( c->walkState == vrc_ctx::WALK_IDLE )
            {
                if( !c->dWalkMax )
                {
                    VRC_HIP_CHECK( hipMalloc( &c->dWalkMax, sizeof( vrc_walk_count ) ) );
                    VRC_HIP_CHECK( hipHostMalloc( &c->hWalkMax, sizeof( vrc_walk_count ) ) );
                    VRC_HIP_CHECK( hipEventCreateWithFlags( &c->evWalk, hipEventDisableTiming ) );
                }
                walkCount = true;
                c->walkLeanAsked = leanAsked;
                c->walkGen = gen;
                c->walkSlotInfo = f.slotInfo;
                c->walkCacheUsed = 1;
            }
            else if( c->walkState == vrc_ctx::WALK_COUNTING )
            {
                c->walkCacheUsed = 2;
                const hipError_t q = hipEventQuery( c->evWalk );
                if( q == hipErrorNotReady )
                    (void)hipGetLastError(); /* (not an error: nothing later may find it there) */
                else if( q != hipSuccess )
                    VRC_HIP_CHECK( q );
                if( q == hipSuccess )
                {
                    const uint32_t k = c->hWalkMax->longest > 0u ? c->hWalkMax->longest : 1u;
                    if( !fits( k ) )
                        c->walkCacheUsed = 0; /* over the budget or the offset limit: this view stays on the walk */
                    else if( byContent && 2u * c->hWalkMax->gathers > c->hWalkMax->visits )
                        c->walkCacheUsed = 0; /* most visits gather: so does this one */
                    else
                    {
                        const size_t words = ( 1u + 4u * (size_t)k ) * plane;
                        if( words > c->dWalkWords )
                        {
                            VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
                            if( c->dWalk ) VRC_HIP_CHECK( hipFree( c->dWalk ) );
                            c->dWalk = nullptr;
                            c->dWalkWords = 0;
                            VRC_HIP_CHECK( hipMalloc( &c->dWalk, words * sizeof( uint32_t ) ) );
                            c->dWalkWords = words;
                        }
                        c->walkK = k;
                        c->walkLean = c->walkLeanAsked && c->hWalkMax->notLean == 0u;
                        c->walkGathers = c->hWalkMax->gathers;
                        walkRecord = true;
                        c->walkCacheUsed = 3;
                    }
                }
            }
            else
                c->walkCacheUsed = 4;
        }
        if( walkRecord || c->walkCacheUsed == 4 )
        {
            f.walkCache = c->dWalk;
            f.walkPlane = (uint32_t)plane;
            f.walkK = c->walkK;
            f.walkLean = c->walkLean ? 1u : 0u;
            f.walkSlots = (uint32_t)nSlots;
            c->walkLeanUsed = ( c->walkLean && c->walkCacheUsed == 4 ) ? 1 : 0;
            /* the uniform-only instance (vrc_kernels_walk.hip): a replayed lean frame none of whose visits gathers --
             * by the count pass of these lists, which is still the answer while the pool has taken no upload and the
             * words are the ones it read.  Where the lists outlive that (VRC_WALK_CACHE_ALWAYS) the frame goes back to
             * the lean instance and keeps them */
            if( c->walkLeanUsed && c->optWalkUniformOnly && c->walkGathers == 0ull && c->walkGen == gen &&
                c->walkSlotInfo == f.slotInfo )
            {
                f.walkLean = VRC_WALK_LEAN_UNIFORM;
                c->walkUniformUsed = 1;
            }
        }
        else if( walkCount )
            f.walkLean = leanAsked ? 1u : 0u; /* (the count pass: check every visit) */
    }
    a.classifier = vrc_make_classifier( lp );

    /* order the march after every brick upload issued so far (fixes quirk Q9) */
    {
        const int rc = ctx_wait_uploads( c, pool );
        if( rc != VRC_OK )
            return rc;
    }
    if( walkCount )
    {
        VRC_HIP_CHECK( hipMemsetAsync( c->dWalkMax, 0, sizeof( vrc_walk_count ), c->stream ) );
        VRC_HIP_CHECK( vrc_launch_walk_record( a, c->dWalkMax, c->stream ) );
        VRC_HIP_CHECK( hipMemcpyAsync( c->hWalkMax, c->dWalkMax, sizeof( vrc_walk_count ), hipMemcpyDeviceToHost, c->stream ) );
        VRC_HIP_CHECK( hipEventRecord( c->evWalk, c->stream ) );
        std::memcpy( &c->walkFrame, &f, sizeof( f ) );
        c->walkState = vrc_ctx::WALK_COUNTING;
        f.walkLean = 0u; /* (asked of the count pass alone) */
    }
    if( walkRecord )
    {
        VRC_HIP_CHECK( vrc_launch_walk_record( a, nullptr, c->stream ) );
        c->walkState = vrc_ctx::WALK_VALID;
        /* this frame still walks: the march below reads none of the planes */
        f.walkCache = nullptr;
        f.walkPlane = f.walkK = 0u;
        f.walkLean = f.walkSlots = 0u;
    }
    if( c->optCount )
        VRC_HIP_CHECK( hipMemsetAsync( c->dCounter, 0, sizeof( unsigned long long ), c->stream ) );
    if( c->optTiming && c->evUsed == c->evRing->pairs.size() )
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
        c->optTiming ? c->evRing->pairs[c->evUsed++] : std::pair< hipEvent_t, hipEvent_t >( nullptr, nullptr );
    vrc_internal_note_kernel_fn( nullptr, 0, 0 ); /* set again by the launchers that report their occupancy */
    /* VRC_OPT_STREAM_MARKERS = 0: the dispatch of a timed march that is one launch carries the pair's second event as its
     * stop event, and that event is also what an upload that recycles a slot waits for.  The pair's first event is
     * recorded in front of the dispatch: the runtime puts a marker on the queue for an attached start event all the
     * same, and a dispatch that carries one holds up a copy queued behind it (profiles/r8_frame_packets.txt).  A
     * launcher says whether it attached the event; the marches of several launches (depth split, ray compaction) do
     * not, and theirs is recorded behind the sequence.  VRC_OPT_STREAM_MARKERS = 1, and a march that is not timed,
     * record the pool's own fence behind the march */
    const bool pairFences = c->optTiming && !c->optStreamMarkers;
    bool attached = false;
    a.stopEvent = pairFences ? evp.second : nullptr;
    a.attached = &attached;
    if( c->optTiming )
        VRC_HIP_CHECK( hipEventRecord( evp.first, c->stream ) );
    VRC_HIP_CHECK( iso         ? vrc_launch_raycast_iso( a, c->stream )
                   : mipDepth  ? vrc_launch_raycast_mip_depth( a, (int)c->optMipFold, c->stream )
                   : mip       ? ( c->optMipFold == VRC_MIP_FOLD_MIN    ? vrc_launch_raycast_minip( a, c->stream )
                                   : c->optMipFold == VRC_MIP_FOLD_MEAN ? vrc_launch_raycast_meanip( a, c->stream )
                                                                        : vrc_launch_raycast_mip( a, c->stream ) )
                   : cdepth    ? vrc_launch_raycast_cdepth( a, c->stream )
                   : preint    ? vrc_launch_raycast_preint( a, c->stream )
                   : shade     ? vrc_launch_raycast_shade( a, c->stream )
                   : useLds    ? vrc_launch_raycast_lds( a, c->stream ) /* (also its per-ray LOD form) */
                   : c->rayLod ? vrc_launch_raycast_raylod( a, c->stream )
                   : c->walkCacheUsed == 4 ? vrc_launch_raycast_replay( a, c->stream )
                               : vrc_launch_raycast( a, c->stream ) );
    if( c->rayCacheUsed == VRC_RAY_STORE )
        c->rayCacheValid = true;
    if( c->optTiming && !attached ) /* (also a frame without tiles, which launches nothing) */
        VRC_HIP_CHECK( hipEventRecord( evp.second, c->stream ) );
    {
        const int rc = pool_fence_behind( pool, c, pairFences ? evp.second : nullptr );
        if( rc != VRC_OK )
            return rc;
    }
    if( c->optCount )
        VRC_HIP_CHECK( hipMemcpyAsync( c->hCounter, c->dCounter, sizeof( unsigned long long ),
                                       hipMemcpyDeviceToHost, c->stream ) );
    c->timed = true; /* a render has happened: vrc_get_stats has something to report */
    c->stats.kernel_variant =
        c->rayLod ? VRC_KERNEL_RAY_LOD
        : useLds  ? VRC_KERNEL_LDS
        : usePacked ? VRC_KERNEL_PACKED
                  : ( useDda ? VRC_KERNEL_GRID_DDA : VRC_KERNEL_REFERENCE_ORDER );
    for( int i = 0; i < 3; ++i )
        c->stats.grid_dims[i] = ( useDda || c->rayLod ) ? (uint32_t)f.gridDim[i] : 0u;
    c->gridWalkUsed = ( useDda || c->rayLod ) ? 1 : 0;
    return VRC_OK;
}

int vrc_post_render( vrc_ctx* c, float* hostRgba )
{
    if( !c )
        return fail( VRC_EINVAL, "vrc_post_render: ctx is NULL" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    {
        const int rc = resolve_clear( c ); /* a frame without a march still ends cleared */
        if( rc != VRC_OK )
            return rc;
    }
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
        return fail( VRC_EINVAL, "vrc_get_projection_values: no VRC_OPT_PROJECTION = MIP vrc_render since the last "
                                 "vrc_pre_render; the values exist from a frame's first MIP pass until the next frame" );
    VRC_HIP_CHECK( hipSetDevice( c->device ) );
    const size_t pixels = c->projState.pixels;
    if( pixels > c->dProjOutPixels )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->dProjOut ) VRC_HIP_CHECK( hipFree( c->dProjOut ) );
        c->dProjOut = nullptr;
        c->dProjOutPixels = 0;
        VRC_HIP_CHECK( hipMalloc( &c->dProjOut, pixels * ( sizeof( float ) + sizeof( uint32_t ) ) ) );
        c->dProjOutPixels = pixels;
    }
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
        return fail( VRC_EINVAL, "vrc_get_projection_depths: no VRC_OPT_PROJECTION = MIP vrc_render since the last "
                                 "vrc_pre_render; the depths exist from a frame's first MIP pass until the next frame" );
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
    if( words > c->dDepthOutWords )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->dDepthOut ) VRC_HIP_CHECK( hipFree( c->dDepthOut ) );
        c->dDepthOut = nullptr;
        c->dDepthOutWords = 0;
        VRC_HIP_CHECK( hipMalloc( &c->dDepthOut, words * sizeof( float ) ) );
        c->dDepthOutWords = words;
    }
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

int vrc_get_projection_gradients( vrc_ctx* c, float* hostG )
{
    if( !c || !hostG )
        return fail( VRC_EINVAL, "vrc_get_projection_gradients: NULL argument" );
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
    {
        const int rc = resolve_clear( c );
        if( rc != VRC_OK )
            return rc;
    }
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
    else if( !c->optTiming )
        c->stats.kernel_ms = 0.f;
    if( c->timed )
    {
        /* the sample counter of the last vrc_render (VRC_OPT_COUNT_SAMPLES) */
        if( c->optCount )
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
    if( c->frameHistCap < bins )
    {
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->dFrameHist ) VRC_HIP_CHECK( hipFree( c->dFrameHist ) );
        if( c->hFrameHist ) VRC_HIP_CHECK( hipHostFree( c->hFrameHist ) );
        c->dFrameHist = nullptr;
        c->hFrameHist = nullptr;
        c->frameHistCap = 0;
        VRC_HIP_CHECK( hipMalloc( &c->dFrameHist, bins * sizeof( unsigned long long ) ) );
        VRC_HIP_CHECK( hipHostMalloc( &c->hFrameHist, bins * sizeof( unsigned long long ) ) );
        c->frameHistCap = bins;
    }
    if( n > c->histRefsCap )
    {
        /* grow the pinned ring and the device list: wait for every copy that reads the old ones */
        VRC_HIP_CHECK( hipStreamSynchronize( c->stream ) );
        if( c->hHistRefs ) VRC_HIP_CHECK( hipHostFree( c->hHistRefs ) );
        if( c->dHistRefs ) VRC_HIP_CHECK( hipFree( c->dHistRefs ) );
        c->hHistRefs = nullptr;
        c->dHistRefs = nullptr;
        c->histRefsCap = 0;
        const size_t cap = std::max< size_t >( 1024, n );
        VRC_HIP_CHECK( hipHostMalloc( &c->hHistRefs, kNodeStages * cap * sizeof( vrc_hist_ref ) ) );
        VRC_HIP_CHECK( hipMalloc( &c->dHistRefs, cap * sizeof( vrc_hist_ref ) ) );
        c->histRefsCap = cap;
        for( int s = 0; s < kNodeStages; ++s )
            c->histRefsUsed[s] = false;
    }
    /* the rows are written on the pool's upload stream */
    {
        const int rc = ctx_wait_uploads( c, pool );
        if( rc != VRC_OK )
            return rc;
    }
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
    {
        /* the context's render fence on the pool (pool_upload) now stands behind this reduction too: an upload that
         * recycles one of these slots does not overwrite its row while the reduction reads it */
        const int rc = pool_fence_behind( pool, c, nullptr );
        if( rc != VRC_OK )
            return rc;
    }
    return VRC_OK;
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
