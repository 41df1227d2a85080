/* vrc_internal.h -- launcher interface between vrc_api.hip (host logic) and
 * vrc_kernels.hip (gfx950 kernels).  Not part of the public C ABI. */
#ifndef VRC_INTERNAL_H
#define VRC_INTERNAL_H

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "vrc_core.h"

/* pixel tile of one wave64 */
#ifndef VRC_TILE_W
#define VRC_TILE_W 8u
#endif
#define VRC_TILE_H ( 64u / VRC_TILE_W )

/* Tile schedule.  The unit of the schedule is a 2x2 block of tiles (16x16 pixels): its four tiles take four
 * consecutive slots, and every raycast kernel runs four waves per workgroup, so the four waves of a
 * workgroup -- same CU, same vector L1 -- march neighbouring tiles and the micro-block lines two of them
 * share are fetched from L2 once (measured on C2 with the gather kernel: -3 % kernel time).  A frame whose
 * tile count is odd in x or y has units with fewer than four tiles: their spare slots hold VRC_NO_TILE.
 *
 * Round 4: the schedule is XCD-aware.  The dispatcher deals workgroups b, b + 1, ... round-robin over the 8 XCDs
 * (MI355X_MICROARCH.md, "Workgroup dispatch") and each XCD has its own L2: workgroup b takes unit (b / 8) of XCD
 * (b % 8)'s list.  A list is made of SUPER-TILES of VRC_SUPER_UNITS x VRC_SUPER_UNITS units (their units in Morton
 * order), dealt to the XCDs heaviest first in snake order.  Measured on C2 (profiles/r4_schedule_and_hbm_requests.txt):
 * the L2s fill whole 128-byte lines (TCC_EA0_RDREQ_128B = every request of these kernels) and fetch 1.9 x the packed (32-bit texel)
 * atlas per trilinear frame, 2.2 x the volume per point-sampled frame; super-tiles of 4 x 4 units (64 x 64 pixels on
 * one XCD) take 7 % of those requests away and no time (neighbouring workgroups drift apart in depth by more than the
 * few steps an L2 remembers), and cost the LDS-staged kernel 5 % (coarser heaviest-first order).  So the product keeps
 * super-tiles of ONE unit -- the heaviest-first order of rounds 1-3, with the XCD of every workgroup explicit -- and
 * the size stays a developer switch.  The schedule has VRC_XCDS x ceil(super-tiles / VRC_XCDS) x VRC_SUPER_UNITS^2
 * units; those outside the frame hold VRC_NO_TILE. */
#define VRC_NO_TILE 0xFFFFFFFFu
#define VRC_WAVES_PER_GROUP 4u
#ifndef VRC_SUPER_UNITS
#define VRC_SUPER_UNITS 1u
#endif
#define VRC_XCDS 8u
__host__ __device__ inline uint32_t vrc_super_x( uint32_t tilesX ) { return ( ( tilesX + 1u ) / 2u + VRC_SUPER_UNITS - 1u ) / VRC_SUPER_UNITS; }
__host__ __device__ inline uint32_t vrc_schedule_units( uint32_t tilesX, uint32_t tilesY )
{
    const uint32_t nSuper = vrc_super_x( tilesX ) * vrc_super_x( tilesY );
    return ( nSuper + VRC_XCDS - 1u ) / VRC_XCDS * VRC_XCDS * VRC_SUPER_UNITS * VRC_SUPER_UNITS;
}
__host__ __device__ inline uint32_t vrc_schedule_slots( uint32_t tilesX, uint32_t tilesY )
{
    return vrc_schedule_units( tilesX, tilesY ) * 4u;
}
/* tile of slot `slot` of unit `unit` (units row-major over the frame): VRC_NO_TILE outside the frame */
__host__ __device__ inline uint32_t vrc_unit_tile( uint32_t unit, uint32_t sub, uint32_t tilesX, uint32_t tilesY )
{
    const uint32_t unitsX = ( tilesX + 1u ) / 2u;
    const uint32_t tx = ( unit % unitsX ) * 2u + ( sub & 1u ), ty = ( unit / unitsX ) * 2u + ( sub >> 1 );
    return ( tx < tilesX && ty < tilesY ) ? ty * tilesX + tx : VRC_NO_TILE;
}
/* the tile a wave takes: from the schedule, or (no schedule) units in row-major order */
__device__ inline uint32_t vrc_slot_tile( const uint32_t* __restrict__ tileOrder, uint32_t slot, uint32_t tilesX,
                                          uint32_t tilesY )
{
    return tileOrder ? tileOrder[slot] : vrc_unit_tile( slot >> 2, slot & 3u, tilesX, tilesY );
}

/* tf: 256 float4 (device).  lut: VRC_TFP_ENTRIES float4 (device): the classified table
 * (rgb*alpha', alpha') with entries 256.. = 0, or with linear the padded transfer function. */
hipError_t vrc_launch_build_lut( const float* tf, vrc_f4* lut, vrc_lut_params p, bool linear,
                                 hipStream_t stream );

/* the first-visit table of the lean replay (vrc_core.h: vrc_first_visit_row) from the classified table `lut` (device,
 * not the padded transfer function): VRC_FIRST_VISIT_ENTRIES x VRC_FIRST_VISIT_ROWS colours at `table` (device), of two
 * floats (grey: what the grey instances stage of an entry, x and w) or four.  One lane per entry, behind the table's own
 * build on `stream` */
hipError_t vrc_launch_build_first_visit( const vrc_f4* lut, void* table, bool grey, hipStream_t stream );

/* row-major brick (size voxels, elemBytes per voxel) -> micro-blocked slot (slot = device
 * pointer to the slot's first element; slotDim = padded slot size in voxels).  A brick smaller
 * than the slot gets its border voxels replicated into the padding.
 * xform: what a voxel undergoes on the way (vrc_core.h: VRC_XF_*; elemBytes is the size of a voxel on both sides).
 * slotInfo (may be NULL): the slot's uniformity word (vrc_core.h: VRC_SLOT_*), which the caller zeroed on `stream`
 * before this call; the kernel ORs into it what it finds.
 * slotMax (may be NULL): the slot's largest stored value (vrc_core.h: vrc_frame::slotMax), zeroed by the caller in the
 * same way; the kernel leaves the word of the voxels it wrote (padding copies repeat voxels of the brick).
 * slotMin (may be NULL): the same for the slot's smallest stored value (vrc_frame::slotMin). */
hipError_t vrc_launch_repack_brick( const void* srcRowMajor, void* slot, uint32_t elemBytes,
                                    const uint32_t size[3], const uint32_t slotDim[3],
                                    hipStream_t stream, uint32_t* slotInfo = nullptr,
                                    uint32_t xform = VRC_XF_NONE, uint32_t* slotMax = nullptr,
                                    uint32_t* slotMin = nullptr );

/* atlas -> tap-packed atlas (vrc_core.h): the packed texels of elements [firstElem, firstElem + nElems) of the atlas of
 * 8- or 16-bit voxels (whole slots; the packed atlas holds vrc_packed_elems( atlas elements ) texels of
 * VRC_PK_TEXEL( elemBytes ) bytes) */
hipError_t vrc_launch_pack_slots( const void* atlas, void* packed, uint64_t firstElem, uint64_t nElems,
                                  const uint32_t slotDim[3], uint32_t elemBytes, hipStream_t stream );

/* inverse, for tests: logical atlas region -> row-major (xform: VRC_XF_NONE or VRC_XF_FLIP, its own inverse) */
hipError_t vrc_launch_read_region( const void* atlas, void* dstRowMajor, uint32_t elemBytes,
                                   const uint32_t origin[3], const uint32_t size[3],
                                   const vrc_layout& lay, hipStream_t stream, uint32_t xform = VRC_XF_NONE );

/* brick histograms (vrc_kernels.hip): an entry is a region of one slot and the row of `rows` its counts are added to
 * (uint32, binCount per row; the caller zeroes the rows).  Bin = v / (typeRange / binCount); 8- or 16-bit voxels,
 * binCount a divisor of the type's range, at most VRC_HIST_MAX_BINS.  maxRegionVoxels: the largest region of the list
 * (sizes the launch).  one != NULL: a single entry passed by value (no device list) */
#define VRC_HIST_MAX_BINS 4096u
struct vrc_hist_entry
{
    uint64_t base;      /* element offset of the slot in the atlas */
    uint32_t origin[3]; /* region, slot-local voxels */
    uint32_t size[3];
    uint32_t row;
    uint32_t pad;
};
hipError_t vrc_launch_bin_bricks( const void* atlas, uint32_t elemBytes, const uint32_t slotDim[3],
                                  const vrc_hist_entry* dEntries, uint32_t nEntries, const vrc_hist_entry* one,
                                  uint64_t maxRegionVoxels, uint32_t binCount, uint32_t* rows, hipStream_t stream );
/* frame histogram: out[b] = (out[b] if accumulate) + sum_i rows[refs[i].row][b] * refs[i].scale (uint64) */
struct vrc_hist_ref
{
    uint32_t row;
    uint32_t pad;
    uint64_t scale;
};
hipError_t vrc_launch_frame_histogram( const uint32_t* rows, uint32_t binCount, const vrc_hist_ref* dRefs, uint32_t n,
                                       unsigned long long* out, bool accumulate, hipStream_t stream );

#define VRC_MAX_ERT_PARTS 8

struct vrc_raycast_args
{
    vrc_frame frame;
    const vrc_dev_node* nodes;
    const int32_t* gridTable; /* NULL for the reference-order kernel */
    const void* atlas;
    const vrc_f4* lut;
    vrc_f4* pixelBuffer;
    unsigned long long* sampleCounter; /* NULL = do not count */
    const uint32_t* tileOrder;         /* NULL = row-major tile order */
    bool clamp;
    bool gridDda;
    bool fixedStepping; /* VRC_OPT_STEPPING */
    bool linear;        /* VRC_OPT_FILTER = 1 (trilinear) */
    uint32_t elemBytes; /* atlas element size: 1 (u8), 2 (u16; classified per sample) or 4 (float; classified per
                         * sample).  lut holds the padded transfer function whenever samples are classified one by one */
    vrc_classifier classifier;
    bool bigAtlas; /* more than 2^32 voxels: node slot bases are 64-bit (BIG kernel instances) */
    bool greyTable;    /* the transfer function is grey and the frame starts from zero: the two-float table form
                        * (VRC_MODE_GREY) of the point-sampling grid-walk kernel composites the same bits */
    int ertParts;      /* > 1: ray compaction, the march in this many launches (vrc_k_raycast_part); the host sets it
                        * only for the table-driven point-sampling walk kernel and frames below 65536 pixels a side */
    uint32_t* rayList; /* counts[VRC_MAX_ERT_PARTS] | two lists of width * height packed pixels */
    bool packed;     /* trilinear through the tap-packed atlas: atlas = the pool's packed atlas (vrc_march_segment_packed) */
    bool packedWide; /* ... of more than 4 GiB, or of an atlas of more than 2^32 voxels: 64-bit lane pointers instead of
                      * scalar base + 32-bit offset (BIG instances) */
    bool depthSplit; /* two waves per tile, near / far half of every ray (vrc_k_raycast_split): set by the host
                      * only when early ray termination cannot occur in this frame and the frame is cleared */
    /* VRC_OPT_STREAM_MARKERS = 0: the event the march's own dispatch carries as its stop event (NULL = none), and where
     * the launcher says that it did: a launcher whose march is one dispatch hands the event to it (vrc_launch_march) and
     * sets *attached; the forms of several launches (depth split, ray compaction) leave both alone, and vrc_render
     * records the event behind the sequence */
    hipEvent_t stopEvent;
    bool* attached;
    bool shade; /* a shaded composite frame (VRC_OPT_SHADING = 1; frame.shadeAmbient set): vrc_launch_raycast_shade marches it */
    bool cdepth; /* a composite frame that keeps the depth of its rays' crossings (VRC_OPT_COMPOSITE_DEPTH above 0; frame.cdepthTau,
                  * frame.mipMax and frame.mipDepth set): vrc_launch_raycast_cdepth marches it */
    bool preint; /* a pre-integrated composite frame (VRC_OPT_PREINTEGRATION = 1; frame.preintTable set):
                  * vrc_launch_raycast_preint marches it */
    bool slice;  /* a slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE; frame.slicePlane, frame.mipMax and
                  * frame.mipDepth set): vrc_launch_raycast_slice renders it */
};

/* the one dispatch of a single-launch march: with a's stop event if it has one (the dispatch then carries its own
 * completion and end timestamp: no marker packet behind it), else the plain launch */
template < typename... KArgs, typename... Args >
static inline void vrc_launch_march( const vrc_raycast_args& a, void ( *kernel )( KArgs... ), dim3 grid, dim3 block,
                                     uint32_t dynamicLds, hipStream_t stream, Args&&... args )
{
    static_assert( sizeof...( KArgs ) == sizeof...( Args ), "one argument per kernel parameter" );
    if( a.stopEvent )
    {
        hipExtLaunchKernelGGL< KArgs... >( kernel, grid, block, dynamicLds, stream, nullptr, a.stopEvent, 0u,
                                           static_cast< KArgs >( args )... );
        *a.attached = true;
    }
    else
        hipLaunchKernelGGL( kernel, grid, block, dynamicLds, stream, static_cast< KArgs >( args )... );
}

/* the frame's tile schedule (above): order: vrc_schedule_slots() uint32; scratch: VRC_TILE_SCRATCH_WORDS uint32;
 * bucket: one byte per super-tile (at most one per schedule slot) */
#define VRC_TILE_SCRATCH_WORDS 260u
hipError_t vrc_launch_tile_order( const vrc_frame& f, uint32_t* order, uint32_t* scratch,
                                  uint8_t* bucket, hipStream_t stream );

hipError_t vrc_launch_raycast( const vrc_raycast_args& a, hipStream_t stream );

/* The walk cache (vrc_kernels_walk.hip; VRC_OPT_WALK_CACHE).  The replay march exists for the frames vrc_launch_raycast
 * hands to the tile-scheduled grid walk of the table-driven point-sampling march of 8-bit voxels with fixed-point
 * stepping -- vrc_k_raycast<true,false,COUNT,true,VRC_MODE_TABLE or VRC_MODE_GREY,unsigned char,GROUP,false>, the
 * instances the uniform-brick march exists for -- and takes the group size that launcher would (the sizes are defined
 * here, once, for vrc_kernels.hip and vrc_kernels_walk.hip) */
#ifndef VRC_GREY_GROUP
/* samples a lane of the grey form keeps in flight: its two-float colours and table entries leave registers for 14 at
 * five waves per SIMD (93 VGPRs with the sample counter, 82 without); measured on C2 against 8: 0.509 -> 0.481 ms
 * (mem://), 0.512 -> 0.482 ms (noise); 12: 0.491 / 0.484; 16 (96 VGPRs): 0.487 */
#define VRC_GREY_GROUP 14
#endif
#ifndef VRC_SMALL_GROUP
#define VRC_SMALL_GROUP 24 /* samples in flight per lane in launches too small to fill the GPU (latency-bound: 16 -> 24: -5 % on a rank's share of an 8-rank frame, -4 % of a 4-rank frame; 32: -7 % / -3 %) */
#endif
/* launches of at most ~1.5 waves per SIMD slot (256 CUs x 4 SIMDs x 4 waves) are latency-bound:
 * measured 0.153 -> 0.130 ms for an eighth of the C2 frame, 0.538 -> 0.562 ms for the whole */
#ifndef VRC_SMALL_LAUNCH_TILES
#define VRC_SMALL_LAUNCH_TILES 6144u /* (8192 = half a 1024^2 frame: one frame alone 0.303 -> 0.287 ms, three in flight 4428 -> 4365 frames/s: not taken) */
#endif
static inline bool vrc_walk_replay_eligible( const vrc_raycast_args& a )
{
    return a.gridDda && a.gridTable && !a.packed && !a.linear && a.elemBytes == 1 && !a.bigAtlas && !a.clamp &&
           a.fixedStepping && a.ertParts <= 1 && !a.depthSplit && !a.shade && !a.cdepth && !a.preint && !a.slice &&
           VRC_TILE_W == 8u;
}
static inline int vrc_walk_replay_group( const vrc_raycast_args& a )
{
    const uint32_t tiles = ( ( a.frame.width + VRC_TILE_W - 1 ) / VRC_TILE_W ) * ( ( a.frame.height + VRC_TILE_H - 1 ) / VRC_TILE_H );
    return tiles <= VRC_SMALL_LAUNCH_TILES ? VRC_SMALL_GROUP : ( a.greyTable ? VRC_GREY_GROUP : VRC_GROUP );
}
/* what the count pass finds: the longest list of the frame, the visits of all its rays, and those of them whose brick
 * is not known to be uniform (a.frame.slotInfo as it is on `stream`): visits that would take the gather march.  notLean
 * (a.frame.walkLean set): 1 when a visit does not pack into a lean list's word (vrc_core.h: vrc_walk_lean_word) */
struct vrc_walk_count
{
    uint32_t longest, notLean;
    unsigned long long visits, gathers;
};
/* the record form of the grid walk: a.frame.rayMode = VRC_RAY_LOAD; a.frame.walkK = 0: the count pass folds the frame
 * into *result (device memory the caller zeroed on `stream`), nothing else is written; walkK > 0: the record pass fills
 * a.frame.walkCache and result is not used.  Not a march: no kernel note, no stop event */
hipError_t vrc_launch_walk_record( const vrc_raycast_args& a, vrc_walk_count* result, hipStream_t stream );
/* the resolved visit words of a lean frame's lists (vrc_core.h: vrc_walk_resolved_word): f.walkK planes of f.walkPlane
 * words at `resolved` (device), from f.walkCache and f.slotInfo as they are on `stream`.  Not a march: no kernel note, no
 * stop event */
hipError_t vrc_launch_walk_resolve( const vrc_frame& f, uint32_t* resolved, hipStream_t stream );
/* the march of a frame whose lists are valid (a.frame.walkCache, walkPlane, walkK; rayMode = VRC_RAY_LOAD); a.gridTable
 * is not read.  hipErrorInvalidValue for a frame outside the instance set */
hipError_t vrc_launch_raycast_replay( const vrc_raycast_args& a, hipStream_t stream );

/* maximum-intensity projection (vrc_kernels_mip.hip): point or trilinear (a.linear) samples by gathers, reference-order
 * loop or grid walk (a.gridDda); lut = the padded transfer function; frame.mipMax set */
hipError_t vrc_launch_raycast_mip( const vrc_raycast_args& a, hipStream_t stream );
/* ... and its other folds (VRC_OPT_MIP_FOLD; vrc_kernels_minip.hip, vrc_kernels_meanip.hip): the minimum meets in
 * frame.mipMax as the maximum does and skips by frame.slotMin; the mean needs frame.meanSum and frame.meanCount */
hipError_t vrc_launch_raycast_minip( const vrc_raycast_args& a, hipStream_t stream );
hipError_t vrc_launch_raycast_meanip( const vrc_raycast_args& a, hipStream_t stream );

/* the per-pixel state a MIP frame's passes left, as vrc_get_projection_values returns it (vrc_kernels_meanip.hip):
 * values[i] = M of pixel i in the volume's own units (shift: what an offset-binary atlas added to every voxel), counts[i]
 * = the mean's sample count, or whether a maximum / minimum exists.  Device pointers, `pixels` entries each */
struct vrc_projection_state
{
    const uint32_t* mipMax;            /* maximum and minimum */
    const unsigned long long* meanSum; /* mean */
    const uint32_t* meanCount;
    uint32_t pixels;
    uint32_t fold;       /* VRC_FOLD_* */
    uint32_t floatState; /* M is a float / the sum a double (the float atlas, trilinear samples); else integers */
    float shift;
};
hipError_t vrc_launch_projection_values( const vrc_projection_state& st, float* values, uint32_t* counts, hipStream_t stream );

/* the maximum and the minimum with the depth of the projected sample (vrc_kernels_mipdepth.hip; VRC_OPT_MIP_DEPTH,
 * VRC_OPT_MIP_DEPTH_CUE): fold = VRC_FOLD_MAX or VRC_FOLD_MIN, frame.mipDepth set beside frame.mipMax ... */
hipError_t vrc_launch_raycast_mip_depth( const vrc_raycast_args& a, int fold, hipStream_t stream );
/* ... and what vrc_get_projection_depths returns of it: t[i] = D of pixel i, xyz (or NULL) = origin + D * dir of the
 * pixel's ray in the frame f of the last pass (its camera, pixel buffer geometry and row map).  Device pointers */
hipError_t vrc_launch_projection_depths( const vrc_frame& f, const float* depth, uint32_t pixels, float* t, float* xyz,
                                         hipStream_t stream );

/* an isosurface frame (vrc_kernels_iso.hip; VRC_OPT_PROJECTION = VRC_PROJECTION_ISO): the first-crossing fold of the MIP
 * kernel; frame.mipMax, frame.mipDepth and frame.isoGrad set, frame.slotMax = NULL: every sample is taken */
hipError_t vrc_launch_raycast_iso( const vrc_raycast_args& a, hipStream_t stream );

/* a slice frame (vrc_kernels_slice.hip; VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE): a.slice, frame.slicePlane, frame.mipMax
 * and frame.mipDepth set; the culled list of the reference-order form or a look-up in the brick grid (a.gridDda), one
 * point sample or eight taps (a.linear), every atlas type; lut = the padded transfer function.  One launch */
hipError_t vrc_launch_raycast_slice( const vrc_raycast_args& a, hipStream_t stream );

/* a shaded composite frame (vrc_kernels_shade.hip; VRC_OPT_SHADING = 1): a.shade and frame.shadeAmbient set; the
 * reference-order loop or the grid walk (a.gridDda), point or trilinear (a.linear) samples by gathers, every atlas type;
 * lut = the classified table (8-bit point samples) or the padded transfer function, as vrc_launch_raycast takes it */
hipError_t vrc_launch_raycast_shade( const vrc_raycast_args& a, hipStream_t stream );

/* the depth of a composite frame (vrc_kernels_cdepth.hip; VRC_OPT_COMPOSITE_DEPTH above 0): a.cdepth, frame.cdepthTau,
 * frame.mipMax and frame.mipDepth set; the forms, atlas types and lut of vrc_launch_raycast_shade */
hipError_t vrc_launch_raycast_cdepth( const vrc_raycast_args& a, hipStream_t stream );

/* a pre-integrated composite frame (vrc_kernels_preint.hip; VRC_OPT_PREINTEGRATION = 1): a.preint and frame.preintTable
 * set; the forms, atlas types and lut of vrc_launch_raycast_shade (lut is what a uniform brick is marched from) */
hipError_t vrc_launch_raycast_preint( const vrc_raycast_args& a, hipStream_t stream );
/* its table (vrc_core.h: vrc_preint_table_entry): 256 x 256 entries of `kind` (VRC_PREINT_VALUE, VRC_PREINT_TEXEL) from
 * the 256-texel transfer function tf; lut: the classified table the value-indexed diagonal copies (may be NULL for
 * VRC_PREINT_TEXEL).  One launch, float64 */
hipError_t vrc_launch_build_preint( const float* tf, const vrc_f4* lut, vrc_f4* table, vrc_lut_params p, int kind,
                                    hipStream_t stream );

/* LDS-staged form (vrc_kernels_lds.hip): needs gridTable, !clamp, 8x8 tiles */
hipError_t vrc_launch_raycast_lds( const vrc_raycast_args& a, hipStream_t stream );


/* per-ray adaptive LOD form (vrc_kernels_raylod.hip): gridTable = frame.lodLevels cell -> node
 * tables, lut = VRC_MAX_LOD_LEVELS classified tables of VRC_LUT_ENTRIES (u8 point sampling) or the
 * padded transfer function */
hipError_t vrc_launch_raycast_raylod( const vrc_raycast_args& a, hipStream_t stream );

/* shared by the translation units of libvrc_hip.so (vrc_api.hip owns the state) */
#include <string>
struct vrc_ctx;
int vrc_internal_fail( int code, const std::string& msg );          /* sets vrc_last_error, returns code */
void vrc_internal_note_kernel( const char* fmt, ... );               /* the kernel instance a launcher took (vrc_last_kernel) */
void vrc_internal_note_kernel_fn( const void* fn, int threads, size_t dynamicLds ); /* ... and its entry point (vrc_last_kernel_occupancy) */
hipStream_t vrc_internal_ctx_stream( vrc_ctx* ctx, int* deviceOut ); /* the context's render stream + device */

#endif
