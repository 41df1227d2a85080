/*
 * vrc_hip.h -- C ABI of libvrc_hip.so, the MI355X (gfx950) device layer of the volume
 * raycaster.  It replaces, entry point for entry point, the reference's CUDA device layer
 * renderers/cudaRaycaster/cuda/ (classes cuda::Renderer, cuda::TexturePool, cuda::ColorMap,
 * cuda::ClipPlanes, cuda::PixelBufferObject), which the host plugin classes
 * CudaRaycastRenderer / CudaTexturePool / CudaTextureObject call.  Everything here is
 * plain C: opaque handles, PODs, pointers and sizes.  No torch, no C++ types.
 *
 * Reference citations are path:line relative to the reference root.
 *
 * Return convention: 0 = VRC_OK, otherwise a VRC_E* code; vrc_last_error() returns the
 * thread-local message (the reference throws std::runtime_error from checkCudaErrors,
 * cuda/cuda.h:39-53; the C++ shim rethrows the same exception types).
 *
 * Threading (mirrors SURVEY 8b): vrc_pool_* are thread-safe (the reference guards its free
 * list with a mutex, cuda/TexturePool.cu:179-185, and calls copyToSlot from 3 threads);
 * vrc_update/pre_render/render/post_render are single-threaded per context.  Unlike the
 * reference (quirk Q9) every upload is ordered before the next vrc_render by an event.
 */
#ifndef VRC_HIP_H
#define VRC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRC_OK 0
#define VRC_EINVAL 1     /* bad argument */
#define VRC_EHIP 2       /* a HIP runtime call failed (message has hipGetErrorString) */
#define VRC_EFULL 3      /* no free slot in the pool: slot = (-1,-1,-1), TexturePool.cu:180-181 */
#define VRC_ENOMEM 4     /* allocation failed */
#define VRC_EUNSUPPORTED 5 /* unsupported data type / channel count, TexturePool.cu:66-67 */
#define VRC_EHIERARCHY 6  /* vrc_set_ray_lod is on and the node list of vrc_render is not a brick hierarchy
                          * (nothing was rendered; the caller may render its per-brick cut instead) */
#define VRC_ECOMM 7       /* RCCL missing or an RCCL call failed (vrc_comm_*, vrc_gather_tiles) */

typedef struct vrc_ctx vrc_ctx;   /* replaces cuda::Renderer (cuda/Renderer.cuh:69-112) */
typedef struct vrc_pool vrc_pool; /* replaces cuda::TexturePool (cuda/TexturePool.cuh:42-103) */

/* cuda/Renderer.cuh:35-41 -- 12 floats, 48 bytes, same field order */
typedef struct
{
    float textureMin[3];  /* normalized atlas origin of the brick interior */
    float textureSize[3]; /* normalized atlas size of the brick interior */
    float aabbMin[3];     /* world box min */
    float aabbSize[3];    /* world box size */
} vrc_node_data;

/* cuda/Renderer.cuh:46-56, same field order.  Matrices are column-major float[16]. */
typedef struct
{
    float eyePosition[3];
    uint32_t glViewport[4]; /* x, y, w, h; the kernel maps pixel (px,py) of the buffer */
    float invProjMatrix[16];
    float modelViewMatrix[16]; /* carried for ABI shape; unused by the kernel (quirk Q3) */
    float invViewMatrix[16];
    float aabbMin[3];
    float aabbMax[3];
    float nearPlane;
} vrc_view_data;

/* cuda/Renderer.cuh:59-66, same field order */
typedef struct
{
    uint32_t samplesPerRay;
    uint32_t samplesPerPixel;  /* unused by the kernel (quirk Q3) */
    uint32_t maxSamplesPerRay; /* opacity-correction reference, 32 in the reference */
    uint32_t datatype;         /* unused by the kernel (quirk Q2) */
    float dataSourceRange[2];
} vrc_render_data;

/* per-render statistics (not in the reference; feeds bench.py's Msamples/s and roofline) */
typedef struct
{
    float kernel_ms;        /* HIP-event time of the last raycast kernel on the ctx stream */
    uint64_t samples;       /* samples composited by the last vrc_render (0 if counting is off) */
    uint32_t kernel_variant; /* which kernel ran: VRC_KERNEL_* */
    uint32_t grid_dims[3];  /* brick-grid dims used by the DDA kernel (0 if not used) */
    double kernel_ms_sum;   /* sum of HIP-event times of the raycast kernels launched since ... */
    uint32_t kernel_launches; /* ... the previous vrc_get_stats call, and how many they were */
} vrc_stats;

/* ---- options (vrc_set_option) ---------------------------------------------------------- */
#define VRC_OPT_KERNEL 1          /* VRC_KERNEL_AUTO (default) | _REFERENCE_ORDER | _GRID_DDA | _LDS | _PACKED */
#define VRC_OPT_FILTER 2          /* VRC_FILTER_NEAREST (reference parity, default) | VRC_FILTER_TRILINEAR */
#define VRC_OPT_TF_FRAC_BITS 3    /* 8 (default, CUDA 1.8 fixed-point lerp weight) | 0 exact float */
#define VRC_OPT_COUNT_SAMPLES 4   /* 0 (default) | 1: count composited samples (slower kernel) */
#define VRC_OPT_TILE_ORDER 5      /* 1 (default): heaviest-first tile schedule | 0: row-major tiles */
#define VRC_OPT_STEPPING 6        /* sample positions inside a brick: 1 (default) 8.24 fixed-point
                                   * voxel-space increments | 0 the reference's float world-space
                                   * accumulation (cuda/Renderer.cu:208: pos += step) */

#define VRC_OPT_VARIANT 7         /* which of the reference's two raycasters the frame must match:
                                   * VRC_VARIANT_CUDARAYCASTER (default) | VRC_VARIANT_GLRAYCASTER */

#define VRC_OPT_KERNEL_USED 8      /* read-only (vrc_get_option): VRC_KERNEL_* of the last vrc_render, without the
                                   * synchronisation vrc_get_stats implies.  It does not say how the bricks of
                                   * a ray were found: PACKED marches a node list that is not a brick grid in
                                   * list order, as REFERENCE_ORDER does -- VRC_OPT_GRID_WALK_USED says which */

#define VRC_OPT_KERNEL_TIMING 9    /* 1 (default): a HIP event pair around every raycast launch feeds vrc_get_stats'
                                   * kernel times; 0: no events (two host calls less per vrc_render; vrc_get_stats
                                   * then reports 0 ms and 0 launches) */

#define VRC_OPT_DEPTH_SPLIT 10     /* 0 (default) | 1: two waves per 8x8 tile, one for the bricks in the near and one for
                                   * those in the far half of every ray, composited with `over`: halves the
                                   * latency of launches too small to fill the GPU (a rank's share of a sort-first
                                   * frame) at ~15 % more work.  Same samples (every brick is marched whole by one of
                                   * the two); taken only where exact: frames in which early ray termination cannot
                                   * occur (largest classified opacity ^ most samples per ray), first pass of a
                                   * frame, the point-sampling grid-walk kernel; silently the plain kernel else */

#define VRC_OPT_ERT_COMPACTION 11  /* 0 (default) | 2..8 = P: ray compaction for early ray termination
                                   * (cuda/Renderer.cu:219-226).  The march runs in P launches, one per slab of the
                                   * brick grid along the view axis; after each, a wave-level ballot packs the rays
                                   * that are still below the opacity threshold into a list, and the next launch marches
                                   * 64 live rays per wave from it instead of tiles whose lanes have mostly finished.
                                   * Same bricks, same order, same arithmetic per ray: the frame is bit-identical to
                                   * the single launch.  Pays only for frames in which many, but not all, rays of a
                                   * tile end early (DESIGN.md section 4 has the measurements); the point-sampling
                                   * grid-walk kernel only, silently the plain kernel else.  With per-launch lists:
                                   * vrc_get_ray_counts */

#define VRC_OPT_GREY_TABLE 12      /* 1 (default) | 0.  A transfer function whose red, green and blue are equal in every
                                   * entry (bit for bit) lets the kernels keep (grey, alpha)
                                   * instead of four floats per classified-table entry and per colour: half the
                                   * table bytes in LDS and three fused multiply-adds less per sample.  The three colour
                                   * channels of the reference's blend (cuda/Renderer.cu:83-93) are then the same
                                   * operations on the same numbers, so the frame is bit-identical; first pass of
                                   * a frame only (the pixel starts from zero).  0: always the four-float form */

#define VRC_OPT_PACKED_ATLAS 13    /* 1 (default) | 0.  May VRC_KERNEL_AUTO build the pool's tap-packed atlas (VRC_KERNEL_PACKED:
                                   * 2.25 times the bytes of the brick atlas, on top of the budget given to
                                   * vrc_pool_create) the first time a frame with the trilinear filter could use it?
                                   * 0: AUTO stays with the LDS-staged / gather forms; asking for VRC_KERNEL_PACKED
                                   * explicitly still builds it */

#define VRC_OPT_GRID_WALK_USED 14  /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render found the
                                   * bricks of every ray through the brick grid (the grid walk of GRID_DDA, LDS or
                                   * PACKED on a grid-aligned node set, or per-ray LOD) -- then the order of the node
                                   * list did not matter to it; 0 if it marched the list in its order (the
                                   * reference-order loop of any kernel form), or before the first vrc_render */

#define VRC_OPT_UNIFORM_BRICKS 15   /* 1 (default) | 0.  Every brick upload notes whether all the voxels it wrote (overlap
                                   * included) hold one value.  A wave whose rays are all inside such bricks takes its
                                   * samples from that value's classified-table entry instead of fetching them: same
                                   * samples, same order, same arithmetic -- the same frame and sample count, bit for
                                   * bit -- without the addressing and the gathers (empty space, background, padding).
                                   * Point-sampled 8-bit volumes through the classified table only; the trilinear,
                                   * 16-bit and LDS-staged forms always read the atlas.  0: every brick is fetched */

#define VRC_OPT_PROJECTION 16       /* how a pixel is formed from its ray's samples: VRC_PROJECTION_COMPOSITE (default: the
                                    * reference's emission/absorption compositing with early ray termination) |
                                    * VRC_PROJECTION_MIP (maximum-intensity projection, an extension: see below) |
                                    * VRC_PROJECTION_ISO (shaded isosurface, an extension: "An isosurface frame" below;
                                    * VRC_EINVAL, naming vrc_set_isosurface, on a context that has not called it yet: such
                                    * a context accepts and refuses the values it did before the projection existed) |
                                    * VRC_PROJECTION_SLICE (the volume on a plane, an extension: "A slice frame" below;
                                    * VRC_EINVAL, naming vrc_set_slice, on a context that has not called it yet).  The
                                    * value 3 is no projection and stays refused: the slice is 4 */
#define VRC_PROJECTION_COMPOSITE 0
#define VRC_PROJECTION_MIP 1
#define VRC_PROJECTION_ISO 2
#define VRC_PROJECTION_SLICE 4
#define VRC_OPT_MIP_SKIP 17         /* 1 (default) | 0.  MIP only: a ray does not march a brick whose largest voxel cannot
                                    * beat the maximum the ray already holds (every upload notes it per slot).  The
                                    * maximum does not depend on the order or on samples that cannot raise it: the same
                                    * frame, bit for bit; only vrc_stats.samples falls.  0: every brick is marched */

#define VRC_OPT_MIP_FOLD 18         /* what a MIP frame folds a ray's samples into (read only when VRC_OPT_PROJECTION =
                                    * VRC_PROJECTION_MIP): VRC_MIP_FOLD_MAX (default: the maximum, the MIP frame below
                                    * bit for bit) | VRC_MIP_FOLD_MIN (minimum-intensity projection) | VRC_MIP_FOLD_MEAN
                                    * (mean-intensity / X-ray projection): see "The folds of a MIP frame" below.  Any
                                    * other value: VRC_EINVAL */
#define VRC_MIP_FOLD_MAX 0
#define VRC_MIP_FOLD_MIN 1
#define VRC_MIP_FOLD_MEAN 2

#define VRC_OPT_MIP_DEPTH 19        /* 0 (default) | 1.  MIP only, VRC_MIP_FOLD_MAX and _MIN: keep, beside M, the depth D of
                                    * the sample M was found at ("The depth of a MIP frame" below) for
                                    * vrc_get_projection_depths.  The frame and the values are bit for bit those of 0.
                                    * Any other value: VRC_EINVAL */
#define VRC_OPT_MIP_DEPTH_CUE 20    /* 0 (default) ... 1000: the strength of the depth cue in thousandths.  Above 0 the
                                    * frame tracks depth whatever VRC_OPT_MIP_DEPTH says, and a pixel is darkened by
                                    * where D lies in its ray's interval.  Anything else: VRC_EINVAL */

#define VRC_OPT_STREAM_MARKERS 21   /* 0 (default) | 1.  What vrc_render puts on the stream besides the march.  0: the
                                    * dispatch of a timed march that is one launch carries the second timing event as
                                    * its own stop event, which is also what an upload that recycles a slot waits for,
                                    * and the stream waits for the pool's uploads once per upload, not once per frame:
                                    * a steady-state frame is one marker (the first timing event, or the fence of a
                                    * march that is not timed) and the dispatch.  vrc_stats' times then end with the
                                    * dispatch itself, not with a marker behind it.  1: a wait for the last upload, an
                                    * event recorded before and one behind the march, and a fence recorded behind
                                    * those, every frame (what the library did before the option existed; its times
                                    * include the second marker's latency).  Frames, counts and the ordering against
                                    * uploads are the same either way */

#define VRC_OPT_RAY_CACHE 22        /* 1 (default) | 0.  What a pixel's ray set-up computes -- direction, its reciprocal,
                                    * the interval in the volume's box and the clip planes, the near plane -- depends on
                                    * the camera, the viewport and its offset, the box, the clip planes, the row bands
                                    * and the pixel buffer's size alone.  A vrc_render whose values of those equal the
                                    * ones of the vrc_render before, bit for bit, stores its rays in device memory the
                                    * context owns (40 bytes per pixel, whole 8x8 tiles), and the ones after that load
                                    * them instead of computing them: later passes of a multi-pass frame, frames
                                    * re-rendered while bricks stream in, transfer-function edits, a time series from a
                                    * fixed camera.  The loaded ray is the stored bits: the same frame and sample count.
                                    * A camera that moves every frame computes its rays as before and allocates
                                    * nothing.  The tile-scheduled grid walk of the gather kernels only (GRID_DDA and
                                    * PACKED on a grid-aligned node set): the reference-order loop, the LDS-staged,
                                    * per-ray-LOD and MIP kernels, the depth split, ray compaction and the supersampled
                                    * glRaycaster variant (jittered rays) always compute.  vrc_ctx_set_stream, a changed
                                    * vrc_set_row_map and setting this option to another value start over.  0: always
                                    * compute */
#define VRC_OPT_RAY_CACHE_USED 23   /* read-only (vrc_get_option), no synchronisation: what the last vrc_render did with
                                    * the ray cache -- 0 computed its rays, 1 computed and stored them, 2 loaded them */

#define VRC_OPT_WALK_CACHE 24       /* 1 (default) | 0 | 2.  Which bricks a ray visits, and the interval of each, depend on
                                    * the ray, the brick grid, the node list and the step size, the variant and the clip
                                    * planes -- not on the transfer function, the voxels or early ray termination.  A
                                    * view that stands still over an unchanged node list (transfer-function edits, the
                                    * frames after the last brick arrived) walks the brick grid once: frames that load
                                    * their rays (VRC_OPT_RAY_CACHE_USED = 2) first count the longest list (one small
                                    * extra launch), then record every ray's visits in device memory the context owns
                                    * (4 + 16 bytes per visit and pixel of whole 8x8 tiles, as many visits as the longest
                                    * list has), and from then on march from the lists with a kernel that has no grid
                                    * walk in it (vrc_last_kernel: vrc_k_raycast_replay<...>; vrc_stats.kernel_variant
                                    * stays VRC_KERNEL_GRID_DDA).  The march receives the same bricks, intervals and
                                    * distances in the same order: the same frame and sample count, bit for bit.  The
                                    * two extra launches are no marches: vrc_stats neither times nor counts them.  Only
                                    * the table-driven point-sampling march of 8-bit voxels (VRC_FILTER_NEAREST,
                                    * VRC_OPT_STEPPING 1, bricks with an overlap, slots of at most 248 voxels a side, an
                                    * atlas of at most 2^32 voxels) over a grid-aligned node set: every other frame
                                    * walks.  A camera that moves every frame allocates nothing and launches nothing
                                    * extra.  What starts over: anything that starts the ray cache over, a changed node
                                    * list, step size, variant or clip plane, vrc_ctx_set_stream, a changed
                                    * vrc_set_row_map, and setting this option or the budget to another value; the node
                                    * list and the constants must have been those of the vrc_render before for the count
                                    * to be taken, so passes over alternating node subsets and frames rendered while
                                    * bricks stream in launch nothing extra.  Where a visit gathers voxels the replay
                                    * gains nothing on the walk (measured 1 to 3 % slower), so at 1 the count pass also
                                    * counts the visits whose brick is not known to be uniform, and a view more than
                                    * half of whose visits are such records nothing and stays on the walk (_USED reads 0)
                                    * until a brick upload into the pool or VRC_OPT_UNIFORM_BRICKS changes that; those
                                    * two then also start a replaying view over.  VRC_WALK_CACHE_ALWAYS (2): replay
                                    * whatever the bricks hold; uploads and VRC_OPT_UNIFORM_BRICKS start nothing over.
                                    * 0: walk every frame.  Other values: VRC_EINVAL */
#define VRC_WALK_CACHE_ALWAYS 2
#define VRC_OPT_WALK_CACHE_USED 25  /* read-only (vrc_get_option), no synchronisation: what the last vrc_render did -- 0
                                    * walked; 1 walked and ran the count pass; 2 walked, the count has not arrived yet;
                                    * 3 walked and ran the record pass; 4 replayed the lists */
#define VRC_OPT_WALK_CACHE_BUDGET 26 /* bytes of device memory the lists of this context may take, default
                                    * VRC_WALK_CACHE_DEFAULT_BUDGET.  A view whose lists need more (or more than 2^32
                                    * words) stays on the walk: VRC_OPT_WALK_CACHE_USED then reads 0 (1 and 2 while the
                                    * count is taken, unless not even one visit per ray fits).  Negative: VRC_EINVAL */
#define VRC_OPT_WALK_CACHE_BYTES 27 /* read-only: bytes of device memory the context's lists hold now */
#define VRC_OPT_WALK_LEAN_USED 28   /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render replayed
                                    * lean lists (vrc_last_kernel: vrc_k_raycast_replay<...,lean>), 0 if it did anything
                                    * else.  Where the step size is a power of two, the pool has fewer than 2^20 slots
                                    * and no visit of the view takes 4096 samples or more, a visit's list entry holds
                                    * its sample count and its brick's slot index instead of the segment's length, so
                                    * the replay of a uniform brick neither fetches the node nor counts the steps again.
                                    * Same layout, same bytes, same frame and sample count; every other view records
                                    * and replays the lists as before */
#define VRC_OPT_SHADING 29          /* 0 (default): the composite frame as it is; 1: every sample's colour is lit by the
                                    * volume's gradient at the sample ("A shaded composite frame" below).  Any other
                                    * value: VRC_EINVAL.  Read only when VRC_OPT_PROJECTION = VRC_PROJECTION_COMPOSITE:
                                    * MIP and isosurface frames ignore it */
#define VRC_OPT_SHADING_AMBIENT 30  /* the ambient share of that light in thousandths, 0 ... 1000, default 250; anything
                                    * else: VRC_EINVAL.  ambient = (float)k / 1000.0f */
#define VRC_OPT_COMPOSITE_DEPTH 31  /* 0 (default): a composite frame keeps no depth; 1 ... 999: the opacity threshold in
                                    * thousandths at which every ray's depth is kept ("The depth of a composite frame"
                                    * below).  Anything else: VRC_EINVAL.  Read only when VRC_OPT_PROJECTION =
                                    * VRC_PROJECTION_COMPOSITE: MIP and isosurface frames ignore it */
#define VRC_OPT_PREINTEGRATION 32   /* 0 (default): every sample of a composite frame is classified on its own; 1: every
                                    * step is, from a table pre-integrated over the values at its two ends ("A
                                    * pre-integrated composite frame" below).  Any other value: VRC_EINVAL.  Read only
                                    * when VRC_OPT_PROJECTION = VRC_PROJECTION_COMPOSITE: MIP and isosurface frames
                                    * ignore it */
#define VRC_OPT_PREINT_BUILDS 33    /* read-only: how many times this context has built a pre-integrated table */
#define VRC_OPT_WALK_UNIFORM_ONLY 34 /* 1 (default) | 0.  A view that replays lean lists (VRC_OPT_WALK_LEAN_USED = 1) and
                                    * none of whose visits meets a brick that is not known to be uniform -- by the count
                                    * pass of those lists, and while the pool has taken no upload and VRC_OPT_UNIFORM_BRICKS
                                    * has not changed since that pass, under VRC_WALK_CACHE_ALWAYS too -- is replayed by
                                    * an instance that holds no gather march (vrc_last_kernel:
                                    * vrc_k_raycast_replay<...,uniform,lean>): fewer registers, more waves in flight.  The
                                    * same lists, the same frame and sample count, bit for bit.  Any other view, and
                                    * every view at 0, replays as before; changing the option starts nothing over.  Any
                                    * other value: VRC_EINVAL */
#define VRC_OPT_WALK_UNIFORM_ONLY_USED 35 /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render
                                    * replayed its lists with that instance, 0 if it did anything else */
#define VRC_OPT_STORE_THROUGH 36    /* 1 (default) | 0.  A replayed frame (VRC_OPT_WALK_CACHE_USED = 4) of less than 4 GiB
                                    * writes its pixels with 16-byte write-through stores: the frame streams out of
                                    * the L2 while the march runs, and the kernel ends without a frame of dirty lines
                                    * to write back.  The same frame and sample count, bit for bit; whoever reads the
                                    * pixel buffer behind the frame on the stream sees the same bytes.  Every other
                                    * frame, and every frame at 0, stores as before; changing the option starts
                                    * nothing over.  Any other value: VRC_EINVAL */
#define VRC_OPT_STORE_THROUGH_USED 37 /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render stored
                                    * its pixels that way, 0 if it did anything else */
#define VRC_OPT_FIRST_VISIT_TABLE 38 /* 1 (default) | 0.  A replayed lean frame (VRC_OPT_WALK_LEAN_USED = 1) that starts
                                    * from cleared pixels, without VRC_OPT_COUNT_SAMPLES, takes the result of a ray's
                                    * first visit, where that is a uniform brick of fewer than 256 steps, from a table
                                    * of the classified table's 256 entries by step count instead of compositing it:
                                    * the march's own composites from zero, run once per transfer function (512 KiB or
                                    * 1 MiB of device memory per context).  The table is built by the second frame in
                                    * a row that renders with one transfer function, so an edit a frame pays no
                                    * build.  The same frame, bit for bit.  Every other frame, and every frame at 0,
                                    * marches every visit; changing the option starts nothing over.  Any other value:
                                    * VRC_EINVAL */
#define VRC_OPT_FIRST_VISIT_TABLE_USED 39 /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render
                                    * handed its march the table, 0 if it did anything else */
#define VRC_OPT_LEAN_FREE_MARCH 40  /* 1 (default) | 0.  A replayed lean frame (VRC_OPT_WALK_LEAN_USED = 1) without
                                    * VRC_OPT_COUNT_SAMPLES marches a uniform visit without the early-exit test where
                                    * the visit cannot reach the exit threshold: its start opacity w, its entry's
                                    * opacity e and its step count n are non-negative with w + n e <= 0.99, decided
                                    * per ray and visit.  Every other visit keeps the tested march.  The same frame,
                                    * bit for bit.  Every other frame, and every frame at 0, marches as before;
                                    * changing the option starts nothing over.  Any other value: VRC_EINVAL */
#define VRC_OPT_LEAN_FREE_MARCH_USED 41 /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render
                                    * allowed its march that form, 0 if it did anything else */
#define VRC_OPT_WALK_RESOLVED 42    /* 1 (default) | 0.  A frame replayed by the uniform-only instance
                                    * (VRC_OPT_WALK_UNIFORM_ONLY_USED = 1) without VRC_OPT_COUNT_SAMPLES reads one word
                                    * per visit -- step count, brick value, marched or not -- resolved once from the
                                    * lists and the bricks' uniformity words, instead of a list word and a uniformity
                                    * word per visit.  The words take a fifth more of VRC_OPT_WALK_CACHE_BUDGET beside
                                    * the lists (a view whose lists fit and whose words do not replays as at 0), are
                                    * built by the first such frame and dropped when the lists, the pool's uploads or
                                    * its uniformity words change.  The same frame, bit for bit.  Every other frame,
                                    * and every frame at 0, replays as before; changing the option starts nothing
                                    * over.  Any other value: VRC_EINVAL */
#define VRC_OPT_WALK_RESOLVED_USED 43 /* read-only (vrc_get_option), no synchronisation: 1 if the last vrc_render
                                    * handed its march those words, 0 if it did anything else */
/* 512 MiB per context: a 1024 x 1024 frame of a 1024^3 volume in 128^3 bricks has lists of at most 12 visits in the
 * default view, (1 + 4 x 12) x 4 MiB = 196 MiB (19 visits, 308 MiB, rotated by 30 and 20 degrees), and 31 visits fit;
 * every renderer slot of a pipeline with frames in flight is a context of its own with a budget of its own (six slots
 * of the default view: 1176 MiB in all) */
#define VRC_WALK_CACHE_DEFAULT_BUDGET ( 512ll << 20 )

/* A MIP frame (VRC_OPT_PROJECTION = VRC_PROJECTION_MIP).
 *   Sample set.  A ray's sample set S is exactly what the composite march takes with a transfer function whose alpha
 *     is 0 everywhere: the same ray set-up, global-box and clip-plane interval and near plane; the same node list
 *     order, including the reference's quirk that a brick whose tNear lies beyond the ray's interval ends the ray
 *     (cuda/Renderer.cu:183-186); the same restart per brick, sample positions and count per segment
 *     (VRC_OPT_STEPPING 0 and 1); no early termination.
 *   Value.  M = the maximum over S of the sampled density: VRC_FILTER_NEAREST the voxel's value, in the volume's own
 *     units; VRC_FILTER_TRILINEAR the interpolated float.  A float atlas folds starting from -infinity with a maximum
 *     that keeps M over a sample that is not a number, so NaN samples, quiet or signalling, drop out (a ray whose
 *     samples are all NaN has M = -infinity: a pixel with S not empty, the classification of -infinity).
 *   Pixel, S not empty.  t = TF((M - r0) / (r1 - r0)), r = dataSourceRange, fetched as every sample's is (256 texels,
 *     linear filter, the weight in VRC_OPT_TF_FRAC_BITS bits); no opacity correction and no 255/256 clamp, as no step
 *     length is involved; stored premultiplied, (t.rgb * t.a, t.a), the frame buffer's convention.  Classified once
 *     per ray, after the march.
 *   Pixel, S empty.  Keeps its cleared value.
 *   Passes of one frame (vrc_render several times between vrc_pre_render and vrc_post_render).  The context owns one
 *     running maximum per pixel of the pixel buffer -- internal, caller-owned or row-mapped.  vrc_pre_render
 *     invalidates it, the frame's first pass does not read it, later passes take the maximum with it: after every pass
 *     the frame buffer holds the MIP of the passes so far.  Changing VRC_OPT_PROJECTION between vrc_pre_render and
 *     vrc_post_render: the next vrc_render returns VRC_EINVAL.
 *   Sample count (VRC_OPT_COUNT_SAMPLES).  vrc_stats.samples counts the samples actually taken: with VRC_OPT_MIP_SKIP
 *     = 0 that is |S| summed over the rays.
 * Served: VRC_KERNEL_AUTO, _REFERENCE_ORDER and _GRID_DDA; point samples and trilinear samples (by gathers) of the
 * 8-bit, 16-bit and float atlases, i.e. all seven voxel types (offset binary is monotone: the maximum commutes with
 * it); atlases of more than 2^32 voxels; row maps.  AUTO with the trilinear filter takes the gather form and does not
 * build the tap-packed atlas.  VRC_EINVAL from vrc_render, naming the option: an explicit VRC_KERNEL_LDS or _PACKED,
 * vrc_set_ray_lod on, VRC_VARIANT_GLRAYCASTER.  VRC_OPT_DEPTH_SPLIT and VRC_OPT_ERT_COMPACTION are silently the plain
 * kernel.  VRC_OPT_UNIFORM_BRICKS: a ray whose segment lies in a slot known to hold one value takes max(M, value) and
 * the segment's step count without fetching (point samples of 8- and 16-bit voxels; same frame and count, bit for bit). */

/* The folds of a MIP frame (VRC_OPT_MIP_FOLD).  The sample set S of a ray is the MIP frame's, exactly, whatever the fold:
 * nothing about it is new.  Served, refused (VRC_KERNEL_LDS and _PACKED, vrc_set_ray_lod, VRC_VARIANT_GLRAYCASTER) and
 * silently the plain kernel (VRC_OPT_DEPTH_SPLIT, VRC_OPT_ERT_COMPACTION) as above.  The pixel is one classification of
 * M as above; a ray with S empty keeps its cleared value.  Changing VRC_OPT_MIP_FOLD between vrc_pre_render and
 * vrc_post_render: the next vrc_render returns VRC_EINVAL and names the option, as for a changed projection.
 *   VRC_MIP_FOLD_MAX.  M = the maximum over S: the frame above.
 *   VRC_MIP_FOLD_MIN.  M = the minimum over S.  A float atlas folds starting from +infinity with a comparison that keeps
 *     M over a sample that is not a number: NaN samples drop out, and a ray whose samples are all NaN has M =
 *     +infinity.  Passes meet in the same running word per pixel.  VRC_OPT_MIP_SKIP: a ray does not march a brick whose
 *     SMALLEST stored voxel cannot lower M (every upload notes that per slot too).  VRC_OPT_UNIFORM_BRICKS: min(M,
 *     value) and the step count without fetching.  Both leave the frame bit-identical; only vrc_stats.samples falls
 *     with skipping.
 *   VRC_MIP_FOLD_MEAN.  M = (the sum of the sampled densities) / |S|, classified once.  Passes meet in a running (sum,
 *     count) per pixel of the pixel buffer, which the context owns as it owns the running maximum.  Point samples of
 *     the 8- and 16-bit atlases are summed exactly, in 64-bit integers (of the stored values: an offset-binary
 *     atlas's shift is taken off once per ray); M is that quotient formed in float64 and rounded to float32 once.
 *     Samples of the float atlas and all trilinear samples are accumulated in float64, in the order of the march; NaN
 *     and infinities propagate by IEEE rules, and a NaN mean classifies as a NaN density does (the first texel).
 *     VRC_OPT_MIP_SKIP does nothing.  VRC_OPT_UNIFORM_BRICKS: value x step count is added without fetching (point
 *     samples of 8- and 16-bit voxels; exact).  vrc_stats.samples is always |S|.
 * The running state of a pixel is read as what the current pass makes of it -- an integer for point samples of the 8- and
 * 16-bit atlases, a float (the mean: a float64 sum) for everything else -- so VRC_OPT_FILTER must not change between
 * the passes of one MIP frame, whatever the fold: the library does not check it, and the frame and the read-back values
 * are unspecified if it does.
 * vrc_get_projection_values returns M itself. */

/* The depth of a MIP frame (VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE).  Both options are read only when
 * VRC_OPT_PROJECTION = VRC_PROJECTION_MIP and the fold is VRC_MIP_FOLD_MAX or _MIN; under VRC_MIP_FOLD_MEAN they do
 * nothing: the mean has no position.  Changing either between vrc_pre_render and vrc_post_render: the next vrc_render
 * returns VRC_EINVAL and names the option, as a changed fold does.  With both at 0 a frame launches the kernel instances
 * it launched before the options existed.
 *   Depth of a sample.  The sample set S is the MIP frame's, unchanged.  Sample j (0-based, in march order) of a brick
 *     segment has t_j = tNear + (float)j * stepSize in float32, the product and the sum each rounded (no fused multiply-
 *     add); tNear is the ray parameter of the segment's first sample.  The same formula for VRC_OPT_STEPPING 0 and 1
 *     and for both filters: the depth labels the sample's index, it does not re-derive the position chain.
 *   Depth of a ray.  D = the smallest t_j over the samples of S whose value equals M.  On float atlases that is ==, so a
 *     NaN sample never qualifies; a ray whose samples are all NaN has M = -/+infinity with no sample attaining it, and
 *     D = +infinity.  Equivalently the ray's state (M, D) is folded lexicographically: a strictly better M replaces
 *     both, an equal M replaces D only by a smaller t -- between two samples inside one voxel, between the bricks of
 *     the reference-order loop (whose list order is no visibility order) and between the passes of one frame.
 *   Passes.  The context owns one running depth word per pixel beside the running M: same ownership, same invalidation
 *     by vrc_pre_render, not read by the first pass.  Later passes merge (M, D) by the rule above: after every pass the
 *     pair is that of the passes so far, whatever the split.
 *   VRC_OPT_MIP_SKIP, VRC_OPT_UNIFORM_BRICKS.  With depth on a brick is skipped only if no sample of it can reach M at
 *     all (strictly; for trilinear samples "can equal M" within the interpolation's rounding margin counts as "must be
 *     marched"), or if it cannot beat M and its tNear is not below the D the ray holds.  A uniform slot folds
 *     (value, tNear) by the lexicographic rule and adds the step count without fetching.  Frame, values and depths are
 *     bit-identical with either option on or off; only vrc_stats.samples may differ.
 *   Depth cue.  After the classification t = TF(M) the stored pixel is w * (t.rgb * t.a, t.a), w = 1 - strength * u,
 *     u = clamp((D - tNearGlobal) / (tFarGlobal - tNearGlobal), 0, 1), the interval being the ray's own (global box and
 *     clip planes), the one S is taken from; u = 0 where that interval is empty, u = 1 for D = +infinity.  Float32,
 *     operations in the order written.  Strength 0 is the uncued frame bit for bit. */

/* An isosurface frame (VRC_OPT_PROJECTION = VRC_PROJECTION_ISO; vrc_set_isosurface gives iso_value and ambient).  The
 * pixel shows the first place along its ray where the sampled density reaches iso_value, lit by the volume's gradient
 * there.  VRC_OPT_MIP_FOLD, _DEPTH and _DEPTH_CUE are not read; VRC_OPT_MIP_SKIP is.
 *   Sample set.  S is the MIP frame's, unchanged: the same rays, interval, list-order quirk, restart per brick and sample
 *     positions, for VRC_OPT_STEPPING 0 and 1.
 *   Hit.  A sample hits when its value, as vrc_get_projection_values would report it, is >= iso_value.  For point
 *     samples of the 8- and 16-bit atlases that is an integer comparison of the stored voxel against one threshold formed
 *     once per frame: the ceiling of iso_value plus the offset-binary shift, clamped to the type (and one above the
 *     type's largest value where iso_value lies above it: no voxel hits).  It is exact.  On float atlases and for
 *     trilinear samples it is >= in float32 (for trilinear samples of an offset-binary atlas: against the smallest
 *     stored float whose reported value is >= iso_value, which is the same set), so a NaN sample never hits.
 *   Ray.  D = the smallest t_j = tNear + (float)j * stepSize ("The depth of a MIP frame") over the hitting samples, V
 *     that sample's value.  Two hitting samples with bit-equal t keep the larger V; if V is equal too, either gradient
 *     may stand.  (D, V) is the same whatever the brick loop and however the node list is split into passes, in any
 *     order.  A ray that takes no hitting sample has D = +infinity and its pixel keeps its cleared value.
 *   Gradient.  (x, y, z) = the slot-local voxel the hit sample was read from; for a trilinear sample the voxel the point
 *     sampler addresses at that position, the floor of the brick's voxel coordinate.  g_a = v(a+1) - v(a-1) along each
 *     axis, of stored voxels, indices clamped to the slot (slotDim - 1, as the clamped sampler clamps).  Integer voxels
 *     are differenced in integers (exact; the offset-binary shift cancels), a float atlas in float32 (a NaN tap gives a
 *     NaN component).  G_a = (float)g_a * voxPerWorld_a of the brick's node, one rounded multiply: a world-space
 *     gradient, right across LOD cuts and anisotropic voxels.  The six gathers happen once per ray and pass, after the
 *     march, only for a ray whose D this pass lowered, in that pass's nodes and atlas.
 *   Pixel.  c = TF((iso_value - r0) / (r1 - r0)), fetched as a MIP pixel's is; s = ambient + (1 - ambient) *
 *     |G.dir| / |G|, two-sided, a headlight; s = 1 where |G| is 0 or not finite.  Float32, operations in the order
 *     written (the sums of three left to right), nothing fused.  The stored pixel is (c.rgb * c.a * s, c.a).
 *   Passes.  The context keeps V, D and G per pixel of the pixel buffer, owned and invalidated as the running maximum
 *     and depth of a MIP frame are.  Changing iso_value, ambient or VRC_OPT_PROJECTION between vrc_pre_render and
 *     vrc_post_render: the next vrc_render returns VRC_EINVAL, as a changed fold does.  A vrc_render under
 *     VRC_PROJECTION_ISO before the first vrc_set_isosurface: VRC_EINVAL, naming the function -- and so is the
 *     vrc_set_option that would select the projection on such a context, so that no render gets that far.
 *   Read-backs, valid from the frame's first ISO pass until the next vrc_pre_render.  vrc_get_projection_values: V,
 *     with count 1 where the ray hit and 0 elsewhere.  vrc_get_projection_depths: D and origin + D * dir; depth is
 *     always tracked.  vrc_get_projection_gradients: G, 0 where there is no hit.
 *   VRC_OPT_MIP_SKIP, a run-time value of the same kernel instance.  1: a ray does not march a brick whose slot cannot
 *     reach the threshold (every upload notes the slot's largest voxel; trilinear samples with the interpolation's
 *     rounding margin), nor one whose tNear lies strictly above the D it holds -- the grid walk, which meets bricks by
 *     increasing tNear, ends the ray there (once tNear clears D by the walk's own tie tolerance) -- and it leaves a
 *     segment in front of the first group of samples whose t lies strictly above D.  0: every sample of S is taken, and
 *     vrc_stats.samples is |S| summed over the rays.  Frame, V, D and G are bit-identical either way.
 *   VRC_OPT_UNIFORM_BRICKS.  A slot known to hold one value hits at its segment's first sample or not at all, without
 *     fetching (point samples of 8- and 16-bit voxels); its gradient is 0.  Bit-identical on and off, counts included.
 * Served and refused exactly as a MIP frame: all seven voxel types, both filters (trilinear by gathers), AUTO /
 * REFERENCE_ORDER / GRID_DDA, atlases of more than 2^32 voxels, row maps, caller-owned frame buffers; VRC_EINVAL naming
 * the option for an explicit VRC_KERNEL_LDS or _PACKED, vrc_set_ray_lod on and VRC_VARIANT_GLRAYCASTER;
 * VRC_OPT_DEPTH_SPLIT and VRC_OPT_ERT_COMPACTION are silently the plain kernel.  A depth cue, a "<=" surface, smooth
 * (trilinear) gradients and several isovalues are not part of it. */

/* A slice frame (VRC_OPT_PROJECTION = VRC_PROJECTION_SLICE; vrc_set_slice gives the plane).  The pixel shows the volume
 * where its ray meets one plane -- an axial, coronal, sagittal or oblique cut -- classified by the transfer function, with
 * the value and the position under every pixel to read back.  One sample per ray, at a given ray parameter and not on the
 * ray's sample lattice.  VRC_PROJECTION_SLICE is 4: the value 3 is no projection and stays VRC_EINVAL.
 *   Plane.  (nx, ny, nz, d) in the clip planes' convention: n.x + d = 0; n need not be a unit vector.
 *   Ray.  The pixel's ray, its interval [tNearGlobal, tFarGlobal] (global box and clip planes) and tNearPlane are the
 *     composite frame's, unchanged.  rn = dot(dir, n) and t_p = -(dot(n, origin) + d) / rn in float32, formed in the order
 *     the clip planes form theirs.  The pixel takes its one sample if and only if the ray hits the box, rn != 0 and
 *     max(tNearGlobal, tNearPlane) <= t_p <= tFarGlobal.  There is no VRC_EPSILON in place of rn == 0: a ray that lies in
 *     the plane takes no sample.
 *   Position.  P = origin + dir * t_p, every product and sum rounded, nothing fused.
 *   Brick.  The sample is read from a node of this pass's list whose box contains P, faces included.  The list-order
 *     quirk of the reference loop (a brick with tNear > tFarGlobal ends the ray) is NOT applied: every node is a candidate.
 *     Containment is decided on the ray: t_p lies in the node's interval of the slab test, widened by 2e-6 max(1, |t_p|)
 *     -- a few units in the last place of t_p -- so that a P inside the union of the list's boxes never goes unsampled
 *     because rounding opened a gap between two neighbours.  Where P lies on, or within that rounding of, a face shared
 *     by several nodes, the sample comes from any one of them.  If no node of this pass contains P, the pixel is left to
 *     a later pass.
 *   Sample.  l_a = (P_a - aabbMin_a) * voxPerWorld_a + localOrigin_a, product and sum each rounded, always clamped to
 *     [0, slotDim_a - 1]: one sample per pixel has no un-clamped instance.  VRC_FILTER_NEAREST: the voxel trunc(l).
 *     VRC_FILTER_TRILINEAR: the eight taps and weights of the trilinear gather march at l (texel centres at i + 0.5, taps
 *     clamped to the slot), interpolated x, then y, then z.  V is the value as vrc_get_projection_values reports a MIP
 *     sample: the volume's own units, signed types un-shifted.
 *   Pixel.  A sampled pixel is classified exactly as a MIP pixel is: TF((V - r0) / (r1 - r0)), no opacity correction,
 *     stored (t.rgb * t.a, t.a); a NaN classifies as a NaN density does.  An unsampled pixel keeps its cleared value.
 *   Passes.  The context keeps (V, D = t_p) per pixel of the pixel buffer, in the running words of a MIP frame with depth:
 *     same ownership, same invalidation by vrc_pre_render, not read by the first pass.  A later pass sets only a pixel
 *     whose D is still +infinity.  Changing the plane or VRC_OPT_PROJECTION between vrc_pre_render and vrc_post_render:
 *     the next vrc_render returns VRC_EINVAL (the plane is latched at the frame's first slice pass).  A vrc_render under
 *     VRC_PROJECTION_SLICE before the first vrc_set_slice: VRC_EINVAL, naming the function -- and so is the vrc_set_option
 *     that would select the projection on such a context.
 *   Read-backs, valid from the frame's first slice pass until the next vrc_pre_render.  vrc_get_projection_values: V,
 *     count 1 where the pixel is sampled, else 0.  vrc_get_projection_depths: D and origin + D * dir; depth is always
 *     tracked.  vrc_get_projection_gradients: VRC_EINVAL, as after any frame that is no isosurface frame.
 *   vrc_stats.samples (VRC_OPT_COUNT_SAMPLES): the pixels this pass sampled.
 *   VRC_OPT_UNIFORM_BRICKS.  A slot known to hold one value yields that value without a gather (point samples of 8- and
 *     16-bit voxels).  Frame, V, D and counts are bit-identical with the option on or off.
 * Served: VRC_KERNEL_AUTO, _REFERENCE_ORDER (the nodes its tile culling leaves, the first that contains P) and _GRID_DDA
 * (the cell of P looked up in the brick grid, no walk; the neighbouring cells where rounding put P across a cell face);
 * all seven voxel types, both filters; atlases of more than 2^32 voxels; row maps, caller-owned frame buffers, frames of
 * several passes; VRC_OPT_RAY_CACHE on the grid form (a still view of slice frames loads its rays; to the frames of another
 * projection a slice frame is what a MIP frame is: the rays kept for them are forgotten, and kept again as ever).  Refused
 * as a MIP frame is, VRC_EINVAL
 * naming the option: an explicit VRC_KERNEL_LDS or _PACKED, vrc_set_ray_lod on, VRC_VARIANT_GLRAYCASTER.  Not read:
 * VRC_OPT_MIP_*, VRC_OPT_SHADING, VRC_OPT_COMPOSITE_DEPTH, VRC_OPT_PREINTEGRATION, samplesPerRay and VRC_OPT_STEPPING.
 * Silently the plain slice kernel: VRC_OPT_DEPTH_SPLIT, VRC_OPT_ERT_COMPACTION and VRC_OPT_WALK_CACHE (as a MIP frame: not
 * replayed, VRC_OPT_WALK_CACHE_USED reads 0, nothing is allocated).  With another projection every frame launches the
 * kernel instances it launched before the projection existed, and no memory is allocated for it.
 * Not part of it: thick slabs (a MIP or mean frame between two clip planes is one, quantised to the sample lattice),
 * curved reformats, an opaque or window / level mode that bypasses the transfer function's alpha, a depth cue, gradients
 * at the slice, several planes per frame, per-ray LOD and the LDS / packed forms. */

/* A shaded composite frame (VRC_OPT_PROJECTION = VRC_PROJECTION_COMPOSITE, VRC_OPT_SHADING = 1).  The composite frame
 * with one change: the colour a sample adds is multiplied by a headlight term; its opacity is not.
 *   Samples.  Ray set-up, intervals, node order and its quirks, the restart per brick and the sample positions
 *     (VRC_OPT_STEPPING 0 and 1) are the composite frame's; so is the classification (the classified table for point
 *     samples of 8-bit voxels, the transfer function and the opacity correction per sample otherwise), the 255/256 clamp,
 *     the accumulation across passes and early ray termination at 0.999, which looks at alpha only.
 *   Sample.  With e = (rgb * alpha', alpha') as the unshaded march has it, the shaded march composites (e.rgb * s,
 *     e.alpha'), s = ambient + (1 - ambient) * |G.dir| / |G|: two-sided, dir the ray's unit direction, s = 1 where |G| is 0
 *     or not finite; float32, the operations in the order of an isosurface pixel's s, nothing fused.
 *   Gradient.  G is the isosurface frame's ("An isosurface frame", Gradient), taken at the voxel the POINT sampler
 *     addresses at the sample's position, under both filters: central differences of the stored voxels around it, indices
 *     clamped to the slot, integer atlases differenced in integers (offset binary cancels) and float atlases in float32,
 *     times the node's voxels per world unit.  Interpolated gradients are not part of it.
 *   What follows, bit for bit, against the same context, pool and options with VRC_OPT_SHADING = 0 marched by gathers
 *     (VRC_KERNEL_REFERENCE_ORDER or _GRID_DDA; AUTO with point samples): the alpha channel and vrc_stats.samples are
 *     equal; with VRC_OPT_SHADING_AMBIENT = 1000 the whole frame is; a brick all of whose voxels are equal (mem://)
 *     contributes what it did, with VRC_OPT_UNIFORM_BRICKS 1 (its slot is marched from one table entry, no gathers)
 *     and 0 (the gradients are gathered and are zero).  A sample whose alpha' is 0 adds nothing whatever s is: its six
 *     neighbour voxels are not fetched.  With the option at 0 every frame launches the kernel instances it launched
 *     before the option existed.
 * Served: VRC_KERNEL_AUTO, _REFERENCE_ORDER and _GRID_DDA; both filters (trilinear by gathers: AUTO does not take the
 * LDS-staged form and does not build the tap-packed atlas for a shaded frame); all seven voxel types; atlases of more than
 * 2^32 voxels; the clamped sampler (overlap 0); row maps, caller-owned frame buffers, frames of several passes;
 * VRC_OPT_COUNT_SAMPLES; VRC_OPT_RAY_CACHE as before.  Silently the plain shaded kernel: VRC_OPT_DEPTH_SPLIT,
 * VRC_OPT_ERT_COMPACTION, VRC_OPT_GREY_TABLE (the four-float form, the same frame) and VRC_OPT_WALK_CACHE (a shaded frame
 * is not replayed: VRC_OPT_WALK_CACHE_USED reads 0, nothing is allocated, and the lists an unshaded view recorded are
 * forgotten, to be recorded again when that view returns).  VRC_EINVAL from vrc_render, naming the option: an explicit
 * VRC_KERNEL_LDS or _PACKED, vrc_set_ray_lod on, VRC_VARIANT_GLRAYCASTER, and either shading option changed between
 * vrc_pre_render and vrc_post_render.  Specular terms, movable lights and picking are not part of it. */

/* The depth of a composite frame (VRC_OPT_PROJECTION = VRC_PROJECTION_COMPOSITE, VRC_OPT_COMPOSITE_DEPTH = k, 1 ... 999).
 * The composite frame as it is, and beside it, per pixel, where the ray's accumulated opacity first reaches a threshold:
 * what a click on the picture picks, and a depth image to combine the frame with.  tau = (float)k / 1000.0f, one rounded
 * division; 999 gives exactly the early-exit threshold 0.999f, so a ray that terminates early has crossed.
 *   Frame.  The frame and vrc_stats.samples are those of the same context, pool and options with the option at 0 marched
 *     by gathers (VRC_KERNEL_REFERENCE_ORDER or _GRID_DDA; AUTO with point samples), bit for bit, all four channels.
 *   Depth of a ray.  Take the samples in the order the march composites them (under the reference-order loop: list
 *     order, which is no visibility order).  A_i is the float32 alpha the ray holds after compositing sample i.  The
 *     crossing sample is the first with A_i >= tau.  D = t_j = tNear + (float)j * stepSize of that sample ("The depth of
 *     a MIP frame", Depth of a sample, unchanged: the same formula for both steppings and both filters).  V is that
 *     sample's value as vrc_get_projection_values reports a MIP sample: for a point sample the voxel in the volume's own
 *     units, signed types un-shifted; for a trilinear sample the interpolated float.  A ray that never reaches tau has
 *     D = +infinity and count 0; its pixel is what it would have been anyway.
 *   Passes.  The context owns (D, V) per pixel of the pixel buffer, as it owns a MIP frame's running pair; vrc_pre_render
 *     invalidates it and the frame's first pass does not read it.  A later pass sets the pair only of a pixel whose D is
 *     still +infinity; its alpha comes in from the pixel buffer, as the composite's does.  After every pass of a frame
 *     that started from a cleared buffer: isfinite(D) if and only if the pixel's alpha >= tau.  Changing the option
 *     between vrc_pre_render and vrc_post_render: the next vrc_render returns VRC_EINVAL and names the option.
 *   Read-backs, valid from the frame's first such pass until the next vrc_pre_render.  vrc_get_projection_values: V, and
 *     count 1 where the ray crossed, 0 elsewhere.  vrc_get_projection_depths: D and origin + D * dir.  With the option at
 *     0 both refuse a composite frame as they did.
 *   VRC_OPT_UNIFORM_BRICKS.  A slot known to hold one value is marched from its table entry without fetching (point
 *     samples of 8-bit voxels); D, V, the frame and the counts are bit-identical with the option on or off.
 * Served: VRC_KERNEL_AUTO, _REFERENCE_ORDER and _GRID_DDA; all seven voxel types; both filters (trilinear by gathers: AUTO
 * takes neither the LDS-staged form nor the tap-packed atlas); the clamped sampler; atlases of more than 2^32 voxels; row
 * maps; caller-owned frame buffers; VRC_OPT_COUNT_SAMPLES; VRC_OPT_RAY_CACHE as before.  Silently the plain depth-tracking
 * kernel: VRC_OPT_DEPTH_SPLIT, VRC_OPT_ERT_COMPACTION, VRC_OPT_GREY_TABLE (the four-float form, the same frame) and
 * VRC_OPT_WALK_CACHE (exactly as a shaded frame: not replayed, VRC_OPT_WALK_CACHE_USED reads 0, nothing is allocated,
 * recorded lists are forgotten).  VRC_EINVAL from vrc_render, naming the option: an explicit VRC_KERNEL_LDS or _PACKED,
 * vrc_set_ray_lod on, VRC_VARIANT_GLRAYCASTER, and VRC_OPT_SHADING = 1 together with this option (alpha does not depend
 * on shading: an application that picks in a shaded picture renders the unshaded frame once).  With the option at 0 every
 * frame launches the kernel instances it launched before the option existed.  A depth cue on the composite, shading and
 * depth in one frame, replay from the walk cache, the LDS, packed and per-ray-LOD forms, gradients at the crossing,
 * several thresholds per frame and depth buffers coming in are not part of it. */

/* A pre-integrated composite frame (VRC_OPT_PROJECTION = VRC_PROJECTION_COMPOSITE, VRC_OPT_PREINTEGRATION = 1).
 * The composite frame classifies every sample on its own and so steps over whatever the transfer function does between
 * the values of two consecutive samples; this frame classifies the step: what sample j adds is looked up by the values at
 * both ends of the step that ends in it.
 *   Samples.  Ray set-up, intervals, node order with its quirks, the restart per brick, the sample positions under both
 *     VRC_OPT_STEPPING values, accumulation across passes and early termination at 0.999 on alpha are the composite
 *     frame's, unchanged.  Only what a sample contributes changes.
 *   Pairing.  A brick visit takes samples j = 0 ... n-1 with values d_0 ... d_{n-1}: for a point sample the stored voxel,
 *     for a trilinear sample the interpolated float.  Sample j >= 1 composites E(d_{j-1}, d_j); sample 0 of every visit
 *     composites E(d_0, d_0).  The previous value is NOT carried from one brick visit to the next: every visit stays a
 *     function of its own brick and interval, so that frames split into passes, the reference-order loop, row maps and
 *     a later replay stay consistent with one another; a visit of one sample falls back to the plain classification.
 *   The step's entry.  TF(x) is the 256-texel transfer function read at clamp(x, 0, 255) by exact linear interpolation
 *     between texels floor and floor + 1 (the weight quantisation of VRC_OPT_TF_FRAC_BITS is not applied).
 *     a(x) = min(TF_alpha(x), 255/256), tau(x) = -ln(1 - a(x)), k = maxSamplesPerRay / samplesPerRay, and
 *     x(d) = (d - r0) / (r1 - r0) * 256 - 0.5 the coordinate the plain classification uses (the range moved for signed
 *     pools as there).  For xf != xb, over [xf, xb]:
 *       taubar = int tau dx / (xb - xf),  alpha = 1 - exp(-k taubar),  cbar = int tau TF_rgb dx / int tau dx,
 *       E = (cbar alpha, alpha), and E = 0 where int tau dx = 0.
 *     E is symmetric in its two arguments.  Its opacity is exact for a value that changes linearly across the step; its
 *     colour is the extinction-weighted mean, self-attenuation inside the step ignored.  For xf = xb, E is the plain
 *     classification of that value.
 *   Two tables, 256 x 256 vrc_f4 (1 MiB) in float32, built on the GPU in float64 by one builder; every entry but a
 *     copied diagonal is within 1e-6 of the mathematical value per channel.
 *     Value-indexed (kind 0), for point samples of 8-bit voxels: P[u][v] = E(x(u), x(v)) for stored bytes u, v, indexed
 *       exactly; the diagonal P[v][v] is a copy of the classified table's entry for v, bit for bit, VRC_OPT_TF_FRAC_BITS
 *       included.
 *     Texel-indexed (kind 1), for 16-bit, 32-bit and float voxels and the trilinear filter: T[i][j] = E(i, j) for texel
 *       centres i, j; T[i][i] is the plain classification at x = i with exact float weights.  A sample reads it
 *       bilinearly at (xf, xb) = (clamp(x(d_{j-1}), 0, 255), clamp(x(d_j), 0, 255)), x in float32 (a NaN reads 0): with
 *       i0 = floor(xf), i1 = min(i0 + 1, 255), wf = xf - i0 and j0, j1, wb the same of xb, in float32 (each sum of two
 *       products may be one product and one fused multiply-add),
 *         E = (1 - wb) * ((1 - wf) * T[i0][j0] + wf * T[i1][j0]) + wb * ((1 - wf) * T[i0][j1] + wf * T[i1][j1]).
 *       (Sample 0 of a visit reads it at (x, x): the plain classification at a texel centre, its bilinear blend between.)
 *     A table is rebuilt only when the transfer function, the range, k, VRC_OPT_TF_FRAC_BITS or the kind the frame needs
 *     changed; it is allocated by the first frame that needs it and freed with the context.  VRC_OPT_PREINT_BUILDS
 *     counts the builds.  vrc_get_preintegrated_table reads the last frame's table back.
 *   VRC_OPT_UNIFORM_BRICKS.  A slot known to hold one value v is marched from the classified table's entry for v as it
 *     is in the plain frame; the diagonal being a copy, frame and counts are bit-identical with the option on or off
 *     (point samples of 8-bit voxels).
 * Served: VRC_KERNEL_AUTO, _REFERENCE_ORDER and _GRID_DDA; all seven voxel types; both filters (trilinear by gathers: AUTO
 * takes neither the LDS-staged form nor the tap-packed atlas); the clamped sampler; atlases of more than 2^32 voxels; row
 * maps; caller-owned frame buffers; frames of several passes; VRC_OPT_COUNT_SAMPLES; VRC_OPT_RAY_CACHE as before.
 * Silently the plain pre-integrated kernel: VRC_OPT_DEPTH_SPLIT, VRC_OPT_ERT_COMPACTION, VRC_OPT_GREY_TABLE (the
 * four-float form) and VRC_OPT_WALK_CACHE (exactly as a shaded frame: not replayed, VRC_OPT_WALK_CACHE_USED reads 0,
 * nothing is allocated, recorded lists are forgotten).  VRC_EINVAL from vrc_render, naming the option: an explicit
 * VRC_KERNEL_LDS or _PACKED, vrc_set_ray_lod on, VRC_VARIANT_GLRAYCASTER, VRC_OPT_SHADING = 1 or VRC_OPT_COMPOSITE_DEPTH
 * above 0 together with this option, and the option changed between vrc_pre_render and vrc_post_render.  With the option
 * at 0 every frame launches the kernel instances it launched before the option existed, and no table memory is
 * allocated.  Carrying the value across visits, self-attenuated colour, a grey two-float table, combination with
 * shading or depth, replay from the walk cache, the LDS, packed and per-ray-LOD forms and a table finer than 256 x 256
 * are not part of it. */

#define VRC_VARIANT_CUDARAYCASTER 0 /* renderers/cudaRaycaster/cuda/Renderer.cu:95-230 */
#define VRC_VARIANT_GLRAYCASTER 1   /* renderers/glRaycaster/shaders/fragRaycast.glsl:113-215: pixel centre
                                     * +0.5, hit test t0 <= t1, first sample of a brick snapped to the
                                     * global step lattice, clip planes per brick after the snap (the
                                     * RGBA8 transfer function of GLRaycastRenderer.cpp:188-192 is the
                                     * caller's: pass the quantised table to vrc_update) */

#define VRC_FILTER_NEAREST 0   /* cuda/TexturePool.cu:167 (cudaFilterModePoint): the reference */
#define VRC_FILTER_TRILINEAR 1 /* extension: texel centres at i+0.5, float weights, transfer function
                                * and opacity correction evaluated per sample on the interpolated density.
                                * Voxel i of a brick (overlap border included) has its centre at i + 0.5 in the
                                * brick's voxel coordinate, overlap + (pos - boxMin) / boxSize * blockSize; a tap
                                * outside the brick and its border (only with overlap 0) is clamped to the nearest
                                * voxel, as the point sampler's address is (tests/ref64.py restates this) */

#define VRC_KERNEL_AUTO 0            /* bricks of one size: GRID_DDA (meets them in the reference's order, sample for
                                      * sample); bricks of mixed sizes (an LOD cut): REFERENCE_ORDER up to
                                      * VRC_REFERENCE_ORDER_MAX_NODES bricks -- the reference composites in the host's
                                      * centre-distance order, which is not a visibility order for every ray once
                                      * brick sizes differ (cuda/Renderer.cu:172-199) -- above that GRID_DDA */
#define VRC_REFERENCE_ORDER_MAX_NODES 4096
#define VRC_KERNEL_REFERENCE_ORDER 1 /* O(nodes) loop per ray in host order, cuda/Renderer.cu:172-227 */
#define VRC_KERNEL_GRID_DDA 2        /* 3-D DDA over the brick grid; needs a grid-aligned node set */
#define VRC_KERNEL_LDS 3             /* grid DDA + voxels staged through LDS per wave and round (needs
                                      * overlap >= 1); what AUTO picks for the trilinear filter where the
                                      * tap-packed atlas (VRC_KERNEL_PACKED) is not available */
#define VRC_KERNEL_PACKED 5          /* the trilinear filter through the pool's tap-packed atlas: a second atlas, 2.25 times
                                      * the bytes, whose texel at (x,y,z) holds a voxel and its neighbour along z,
                                      * v[x,y,z] | v[x,y,z+1] << 8 (16-bit voxels: << 16), laid out so that the texels at
                                      * x and x + 1 are always neighbours in memory; allocated and filled on first use
                                      * and kept up to date by every later upload: the eight taps of a sample are TWO
                                      * gathers (rows y and y + 1; 4 bytes each, 8 for 16-bit voxels).  Needs
                                      * VRC_FILTER_TRILINEAR, 8- or 16-bit bricks with overlap >= 1 in slots of at
                                      * most 248 voxels a side, VRC_OPT_TF_FRAC_BITS = 8, VRC_OPT_STEPPING = 1
                                      * (VRC_EINVAL otherwise) and the device memory (VRC_ENOMEM).  Same sample
                                      * positions, weights and arithmetic as the LDS-staged form: the same frame,
                                      * bit for bit.  What AUTO picks for the trilinear filter where all of this
                                      * holds (VRC_OPT_PACKED_ATLAS) */
#define VRC_KERNEL_RAY_LOD 4         /* reported by vrc_get_stats when vrc_set_ray_lod is on; not selectable.  Under
                                      * per-ray LOD VRC_OPT_KERNEL chooses how the hierarchy walk takes its samples:
                                      * AUTO = for the trilinear filter the tap-packed atlas where VRC_KERNEL_PACKED
                                      * applies, else staged through LDS (8- or 16-bit bricks, overlap >= 1,
                                      * VRC_OPT_TF_FRAC_BITS 8), by gathers otherwise; GRID_DDA = gathers; LDS = staged or
                                      * VRC_EINVAL; PACKED = the packed atlas or VRC_EINVAL; vrc_last_kernel names the
                                      * instance that ran */

/* ---- context ---------------------------------------------------------------------------- */
/* cuda::Renderer::Renderer() (cuda/Renderer.cu:234-238); device is explicit (fixes Q11) */
int vrc_ctx_create( int device, vrc_ctx** out );
void vrc_ctx_destroy( vrc_ctx* ctx );
/* launch on a caller-owned hipStream_t (pass the handle as void*); NULL = the ctx's own stream */
int vrc_ctx_set_stream( vrc_ctx* ctx, void* hip_stream );
int vrc_set_option( vrc_ctx* ctx, int option, int64_t value );
int vrc_get_option( vrc_ctx* ctx, int option, int64_t* value );
/* EXTENSION (BASELINE C5): per-ray adaptive LOD.  The reference selects the LOD per brick on the host
 * (livre/core/render/SelectVisibles.cpp:52-68: a brick is fine enough when
 * worldSpacePerVoxel / worldSpacePerPixel * near / (near + distance) <= screenSpaceError at the
 * point of its box nearest to the near plane).  With this on, the node list of vrc_render is a
 * hierarchy of resident bricks (a cut of the octree plus any of its ancestors): boxes of different
 * levels nest; every level is a regular grid of bricks anchored at the min corner of all boxes
 * (border bricks may be smaller, levels need not align with each other: UVF trees), one brick per
 * cell at most; else VRC_EHIERARCHY.  Every ray applies the criterion where it enters a brick: it
 * samples the coarsest level that is fine enough there (else the next coarser one present, else
 * the next finer), with step and opacity exponent scaled by 2^level.  world_space_per_pixel =
 * (frustum.top - frustum.bottom) / window height, as in SelectVisibles.cpp:57.  cudaRaycaster
 * variant only. */
int vrc_set_ray_lod( vrc_ctx* ctx, int enable, float screen_space_error, float world_space_per_pixel );

/* ---- texture pool (brick atlas) ----------------------------------------------------------- */
/* cuda::TexturePool::TexturePool (cuda/TexturePool.cu:101-173).  max_block is the slot size
 * in voxels (block + 2*overlap), max_bytes the atlas budget.  Slot grid and free-list order
 * follow TexturePool.cu:128-144 with VRC_MAX_TEXTURE_3D standing in for maxTexture3D. */
/* vrc_pool_create makes pools of unsigned 8- and 16-bit single-component voxels and returns VRC_EUNSUPPORTED for every
 * other combination; signed, 32-bit and float voxels have vrc_pool_create_typed below. */
#define VRC_MAX_TEXTURE_3D 4096
int vrc_pool_create( vrc_ctx* ctx, size_t bytes_per_voxel, int is_signed, int is_float,
                     size_t n_components, const uint32_t max_block[3], size_t max_bytes,
                     vrc_pool** out );
/* EXTENSION: a pool by voxel type, single component (the reference's GL raycaster samples usampler3D / isampler3D /
 * sampler3D and applies the real dataSourceRange, renderers/glRaycaster/shaders/fragRaycast.glsl:197-203; its CUDA
 * kernel fetches unsigned char only).  vrc_pool_copy_to_slot[_device] takes bricks of that type, everything else is as
 * for vrc_pool_create; VRC_VOXEL_UINT8 / _UINT16 give exactly the pool vrc_pool_create gives.  An unknown type:
 * VRC_EINVAL.  vrc_render_data::dataSourceRange is in the volume's own values for every type.
 *   INT8 / INT16    stored offset-binary (the upload flips the sign bit, v + 128 / + 32768 as an unsigned number, and
 *                   vrc_render moves dataSourceRange by the same amount): every kernel form of the unsigned 8- and
 *                   16-bit pools serves them -- the same frame, bit for bit, as the unsigned pool of v + 128 / + 32768
 *                   with the moved range.  vrc_pool_read_region returns the signed values.
 *   FLOAT32         a float atlas, bricks copied as they are.
 *   UINT32 / INT32  the same float atlas: the upload converts every voxel to float32, round to nearest even, once
 *                   (the conversion GLSL applies per sample).  vrc_pool_read_region returns what the atlas holds:
 *                   float32.
 * The float atlas is point-sampled (classified per sample, as 16-bit voxels are) or filtered trilinearly by the gather
 * kernels: VRC_KERNEL_AUTO, _REFERENCE_ORDER, _GRID_DDA, per-ray LOD by gathers; an explicit VRC_KERNEL_LDS or _PACKED
 * is VRC_EINVAL, also under vrc_set_ray_lod, and VRC_OPT_UNIFORM_BRICKS does not apply.  Voxels that are not finite are
 * not inspected by the upload; a NaN density classifies as the first texel of the transfer function (the clamp of the
 * texel coordinate drops it), +-infinity as the last / first.  Under VRC_FILTER_TRILINEAR a sample with a tap that is
 * NaN has a NaN density; what a sample with an infinite tap comes out as (inf * 0, inf - inf) is unspecified.
 * vrc_pool_histogram, vrc_pool_enable_histograms and vrc_frame_histogram return VRC_EUNSUPPORTED for the five types
 * vrc_pool_create does not make. */
#define VRC_VOXEL_UINT8 0
#define VRC_VOXEL_UINT16 1
#define VRC_VOXEL_UINT32 2
#define VRC_VOXEL_INT8 3
#define VRC_VOXEL_INT16 4
#define VRC_VOXEL_INT32 5
#define VRC_VOXEL_FLOAT32 6
int vrc_pool_create_typed( vrc_ctx* ctx, int voxel_type, const uint32_t max_block[3], size_t max_bytes,
                           vrc_pool** out );
int vrc_pool_voxel_type( const vrc_pool* pool, int* voxel_type );
void vrc_pool_destroy( vrc_pool* pool );
/* cuda::TexturePool::copyToSlot (cuda/TexturePool.cu:175-203): host brick of size[] voxels,
 * tightly packed, x fastest.  Writes the normalized slot origin; on a full pool returns
 * VRC_EFULL and writes (-1,-1,-1).  The host pointer is only borrowed for the call. */
int vrc_pool_copy_to_slot( vrc_pool* pool, const void* host_brick, const uint32_t size[3],
                           float slot_out[3] );
/* same, but the brick already lives in device memory (row-major, tightly packed) */
int vrc_pool_copy_to_slot_device( vrc_pool* pool, const void* device_brick,
                                  const uint32_t size[3], float slot_out[3] );
/* cuda::TexturePool::releaseSlot (cuda/TexturePool.cu:210-214) */
int vrc_pool_release_slot( vrc_pool* pool, const float slot[3] );
/* getSlotMemSize / getTextureSize / getTextureMem (cuda/TexturePool.cuh:80-95) + free count */
int vrc_pool_info( const vrc_pool* pool, size_t* slot_bytes, uint32_t atlas_dim[3],
                   size_t* atlas_bytes, uint32_t slots[3], uint32_t* free_slots );
/* block until every pending upload of the pool has landed in HBM */
int vrc_pool_synchronize( vrc_pool* pool );
/* debug/test: read back the voxel at logical atlas coordinate (x,y,z) region into host memory,
 * row-major; used by the parity tests to check the atlas layout transform.  Voxels come back in the pool's type,
 * except from a pool of 32-bit integers: float32, what its atlas holds (vrc_pool_create_typed) */
int vrc_pool_read_region( vrc_pool* pool, const uint32_t origin[3], const uint32_t size[3],
                          void* host_out );

/* Histogram of a resident brick as a side kernel (the reference bins the CPU copy,
 * livre/lib/cache/HistogramObject.cpp:36-119): voxels [origin, origin+size) of the slot in
 * slot-local coordinates (origin = overlap, size = the node's voxel box: the interior, :94-97);
 * integral voxels are binned over the type's range, bin = v / (range / bin_count) (:104-110);
 * every voxel adds scale_factor (8^(depth-1-level), :158-162).  bin_count must divide the range
 * (256 for uint8, 1024 for uint16 in the reference, :167-176).  Synchronous; host_bins receives
 * bin_count values. */
int vrc_pool_histogram( vrc_pool* pool, const float slot[3], const uint32_t origin[3],
                        const uint32_t size[3], uint32_t bin_count, uint64_t scale_factor,
                        uint64_t* host_bins );
/* Per-slot histograms kept by the pool (the reference's HistogramCache, livre/lib/cache/HistogramObject.cpp:134-205,
 * here binned on the GPU when a brick lands).  bin_count > 0 turns them on: a device table of bin_count uint32 counts
 * per slot; the slots resident now are binned by one launch, every later vrc_pool_copy_to_slot[_device] bins its
 * brick's interior [overlap, size - overlap) on the upload stream behind its repack, and vrc_pool_release_slot
 * invalidates the slot's row.  bin_count must divide the voxel type's range (256 for uint8, 1024 for uint16 in the
 * reference, :164-176; at most 4096).  bin_count = 0 turns them off and frees the table (waits for the device).  Off by
 * default: without this call nothing is allocated or launched. */
int vrc_pool_enable_histograms( vrc_pool* pool, uint32_t bin_count, const uint32_t overlap[3] );
/* Frame histogram on ctx's stream: sum over the n nodes of row(slots[i]) * scales[i] (scale 8^(depth-1-level),
 * HistogramObject.cpp:158-161) into a uint64 histogram the context owns; accumulate = 1 adds to the one there (the
 * passes of one frame).  Every slot must hold a binned brick (VRC_EINVAL otherwise).  Deterministic (one owner per
 * bin, integer sums).  Enqueued behind the pool's uploads and before the context's render fence of the pool, so an
 * upload that recycles one of these slots waits for it. */
int vrc_frame_histogram( vrc_ctx* ctx, vrc_pool* pool, const float* slots /* n x 3 */, const uint64_t* scales,
                         uint32_t n, int accumulate );
/* copy the context's frame histogram to the host (waits for ctx's stream only).  bin_count must be that of the last
 * vrc_frame_histogram; VRC_EINVAL before the first */
int vrc_get_frame_histogram( vrc_ctx* ctx, uint64_t* host_bins, uint32_t bin_count );

/* ---- renderer ----------------------------------------------------------------------------- */
/* cuda::Renderer::update (cuda/Renderer.cu:245-250): 256 RGBA float texels as
 * lexis ColorMap::sampleColors<float>(256,0,256,0) yields them (cuda/ColorMap.cu:56-65), and
 * up to 6 clip planes (nx,ny,nz,d) (cuda/ClipPlanes.cu:32-46).  n_planes == 0 clears the
 * planes (the reference keeps stale ones, an obvious slip). */
int vrc_update( vrc_ctx* ctx, const float tf_rgba[256 * 4], const float* planes, uint32_t n_planes );
/* cuda::Renderer::preRender (cuda/Renderer.cu:252-257) + PixelBufferObject::resize/mapBuffer
 * (cuda/PixelBufferObject.cu:43-81): (re)allocate W x H float4 and clear it to 0.
 * W = glViewport[2], H = glViewport[3] (the reference's w-x / h-y is quirk Q10). */
int vrc_pre_render( vrc_ctx* ctx, const vrc_view_data* view );
/* render into caller-owned device memory instead (the reference renders into a GL-owned PBO):
 * width*height float4, cleared by vrc_pre_render like the internal one.  NULL returns to the
 * internal buffer. */
int vrc_set_framebuffer( vrc_ctx* ctx, void* device_rgba, uint32_t width, uint32_t height );
int vrc_get_framebuffer( vrc_ctx* ctx, void** device_rgba, uint32_t* width, uint32_t* height );
/* Sort-first row bands in ONE launch: the pixel buffer holds n_rows rows, row i of it being
 * frame row frame_rows[i] of the frame described by glViewport (whose w,h stay the FULL frame).
 * Takes effect at the next vrc_pre_render (buffer = glViewport.w x n_rows).  n_rows = 0 returns
 * to the plain case (buffer = glViewport.w x glViewport.h).  Rays are those of the full frame,
 * bit for bit.  (Replaces Equalizer's per-channel pixel viewport, livre/eq/Channel.cpp:272-290,
 * for a non-contiguous set of rows.) */
int vrc_set_row_map( vrc_ctx* ctx, const uint32_t* frame_rows, uint32_t n_rows );
/* cuda::Renderer::render (cuda/Renderer.cu:274-297): node table H2D + one rayCast pass that
 * accumulates into the pixel buffer.  nodes are in the host's front-to-back order. */
int vrc_render( vrc_ctx* ctx, const vrc_view_data* view, const vrc_node_data* nodes,
                uint32_t n_nodes, const vrc_render_data* render, vrc_pool* pool );
/* cuda::Renderer::postRender (cuda/Renderer.cu:299-326): the reference unmaps the PBO and
 * glDrawPixels it; here the frame is complete on the stream and, if host_rgba is non-NULL,
 * copied to W*H*4 floats of host memory (synchronous). */
int vrc_post_render( vrc_ctx* ctx, float* host_rgba );
int vrc_synchronize( vrc_ctx* ctx );
int vrc_get_stats( vrc_ctx* ctx, vrc_stats* out );
/* Ray compaction (VRC_OPT_ERT_COMPACTION = P) of the last vrc_render: counts[p] = rays still alive after launch p
 * (p = 0..P-2: the length of the list launch p + 1 marched), 0 for the rest of the 8 entries; *parts = P, or 0 when
 * that render did not use compaction.  Waits for the render. */
int vrc_get_ray_counts( vrc_ctx* ctx, uint32_t counts[8], int* parts );

/* The projected values of a MIP frame, any fold: M per pixel, for window / level and for measurements (the frame
 * buffer holds only its classification).  Synchronous on the context's stream.  W x H entries, those of the pixel buffer
 * the frame's last MIP vrc_render wrote -- internal, caller-owned or row-mapped (then H is the number of mapped rows).
 *   host_values[i]  M in the volume's own units: signed voxel types are un-shifted, a float M is returned as it is;
 *                   unspecified where the count is 0.
 *   host_counts[i]  (may be NULL)  VRC_MIP_FOLD_MEAN: the samples of the pixel over the passes so far; _MAX and _MIN: 1
 *                   where S is not empty, else 0.
 * Valid from a frame's first MIP vrc_render until the next vrc_pre_render; VRC_EINVAL otherwise (before any MIP render,
 * after a composite frame). */
int vrc_get_projection_values( vrc_ctx* ctx, float* host_values, uint32_t* host_counts );

/* The depths of a MIP frame rendered with depth tracking (VRC_OPT_MIP_DEPTH = 1 or VRC_OPT_MIP_DEPTH_CUE > 0; fold
 * _MAX or _MIN).  Validity, synchronisation and buffer geometry are those of vrc_get_projection_values; VRC_EINVAL,
 * naming the reason, also when the frame's MIP passes ran without depth tracking or with the mean fold.
 *   host_t[i]    D, the ray parameter of the nearest sample that equals M; +infinity where S is empty (and for a ray
 *                whose samples are all NaN: the counts of vrc_get_projection_values tell the two apart).
 *   host_xyz     (may be NULL; W x H x 3)  origin + D * dir of the pixel's ray in float32, product and sum each rounded,
 *                for the frame row the pixel shows under a row map; unspecified where D is not finite. */
int vrc_get_projection_depths( vrc_ctx* ctx, float* host_t, float* host_xyz );

/* The isosurface of VRC_PROJECTION_ISO frames ("An isosurface frame" above).  iso_value: in the volume's own units, as
 * dataSourceRange is (signed types un-shifted); ambient: the unlit share of the shading, in [0, 1].  VRC_EINVAL, naming
 * the argument, for a NaN or an ambient outside that range; the values set before stay. */
int vrc_set_isosurface( vrc_ctx* ctx, float iso_value, float ambient );
/* The gradients of an isosurface frame: host_g[3 i + a] = G_a of pixel i, 0 where the ray did not hit.  Validity,
 * synchronisation and buffer geometry are those of vrc_get_projection_values; VRC_EINVAL after a frame of another
 * projection. */
int vrc_get_projection_gradients( vrc_ctx* ctx, float* host_g /* W x H x 3 */ );

/* The plane of VRC_PROJECTION_SLICE frames ("A slice frame" above): plane = (nx, ny, nz, d), the points with
 * n.x + d = 0, in world coordinates as the clip planes of vrc_update are.  VRC_EINVAL, naming the argument, for NULL, an
 * entry that is not finite or a zero normal; the plane set before stays. */
int vrc_set_slice( vrc_ctx* ctx, const float plane[4] );

/* The table the last pre-integrated vrc_render of this context used ("A pre-integrated composite frame" above):
 * host_rgba[(row * 256 + col) * 4 + channel]; *kind (may be NULL) = 0 for the value-indexed table, 1 for the
 * texel-indexed one.  Synchronous on the context's stream.  VRC_EINVAL before any such render. */
int vrc_get_preintegrated_table( vrc_ctx* ctx, float* host_rgba /* 256 x 256 x 4 */, int* kind );

/* ---- sort-first tile exchange (multi-GPU) ------------------------------------------------------- */
/* One process per GPU renders row bands of the frame (vrc_set_row_map); the display rank receives
 * them over RCCL (xGMI inside a node) directly at their rows of the full frame.  This is the step
 * eq::Compositor::assembleFrame performs for the reference's sort-first compounds
 * (livre/eq/Channel.cpp:519-523; tiles: livre/eq/Channel.cpp:272-290) for a host without Equalizer.
 * No brick data moves between ranks.  RCCL is bound at run time (librccl.so.1); without it every
 * call below returns VRC_ECOMM except for a world of one rank. */
typedef struct vrc_comm vrc_comm;
#define VRC_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
/* ncclGetUniqueId: called by ONE rank; the caller hands the bytes to every rank (any transport) */
int vrc_comm_unique_id( uint8_t id_out[VRC_COMM_ID_BYTES] );
/* ncclCommInitRank on ctx's device; collective over the `world` ranks.  world == 1 needs no id
 * (may be NULL) and no RCCL. */
int vrc_comm_create( vrc_ctx* ctx, int rank, int world, const uint8_t id[VRC_COMM_ID_BYTES], vrc_comm** out );
void vrc_comm_destroy( vrc_comm* comm );
int vrc_comm_info( const vrc_comm* comm, int* rank, int* world );
/* one row band of the frame: rows [frame_row, frame_row + rows) are rendered by `rank` */
typedef struct
{
    uint32_t rank;
    uint32_t frame_row;
    uint32_t rows;
} vrc_band;
/* Collective over the communicator, asynchronous on hip_stream (NULL: ctx's render stream, i.e. behind
 * the vrc_render calls that produced the bands; another stream is made to wait for what ctx's render
 * stream holds at the time of the call).  `bands` lists every band of the width x height frame, identical
 * on all ranks; a rank's bands lie stacked in `local` in list order (what vrc_set_row_map renders),
 * width x rows RGBA32F each.  On rank `root` band b lands at row bands[b].frame_row of `frame` (its
 * own bands by device copies); `frame` is ignored elsewhere.  n_frames > 1 moves that many consecutive
 * frames with one group of sends/receives: frame f of a rank starts local_frame_stride bytes after
 * frame f-1 in `local`, and frame_stride bytes in `frame`.  Every band must lie inside the frame
 * (frame_row + rows <= height, checked in 64 bits) and a frame stride must hold a frame: nothing is
 * queued on any rank otherwise (VRC_EINVAL). */
int vrc_gather_tiles( vrc_ctx* ctx, vrc_comm* comm, const vrc_band* bands, uint32_t n_bands, uint32_t width,
                      uint32_t height, uint32_t n_frames, const void* local_device, size_t local_frame_stride,
                      void* frame_device, size_t frame_stride, int root, void* hip_stream );

const char* vrc_last_error( void );
/* the kernel instance the calling thread's last vrc_render launched (template arguments spelled as rocprofv3 prints
 * them), "" before the first: lets a benchmark check that a profile it quotes is a profile of what it ran */
const char* vrc_last_kernel( void );
/* ... and how many workgroups of it the runtime says a compute unit holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor:
 * registers, LDS and wave slots together), with the workgroup size: the occupancy the kernels' launch bounds ask for,
 * checkable without a profiler.  The vrc_k_raycast instances only (VRC_EINVAL after another kernel). */
int vrc_last_kernel_occupancy( int* workgroups_per_cu, int* threads_per_workgroup );
/* ABI version of this header */
#define VRC_ABI_VERSION 4 /* 3: vrc_gather_tiles takes the frame height; 4: VRC_KERNEL_PACKED, VRC_OPT_PACKED_ATLAS, vrc_last_kernel_occupancy
                           * (added since without a new number, as symbols a caller may bind weakly: the frame histogram,
                           * vrc_pool_create_typed / vrc_pool_voxel_type, vrc_get_projection_values,
                           * vrc_get_projection_depths, vrc_set_isosurface, vrc_get_projection_gradients,
                           * vrc_get_preintegrated_table, vrc_set_slice; as option
                           * values only: VRC_PROJECTION_ISO, VRC_PROJECTION_SLICE, VRC_OPT_PROJECTION, VRC_OPT_MIP_SKIP,
                           * VRC_OPT_MIP_FOLD, VRC_OPT_MIP_DEPTH, VRC_OPT_MIP_DEPTH_CUE) */
/* = VRC_ABI_VERSION for the product build; -VRC_ABI_VERSION for a developer build of the library (compiled with
 * -DVRC_DEV_BUILD: experiment switches, statistics, ablations that render wrong pixels on purpose) */
int vrc_abi_version( void );
int vrc_is_dev_build( void );

#ifdef __cplusplus
}
#endif
#endif /* VRC_HIP_H */
